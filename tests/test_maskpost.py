"""Mask post-processing, the part that needs no device: the structuring elements of uwm_mask_element against the tables of
DESIGN.md §8b, the golden file against the numpy restatement (tests/maskpost_ref.py), the restatement against scipy where scipy
is installed, and the argument checks of the device entry points, which fail before any launch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maskpost_ref as R  # noqa: E402

ELLIPSES = {
    (2, 2): "01 11",
    (3, 3): "010 111 010",
    (4, 4): "0010 1111 1111 1111",
    (5, 5): "00100 11111 11111 11111 00100",
    (6, 6): "000100 011111 111111 111111 111111 011111",
    (7, 7): "0001000 0111110 1111111 1111111 1111111 0111110 0001000",
    (9, 9): "000010000 011111110 011111110 111111111 111111111 111111111 011111110 011111110 000010000",
    (11, 11): "00000100000 00111111100 01111111110 " + "11111111111 " * 5 + "01111111110 00111111100 00000100000",
}


def _table(rows):
    return np.array([[int(ch) for ch in r] for r in rows.split()], np.uint8)


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from unet_watermark_amd import _lib
    _lib.lib()
    return _lib


@pytest.mark.parametrize("wh", sorted(ELLIPSES))
def test_ellipse_tables(L, wh):
    from unet_watermark_amd.postprocess import structuring_element
    want = _table(ELLIPSES[wh])
    assert np.array_equal(structuring_element("ellipse", wh), want)
    assert np.array_equal(structuring_element(2, wh), want)
    assert np.array_equal(R.ellipse(*wh), want)


def test_line_and_rect_elements(L):
    from unet_watermark_amd.postprocess import structuring_element
    assert np.array_equal(structuring_element("rect", (5, 1)), np.ones((1, 5), np.uint8))
    assert np.array_equal(structuring_element("rect", (1, 5)), np.ones((5, 1), np.uint8))
    assert np.array_equal(structuring_element("rect", 15), np.ones((15, 15), np.uint8))
    for w in range(1, 16):                                    # every size the ABI takes, against the restatement
        for h in range(1, 16):
            assert np.array_equal(structuring_element("ellipse", (w, h)), R.ellipse(w, h)), (w, h)


def test_element_rejects_bad_arguments(L):
    from unet_watermark_amd.postprocess import structuring_element
    lib = L.lib()
    buf = (C.c_uint8 * 256)()
    for shape, kw, kh in ((0, 0, 3), (0, 3, 0), (2, 16, 3), (2, 3, 16), (1, 3, 3), (7, 3, 3), (0, -1, 3)):
        assert lib.uwm_mask_element(shape, kw, kh, buf) != 0
        assert lib.uwm_last_error()
    assert lib.uwm_mask_element(2, 3, 3, None) != 0
    with pytest.raises(ValueError):
        structuring_element("ellipse", (16, 3))
    with pytest.raises(ValueError):
        structuring_element("cross", (3, 3))


def test_golden_file_equals_the_restatement():
    have = dict(np.load(R.GOLDEN_PATH))
    want = R.build_golden()
    assert sorted(have) == sorted(want)
    for k in want:
        assert have[k].dtype == want[k].dtype and np.array_equal(have[k], want[k]), k
    assert os.path.getsize(R.GOLDEN_PATH) < 200 * 1024


def test_golden_case_list_and_pixel_counts():
    cases = {name: (x, exp) for name, x, exp in R.load_golden()}
    for name, counts in R.EXPECTED_COUNTS.items():
        x, exp = cases[name]
        got = tuple(int((exp[t][0] > 127).sum()) for t in R.MASK_TYPES)
        assert got == counts, (name, got)
        for t, c in zip(R.MASK_TYPES, counts):
            assert int(exp[t][1][:, 2].sum()) == c
    assert cases["one_pixel"][0].shape == (1, 1, 1) and cases["row130"][0].shape == (1, 1, 130)
    # exact tie of the two largest: the first in raster order wins, rows / columns 22..57
    out, summary = cases["tie"][1]["watermark"]
    ys, xs = np.nonzero(out[0])
    assert (ys.min(), ys.max(), xs.min(), xs.max()) == (22, 57, 22, 57) and summary[0, 0] == 2
    out, summary = cases["tie_corner"][1]["watermark"]
    assert out[0, 0, 0] == 255 and out[0, -1, -1] == 0 and summary[0, 3] == 0
    # the `< 500` / `> 200` branch keeps both small blobs
    assert cases["sq3x2"][1]["watermark"][1][0, :3].tolist() == [2, 265, 530]
    assert cases["empty"][1]["watermark"][1][0].tolist() == [0, 0, 0, -1]
    for h, w in R.SEEDED_SIZES:
        assert cases[f"seeded_{h}x{w}_n1"][0].shape == (1, h, w) and cases[f"seeded_{h}x{w}_n3"][0].shape == (3, h, w)
        b = cases[f"seeded_{h}x{w}_n3"][0]
        assert not np.array_equal(b[0], b[1]) and not np.array_equal(b[1], b[2])


def test_restatement_morphology_equals_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    m = R.synth(100, 130, 7)
    for s in (3, 5, 7, 9, 11):                                # odd ellipses are symmetric: the conventions coincide
        k = R.ellipse(s, s)
        assert np.array_equal(R.dilate(m, k), ndi.binary_dilation(m, structure=k)), s
        assert np.array_equal(R.erode(m, k), ndi.binary_erosion(m, structure=k, border_value=1)), s


def test_restatement_labelling_equals_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for h, w, seed in ((64, 64, 1), (37, 200, 2), (333, 517, 3)):
        m = R.synth(h, w, seed)
        lab, n = ndi.label(m, structure=np.ones((3, 3), int))
        labels, areas = R.components(m)
        assert (labels > 0).tolist() == m.tolist()
        pairs = set(zip(lab[m].tolist(), labels[m].tolist()))        # same partition: a bijection between the label sets
        assert len(pairs) == n == len({a for a, _ in pairs}) == len({b for _, b in pairs})
        ids = np.nonzero(areas.reshape(-1))[0]
        assert len(ids) == n
        for i in ids:                                                # id = first pixel in raster order; area = pixel count
            assert labels.reshape(-1)[i] == i + 1 and areas.reshape(-1)[i] == int((labels == i + 1).sum())
            assert np.nonzero(labels.reshape(-1) == i + 1)[0][0] == i


def test_restatement_labelling_without_scipy():
    """the same properties from first principles on a small mask (flood fill), so the labelling is checked where scipy is missing"""
    m = R.synth(40, 70, 11)
    labels, areas = R.components(m)
    seen = np.zeros_like(m)
    H, W = m.shape
    for p in range(H * W):
        y, x = divmod(p, W)
        if not m[y, x] or seen[y, x]:
            continue
        stack, comp = [(y, x)], []
        seen[y, x] = True
        while stack:
            cy, cx = stack.pop()
            comp.append((cy, cx))
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    ny, nx = cy + dy, cx + dx
                    if 0 <= ny < H and 0 <= nx < W and m[ny, nx] and not seen[ny, nx]:
                        seen[ny, nx] = True
                        stack.append((ny, nx))
        for cy, cx in comp:
            assert labels[cy, cx] == p + 1
        assert areas[y, x] == len(comp)
    assert int(areas.sum()) == int(m.sum()) and (labels[~m] == 0).all()


def test_device_entry_points_check_arguments_before_any_launch(L):
    """every bad call returns non-zero with a message; none of them reaches a launch (there is no device here, and the pointers
    are not device memory)"""
    lib = L.lib()
    buf = (C.c_uint8 * 4096)()
    p = C.cast(buf, C.c_void_p)
    ws_bytes = lib.uwm_mask_workspace_bytes(1, 8, 8)
    assert ws_bytes > 0 and lib.uwm_mask_workspace_bytes(0, 8, 8) == 0 and lib.uwm_mask_workspace_bytes(1, 65536, 65536) == 0
    assert lib.uwm_mask_workspace_bytes(3, 768, 1024) >= 3 * 768 * 1024 * 8

    def bad(rc, word):
        assert rc != 0
        msg = lib.uwm_last_error().decode()
        assert word in msg, msg

    bad(lib.uwm_optimize_mask(None, p, 1, 8, 8, 0, None, p, ws_bytes, None), "null")
    bad(lib.uwm_optimize_mask(p, None, 1, 8, 8, 0, None, p, ws_bytes, None), "null")
    bad(lib.uwm_optimize_mask(p, p, 1, 8, 8, 0, None, None, ws_bytes, None), "workspace")
    bad(lib.uwm_optimize_mask(p, p, 0, 8, 8, 0, None, p, ws_bytes, None), ">= 1")
    bad(lib.uwm_optimize_mask(p, p, 1, 0, 8, 0, None, p, ws_bytes, None), ">= 1")
    bad(lib.uwm_optimize_mask(p, p, 1, 8, -1, 0, None, p, ws_bytes, None), ">= 1")
    bad(lib.uwm_optimize_mask(p, p, 1, 65536, 65536, 0, None, p, ws_bytes, None), "2^31")
    bad(lib.uwm_optimize_mask(p, p, 1, 8, 8, 3, None, p, ws_bytes, None), "mask type")
    bad(lib.uwm_optimize_mask(p, p, 1, 8, 8, -1, None, p, ws_bytes, None), "mask type")
    bad(lib.uwm_optimize_mask(p, p, 1, 8, 8, 0, None, p, ws_bytes - 1, None), "too small")
    bad(lib.uwm_op_morph(None, p, 1, 8, 8, 1, 2, 3, 3, 1, p, ws_bytes, None), "null")
    bad(lib.uwm_op_morph(p, p, 1, 8, 8, 1, 1, 3, 3, 1, p, ws_bytes, None), "shape")
    bad(lib.uwm_op_morph(p, p, 1, 8, 8, 1, 2, 16, 3, 1, p, ws_bytes, None), "1..15")
    bad(lib.uwm_op_morph(p, p, 1, 8, 8, 1, 2, 3, 0, 1, p, ws_bytes, None), "1..15")
    bad(lib.uwm_op_morph(p, p, 1, 8, 8, 1, 2, 3, 3, 0, p, ws_bytes, None), "iterations")
    bad(lib.uwm_op_morph(p, p, 1, 8, 8, 1, 2, 3, 3, 1, p, 16, None), "too small")
    bad(lib.uwm_op_morph(p, p, 1, 8, 0, 1, 2, 3, 3, 1, p, ws_bytes, None), ">= 1")
    bad(lib.uwm_op_components(p, None, p, 1, 8, 8, p, ws_bytes, None), "null")
    bad(lib.uwm_op_components(p, p, None, 1, 8, 8, p, ws_bytes, None), "null")
    bad(lib.uwm_op_components(p, p, p, 1, 8, 8, None, ws_bytes, None), "workspace")
    bad(lib.uwm_op_components(p, p, p, 1, 8, 8, p, 0, None), "too small")
    bad(lib.uwm_op_components(p, p, p, 0, 8, 8, p, ws_bytes, None), ">= 1")


def test_python_layer_has_no_cpu_fallback_and_names_the_types(L):
    import unet_watermark_amd as U
    from unet_watermark_amd import postprocess as PP
    m = torch.zeros(8, 8, dtype=torch.uint8)
    for fn in (lambda: U.optimize_mask(m), lambda: U.morphology(m, "dilate", "ellipse", 3), lambda: U.connected_components(m)):
        with pytest.raises(RuntimeError, match="runs only on a HIP device"):
            fn()
    with pytest.raises(ValueError, match="'watermark', 'text', 'mixed'"):
        U.optimize_mask(m, "logo")
    assert PP.MASK_TYPES == {"watermark": 0, "text": 1, "mixed": 2}


def test_cli_and_predictor_take_the_mask_type(L, monkeypatch):
    import inspect
    from unet_watermark_amd import cli
    from unet_watermark_amd.predict import WatermarkPredictor
    with pytest.raises(SystemExit):
        cli.main(["predict", "--input", "a", "--output", "b", "--model", "c", "--mask-type", "logo"])
    for name in ("predict_mask", "predict_mask_u8"):
        assert inspect.signature(getattr(WatermarkPredictor, name)).parameters["mask_type"].default is None
    assert inspect.signature(WatermarkPredictor.predict_mask_u8).parameters["return_summary"].default is False
