"""Text-feature enhancement, the part that needs no device.  tests/textenh_ref.py restates the reference's _enhance_text_features in
the literal form (cv2's Canny loop with prev_flag, stack and map; CLAHE's explicit border copy); the kernels (csrc/text_enhance.hip)
compute the hysteresis as a component property and read borders by index.  Here the literal form is held to the kernels' form and to
independent library routines: Canny to candidates labelled by scipy.ndimage.label, Sobel and the sharpening filter to
scipy.ndimage.correlate, the dilation to maskpost_ref.dilate, CLAHE to augment_ext_ref.clahe_plane where the padding rules agree and
to a hand-computed case where they differ.  Then the claims the GPU test's cases rest on, the command line and the new symbols."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ext_ref as AE  # noqa: E402
import maskpost_ref as M  # noqa: E402
import textenh_ref as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("uwm_text_enhance_workspace_bytes", "uwm_text_enhance_ragged")
EIGHT = np.ones((3, 3), dtype=np.int64)


def component_canny(plane):
    """the form the kernels use: the candidates of the 8-connected components that hold a strong one"""
    cand, strong = T.candidates(plane)
    lab, _ = ndimage.label(cand, structure=EIGHT)
    keep = np.unique(lab[strong])
    return (np.isin(lab, keep[keep > 0]) & cand).astype(np.uint8) * 255


def ridge(strong_at_end):
    """a vertical step of 20 grey levels (magnitude 80: weak) over 40 rows; strong_at_end: the last two rows step by 60"""
    p = np.full((40, 24), 100, dtype=np.uint8)
    p[:, 12:] = 120
    if strong_at_end:
        p[38:, 12:] = 160
    return p


def ramp_with_ties():
    """a flat ramp of slope 10 per column (every magnitude 4 * 2 * 10 = 80: ties everywhere) next to steps"""
    p = np.zeros((20, 30), dtype=np.int64)
    p[:, :10] = 10 * np.arange(10)[None, :]
    p[:, 10:] = 250
    p[12:, 20:] = 60
    return p.astype(np.uint8)


HAND_MADE = {"weak-only ridge": ridge(False), "ridge, strong at the far end": ridge(True), "ties along a ramp": ramp_with_ties()}


def test_literal_canny_equals_the_component_form_on_random_images():
    rng = np.random.default_rng(7)
    seen_dropped = 0
    for k in range(12):
        h, w = int(rng.integers(16, 48)), int(rng.integers(16, 64))
        plane = T.gray(T._blocks(rng, h, w, step=int(rng.integers(2, 7)))) if k % 2 else rng.integers(90, 140, (h, w)).astype(np.uint8)
        lit = T.canny(plane)
        assert np.array_equal(lit, component_canny(plane)), (k, h, w)
        cand, _ = T.candidates(plane)
        seen_dropped += int((cand & (lit == 0)).sum())
    assert seen_dropped > 0          # hysteresis dropped weak candidates somewhere: the comparison is no tautology


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_literal_canny_equals_the_component_form_on_hand_made_images(name):
    plane = HAND_MADE[name]
    lit = T.canny(plane)
    assert np.array_equal(lit, component_canny(plane))
    cand, strong = T.candidates(plane)
    if name == "weak-only ridge":
        assert cand.sum() == 40 and strong.sum() == 0 and lit.sum() == 0
    elif name == "ridge, strong at the far end":
        assert strong.any() and np.argwhere(strong)[:, 0].min() >= 36 and lit[0].any()      # the far end pulls the whole ridge in
    else:
        dx, dy = T.sobel(plane)
        m = np.abs(dx) + np.abs(dy)
        assert (m[:, 1:9] == 80).all() and not cand[:, 2:9].any()      # a tie on the left fails `>`: nothing inside a flat ramp survives
        assert cand[:, 1].all()                                        # ... but its first pixel does: 80 > 40 (replicated border) and 80 >= 80
        assert lit.any()


def test_sobel_and_sharpen_equal_scipy_correlate():
    rng = np.random.default_rng(11)
    kx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], dtype=np.int64)
    for h, w in ((16, 16), (17, 23), (5, 40)):
        plane = rng.integers(0, 256, (h, w)).astype(np.uint8)
        dx, dy = T.sobel(plane)
        assert np.array_equal(dx, ndimage.correlate(plane.astype(np.int64), kx, mode="nearest"))
        assert np.array_equal(dy, ndimage.correlate(plane.astype(np.int64), kx.T, mode="nearest"))
        img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        want = np.stack([np.clip(ndimage.correlate(img[..., c].astype(np.int64), T.SHARPEN, mode="mirror"), 0, 255) for c in range(3)], axis=-1)
        assert np.array_equal(T.sharpen(img), want.astype(np.uint8))


def test_dilate2_equals_the_ellipse_2x2_dilation():
    rng = np.random.default_rng(13)
    k = M.ellipse(2, 2)
    assert np.array_equal(k, [[0, 1], [1, 1]])
    for h, w in ((1, 1), (16, 16), (17, 23)):
        e = (rng.random((h, w)) < 0.2)
        assert np.array_equal(T.dilate2(e.astype(np.uint8) * 255) > 0, M.dilate(e, k))


def test_boost_is_the_table_of_truncated_float32_products():
    v = np.arange(256, dtype=np.uint8)
    img = np.repeat(v[None, :, None], 3, axis=2)
    table = np.minimum(v.astype(np.float32) * np.float32(1.2), np.float32(255)).astype(np.uint8)
    assert np.array_equal(T.boost(img, np.full((1, 256), 255, np.uint8))[0, :, 1], table)
    assert np.array_equal(T.boost(img, np.zeros((1, 256), np.uint8)), img)
    assert table[212] == 254 and table[213] == 255 and table[5] == 6 and table[4] == 4


@pytest.mark.parametrize("shape", ((16, 16), (40, 64), (17, 23), (33, 130), (96, 200)))
def test_clahe_equals_the_augmentation_restatement_where_the_padding_rules_agree(shape):
    """both sides divide by 8, or neither does: round-up and cv2's rule give the same padded size"""
    h, w = shape
    assert (h % 8 == 0) == (w % 8 == 0)
    rng = np.random.default_rng(h * 1000 + w)
    plane = T.gray(T._blocks(rng, h, w))
    bottom, right, th, tw = T.clahe_geometry(h, w)
    assert (h + bottom, w + right, th, tw) == AE._tile_geometry(h, w)
    assert np.array_equal(T.clahe(plane), AE.clahe_plane(plane, T.clahe_clip(th, tw)))


def test_clahe_padding_where_the_rules_differ_16x20():
    """16 x 20: 20 % 8 = 4, so cv2 extends the right by 4 AND the bottom by a full 8: 24 x 24, tiles 3 x 3 (round-up would give
    16 x 24, tiles 2 x 3), clip limit max(int(2 * 9 / 256), 1) = 1.  By hand, for the image whose pixel (y, x) is 8 y + x: tile
    (7, 7) is padded rows 21..23 = rows 9, 8, 7 and padded columns 21..23 = columns 17, 16, 15, i.e. the nine values 8 r + c."""
    assert T.clahe_geometry(16, 20) == (8, 4, 3, 3) and AE._tile_geometry(16, 20)[2:] == (2, 3)
    assert T.clahe_geometry(16, 24) == (0, 0, 2, 3) and T.clahe_geometry(17, 24) == (7, 8, 3, 4)
    assert T.clahe_clip(3, 3) == 1 and T.clahe_clip(90, 160) == 112
    plane = (8 * np.arange(16)[:, None] + np.arange(20)[None, :]).astype(np.uint8)
    pad = T.border_reflect101(plane, 8, 4)
    assert pad.shape == (24, 24)
    assert np.array_equal(pad[21:24, 21:24], [[8 * r + c for c in (17, 16, 15)] for r in (9, 8, 7)])
    assert np.array_equal(pad, plane[AE.A.reflect101(np.arange(24), 16)][:, AE.A.reflect101(np.arange(24), 20)])
    # the table of tile (7, 7): the nine values are distinct, so no bin exceeds the limit 1, nothing is redistributed, and the table
    # is rint(count of values <= v) * (255 / 9))
    vals = np.array([8 * r + c for r in (9, 8, 7) for c in (17, 16, 15)])
    want = np.rint((vals[None, :] <= np.arange(256)[:, None]).sum(axis=1).astype(np.float32) * (np.float32(255.0) / np.float32(9))).astype(np.uint8)
    assert np.array_equal(T.clahe_luts(plane)[7, 7], want)
    # the tile of the round-up rule is another one: the results differ
    assert not np.array_equal(T.clahe(plane), AE.clahe_plane(plane, 1))


def test_the_gpu_cases_are_what_they_claim():
    cases = dict(T.images())
    res = {k: T.text_enhance(v) for k, v in cases.items()}
    assert res["constant"][2] == T.DONE and not res["constant"][1].any() and np.array_equal(res["constant"][0], cases["constant"])
    assert res["small 12x40"][2] == T.COPIED and np.array_equal(res["small 12x40"][0], cases["small 12x40"])
    e = res["borders"][1]
    assert e[0].any() and e[-1].any() and e[:, 0].any() and e[:, -1].any()
    for name in ("least 16x16", "17x23", "16x20", "40x64", "33x130"):
        assert res[name][1].any() and not res[name][1].all(), name
    # the spiral: ONE component of weak candidates through all 64 tiles, one strong pixel at the inner end; without it nothing is left
    img, end = T.spiral(True)
    cl = T.clahe(T.gray(img))
    cand, strong = T.candidates(cl)
    lab, n = ndimage.label(cand, structure=EIGHT)
    assert n == 1 and strong.sum() == 1 and tuple(np.argwhere(strong)[0]) == end
    ys, xs = np.nonzero(cand)
    assert len(set(zip((ys // 12).tolist(), (xs // 25).tolist()))) == 64
    assert (T.canny(cl) > 0).sum() == cand.sum()
    cand_w, strong_w = T.candidates(T.clahe(T.gray(T.spiral(False)[0])))
    assert cand_w.sum() > 2000 and not strong_w.any() and not res["spiral weak"][1].any()
    assert np.array_equal(res["spiral weak"][0], T.sharpen(cases["spiral weak"]))


def test_the_parser_takes_text_enhance_and_predict_refuses_it_on_the_host_path(tmp_path):
    from unet_watermark_amd.cli import build_parser, predict_command
    base = ["predict", "--input", str(tmp_path), "--output", str(tmp_path / "out"), "--model", "none.pth"]
    args = build_parser().parse_args(base + ["--resize", "device", "--text-enhance", "--mask-type", "text"])
    assert args.text_enhance is True and args.resize == "device"
    assert build_parser().parse_args(base).text_enhance is False
    with pytest.raises(ValueError, match="--text-enhance needs --resize device"):
        predict_command(build_parser().parse_args(base + ["--resize", "host", "--text-enhance"]))
    assert not (tmp_path / "out").exists()          # refused before anything was made


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from unet_watermark_amd import _lib
    _lib.lib()
    return _lib


def test_the_library_exports_the_new_symbols_and_the_header_declares_them(L):
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "uwm.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in L.SIGNATURES
        assert f" {name}(" in header, name


def test_uwm_text_enhance_ragged_checks_arguments_before_any_launch(L):
    """no device is needed: every bad call returns non-zero with a message that names the call, before the first launch"""
    lib = L.lib()
    assert lib.uwm_text_enhance_workspace_bytes(0, 1) == 0 and b"total_pixels" in lib.uwm_last_error()
    assert lib.uwm_text_enhance_workspace_bytes(100, 0) == 0 and b"N must be" in lib.uwm_last_error()
    need = lib.uwm_text_enhance_workspace_bytes(1000, 2)
    assert need >= 2 * 64 * 256 + 12 * 1000
    base = dict(inp=0x10000, out=0x20000, nbytes=3000, descs=0x30000, N=2, C=3, max_pixels=1000, total=1000, edges=0, ebytes=0, ed=0,
                ws=0x40000, wsb=need, stream=0)
    bad = [(dict(inp=0), "null"), (dict(ws=0), "null"), (dict(C=1), "C must be 3"), (dict(N=0), "N must be"), (dict(N=70000), "N must be"),
           (dict(nbytes=0), "bytes"), (dict(max_pixels=0), "max_pixels"), (dict(max_pixels=(1 << 30) + 1), "max_pixels"),
           (dict(total=0), "total_pixels"), (dict(out=0x10000), "overlap"), (dict(out=0x10000 + 2999), "overlap"),
           (dict(edges=0x50000), "edge_descs"), (dict(edges=0x50000, ed=0x60000, ebytes=0), "edges_bytes"),
           (dict(edges=0x20010, ed=0x60000, ebytes=1000), "overlap"), (dict(descs=0x30004), "aligned"), (dict(ws=0x40004), "aligned"),
           (dict(wsb=need - 1), "workspace too small")]
    for kw, word in bad:
        v = {**base, **kw}
        rc = lib.uwm_text_enhance_ragged(v["inp"], v["out"], v["nbytes"], v["descs"], v["N"], v["C"], v["max_pixels"], v["total"], v["edges"],
                                         v["ebytes"], v["ed"], v["ws"], v["wsb"], v["stream"])
        msg = lib.uwm_last_error().decode()
        assert rc != 0 and "uwm_text_enhance_ragged" in msg and word in msg, (kw, msg)


def test_the_python_entry_points_have_no_cpu_fallback(L):
    import torch
    from unet_watermark_amd import textenh
    with pytest.raises(RuntimeError, match="HIP device"):
        textenh.text_enhance_ragged(torch.zeros(768, dtype=torch.uint8), np.zeros(1, [("offset", "<i8"), ("h", "<i4"), ("w", "<i4")]))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            textenh.enhance_text_features([np.zeros((16, 16, 3), np.uint8)])
