"""uwm_optimize_masks_ragged on the device: ragged batches of the golden case list (tests/golden/maskpost.npz), word-boundary
shapes against the uniform call, the 'none' type against the restatement (tests/maskpost_ragged_ref.py), in-place use,
repeatability, misfits, and a call without stats.  Everything is integer work: every comparison is byte equality."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maskpost_ragged_ref as RR  # noqa: E402
import maskpost_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0x5A                                   # what gaps, guard band and untouched regions must keep
GUARD = 64
CODES = {"watermark": 0, "text": 1, "mixed": 2, "none": 3}


@pytest.fixture(scope="module")
def U(cuda):
    import __graft_entry__ as g
    g.build()
    import unet_watermark_amd as U
    return U


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _layout(shapes, rng):
    """mask descriptors at ANY alignment with gaps of 1..7 bytes in front of, between and behind the masks -> (descs, total bytes)"""
    from unet_watermark_amd.data import DESC_DTYPE
    descs = np.zeros(len(shapes), DESC_DTYPE)
    off = int(rng.integers(1, 8))
    for i, (h, w) in enumerate(shapes):
        descs[i] = (off, h, w)
        off += h * w + int(rng.integers(1, 8))
    return descs, off


def _pack(images, descs, nbytes):
    buf = np.full(nbytes + GUARD, FILL, np.uint8)
    for im, d in zip(images, descs):
        o = int(d["offset"])
        buf[o:o + im.size] = im.reshape(-1)
    return buf


def _region(buf, d):
    o, h, w = int(d["offset"]), int(d["h"]), int(d["w"])
    return buf[o:o + h * w].reshape(h, w)


def _call(cuda, buf, descs, nbytes, mask_type, max_pixels=None, rows=None, inplace=False, with_stats=True):
    """the ABI call on a host buffer of nbytes + GUARD bytes, of which the call is told nbytes -> (out buffer, stats (N, 8) or None)"""
    from unet_watermark_amd import _lib as L
    from unet_watermark_amd.data import descs_tensor
    lib = L.lib()
    n = len(descs)
    if max_pixels is None:
        max_pixels = int((descs["h"].astype(np.int64) * descs["w"]).max())
    if rows is None:
        rows = int(descs["h"].sum())
    src = torch.from_numpy(buf).to(cuda)
    dst = src if inplace else torch.full_like(src, FILL)
    dd = descs_tensor(descs, cuda)
    stats = torch.full((n, 8), -77, dtype=torch.int64, device=cuda) if with_stats else None
    need = lib.uwm_mask_ragged_workspace_bytes(n, nbytes, rows)
    assert need > 0
    ws = torch.empty(need + 256, dtype=torch.uint8, device=cuda)
    ws[need:] = FILL
    L.check(lib.uwm_optimize_masks_ragged(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), nbytes, C.c_void_p(dd.data_ptr()), n,
                                          CODES[mask_type], max_pixels, rows, C.c_void_p(stats.data_ptr() if with_stats else 0),
                                          C.c_void_p(ws.data_ptr()), need, C.c_void_p(L.stream_ptr(cuda))))
    torch.cuda.synchronize(cuda)
    assert bool((ws[need:] == FILL).all()), "a write behind the workspace"
    if not inplace:
        assert torch.equal(src.cpu(), torch.from_numpy(buf)), "the input was written"
    return dst.cpu().numpy(), (stats.cpu().numpy() if with_stats else None)


def _untouched(out, descs, nbytes, skip=()):
    """everything outside the images' regions (gaps, guard band) and the regions of `skip` still hold the fill byte"""
    covered = np.zeros(len(out), bool)
    for i, d in enumerate(descs):
        if i not in skip:
            o = int(d["offset"])
            covered[o:o + int(d["h"]) * int(d["w"])] = True
    assert (out[~covered] == FILL).all(), "a write outside the masks"
    assert (out[nbytes:] == FILL).all(), "a write into the guard band"


def _kept_of_output(out):
    """count and largest area of the output's components (= the kept ones: tests/test_maskpost_ragged.py)"""
    _, areas = R.components(out > 127)
    a = areas[areas > 0]
    return [len(a), int(a.max()) if len(a) else 0]


@pytest.mark.parametrize("mask_type", R.MASK_TYPES)
def test_golden_cases_in_ragged_batches(U, cuda, golden, mask_type):
    """every image of the golden file, dealt round-robin into three batches so that 1 x 1 and 1 x 130 ride with 768 x 1024"""
    images = [(img, out, summary) for _, batch, want in golden for img, out, summary in zip(batch, *want[mask_type])]
    assert len(images) == 30
    rng = np.random.default_rng(41)
    for b in range(3):
        part = images[b::3]
        descs, nbytes = _layout([im.shape for im, _, _ in part], rng)
        out, stats = _call(cuda, _pack([im for im, _, _ in part], descs, nbytes), descs, nbytes, mask_type)
        _untouched(out, descs, nbytes)
        for i, ((img, want, summary), d) in enumerate(zip(part, descs)):
            assert np.array_equal(_region(out, d), want), (mask_type, b, i, img.shape)
            assert stats[i].tolist() == [int(v) for v in summary] + _kept_of_output(want) + [img.size, 0], (mask_type, b, i, img.shape)
    assert {(1, 1), (1, 130), (768, 1024)} <= {im.shape for im, _, _ in images}


WORD_SHAPES = ((1, 1), (1, 63), (1, 64), (1, 65), (7, 1), (64, 64), (65, 63), (2, 129), (37, 200))


def _word_images():
    g = np.random.default_rng(42)
    return [(R.synth(h, w, 200 + i) if h * w > 4000 else g.random((h, w)) < 0.6).astype(np.uint8) * 255 for i, (h, w) in enumerate(WORD_SHAPES)]


@pytest.mark.parametrize("mask_type", R.MASK_TYPES)
def test_word_boundary_shapes_equal_the_uniform_call(U, cuda, mask_type):
    images = _word_images()
    descs, nbytes = _layout(WORD_SHAPES, np.random.default_rng(43))
    out, stats = _call(cuda, _pack(images, descs, nbytes), descs, nbytes, mask_type)
    _untouched(out, descs, nbytes)
    for im, d, row in zip(images, descs, stats):
        want, summary = U.optimize_mask(torch.from_numpy(im).to(cuda), mask_type, return_summary=True)
        want = want.cpu().numpy()
        assert np.array_equal(_region(out, d), want), (mask_type, im.shape)
        assert row.tolist() == summary.cpu().tolist() + _kept_of_output(want) + [im.size, 0], (mask_type, im.shape)


def _none_batch():
    planes = [v[0] for v in RR.stress_planes().values()] + [R.synth(333, 517, 77)]
    return [p.astype(np.uint8) * 255 for p in planes]


def test_none_type_equals_the_restatement(U, cuda):
    images = _none_batch()
    descs, nbytes = _layout([im.shape for im in images], np.random.default_rng(44))
    out, stats = _call(cuda, _pack(images, descs, nbytes), descs, nbytes, "none")
    _untouched(out, descs, nbytes)
    for im, d, row in zip(images, descs, stats):
        want, want_row = RR.optimize(im, "none")
        assert np.array_equal(_region(out, d), want) and row.tolist() == want_row, (im.shape, row.tolist(), want_row)
        assert row[4] == row[0] and row[5] == row[1]
    assert stats[:4, :2].tolist() == [[1, 4225], [1, 4290], [1, 4322], [2145, 1]]


@pytest.mark.parametrize("mask_type", RR.TYPES)
def test_in_place_and_a_second_run_give_the_same_bytes(U, cuda, mask_type):
    images = _word_images() + _none_batch()
    descs, nbytes = _layout([im.shape for im in images], np.random.default_rng(45))
    buf = _pack(images, descs, nbytes)
    out, stats = _call(cuda, buf, descs, nbytes, mask_type)
    again, stats2 = _call(cuda, buf, descs, nbytes, mask_type)
    assert np.array_equal(out, again) and np.array_equal(stats, stats2)
    inplace, stats3 = _call(cuda, buf, descs, nbytes, mask_type, inplace=True)
    assert np.array_equal(inplace, out) and np.array_equal(stats3, stats)
    none, no_stats = _call(cuda, buf, descs, nbytes, mask_type, with_stats=False)      # stats = NULL runs
    assert no_stats is None and np.array_equal(none, out)


def test_larger_capacities_change_nothing(U, cuda):
    """max_pixels and rows are capacities: the same batch under generous ones gives the same bytes"""
    images = _word_images()
    descs, nbytes = _layout(WORD_SHAPES, np.random.default_rng(46))
    buf = _pack(images, descs, nbytes)
    out, stats = _call(cuda, buf, descs, nbytes, "watermark")
    big, stats2 = _call(cuda, buf, descs, nbytes, "watermark", max_pixels=3_000_000, rows=50_000)
    assert np.array_equal(out, big) and np.array_equal(stats, stats2)


@pytest.mark.parametrize("mask_type", ("watermark", "none"))
def test_misfits_cost_only_themselves(U, cuda, mask_type):
    from unet_watermark_amd.data import DESC_DTYPE
    rng = np.random.default_rng(47)
    shapes = [(20, 30), (5, 5), (8, 8), (40, 50), (10, 10), (6, 7), (25, 8), (3, 3)]
    descs, nbytes = _layout(shapes, rng)
    images = [(rng.random(s) < 0.7).astype(np.uint8) * 255 for s in shapes]
    buf = _pack(images, descs, nbytes)
    descs = descs.astype(DESC_DTYPE)
    descs[1]["h"] = 0                                        # a zero side
    descs[2]["offset"] = nbytes - 10                         # its region leaves [0, mask_bytes) (and would reach the guard band)
    descs[5]["offset"] = -4                                  # ... at the other end
    max_pixels = 1500                                        # image 3 has 2000 pixels
    rows = 20 + 10 + 24                                      # images 0 and 4 fit; image 6 (25 rows) does not, nor image 7 after it
    want_misfit = [False, True, True, True, False, True, True, True]
    assert RR.misfits(descs, nbytes, max_pixels, rows) == want_misfit
    out, stats = _call(cuda, buf, descs, nbytes, mask_type, max_pixels=max_pixels, rows=rows)
    good = [i for i, m in enumerate(want_misfit) if not m]
    assert (out[nbytes:] == FILL).all() and (out[:int(descs[0]["offset"])] == FILL).all()
    covered = np.zeros(len(out), bool)
    for i in good:
        o = int(descs[i]["offset"])
        covered[o:o + images[i].size] = True
        want, row = RR.optimize(images[i], mask_type)
        assert np.array_equal(_region(out, descs[i]), want) and stats[i].tolist() == row, (i, stats[i].tolist(), row)
    assert (out[~covered] == FILL).all(), "a misfit's bytes were written"
    for i, m in enumerate(want_misfit):
        if m:
            assert stats[i].tolist() == RR.MISFIT_ROW, (i, stats[i].tolist())
    # the same batch with room for everything that is well-formed: only the malformed ones stay misfits
    out2, stats2 = _call(cuda, buf, descs, nbytes, mask_type, max_pixels=4000, rows=500)
    assert stats2[:, 7].tolist() == [0, 1, 1, 0, 0, 1, 0, 0]
    for i in (0, 3, 4, 6, 7):
        want, row = RR.optimize(images[i], mask_type)
        assert np.array_equal(_region(out2, descs[i]), want) and stats2[i].tolist() == row, i


def test_python_entry_point(U, cuda):
    """postprocess.optimize_masks_ragged: host descriptors, a new output buffer, the stats tensor"""
    from unet_watermark_amd.postprocess import optimize_masks_ragged
    images = _word_images()
    descs, nbytes = _layout(WORD_SHAPES, np.random.default_rng(48))
    buf = torch.from_numpy(_pack(images, descs, nbytes)[:nbytes].copy()).to(cuda)
    out, stats = optimize_masks_ragged(buf, descs, "text", return_stats=True)
    assert out.data_ptr() != buf.data_ptr() and stats.shape == (len(images), 8) and stats.dtype == torch.int64
    same = optimize_masks_ragged(buf.clone(), descs, "text")
    assert torch.equal(same, out)
    for im, d, row in zip(images, descs, stats.cpu().numpy()):
        want, summary = U.optimize_mask(torch.from_numpy(im).to(cuda), "text", return_summary=True)
        assert np.array_equal(_region(out.cpu().numpy(), d), want.cpu().numpy()) and row[:4].tolist() == summary.cpu().tolist()
    with pytest.raises(ValueError):
        optimize_masks_ragged(buf, descs, "auto")
    with pytest.raises(RuntimeError):
        optimize_masks_ragged(buf.cpu(), descs, "text")
