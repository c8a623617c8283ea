"""Ragged mask post-processing, the part that needs no device: the kept-component statistics of the restatement
(tests/maskpost_ragged_ref.py) against an independent labelling of the golden outputs, hand-computed planes for the 'none' type,
the new symbols of libuwm.so and their argument checks, which fail before any launch.  Every comparison is exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maskpost_ragged_ref as RR  # noqa: E402
import maskpost_ref as R  # noqa: E402

NEW_SYMBOLS = ("uwm_mask_ragged_workspace_bytes", "uwm_optimize_masks_ragged")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from unet_watermark_amd import _lib
    _lib.lib()
    return _lib


def test_kept_statistics_equal_a_relabelling_of_the_golden_outputs():
    """the optimised mask is a union of whole components of the pre-selection plane, so the kept components (from _chain,
    components and the keep rules) are exactly the components of the output: count and largest area against scipy's labelling
    with the 3 x 3 (8-connected) structure, for every image and type of the golden file"""
    ndimage = pytest.importorskip("scipy").ndimage
    checked = 0
    for name, batch, want in R.load_golden():
        for t in R.MASK_TYPES:
            outs, sums = want[t]
            for img, out, summary in zip(batch, outs, sums):
                got_out, row = RR.optimize(img, t)
                assert np.array_equal(got_out, out), (name, t)
                assert row[:4] == [int(v) for v in summary], (name, t)
                lab, n = ndimage.label(out > 127, structure=np.ones((3, 3), int))
                sizes = np.bincount(lab.reshape(-1))[1:]
                assert row[4] == n and row[5] == (int(sizes.max()) if n else 0), (name, t, row, n)
                assert row[2] == int(sizes.sum()) and row[6] == img.size and row[7] == 0
                checked += 1
    assert checked == 90


def test_none_type_on_hand_computed_planes():
    planes = RR.stress_planes()
    assert {k: v[1:] for k, v in planes.items()} == {"checkerboard": (1, 4225), "comb": (1, 4290), "serpentine": (1, 4322),
                                                     "isolated": (2145, 1)}
    for name, (plane, ncomp, largest) in planes.items():
        assert plane.shape == (65, 130)
        out, row = RR.optimize(plane.astype(np.uint8) * 255, "none")
        assert np.array_equal(out > 127, plane), name
        assert row == [ncomp, largest, int(plane.sum()), 0, ncomp, largest, 65 * 130, 0], (name, row)
    assert int(planes["isolated"][0].sum()) == 2145 and int(planes["checkerboard"][0].sum()) == 4225


def test_keep_rules_and_the_misfit_rule_of_the_restatement():
    assert RR.kept_areas([499, 201, 200, 3], "watermark").tolist() == [499, 201]
    assert RR.kept_areas([500, 499, 300], "watermark").tolist() == [500]
    assert RR.kept_areas([500, 500], "watermark").tolist() == [500]                   # the first of equals, alone
    assert RR.kept_areas([51, 50], "text").tolist() == [51] and RR.kept_areas([101, 100], "mixed").tolist() == [101]
    assert RR.kept_areas([1, 2], "none").tolist() == [1, 2] and RR.kept_areas([], "text").tolist() == []
    d = np.zeros(5, [("offset", "<i8"), ("h", "<i4"), ("w", "<i4")])
    d[0] = (0, 4, 4); d[1] = (16, 0, 3); d[2] = (16, 5, 4); d[3] = (90, 3, 4); d[4] = (36, 2, 2)
    assert RR.misfits(d, 100, 16, 100) == [False, True, True, True, False]            # a zero side, too many pixels, leaves the buffer
    assert RR.misfits(d, 100, 20, 9) == [False, True, False, True, True]              # rows: 4 + 5 fit, 2 more do not
    assert RR.misfits(d[:1], 16, 16, 1) == [True] and RR.misfits(d[:1], 16, 16, 4) == [False]


def test_the_new_symbols_are_exported_and_declared(L):
    lib = L.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "uwm.h")).read()
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES and getattr(lib, name) is not None
        assert name + "(" in header
    assert "UWM_MASK_NONE = 3" in header
    one = lib.uwm_mask_ragged_workspace_bytes(1, 64, 1)
    assert one > 0 and one % 256 == 0
    # three planes of mask_bytes / 64 + rows words, labels and areas of mask_bytes ints
    big = lib.uwm_mask_ragged_workspace_bytes(4, 1 << 20, 4096)
    assert big >= 3 * 8 * ((1 << 20) // 64 + 4096) + 2 * 4 * (1 << 20)
    assert lib.uwm_mask_ragged_workspace_bytes(4, 1 << 20, 8192) > big
    for bad in ((0, 64, 1), (-1, 64, 1), (65536, 64, 1), (1, 0, 1), (1, 64, 0), (1, 64, -5), (1, 1 << 41, 1), (1, 64, 1 << 41)):
        assert lib.uwm_mask_ragged_workspace_bytes(*bad) == 0, bad
        assert "uwm_mask_ragged_workspace_bytes" in lib.uwm_last_error().decode()


def _host_block():
    buf = (C.c_uint8 * 8192)()
    p = C.c_void_p(C.addressof(buf) + (-C.addressof(buf)) % 16)
    return buf, p, C.c_void_p(p.value + 4)


def test_uwm_optimize_masks_ragged_checks_arguments_before_any_launch(L):
    """a null pointer, N / mask_bytes / max_pixels / rows below 1 or too large, an unknown type, a misaligned pointer, a workspace
    that is too small: every such call returns non-zero with a message and none reaches a launch (the pointers are host memory)"""
    lib = L.lib()
    keep, p, odd4 = _host_block()
    need = lib.uwm_mask_ragged_workspace_bytes(1, 64, 8)
    base = dict(inp=p, out=p, mask_bytes=64, descs=p, N=1, mask_type=0, max_pixels=64, rows=8, stats=p, ws=p, ws_bytes=need, st=None)

    def bad(word, **kw):
        rc = lib.uwm_optimize_masks_ragged(*[kw.get(k, v) for k, v in base.items()])
        assert rc != 0, kw
        msg = lib.uwm_last_error().decode()
        assert "uwm_optimize_masks_ragged" in msg and word in msg, msg

    for k in ("inp", "out", "descs", "ws"):
        bad("null", **{k: None})
    for k in ("N", "mask_bytes", "max_pixels", "rows"):
        bad(">= 1", **{k: 0})
    bad(">= 1", N=-3); bad(">= 1", rows=-1); bad(">= 1", max_pixels=-7)
    bad("too large", N=65536)
    bad("too large", max_pixels=2 ** 31 - 1)
    bad("too large", rows=1 << 41)
    bad("too large", mask_bytes=1 << 41)
    for t in (-1, 4, 99):
        bad("unknown mask type", mask_type=t)
    for k in ("descs", "stats", "ws"):
        bad("aligned", **{k: odd4})
    bad("too small", ws_bytes=need - 1)
    bad("too small", N=3)
    bad("too small", rows=4096)
