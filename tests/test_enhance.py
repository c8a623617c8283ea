"""Mask enhancement, the part that needs no device: the two exact reductions the device chain rests on (tests/enhance_ref.py:
enhance_literal == enhance_reduced on every case of the GPU test; the bilateral step is the identity on {0,255} images), the
ellipse spans, the Gaussian taps of the library, the new symbols and their argument checks, which fail before any launch, the
command line's parser, and a condition on the cases themselves: every stage of the chain matters on at least one of them.

A case is one parameter set of enhance_ref.PARAMS on its batch (enhance_ref.batch_for).  The tiny images (1 x 1 .. 3 x 5) cannot
avoid being filled by an element larger than themselves, so "no output all 0 or all 255 unless the input is" is asked of every
image whose sides are at least 33 at every parameter set it runs at, and of each case's batch as a whole."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import enhance_ref as E  # noqa: E402

NEW_SYMBOLS = ("uwm_enhance_masks_workspace_bytes", "uwm_enhance_masks_ragged", "uwm_enhance_gauss_taps")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from unet_watermark_amd import _lib
    _lib.lib()
    return _lib


def lib_taps(lib, blur_kernel):
    """-> (effective k, float32 taps) from uwm_enhance_gauss_taps"""
    buf = (C.c_float * 63)()
    k = lib.uwm_enhance_gauss_taps(blur_kernel, buf)
    return k, np.array(buf[:k], np.float32)


def ref_taps(lib, blur_kernel):
    """what the restatement is fed: None for no blur, else the library's very taps"""
    return None if blur_kernel == 0 else lib_taps(lib, blur_kernel)[1]


@pytest.fixture(scope="module")
def reduced(L):
    """{(params, image index): enhance_reduced}, computed once"""
    lib = L.lib()
    return {(p, i): E.enhance_reduced(im, ref_taps(lib, p[1]), p[0], p[2]) for p in E.PARAMS for i, im in enumerate(E.batch_for(p))}


def test_the_literal_chain_equals_the_reduced_chain_on_every_case(L, reduced):
    lib = L.lib()
    for p in E.PARAMS:
        taps = ref_taps(lib, p[1])
        for i, im in enumerate(E.batch_for(p)):
            assert np.array_equal(E.enhance_literal(im, taps, p[0], p[2]), reduced[(p, i)]), (p, im.shape)


@pytest.mark.parametrize("shape", ((1, 1), (3, 5), (40, 40)))
def test_bilateral_then_threshold_is_the_identity_on_binary_images(shape):
    g = np.random.default_rng(shape[0] * 100 + shape[1])
    for density in (0.5, 0.05, 0.95):
        u = ((g.random(shape) < density) * 255).astype(np.uint8)
        assert np.array_equal(np.where(E.bilateral_9_75_75(u) > 127, 255, 0), u), (shape, density)
    # the two extremes the issue names: a lone 255 among zeros, a lone 0 among 255s
    u = np.zeros((21, 21), np.uint8); u[10, 10] = 255
    b = E.bilateral_9_75_75(u)
    assert b[10, 10] == 222 and b[10, 11] < 10
    b = E.bilateral_9_75_75(255 - u)
    assert b[10, 10] == 33 and b[10, 11] > 245


def test_ellipse_spans(L):
    lib = L.lib()
    for size in range(1, 16, 2):
        out = np.zeros((size, size), np.uint8)
        assert lib.uwm_mask_element(2, size, size, C.c_void_p(out.ctypes.data)) == 0
        assert np.array_equal(out, E.ellipse(size)), size
    assert E.ellipse_dx(1) == [0] and E.ellipse_dx(5) == [0, 2, 2, 2, 0] and E.ellipse_dx(7) == [0, 2, 3, 3, 3, 2, 0]
    for size in (21, 31, 63):
        dx = E.ellipse_dx(size)
        assert dx == dx[::-1] and dx[size // 2] == size // 2 and dx[0] == 0, size
        assert all(a <= b for a, b in zip(dx[:size // 2], dx[1:size // 2 + 1])), size
        k = E.ellipse(size)
        assert np.array_equal(k, k[::-1]) and np.array_equal(k, k[:, ::-1]) and k[size // 2].all()


def test_gauss_taps(L):
    lib = L.lib()
    tables = {1: [1.0], 3: [.25, .5, .25], 5: [.0625, .25, .375, .25, .0625], 7: [.03125, .109375, .21875, .28125, .21875, .109375, .03125]}
    for k, want in tables.items():
        got_k, taps = lib_taps(lib, k)
        assert got_k == k and taps.tolist() == want, k
    for even in range(0, 63, 2):
        k, taps = lib_taps(lib, even)
        k1, taps1 = lib_taps(lib, even + 1)
        assert k == even + 1 == k1 and np.array_equal(taps, taps1), even
    for k in range(9, 64, 2):
        got_k, taps = lib_taps(lib, k)
        want = E.gauss_taps_formula(k)
        assert got_k == k and len(taps) == k
        assert (np.abs(taps.astype(np.float64) - want) <= np.spacing(want.astype(np.float32))).all(), k
        assert abs(float(taps.astype(np.float64).sum()) - 1.0) < 1e-6, k
        assert np.array_equal(taps, taps[::-1])
    assert abs(float(lib_taps(lib, 15)[1][7]) - 0.1540096) < 1e-7
    for k, sigma in ((15, 2.6), (21, 3.5), (31, 5.0)):
        assert abs(((k - 1) * 0.5 - 1) * 0.3 + 0.8 - sigma) < 1e-12
    buf = (C.c_float * 63)()
    for bad in (-1, 64, 1000):
        assert lib.uwm_enhance_gauss_taps(bad, buf) == 0
        msg = lib.uwm_last_error().decode()
        assert "uwm_enhance_gauss_taps" in msg and "blur_kernel" in msg
    assert lib.uwm_enhance_gauss_taps(15, None) == 0 and "null" in lib.uwm_last_error().decode()


def test_the_new_symbols_are_exported_and_declared(L):
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "uwm.h")).read()
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES and getattr(lib, name) is not None
        assert name + "(" in header
    assert "mask_enhance.hip" in L.SOURCES
    one = lib.uwm_enhance_masks_workspace_bytes(1, 64)
    assert one > 0 and one % 256 == 0
    big = lib.uwm_enhance_masks_workspace_bytes(4, 1 << 20)
    assert 2 << 20 <= big < (2 << 20) + 4096                # two byte planes and the records: no float plane
    for bad in ((0, 64), (-1, 64), (65536, 64), (1, 0), (1, 1 << 41)):
        assert lib.uwm_enhance_masks_workspace_bytes(*bad) == 0, bad
        assert "uwm_enhance_masks_workspace_bytes" in lib.uwm_last_error().decode()


def _host_block():
    buf = (C.c_uint8 * 8192)()
    p = C.c_void_p(C.addressof(buf) + (-C.addressof(buf)) % 16)
    return buf, p, C.c_void_p(p.value + 4)


def test_uwm_enhance_masks_ragged_checks_arguments_before_any_launch(L):
    """every such call returns non-zero with a message that names the function and the argument, and none reaches a launch (the
    pointers are host memory)"""
    lib = L.lib()
    keep, p, odd4 = _host_block()
    need = lib.uwm_enhance_masks_workspace_bytes(1, 64)
    assert 0 < need <= 4096
    base = dict(inp=p, out=p, mask_bytes=64, descs=p, N=1, expand_pixels=10, blur_kernel=15, smooth_iterations=2, max_pixels=64, stats=p,
                ws=p, ws_bytes=need, st=None)

    def bad(word, **kw):
        rc = lib.uwm_enhance_masks_ragged(*[kw.get(k, v) for k, v in base.items()])
        assert rc != 0, kw
        msg = lib.uwm_last_error().decode()
        assert "uwm_enhance_masks_ragged" in msg and word in msg, msg

    for k in ("inp", "out", "descs", "ws"):
        bad("null", **{k: None})
    for k in ("N", "mask_bytes", "max_pixels"):
        bad(">= 1", **{k: 0})
    bad(">= 1", N=-3); bad(">= 1", max_pixels=-7)
    bad("too large", N=65536)
    bad("too large", max_pixels=2 ** 31 - 1)
    bad("too large", mask_bytes=1 << 41)
    bad("expand_pixels", expand_pixels=32); bad("expand_pixels", expand_pixels=-1)
    bad("blur_kernel", blur_kernel=64); bad("blur_kernel", blur_kernel=-1)
    bad("smooth_iterations", smooth_iterations=9); bad("smooth_iterations", smooth_iterations=-1)
    for k in ("descs", "stats", "ws"):
        bad("aligned", **{k: odd4})
    bad("too small", ws_bytes=need - 1)
    bad("too small", mask_bytes=4096)


def test_the_python_entry_points_refuse_a_host_tensor(L):
    import torch
    from unet_watermark_amd import postprocess as P
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.enhance_mask(torch.zeros((4, 4), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.enhance_masks_ragged(torch.zeros(16, dtype=torch.uint8), np.zeros(1, [("offset", "<i8"), ("h", "<i4"), ("w", "<i4")]))
    for kw in (dict(expand_pixels=32), dict(blur_kernel=64), dict(smooth_iterations=9), dict(expand_pixels=-1)):
        with pytest.raises(ValueError):
            P.enhance_mask(torch.zeros((4, 4), dtype=torch.uint8), **kw)


def test_cli_parser():
    from unet_watermark_amd.cli import build_parser
    ps = build_parser()
    a = ps.parse_args(["enhance-masks", "--mask-dir", "m", "--output-dir", "o"])
    assert (a.mask_dir, a.output_dir, a.in_place, a.expand_pixels, a.blur_kernel, a.smooth_iterations, a.batch_size) == ("m", "o", False, 10, 15, 2, 16)
    a = ps.parse_args(["enhance-masks", "--mask-dir", "m", "--in-place", "--expand-pixels", "15", "--blur-kernel", "21",
                       "--smooth-iterations", "1", "--batch-size", "4"])
    assert (a.output_dir, a.in_place, a.expand_pixels, a.blur_kernel, a.smooth_iterations, a.batch_size) == (None, True, 15, 21, 1, 4)
    for argv in (["enhance-masks", "--mask-dir", "m"], ["enhance-masks", "--mask-dir", "m", "--output-dir", "o", "--in-place"],
                 ["enhance-masks", "--output-dir", "o"]):
        with pytest.raises(SystemExit):
            ps.parse_args(argv)
    sub =[act for act in ps._actions if hasattr(act, "choices") and act.choices and "enhance-masks" in act.choices][0]
    text = " ".join(sub.choices["enhance-masks"].format_help().split())
    assert "Pillow" in text and "--in-place" in text


def test_every_stage_matters_on_the_cases(L, reduced):
    lib = L.lib()
    assert E.PARAMS[:2] == ((10, 15, 2), (15, 21, 2)) and len(E.PARAMS) == 8
    shapes = {im.shape for im in E.images()}
    assert {(1, 1), (1, 9), (7, 1), (3, 5), (33, 65), (64, 64), (96, 200), (E.TILE + 1, E.TILE + 1)} <= shapes
    assert {im.shape for im in E.batch_for(E.PARAMS[-1])} == {(1, 1), (1, 9), (7, 1), (3, 5)}
    differs = dict.fromkeys(E.STAGES, False)
    for p in E.PARAMS:
        taps = ref_taps(lib, p[1])
        whole = []
        for i, im in enumerate(E.batch_for(p)):
            want = reduced[(p, i)]
            assert set(np.unique(want)) <= {0, 255}
            whole.append(want.reshape(-1))
            uniform_in = im.min() == im.max() and im[0, 0] in (0, 255)
            if min(im.shape) >= 33 and not uniform_in:
                assert 0 < int((want > 127).sum()) < want.size, (p, im.shape)
            if uniform_in:
                assert (want == im).all(), (p, im.shape)
            for stage in E.STAGES:
                if not differs[stage] and not np.array_equal(E.enhance_reduced(im, taps, p[0], p[2], skip=stage), want):
                    differs[stage] = True
        whole = np.concatenate(whole)
        assert 0 < int((whole > 127).sum()) < whole.size, p
    assert all(differs.values()), differs
