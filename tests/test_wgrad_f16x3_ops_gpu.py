"""Op-level tests of wgrad_f16x3.hip (uwm_op_wgrad force_igemm 6: the direct 3x3 / stride-1 weight gradient of the fp16x3 precision
modes) against tests/f16x3_ref.py: the emulation of the very split products the launch asks for (uwm_op_set_f16x3_products) and the
fp64 truth.  Every launch has Kpad = 9 * Ctot.

Bars (tests/test_f16x3_ref.py shows what they can tell apart on these operands):
  * dW against emu(nprod): 3e-5 of the true gradient's range — test_wgrad_f16x3_direct's bar, relative to the range with no
    max(1, .) (dY is ~ 1e-6 here; the left half of the image a further 1e-3 smaller);
  * nprod 3: error against the fp64 truth, relative to dW's range, within 4x the exact-fp32 kernel's own error + 1e-7
    (force_igemm 1 on the same operands, staged by the reference into one plain source) — test_conv_f16x3_error_vs_fp64_and_range's
    rule.  Not at X ~ 1e-3: below fp16's normal range the low half of X has an absolute step, as the forward range test documents;
  * dW is accumulated into: += on the one-split path is bit-exact, partial images + reduce to 4 * 2^-24 * (|prefill| + |gradient|);
  * two launches are bit-identical; a rejected call, and an all-zero dY, leave a prefilled dW bit-unchanged.
Shapes: f16x3_ref.WGRAD_SHAPES, one per branch of the stage walk, the tile walk and the grid, the smallest that reaches it;
which branch a case reaches (f16x3_ref.WGRAD_CLAIMS) holds on any card of 64 CUs or more as long as UWM_WG16_CUS — read once per
process by the launcher — is unset.  With UWM_WGRAD_F16X3_REPORT=<file> the largest figure of every case is written there
(profiles/wgrad_f16x3_op_tests_mi355x.txt is such a run).
"""
import contextlib
import ctypes as C
import functools
import os

import pytest
import torch

from tests import f16x3_ref as R
from tests.util import nhwc, unpack_w, src, P, stream

pytestmark = pytest.mark.gpu

_REPORT = {}


def lib():
    from unet_watermark_amd import _lib as L
    return L


@pytest.fixture(scope="module", autouse=True)
def _report_file():
    yield
    path = os.environ.get("UWM_WGRAD_F16X3_REPORT")
    if path and _REPORT:
        with open(path, "w") as f:
            f.write("# tests/test_wgrad_f16x3_ops_gpu.py: largest observed figure per case (err = max |gpu - emu(nprod)| in bars of 3e-5 * range of the\n"
                    "# true gradient; fp64 / direct = error against the fp64 truth relative to dW's range, and the exact-fp32 kernel's (force_igemm 1);\n"
                    "# vs3 = distance of an nprod 1 / 2 result from the nprod 3 result, in bars; acc = error of dW += in units of its bound)\n")
            for k in sorted(_REPORT):
                f.write(f"{k:58s} " + "  ".join(f"{n} {v:.3e}" for n, v in _REPORT[k].items()) + "\n")


def _note(name, **figs):
    e = _REPORT.setdefault(name, {})
    for k, v in figs.items():
        e[k] = max(e.get(k, 0.0), float(v))
    print(name, "  ".join(f"{k} {float(v):.3e}" for k, v in figs.items()))


@contextlib.contextmanager
def _products(n):
    """uwm_op_set_f16x3_products(n) for the body, 3 again afterwards"""
    L = lib()
    L.check(L.lib().uwm_op_set_f16x3_products(n))
    try:
        yield
    finally:
        L.lib().uwm_op_set_f16x3_products(3)


def _launch(dev, sources, dy, coutp, wrows, dw=None, force=6, kpad=None, stride=1):
    """uwm_op_wgrad of NCHW sources and dy [N][wrows][Ho][Wo] -> (rc, dw [wrows][Kpad], zeros unless given)"""
    L = lib()
    keep, ss = [], []
    for s in sources:
        xd = nhwc(s["x"]).to(dev)
        sc = s["scale"].to(dev) if s["scale"] is not None else None
        sh = s["shift"].to(dev) if s["shift"] is not None else None
        keep += [xd, sc, sh]
        ss.append(src(xd, sc, sh, relu=s["relu"], up=s["up"]))
    n, _, ho, wo = dy.shape
    dyd = nhwc(dy, coutp).to(dev)
    ctot = sum(s["x"].shape[1] for s in sources)
    kpad = kpad or 9 * ctot
    if dw is None:
        dw = torch.zeros(wrows, kpad, device=dev)
    rc = L.lib().uwm_op_wgrad(C.byref(ss[0]), C.byref(ss[1]) if len(ss) > 1 else None, P(dyd), n, ho, wo, coutp, wrows, kpad, 3, 3,
                              stride, 1, P(dw), force, stream())
    torch.cuda.synchronize()
    return rc, dw


def _run(dev, c, dw=None):
    rc, dw = _launch(dev, c["sources"], c["dy"], c["coutp"], c["wrows"], dw)
    lib().check(rc)
    return dw


def _plain(x):
    return {"x": x, "scale": None, "shift": None, "relu": 0, "up": 0}


def _unpack(dw, c):
    return unpack_w(dw.cpu(), c["wrows"], c["cin"], 3, 3).double()


@functools.lru_cache(maxsize=None)
def _direct_err(dev, shape, form, mag, xmag):
    """the exact-fp32 kernel's own error (force_igemm 1) on the staged operands of a case, relative to dW's range"""
    c = R.wgrad_case(shape, form, mag, xmag)
    x = R.staged(c["sources"]).float()
    rc, dw = _launch(dev, [_plain(x)], c["dy"], c["coutp"], c["wrows"], force=1)
    lib().check(rc)
    ref = R.wgrad64(x.double(), c["dy"].double())
    return float((_unpack(dw, c) - ref).abs().max()) / R.out_range(ref)


def _check(dev, shape, form, nprod=3, mag=R.DY_SMALL, xmag=1.0, rule4=True):
    """one launch against emu(nprod) (and, nprod 3, the fp64 truth beside the exact-fp32 kernel) -> dw"""
    c = R.wgrad_case(shape, form, mag, xmag)
    dw = _run(dev, c)
    name = f"wgrad {shape}/{form} dy {mag:g} x {xmag:g} nprod {nprod}"
    assert torch.isfinite(dw).all(), name
    got, truth = _unpack(dw, c), R.wgrad_ref(shape, form, 0, mag, xmag)
    rng = R.out_range(truth)
    bar = R.WGRAD_BAR * rng
    err = float((got - R.wgrad_ref(shape, form, nprod, mag, xmag)).abs().max())
    figs = {"err": err / bar}
    if nprod == 3:
        figs["fp64"] = float((got - truth).abs().max()) / rng
        if rule4:
            figs["direct"] = _direct_err(dev, shape, form, mag, xmag)
    _note(name, **figs)
    assert err < bar, (name, err, bar)
    if nprod == 3 and rule4:
        assert figs["fp64"] < 4 * figs["direct"] + 1e-7, (name, figs)
    return dw


@pytest.mark.parametrize("shape,form", R.wgrad_cases())
def test_wgrad(cuda, shape, form):
    """every branch of the stage walk (1, 2, 3, 7 stages; an uneven last split), the tile walk (half-empty and over-hanging row
    tiles, wrows < Cout, halos from neighbouring tiles), the grid (1 .. 12 workgroups), both stage geometries and every input
    form, three products; twice the same launch is bit-identical"""
    dw = _check(cuda, shape, form)
    assert torch.equal(_run(cuda, R.wgrad_case(shape, form)), dw)


@pytest.mark.parametrize("nprod", [1, 2, 3])
@pytest.mark.parametrize("shape", ["one_stage", "uneven", "wx16_split"])
def test_wgrad_product_counts(cuda, shape, nprod):
    """the launched count is the arithmetic of that count (more than 3 bars from any other: test_f16x3_ref.py), and 1 and 2 products
    are more than a bar away from what 3 give on the card"""
    with _products(nprod):
        dw = _check(cuda, shape, "lazy", nprod)
    if nprod < 3:
        c = R.wgrad_case(shape, "lazy")
        d = float((_unpack(dw, c) - _unpack(_run(cuda, c), c)).abs().max())
        bar = R.WGRAD_BAR * R.out_range(R.wgrad_ref(shape, "lazy", 0))
        _note(f"wgrad {shape}/lazy dy {R.DY_SMALL:g} x 1 nprod {nprod}", vs3=d / bar)
        assert d > bar, (shape, nprod, d, bar)


@pytest.mark.parametrize("shape", ["one_stage", "uneven"])
def test_wgrad_accumulates(cuda, shape):
    """dW += gradient: `one_stage` adds straight into dW (bit-equal to prefill + gradient in fp32), `uneven` through partial images
    and the reduce (its own add order: within 4 * 2^-24 * (|prefill| + |gradient|) elementwise)"""
    c = R.wgrad_case(shape, "lazy")
    g0 = _run(cuda, c).cpu()
    pre = torch.randn(g0.shape, generator=torch.Generator().manual_seed(5)) * R.out_range(R.wgrad_ref(shape, "lazy", 0))
    got = _run(cuda, c, pre.clone().to(cuda)).cpu()
    want = pre + g0
    nsplit = R.WGRAD_CLAIMS[shape][2]
    bound = 4 * 2.0 ** -24 * (pre.abs() + g0.abs()).double()
    diff = (got.double() - want.double()).abs()
    _note(f"wgrad {shape}/lazy accumulate ({nsplit} split{'s' if nsplit > 1 else ''})", acc=float((diff / bound.clamp_min(1e-300)).max()))
    assert bool((got != pre).any())
    if nsplit == 1:
        assert torch.equal(got, want), float(diff.max())
    else:
        assert bool((diff <= bound).all()), float((diff / bound.clamp_min(1e-300)).max())


def test_wgrad_ranges(cuda):
    """dY ~ 1e3 (the bar scales with the gradient's range), X ~ 300, X ~ 1e-3 (against the emulation alone), and dY all zero: xs stays
    1 and a prefilled dW comes back bit-unchanged"""
    for shape, form, mag, xmag in R.WGRAD_RANGES:
        _check(cuda, shape, form, 3, mag, xmag, rule4=xmag >= 0.01)
    c = R.wgrad_case("halo", "lazy", 0.0)
    pre = torch.randn(c["wrows"], 9 * c["cin"], generator=torch.Generator().manual_seed(6))
    assert torch.equal(_run(cuda, c, pre.clone().to(cuda)).cpu(), pre)


def test_wgrad_rejections(cuda):
    """force_igemm 6 on a shape wgrad_f16x3.hip does not take (32 outputs, nothing up-sampled: no other fp16x3 kernel takes it
    either) is an error, and dW keeps the pattern it held"""
    L = lib()
    g = torch.Generator().manual_seed(3)

    def refused(what, chans, h, w, stride=1, kpad_extra=0):
        sources = [_plain(torch.randn(1, ch, h, w, generator=g)) for ch in chans]
        ctot = sum(chans)
        dy = torch.randn(1, 32, h // stride, w // stride, generator=g)
        pre = torch.arange(32 * (9 * ctot + kpad_extra), dtype=torch.float32).reshape(32, -1) * 0.5 - 7.0
        rc, dw = _launch(cuda, sources, dy, 32, 32, pre.clone().to(cuda), kpad=9 * ctot + kpad_extra, stride=stride)
        assert rc != 0, what
        assert L.lib().uwm_last_error()
        assert torch.equal(dw.cpu(), pre), what

    refused("W = 24", [32], 8, 24)
    refused("H = 6 at W = 32", [32], 6, 32)
    refused("Ctot = 48", [48], 8, 32)
    refused("C0 = 16 of 64", [16, 48], 8, 32)
    refused("stride 2", [32], 8, 64, stride=2)
    refused("Kpad = 9 * Ctot + 32", [32], 8, 32, kpad_extra=32)
