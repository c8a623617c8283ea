"""Op-level tests of conv_f16x3v2.hip (codes 607 = the routed 8-wave kernel, 605 = the 4-wave kernel) in both of its roles, and of the
dgrad role of conv_f16x3.hip (602), against tests/f16x3_ref.py: the emulation of the very split products the launch asks for
(uwm_op_set_f16x3_products) and the fp64 truth.

Bars (tests/test_f16x3_ref.py shows what they can tell apart on these operands):
  * output against emu(nprod): 2e-5 * max(1, output range) — _conv_case's fp32-accumulation bar; a dgrad's in units of its dY
    magnitude (dx / 1e-6 resp. dx / 1e3: against the literal max(1, range) a 1e-6 gradient would be held to nothing);
  * nprod 3: error against the fp64 truth, relative to each output channel's range, within 4x the exact-fp32 direct kernel's own
    error on the same operands (cfg 164) + 1e-7 — test_conv_f16x3_error_vs_fp64_and_range's rule.  The direct kernel takes the
    staged input (transform, up-sampling and concat done by the reference); a dgrad's direct error is its layer's plain convolution's;
  * BatchNorm statistics / fused BatchNorm-backward sums: _conv_case's bars, in the same units;
  * outputs are NaN-prefilled: finite everywhere afterwards, exactly zero where a dgrad's mask says so; a rejected call leaves
    every NaN in place.
Shapes: whole 8 x 32 tiles, one per branch of the kernel's chunk walk and tile walk (f16x3_ref.FWD_SHAPES).  With
UWM_F16X3V2_REPORT=<file> the largest error of every case is written there (profiles/f16x3v2_op_tests_mi355x.txt is such a run).
"""
import contextlib
import ctypes as C
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from tests import f16x3_ref as R
from tests.util import nhwc, nchw, pack_w, src, P, stream

pytestmark = pytest.mark.gpu

V2_CODES = (607, 605)
_REPORT = {}


def lib():
    from unet_watermark_amd import _lib as L
    return L


@pytest.fixture(scope="module", autouse=True)
def _report_file():
    yield
    path = os.environ.get("UWM_F16X3V2_REPORT")
    if path and _REPORT:
        with open(path, "w") as f:
            f.write("# tests/test_f16x3v2_ops_gpu.py: largest observed figure per case (err = max |gpu - emu(nprod)| in bars of 2e-5 * max(1, range);\n"
                    "# fp64 / direct = error against the fp64 truth relative to the channel range, and the exact-fp32 direct kernel's (cfg 164);\n"
                    "# sum / sumsq = statistics error in units of their bar)\n")
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


def _chan_rel(got, truth):
    """largest error relative to each channel's range (test_conv_f16x3_error_vs_fp64_and_range's measure)"""
    return float(((got - truth).abs() / truth.abs().amax((0, 2, 3), keepdim=True)).max())


def _stats_check(name, stats, ref, c, unit=1.0):
    """_conv_case's statistics bars on (sum, sum of squares) of ref, in units of `unit`"""
    ssum, ssq = stats[:c].cpu() / unit, stats[c:2 * c].cpu() / unit ** 2
    rs, rq = (ref / unit).sum((0, 2, 3)), ((ref / unit) ** 2).sum((0, 2, 3))
    b1 = 1e-5 * rs.abs() + 1e-5 * max(1.0, float(rs.abs().max()))
    b2 = 1e-5 * rq.abs() + 1e-5 * float(rq.abs().max())
    e1, e2 = float(((ssum - rs).abs() / b1).max()), float(((ssq - rq).abs() / b2).max())
    _note(name, sum=e1, sumsq=e2)
    assert e1 <= 1.0 and e2 <= 1.0, (name, e1, e2)


def _conv_launch(dev, sources, wt, bias, n, cout, cfg, y=None):
    """uwm_op_conv of NCHW sources -> (rc, y NHWC NaN-prefilled, stats)"""
    L = lib()
    keep, ss = [], []
    for s in sources:
        xd = nhwc(s["x"]).to(dev)
        sc = s["scale"].to(dev) if s["scale"] is not None else None
        sh = s["shift"].to(dev) if s["shift"] is not None else None
        keep += [xd, sc, sh]
        ss.append(src(xd, sc, sh, relu=s["relu"], up=s["up"]))
    h, w = sources[0]["x"].shape[2] << sources[0]["up"], sources[0]["x"].shape[3] << sources[0]["up"]
    wp, kpad = pack_w(wt)
    wp = wp.to(dev)
    bd = bias.to(dev) if bias is not None else None
    if y is None:
        y = torch.full((n, h, w, cout), float("nan"), device=dev)
    stats = torch.zeros(2 * cout, dtype=torch.float64, device=dev)
    rc = L.lib().uwm_op_conv(C.byref(ss[0]), C.byref(ss[1]) if len(ss) > 1 else None, P(wp), cout, kpad, 3, 3, 1, 1, n, cout,
                             P(bd), P(y), P(stats), cfg, stream())
    torch.cuda.synchronize()
    return rc, y, stats


def _plain(x):
    return {"x": x, "scale": None, "shift": None, "relu": 0, "up": 0}


@functools.lru_cache(maxsize=None)
def _direct_fwd_err(dev, shape, form):
    """the exact-fp32 direct kernel's own error (cfg 164) on the staged operands of a forward case"""
    c = R.fwd_case(shape, form)
    x = R.staged(c["sources"]).float()
    rc, y, _ = _conv_launch(dev, [_plain(x)], c["w"], c["bias"], c["n"], c["cout"], 164)
    lib().check(rc)
    ref = F.conv2d(x.double(), c["w"].double(), c["bias"].double() if c["bias"] is not None else None, 1, 1)
    return _chan_rel(nchw(y.cpu()).double(), ref)


@functools.lru_cache(maxsize=None)
def _direct_dgrad_err(dev, shape, mag):
    """... on a dgrad layer's plain convolution (dY with the mirrored filters)"""
    c = R.dgrad_case(shape, "plain", mag)
    wd = R.dgrad_filters(c["w"])
    rc, y, _ = _conv_launch(dev, [_plain(c["dy"])], wd, None, c["n"], c["cin"], 164)
    lib().check(rc)
    return _chan_rel(nchw(y.cpu()).double(), F.conv2d(c["dy"].double(), wd.double(), None, 1, 1))


def _fwd_check(dev, shape, form, cfg, nprod=3):
    c = R.fwd_case(shape, form)
    rc, y, stats = _conv_launch(dev, c["sources"], c["w"], c["bias"], c["n"], c["cout"], cfg)
    lib().check(rc)
    name = f"fwd {shape}/{form} cfg {cfg} nprod {nprod}"
    assert torch.isfinite(y).all(), name
    got = nchw(y.cpu()).double()
    emu = R.fwd_ref(shape, form, nprod)
    bar = R.BAR * max(1.0, R.out_range(emu))
    err = float((got - emu).abs().max())
    figs = {"err": err / bar}
    if nprod == 3:
        figs["fp64"], figs["direct"] = _chan_rel(got, R.fwd_ref(shape, form, 0)), _direct_fwd_err(dev, shape, form)
    _note(name, **figs)
    assert err < bar, (name, err, bar)
    if nprod == 3:
        assert figs["fp64"] < 4 * figs["direct"] + 1e-7, (name, figs)
    _stats_check(name, stats, emu, c["cout"])
    return y


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("shape,form", R.fwd_cases())
def test_forward(cuda, shape, form):
    """every branch of the chunk walk and the tile walk, every input form, on both kernels of conv_f16x3v2.hip; where the layer has
    output rows % 64 == 32, code 600 must take the routed kernel: bit-equal to 607 (conv_f16x3.hip adds in another order)"""
    ys = {cfg: _fwd_check(cuda, shape, form, cfg) for cfg in V2_CODES}
    if shape in ("96to96", "128to160"):
        y600 = _fwd_check(cuda, shape, form, 600)
        assert torch.equal(y600, ys[607]), "code 600 did not take conv_f16x3v2.hip's kernel"
        c = R.fwd_case(shape, form)
        rc, y602, _ = _conv_launch(cuda, c["sources"], c["w"], c["bias"], c["n"], c["cout"], 602)
        lib().check(rc)
        assert not torch.equal(y602, ys[607])         # (or bit-equality would tell nothing)


@pytest.mark.parametrize("nprod", [1, 2])
@pytest.mark.parametrize("shape", ["64to32", "96to96"])
def test_forward_product_counts(cuda, shape, nprod):
    """nprod 1 and 2 against the emulation of exactly those products (more than 3 bars away from any other count)"""
    with _products(nprod):
        for form in (R.FWD_FORMS_96 if shape == "96to96" else R.FWD_FORMS):
            for cfg in V2_CODES:
                _fwd_check(cuda, shape, form, cfg, nprod)


# ------------------------------------------------------------------------------------------------------------------ dgrad
def _dgrad_launch(dev, c, cfg, bn=None, nrep=1, dx=None):
    """uwm_op_dgrad_f16x3 of a dgrad case -> (rc, dx NHWC NaN-prefilled, sums [nrep][stride] or None).  bn: None | 'mask' | 'y'"""
    L = lib()
    n, h, w, cin, cout = c["n"], c["h"], c["w_"], c["cin"], c["cout"]
    dev_of = lambda t: nhwc(t).to(dev) if t is not None else None
    vec = lambda t: t.to(dev) if t is not None else None
    dy, add, mask, yb = dev_of(c["dy"]), dev_of(c["addend"]), dev_of(c["mask"]), dev_of(c["y"]) if bn == "y" else None
    msc, msh, mean, rstd = vec(c["mscale"]), vec(c["mshift"]), vec(c["mean"]) if bn else None, vec(c["rstd"]) if bn else None
    wp, kpad = pack_w(c["w"])
    wp = wp.to(dev)
    if dx is None:
        dx = torch.full((n, h, w, cin), float("nan"), device=dev)
    stride = 2 * cin + 8
    sums = torch.zeros(nrep, stride, dtype=torch.float64, device=dev) if bn else None
    rc = L.lib().uwm_op_dgrad_f16x3(P(dy), n, h, w, cout, cout, P(wp), kpad, cin, P(add), P(mask), P(msc), P(msh), P(mean), P(rstd),
                                    P(yb), P(sums), nrep, stride, P(dx), cfg, stream())
    torch.cuda.synchronize()
    return rc, dx, sums


def _dgrad_check(dev, shape, form, cfg, nprod=3, mag=R.DY_SMALL):
    c = R.dgrad_case(shape, form, mag)
    rc, dx, _ = _dgrad_launch(dev, c, cfg)
    lib().check(rc)
    name = f"dgrad {shape}/{form} dy {mag:g} cfg {cfg} nprod {nprod}"
    assert torch.isfinite(dx).all(), name
    got = nchw(dx.cpu()).double()
    if c["mask"] is not None:
        assert bool((got[R.mask_sign(c["mask"], c["mscale"], c["mshift"]) <= 0] == 0).all()), name
    emu = R.dgrad_ref(shape, form, nprod, mag)
    bar = R.BAR * max(1.0, R.out_range(emu) / mag) * mag
    err = float((got - emu).abs().max())
    figs = {"err": err / bar}
    if nprod == 3:
        figs["fp64"], figs["direct"] = _chan_rel(got, R.dgrad_ref(shape, form, 0, mag)), _direct_dgrad_err(dev, shape, mag)
    _note(name, **figs)
    assert err < bar, (name, err, bar)
    if nprod == 3:
        assert figs["fp64"] < 4 * figs["direct"] + 1e-7, (name, figs)


@pytest.mark.parametrize("form", R.DGRAD_FORMS)
@pytest.mark.parametrize("shape", list(R.DGRAD_SHAPES))
def test_dgrad(cuda, shape, form):
    """the dgrad role as the backward launches it (tap-mirrored bank from the forward weights, dY ~ 1e-6 scaled by a power of
    two, addend, mask, mscale / mshift) on 607, 605 and conv_f16x3.hip's 602"""
    for cfg in V2_CODES + (602,):
        _dgrad_check(cuda, shape, form, cfg)


def test_dgrad_large_dy(cuda):
    for cfg in V2_CODES + (602,):
        _dgrad_check(cuda, "96from32", "addmask", cfg, mag=R.DY_LARGE)


@pytest.mark.parametrize("nprod", [1, 2])
def test_dgrad_product_counts(cuda, nprod):
    with _products(nprod):
        for form in R.DGRAD_FORMS:
            for cfg in V2_CODES + (602,):
                _dgrad_check(cuda, "96from32", form, cfg, nprod)


@pytest.mark.parametrize("with_y", [False, True], ids=["mask", "bnb_y"])
@pytest.mark.parametrize("nrep", [1, 4])
@pytest.mark.parametrize("shape", list(R.DGRAD_SHAPES))
def test_dgrad_bn_backward_sums(cuda, shape, nrep, with_y):
    """the fused BatchNorm-backward sums: sum v and sum v (y - mean) rstd over the masked result v (fp64), y = the mask tensor or
    bnb_y; replicas added up in fp64; nothing written between the replicas; dx bit-identical between two launches, the sums
    (fp64 atomics) to rounding"""
    form, mag = "addmask_affine", R.DY_SMALL
    c = R.dgrad_case(shape, form, mag)
    cin = c["cin"]
    v = R.dgrad_ref(shape, form, 0, mag) / mag
    yraw = (c["y"] if with_y else c["mask"]).double()
    yhat = (yraw - c["mean"].double()[None, :, None, None]) * c["rstd"].double()[None, :, None, None]
    r1, r2 = v.sum((0, 2, 3)), (v * yhat).sum((0, 2, 3))
    b1 = 1e-5 * r1.abs() + 1e-5 * max(1.0, float(r1.abs().max()))
    b2 = 1e-5 * r2.abs() + 1e-5 * float(r2.abs().max())
    for cfg in V2_CODES + (602,):
        name = f"bnsums {shape} nrep {nrep} {'bnb_y' if with_y else 'mask'} cfg {cfg}"
        rc, dx, sums = _dgrad_launch(cuda, c, cfg, bn="y" if with_y else "mask", nrep=nrep)
        lib().check(rc)
        rc, dx2, sums2 = _dgrad_launch(cuda, c, cfg, bn="y" if with_y else "mask", nrep=nrep)
        lib().check(rc)
        assert torch.isfinite(dx).all() and torch.equal(dx, dx2), name
        emu = R.dgrad_ref(shape, form, 3, mag)
        assert float((nchw(dx.cpu()).double() - emu).abs().max()) < R.BAR * max(1.0, R.out_range(emu) / mag) * mag, name
        s, s2 = sums.cpu(), sums2.cpu()
        assert bool((s[:, 2 * cin:] == 0).all()), name
        if nrep > 1 and cfg != 602:                      # (second form: one workgroup per tile and 32 channels, replica = workgroup & (nrep - 1))
            ngrid = c["n"] * (c["h"] // 8) * (c["w_"] // 32) * (cin // 32)
            assert int((s[:, :cin].abs().sum(1) > 0).sum()) == min(nrep, ngrid), name
        tot, tot2 = s.sum(0) / mag, s2.sum(0) / mag
        e1, e2 = float(((tot[:cin] - r1).abs() / b1).max()), float(((tot[cin:2 * cin] - r2).abs() / b2).max())
        _note(name, sum=e1, sumsq=e2)
        assert e1 <= 1.0 and e2 <= 1.0, (name, e1, e2)
        assert torch.allclose(tot, tot2, rtol=1e-9, atol=1e-9 * float(tot.abs().max())), name


# ------------------------------------------------------------------------------------------------------------------ rejections
def test_rejections(cuda):
    """shapes and codes the kernel does not take are errors, and nothing is launched: the NaN-prefilled output stays untouched"""
    L = lib()
    g = torch.Generator().manual_seed(3)

    def fwd(cin, cout, h, w, cfg):
        rc, y, _ = _conv_launch(cuda, [_plain(torch.randn(1, cin, h, w, generator=g))], torch.randn(cout, cin, 3, 3, generator=g), None, 1, cout, cfg)
        assert rc != 0 and bool(torch.isnan(y).all()), (cin, cout, h, w, cfg)
        assert L.lib().uwm_last_error()

    def dgrad(cin, cout, h, w, cfg):
        c = {"n": 1, "h": h, "w_": w, "cin": cin, "cout": cout, "dy": torch.randn(1, cout, h, w, generator=g),
             "w": torch.randn(cout, cin, 3, 3, generator=g), "addend": None, "mask": None, "mscale": None, "mshift": None}
        rc, dx, _ = _dgrad_launch(cuda, c, cfg)
        assert rc != 0 and bool(torch.isnan(dx).all()), (cin, cout, h, w, cfg)

    for cfg in V2_CODES:
        fwd(32, 32, 8, 48, cfg)             # Wo = 48: no whole 32-pixel tiles
        fwd(32, 32, 12, 32, cfg)            # Ho = 12: no whole 8-row tiles
        fwd(32, 48, 8, 32, cfg)             # Cout = 48: no whole 32-channel fragments
        dgrad(32, 32, 8, 48, cfg)
        dgrad(32, 32, 12, 32, cfg)
        dgrad(48, 32, 8, 32, cfg)
    for cfg in (604, 606):                  # removed forms
        fwd(32, 32, 8, 32, cfg)
        dgrad(32, 32, 8, 32, cfg)
    try:
        for n in (0, 4, -1):
            assert L.lib().uwm_op_set_f16x3_products(n) != 0
        # a refused count changes nothing: the next launch still runs three products
        _fwd_check(cuda, "32to32", "plain", 607)
    finally:
        L.lib().uwm_op_set_f16x3_products(3)
