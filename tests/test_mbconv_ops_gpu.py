"""Operator-level parity of the MBConv plumbing (csrc/mbconv.hip: swish, squeeze pooling, the SE fully-connected pair, channel
scale, block output, drop-connect row scale) and of the depthwise BatchNorm statistics (colstats + bn_finalize) against plain
torch on the CPU in float64, at the smallest shapes that reach every branch the published EfficientNet sizes run.

Bars (those of test_bn_backward_act_matches_autograd, none invented here):
  element-wise outputs   |got - ref| < 3e-5 * max|ref| + 1e-6
  reduced quantities     |got - ref| <= 1e-4 * |ref| + 1e-4 * max|ref|
  BatchNorm mean / rstd / running statistics: 1e-4 absolute (the bar the model tests hold the buffers to)
Every assertion prints its worst error as a fraction of its bar (pytest -s shows the margins).

The launch constants of mbconv.hip are mirrored below; each test asserts the branch condition it exists for, so a retune of
the constants fails here instead of silently un-testing the branch."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.util import P, stream, rup

pytestmark = pytest.mark.gpu

K_MAX_B = 256 * 8          # mbconv.hip kMaxB: the grid clamp of nb()
NAN = float("nan")
SENTINEL = 777.0


def lib():
    from unet_watermark_amd import _lib as L
    return L


def pick_cw(c):
    """mbconv.hip pick_cw: the largest divisor of C that is a multiple of 4 and <= 1024"""
    for d in range(1, c + 1):
        if c % d == 0 and c // d <= 1024 and (c // d) % 4 == 0:
            return c // d
    return 0


def tiles(c):
    cw = pick_cw(c)
    tc = cw // 4
    return cw, tc, 256 // tc


def nb(work, per):
    return max(1, min(K_MAX_B, -(-work // per)))


def se_max_parts(c):
    """kSeMaxParts as the library reports it: se_reduce_scratch_floats(1, C) / C"""
    return lib().lib().uwm_op_se_scratch_floats(1, c) // c


def se_parts(hw, c):
    """(parts launched, parts the hw split asks for before the cap)"""
    tr = tiles(c)[2]
    want = -(-hw // (tr * 16))
    return max(1, min(want, se_max_parts(c))), want


def check_elem(name, got, ref):
    """element-wise bar; got: fp32 tensor, ref: float64"""
    got = got.detach().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: output not fully written"
    err = float((got.double() - ref).abs().max())
    bar = 3e-5 * float(ref.abs().max()) + 1e-6
    print(f"  {name}: max err {err:.3e}  bar {bar:.3e}  ({err / bar:.3f} of bar)")
    assert err < bar, f"{name}: {err:.3e} >= {bar:.3e}"
    return err / bar


def check_red(name, got, ref):
    """bar of a reduced quantity: rtol 1e-4, atol 1e-4 * max|ref|"""
    got = got.detach().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: output not fully written"
    bar = 1e-4 * ref.abs() + 1e-4 * float(ref.abs().max())
    frac = float(((got.double() - ref).abs() / bar).max())
    print(f"  {name}: worst error {frac:.3e} of its bar (max|ref| {float(ref.abs().max()):.3e})")
    assert frac <= 1.0, f"{name}: {frac:.3f} of the bar"
    return frac


def check_abs(name, got, ref, bar=1e-4):
    got = got.detach().cpu()
    assert bool(torch.isfinite(got).all()), f"{name}: output not fully written"
    err = float((got.double() - ref).abs().max())
    print(f"  {name}: max abs err {err:.3e}  bar {bar:.1e}")
    assert err <= bar, f"{name}: {err:.3e} > {bar:.1e}"
    return err


def swish(z):
    return z * torch.sigmoid(z)


# ------------------------------------------------------------------ a. swish + squeeze pooling, plain / product reductions
SE_CASES = [(2, 48, 4), (3, 48, 1501), (1, 16, 66001), (2, 2688, 1089), (2, 3840, 64), (2, 1104, 33)]


def _se_branch(n, c, hw):
    """the branch each case exists for (issue table), from the mirrored launch arithmetic"""
    cw, tc, tr = tiles(c)
    parts, want = se_parts(hw, c)
    cap = se_max_parts(c)
    ps = parts * tr                                   # pixel stride of a thread
    if (n, c, hw) == (2, 48, 4):
        assert hw < tr == 21 and parts == 1 and 256 % tc != 0
    elif (n, c, hw) == (3, 48, 1501):
        assert parts == 5 and hw % 2 == 1
    elif (n, c, hw) == (1, 16, 66001):
        assert tr == 64 and want > cap == parts == 64
        assert hw // ps >= 2 and hw % ps != 0         # threads take q and q + 1 pixels, q >= 2: pair loop and odd tail
    elif (n, c, hw) == (2, 2688, 1089):
        assert cw == 896 and c // cw == 3 and tr == 1 and want > cap == parts
        assert (hw // ps, hw % ps) == (17, 1)         # 17 pixels per thread (8 pairs + tail), one thread 18
    elif (n, c, hw) == (2, 3840, 64):
        assert c // cw == 4
    elif (n, c, hw) == (2, 1104, 33):
        assert cw == 552 and 256 - tc * tr == 118
    else:
        raise AssertionError("case without a branch condition")
    return parts


@pytest.mark.parametrize("n,c,hw", SE_CASES)
def test_swish_pool_and_se_reduce(cuda, n, c, hw):
    """se_reduce_hw + se_reduce_finish in their three forms: act_out = swish(y*scale + shift) with pool = mean_hw(act_out),
    out = mult * sum_hw a, out = mult * sum_hw a*b.  The pool row of a sample equals, bit for bit, the row of a call on that
    sample alone (the "bit-identical ... across batch sizes" invariant stated above se_reduce_hw_kernel)."""
    L = lib()
    parts = _se_branch(n, c, hw)
    g = torch.Generator().manual_seed(1000 + c + hw)
    y = torch.randn(n, hw, c, generator=g) * 2 + 0.7
    scale = (torch.rand(c, generator=g) + 0.5) * 0.5                  # gamma * rstd of a sigma = 2 input
    shift = torch.randn(c, generator=g) * 0.5
    b = torch.randn(n, hw, c, generator=g) + 0.5
    mult = 0.375
    act_ref = swish(y.double() * scale.double() + shift.double())
    pool_ref = act_ref.mean(1)
    sum_ref = mult * y.double().sum(1)
    prod_ref = mult * (y.double() * b.double()).sum(1)

    yd, bd, sc, sh = y.to(cuda), b.to(cuda), scale.to(cuda), shift.to(cuda)
    nscr = L.lib().uwm_op_se_scratch_floats(n, c)
    assert nscr >= parts * n * c

    def fresh(*shape):
        return torch.full(shape, NAN, device=cuda)

    act, pool, part = fresh(n, hw, c), fresh(n, c), fresh(nscr)
    L.check(L.lib().uwm_op_swish_pool(P(yd), P(sc), P(sh), n, hw, c, P(act), P(pool), P(part), stream()))
    out_a, part_a = fresh(n, c), fresh(nscr)
    L.check(L.lib().uwm_op_se_reduce(P(yd), None, n, hw, c, mult, P(out_a), P(part_a), stream()))
    out_ab, part_ab = fresh(n, c), fresh(nscr)
    L.check(L.lib().uwm_op_se_reduce(P(yd), P(bd), n, hw, c, mult, P(out_ab), P(part_ab), stream()))
    torch.cuda.synchronize()
    print(f"\nse_reduce N {n} C {c} hw {hw}: {parts} parts")
    check_elem("act_out", act, act_ref)
    check_red("pool", pool, pool_ref)
    check_red("sum a", out_a, sum_ref)
    check_red("sum a*b", out_ab, prod_ref)
    for i in range(n if n > 1 else 0):
        act1, pool1, part1 = fresh(1, hw, c), fresh(1, c), fresh(L.lib().uwm_op_se_scratch_floats(1, c))
        L.check(L.lib().uwm_op_swish_pool(P(yd[i:i + 1]), P(sc), P(sh), 1, hw, c, P(act1), P(pool1), P(part1), stream()))
        torch.cuda.synchronize()
        assert torch.equal(pool1[0], pool[i]), f"pool row {i} depends on the batch size"
        assert torch.equal(act1[0], act[i])


# ------------------------------------------------------------------ b. SE fully-connected pair
FC_CASES = [(2, 48, 12), (3, 144, 6), (2, 240, 10), (16, 32, 8), (2, 2688, 112), (1, 3840, 160)]


def _garbage_pads(w, logical, g):
    """finite garbage (+-3) in the pad columns: the arena keeps them zero, but no kernel may depend on that"""
    pad = w.shape[1] - logical
    if pad:
        w[:, logical:] = (torch.randint(0, 2, (w.shape[0], pad), generator=g).float() * 2 - 1) * 3
    return w


def _fc_weights(c, nsq, g):
    k1, k2 = rup(rup(c, 4), 32), rup(rup(nsq, 4), 32)                 # Kpad of the two 1x1 layers (add_conv)
    w1 = torch.zeros(nsq, k1); w1[:, :c] = torch.randn(nsq, c, generator=g) / c ** 0.5
    w2 = torch.zeros(c, k2); w2[:, :nsq] = torch.randn(c, nsq, generator=g) / nsq ** 0.5
    b1, b2 = torch.randn(nsq, generator=g) * 0.3, torch.randn(c, generator=g) * 0.3
    return _garbage_pads(w1, c, g), b1, _garbage_pads(w2, nsq, g), b2, k1, k2


@pytest.mark.parametrize("n,c,nsq", FC_CASES)
def test_se_fc_forward_backward(cuda, n, c, nsq):
    """se_fc1 + se_fc2 and se_fc_bwd_a + se_fc_bwd_b against autograd of s = sigmoid(W2 swish(W1 pool + b1) + b2) in fp64.
    W1 / W2 carry finite garbage in their pad columns; the pad columns of gw1 / gw2 keep their sentinel (the optimizer walks
    the whole arena and relies on pads staying zero).  The backward's LDS float atomics make it order-dependent, so nothing
    here asks for bit-reproducibility."""
    L = lib()
    if (n, c, nsq) == (3, 144, 6):
        assert nsq % 4 != 0
    if (n, c, nsq) == (16, 32, 8):
        assert n * c > c * nsq                                        # se_fc_bwd_b's work = max(...) is set by N*C
    if (n, c, nsq) == (2, 2688, 112):
        assert -(-c // 256) == 11 and c % 256 != 0                    # 11 workgroups in y, the last one ragged
    g = torch.Generator().manual_seed(2000 + c + nsq)
    w1, b1, w2, b2, k1, k2 = _fc_weights(c, nsq, g)
    pool = torch.randn(n, c, generator=g) * 0.5 + 0.3
    gs = torch.randn(n, c, generator=g) + 0.5

    w1r = w1[:, :c].double().requires_grad_(); w2r = w2[:, :nsq].double().requires_grad_()
    b1r = b1.double().requires_grad_(); b2r = b2.double().requires_grad_()
    poolr = pool.double().requires_grad_()
    hpre_ref = poolr @ w1r.t() + b1r
    hid_ref = swish(hpre_ref)
    z2 = hid_ref @ w2r.t() + b2r
    z2.retain_grad()
    s_ref = torch.sigmoid(z2)
    s_ref.backward(gs.double())

    dv = lambda t: t.contiguous().to(cuda)
    w1d, b1d, w2d, b2d, poold = dv(w1), dv(b1), dv(w2), dv(b2), dv(pool)
    hpre, hid, s = (torch.full(sh, NAN, device=cuda) for sh in ((n, nsq), (n, nsq), (n, c)))
    L.check(L.lib().uwm_op_se_fc(P(poold), P(w1d), P(b1d), k1, P(w2d), P(b2d), k2, n, c, nsq, P(hpre), P(hid), P(s), stream()))
    torch.cuda.synchronize()
    print(f"\nse_fc N {n} C {c} nsq {nsq} (K1pad {k1}, K2pad {k2})")
    check_elem("hpre", hpre, hpre_ref.detach())
    check_elem("hid", hid, hid_ref.detach())
    check_elem("s", s, s_ref.detach())

    # backward from the reference's forward values, so that it is judged alone
    gsd, sd, hpd = dv(gs), dv(s_ref.detach().float()), dv(hpre_ref.detach().float())
    gpool, acc1 = torch.full((n, c), NAN, device=cuda), torch.full((n, nsq), NAN, device=cuda)
    gw1, gw2 = torch.full((nsq, k1), SENTINEL, device=cuda), torch.full((c, k2), SENTINEL, device=cuda)
    gb1, gb2 = torch.full((nsq,), NAN, device=cuda), torch.full((c,), NAN, device=cuda)
    L.check(L.lib().uwm_op_se_fc_backward(P(gsd), P(sd), P(hpd), P(poold), P(w1d), k1, P(w2d), k2, n, c, nsq, P(gpool), P(acc1),
                                          P(gw1), P(gb1), P(gw2), P(gb2), stream()))
    torch.cuda.synchronize()
    check_red("gs -> gz2", gsd, z2.grad)
    check_red("gpool", gpool, poolr.grad)
    check_red("gw1", gw1[:, :c], w1r.grad)
    check_red("gb1", gb1, b1r.grad)
    check_red("gw2", gw2[:, :nsq], w2r.grad)
    check_red("gb2", gb2, b2r.grad)
    assert bool((gw1[:, c:] == SENTINEL).all()), "se_fc_bwd_b stored into the pad columns of gw1"
    assert bool((gw2[:, nsq:] == SENTINEL).all()), "se_fc_bwd_b stored into the pad columns of gw2"


# ------------------------------------------------------------------ c. element-wise kernels, below and past the grid clamp
EW_CASES = [(2, 35, 24), (3, 2401, 304)]
DROP_P = 0.2


@functools.lru_cache(maxsize=None)
def _ew_inputs(n, hw, c):
    """inputs shared by the four element-wise tests of a shape (never modified)"""
    n4, per_img4 = n * hw * c // 4, hw * c // 4
    if (n, hw, c) == EW_CASES[1]:
        assert n * hw * c == 2_189_712
        assert -(-n4 // 256) > K_MAX_B == nb(n4, 256)                 # clamped: every thread goes round the grid-stride loop again
        assert per_img4 % 256 != 0                                    # a workgroup straddles two samples
    else:
        assert -(-n4 // 256) < K_MAX_B
    g = torch.Generator().manual_seed(3000 + c)
    y = torch.randn(n, hw, c, generator=g) * 2 + 0.7
    scale = (torch.rand(c, generator=g) + 0.5) * 0.5
    shift = torch.randn(c, generator=g) * 0.5
    s = torch.rand(n, c, generator=g) + 0.25
    ident = torch.randn(n, hw, c, generator=g)
    keep = torch.tensor([1.0 / (1.0 - DROP_P), 0.0, 1.0 / (1.0 - DROP_P)][:n])
    return y, scale, shift, s, ident, keep


@pytest.mark.parametrize("n,hw,c", EW_CASES)
def test_swish_elementwise(cuda, n, hw, c):
    """swish_fwd: out = swish(y*scale + shift)"""
    L = lib()
    y, scale, shift, _, _, _ = _ew_inputs(n, hw, c)
    out = torch.full((n, hw, c), NAN, device=cuda)
    t = [y.to(cuda), scale.to(cuda), shift.to(cuda)]
    L.check(L.lib().uwm_op_swish(P(t[0]), P(t[1]), P(t[2]), n * hw, c, P(out), stream()))
    torch.cuda.synchronize()
    print(f"\nswish N {n} hw {hw} C {c}")
    check_elem("swish", out, swish(y.double() * scale.double() + shift.double()))


@pytest.mark.parametrize("n,hw,c", EW_CASES)
def test_se_scale_elementwise(cuda, n, hw, c):
    """se_scale: out[n][p][c] = a[n][p][c] * s[n][c], a single fp32 multiply: equal to the fp32 product bit for bit"""
    L = lib()
    y, _, _, s, _, _ = _ew_inputs(n, hw, c)
    out = torch.full((n, hw, c), NAN, device=cuda)
    t = [y.to(cuda), s.to(cuda)]
    L.check(L.lib().uwm_op_se_scale(P(t[0]), P(t[1]), n, hw, c, P(out), stream()))
    torch.cuda.synchronize()
    print(f"\nse_scale N {n} hw {hw} C {c}")
    check_elem("se_scale", out, y.double() * s.double()[:, None, :])
    assert torch.equal(out.cpu(), y * s[:, None, :])


@pytest.mark.parametrize("n,hw,c", EW_CASES)
def test_rowscale_elementwise(cuda, n, hw, c):
    """rowscale: out = g * rowscale[n]; the dropped sample is exactly zero, the rest the fp32 product bit for bit"""
    L = lib()
    y, _, _, _, _, keep = _ew_inputs(n, hw, c)
    out = torch.full((n, hw, c), NAN, device=cuda)
    t = [y.to(cuda), keep.to(cuda)]
    L.check(L.lib().uwm_op_rowscale(P(t[0]), P(t[1]), n, hw, c, P(out), stream()))
    torch.cuda.synchronize()
    print(f"\nrowscale N {n} hw {hw} C {c}")
    check_elem("rowscale", out, y.double() * keep.double()[:, None, None])
    assert torch.equal(out.cpu(), y * keep[:, None, None])
    assert bool((out[1] == 0).all())


@pytest.mark.parametrize("use_id", [False, True], ids=["noid", "id"])
@pytest.mark.parametrize("use_rs", [False, True], ids=["nors", "rs"])
@pytest.mark.parametrize("n,hw,c", EW_CASES)
def test_mb_out_elementwise(cuda, n, hw, c, use_rs, use_id):
    """mb_out: out = (y*scale + shift) * rowscale[n] + id with rowscale / id each given or NULL.  A dropped sample's output is
    exactly id (exactly zero without id)."""
    L = lib()
    y, scale, shift, _, ident, keep = _ew_inputs(n, hw, c)
    ref = y.double() * scale.double() + shift.double()
    if use_rs:
        ref = ref * keep.double()[:, None, None]
    if use_id:
        ref = ref + ident.double()
    out = torch.full((n, hw, c), NAN, device=cuda)
    t = [y.to(cuda), scale.to(cuda), shift.to(cuda), keep.to(cuda) if use_rs else None, ident.to(cuda) if use_id else None]
    L.check(L.lib().uwm_op_mb_out(P(t[0]), P(t[1]), P(t[2]), P(t[3]), P(t[4]), n, hw, c, P(out), stream()))
    torch.cuda.synchronize()
    print(f"\nmb_out N {n} hw {hw} C {c} rowscale {use_rs} id {use_id}")
    check_elem("mb_out", out, ref)
    if use_rs:
        assert torch.equal(out[1].cpu(), ident[1] if use_id else torch.zeros(hw, c))


# ------------------------------------------------------------------ d. BatchNorm statistics of a depthwise layer
BN_EPS, BN_MOM = 1e-3, 0.01                                           # the EfficientNet encoder's
STATS_CASES = [(5, 48), (2 * 24 * 40, 32), (120, 2688), (16800, 960)]


def _run_bn_stats(cuda, y, gamma, beta, rm, rv, update):
    L = lib()
    npix, c = y.shape
    dv = lambda t: t.clone().to(cuda)
    yd, gd, bd, rmd, rvd = dv(y), dv(gamma), dv(beta), dv(rm), dv(rv)
    sums = torch.full((2 * c,), NAN, dtype=torch.float64, device=cuda)
    outs = [torch.full((c,), NAN, device=cuda) for _ in range(4)]
    L.check(L.lib().uwm_op_bn_stats(P(yd), npix, c, P(gd), P(bd), BN_EPS, BN_MOM, update, P(rmd), P(rvd), P(sums), P(outs[0]),
                                    P(outs[1]), P(outs[2]), P(outs[3]), stream()))
    torch.cuda.synchronize()
    return outs, rmd.cpu(), rvd.cpu(), sums.cpu()


@pytest.mark.parametrize("npix,c", STATS_CASES)
def test_bn_stats(cuda, npix, c):
    """colstats + bn_finalize as a depthwise layer's training forward runs them: mean, rstd, scale, shift and the running
    statistics (momentum 0.01, unbiased variance) from non-trivial starting values against fp64; with update_running = 0 the
    running buffers stay bit-unchanged."""
    cw, tc, tr = tiles(c)
    if (npix, c) == (5, 48):
        assert npix < tr
    if (npix, c) == (1920, 32):
        assert 1 < nb(npix, tr * 8) < K_MAX_B
    if (npix, c) == (120, 2688):
        assert c // cw == 3
    if (npix, c) == (16800, 960):
        assert -(-npix // (tr * 8)) > K_MAX_B == nb(npix, tr * 8)
    g = torch.Generator().manual_seed(4000 + c + npix)
    y = torch.randn(npix, c, generator=g) * 2 + 0.7
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.5
    rm, rv = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    y64 = y.double()
    mean = y64.mean(0); var = y64.var(0, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + BN_EPS)
    scale = gamma.double() * rstd; shift = beta.double() - mean * scale
    unb = var * npix / (npix - 1)
    rm_t, rv_t = rm.double().clone(), rv.double().clone()             # the reference is torch's own batch_norm
    z = F.batch_norm(y64, rm_t, rv_t, gamma.double(), beta.double(), True, BN_MOM, BN_EPS)
    assert torch.allclose(z, y64 * scale + shift, rtol=0, atol=1e-9)
    assert torch.allclose(rm_t, (1 - BN_MOM) * rm.double() + BN_MOM * mean, rtol=0, atol=1e-12)
    assert torch.allclose(rv_t, (1 - BN_MOM) * rv.double() + BN_MOM * unb, rtol=0, atol=1e-12)
    (m_, r_, sc_, sh_), rm1, rv1, _ = _run_bn_stats(cuda, y, gamma, beta, rm, rv, 1)
    print(f"\nbn_stats npix {npix} C {c}")
    check_abs("mean", m_, mean)
    check_abs("rstd", r_, rstd)
    check_elem("scale", sc_, scale)
    check_elem("shift", sh_, shift)
    check_abs("running_mean", rm1, (1 - BN_MOM) * rm.double() + BN_MOM * mean)
    check_abs("running_var", rv1, (1 - BN_MOM) * rv.double() + BN_MOM * unb)
    outs0, rm0, rv0, _ = _run_bn_stats(cuda, y, gamma, beta, rm, rv, 0)
    assert torch.equal(rm0, rm) and torch.equal(rv0, rv), "update_running = 0 touched the running buffers"
    assert all(torch.equal(a, b) or (a - b).abs().max() <= 1e-6 * float(b.abs().max()) for a, b in zip(outs0, (m_, r_, sc_, sh_)))


def test_bn_stats_single_pixel(cuda):
    """count == 1 (npix 1, C 4): the unbiased-variance factor count / (count - 1) must not divide by zero; the running variance
    takes the biased variance, which is 0, instead.  The variance the kernel forms is fl32(x^2) - x^2 in double, so it is held
    to the arithmetic bound of the 16-sigma test with var64 = 0, not to zero."""
    g = torch.Generator().manual_seed(4001)
    y = torch.randn(1, 4, generator=g) * 2 + 0.7
    gamma, beta = torch.rand(4, generator=g) + 0.5, torch.randn(4, generator=g) * 0.5
    rm, rv = torch.randn(4, generator=g), torch.rand(4, generator=g) + 0.5
    (m_, r_, sc_, sh_), rm1, rv1, sums = _run_bn_stats(cuda, y, gamma, beta, rm, rv, 1)
    print("\nbn_stats npix 1 C 4")
    assert all(bool(torch.isfinite(t).all()) for t in (m_, r_, sc_, sh_, rm1, rv1))
    check_abs("mean", m_, y[0].double())
    check_abs("running_mean", rm1, (1 - BN_MOM) * rm.double() + BN_MOM * y[0].double())
    check_abs("running_var", rv1, (1 - BN_MOM) * rv.double())
    got_var = sums[4:] - sums[:4] ** 2
    assert bool((got_var.abs() <= 8 * 2.0 ** -24 * y[0].double() ** 2).all())
    check_elem("y*scale + shift", y.to(cuda) * sc_ + sh_, beta.double()[None, :])     # the layer's output is beta, whatever rstd


def test_bn_stats_variance_at_16_sigma(cuda):
    """Channel means of +-16 sigma.  colstats forms E[x^2] - E[x]^2 from fp32 per-thread partial sums (added in double after
    that), so its variance cannot match a two-pass result; what that arithmetic allows is
        |var - var64| <= 8 * 2^-24 * (mean^2 + var)
    (the 8: three bits for a thread's partial sums of at most a few dozen terms).  The test prints the measured ratio.
    Measured ratio on the MI355X: not recorded yet (emulating the kernel's arithmetic on the CPU, fp32 squares and fp32
    partial sums of 8 terms added in double, gives a ratio of 0.23 against the 8 allowed)."""
    npix, c = 2 * 24 * 40, 32
    assert -(-npix // nb(npix, tiles(c)[2] * 8) // tiles(c)[2]) <= 48          # terms a thread accumulates
    g = torch.Generator().manual_seed(4242)
    sigma = torch.rand(c, generator=g) * 1.5 + 0.5
    sign = torch.randint(0, 2, (c,), generator=g).float() * 2 - 1
    y = torch.randn(npix, c, generator=g) * sigma + 16 * sigma * sign
    y64 = y.double()
    mean, var = y64.mean(0), y64.var(0, unbiased=False)
    assert float((mean.abs() / var.sqrt()).min()) > 15
    (m_, r_, _, _), _, _, sums = _run_bn_stats(cuda, y, torch.ones(c), torch.zeros(c), torch.zeros(c), torch.ones(c), 0)
    got_var = sums[c:] / npix - (sums[:c] / npix) ** 2
    ratio = float(((got_var - var).abs() / (2.0 ** -24 * (mean ** 2 + var))).max())
    print(f"\nbn_stats 16 sigma: |var - var64| / (2^-24 (mean^2 + var)) = {ratio:.3f} (allowed 8)")
    assert ratio <= 8.0, ratio
    check_abs("mean", m_, mean)


# ------------------------------------------------------------------ f. the block tail as the model chains it
@pytest.mark.parametrize("n,c,h,w,nsq", [(3, 144, 20, 28, 6), (2, 672, 33, 33, 28)])
def test_mbconv_tail_chain(cuda, n, c, h, w, nsq):
    """The entries wired in the model's order, from the depthwise output y to the block output and back:
    forward  bn_stats -> swish_pool -> se_fc -> se_scale -> [projection] -> mb_out (drop connect + identity),
    backward rowscale -> [projection] -> se_reduce(g, a1) -> se_fc_backward -> bn_backward_act(se_s, gpool),
    against fp64 autograd of the same tail.  The projection convolution and its BatchNorm, which have their own tests, are
    stood in for by the per-channel affine map mb_out applies (scale2, shift2), its backward by a multiply with scale2.
    Pins the contracts between the kernels: who divides by hw, that gs arrives as gz2, the hpre / hid layout."""
    L = lib()
    hw = h * w
    if c == 672:
        parts, want = se_parts(hw, c)
        assert want > parts == se_max_parts(c)                        # capped reduce
    g = torch.Generator().manual_seed(6000 + c)
    y = torch.randn(n, hw, c, generator=g) * 2 + 0.7
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.5
    w1, b1, w2, b2, k1, k2 = _fc_weights(c, nsq, g)
    scale2, shift2 = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    ident = torch.randn(n, hw, c, generator=g)
    keep = torch.tensor([1.0 / (1.0 - DROP_P), 0.0, 1.0 / (1.0 - DROP_P)][:n]) if n == 3 else torch.full((n,), 1.0 / (1.0 - DROP_P))
    dz = torch.randn(n, hw, c, generator=g) + 0.5

    # ---- fp64 reference
    yr = y.double().requires_grad_()
    gr, br = gamma.double().requires_grad_(), beta.double().requires_grad_()
    w1r = w1[:, :c].double().requires_grad_(); w2r = w2[:, :nsq].double().requires_grad_()
    b1r = b1.double().requires_grad_(); b2r = b2.double().requires_grad_()
    z = F.batch_norm(yr.reshape(n * hw, c), None, None, gr, br, True, BN_MOM, BN_EPS).reshape(n, hw, c)
    a1 = swish(z)
    s_ref = torch.sigmoid(swish(a1.mean(1) @ w1r.t() + b1r) @ w2r.t() + b2r)
    a2_ref = a1 * s_ref[:, None, :]
    out_ref = (a2_ref * scale2.double() + shift2.double()) * keep.double()[:, None, None] + ident.double()
    out_ref.backward(dz.double())

    # ---- the kernels
    dv = lambda t: t.contiguous().to(cuda)
    fresh = lambda *sh: torch.full(sh, NAN, device=cuda)
    yd, gd, bd = dv(y), dv(gamma), dv(beta)
    w1d, b1d, w2d, b2d = dv(w1), dv(b1), dv(w2), dv(b2)
    sc2d, sh2d, idd, keepd, dzd = dv(scale2), dv(shift2), dv(ident), dv(keep), dv(dz)
    rm, rv = torch.zeros(c, device=cuda), torch.ones(c, device=cuda)
    sums = torch.full((2 * c,), NAN, dtype=torch.float64, device=cuda)
    mean, rstd, scale, shift = (fresh(c) for _ in range(4))
    lb = L.lib()
    L.check(lb.uwm_op_bn_stats(P(yd), n * hw, c, P(gd), P(bd), BN_EPS, BN_MOM, 1, P(rm), P(rv), P(sums), P(mean), P(rstd), P(scale),
                               P(shift), stream()))
    a1d, pool, part = fresh(n, hw, c), fresh(n, c), fresh(lb.uwm_op_se_scratch_floats(n, c))
    L.check(lb.uwm_op_swish_pool(P(yd), P(scale), P(shift), n, hw, c, P(a1d), P(pool), P(part), stream()))
    se_buf = fresh(n * c + n * rup(nsq, 4) + n * nsq)                 # the workspace layout: s | hpre (rows of rup(nsq, 4) reserved) | hid
    sd, hpre, hid = se_buf[:n * c], se_buf[n * c:], se_buf[n * c + n * rup(nsq, 4):]
    L.check(lb.uwm_op_se_fc(P(pool), P(w1d), P(b1d), k1, P(w2d), P(b2d), k2, n, c, nsq, P(hpre), P(hid), P(sd), stream()))
    a2d, out = fresh(n, hw, c), fresh(n, hw, c)
    L.check(lb.uwm_op_se_scale(P(a1d), P(sd), n, hw, c, P(a2d), stream()))
    L.check(lb.uwm_op_mb_out(P(a2d), P(sc2d), P(sh2d), P(keepd), P(idd), n, hw, c, P(out), stream()))
    g_o = fresh(n, hw, c)
    L.check(lb.uwm_op_rowscale(P(dzd), P(keepd), n, hw, c, P(g_o), stream()))
    g_m = g_o * sc2d                                                  # the projection's backward
    gs, acc1, gpool = fresh(n, c), fresh(n, nsq), fresh(n, c)
    L.check(lb.uwm_op_se_reduce(P(g_m), P(a1d), n, hw, c, 1.0, P(gs), P(part), stream()))
    gw1, gw2 = torch.full((nsq, k1), SENTINEL, device=cuda), torch.full((c, k2), SENTINEL, device=cuda)
    gb1, gb2 = fresh(nsq), fresh(c)
    L.check(lb.uwm_op_se_fc_backward(P(gs), P(sd), P(hpre), P(pool), P(w1d), k1, P(w2d), k2, n, c, nsq, P(gpool), P(acc1), P(gw1),
                                     P(gb1), P(gw2), P(gb2), stream()))
    dy, dgam, dbet = fresh(n, hw, c), fresh(c), fresh(c)
    scr = torch.empty(2 * c, dtype=torch.float64, device=cuda)
    L.check(lb.uwm_op_bn_backward_act(P(g_m), P(yd), P(mean), P(rstd), P(gd), P(scale), P(shift), P(sd), P(gpool), n, hw, c, P(scr),
                                      P(dy), P(dgam), P(dbet), None, stream()))
    torch.cuda.synchronize()
    print(f"\nMBConv tail N {n} C {c} {h}x{w} nsq {nsq}")
    check_elem("a2", a2d, a2_ref.detach())
    check_elem("out", out, out_ref.detach())
    check_red("gw1", gw1[:, :c], w1r.grad)
    check_red("gb1", gb1, b1r.grad)
    check_red("gw2", gw2[:, :nsq], w2r.grad)
    check_red("gb2", gb2, b2r.grad)
    check_red("dgamma", dgam, gr.grad)
    check_red("dbeta", dbet, br.grad)
    check_elem("dy", dy, yr.grad)
    assert bool((gw1[:, c:] == SENTINEL).all()) and bool((gw2[:, nsq:] == SENTINEL).all())
