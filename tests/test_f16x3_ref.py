"""tests/f16x3_ref.py pinned on the CPU, on the very operands tests/test_f16x3v2_ops_gpu.py launches the kernels with.

The GPU tests hold a kernel's output to BAR * max(1, output range) of the emulation of ITS product count.  That is only a test of
the split arithmetic if, on these operands,
  1. the three-product emulation is the convolution: within 1e-6 of the output range of the fp64 truth;
  2. one product is far from it: emu(1) misses the truth by more than 10 bars;
  3. two products are told from three: emu(2) and emu(3) differ by more than 3 bars
     (2 and 3: a kernel that runs the wrong product count cannot pass);
  4. the row scale is immaterial: the row maximum in [2^10, 2^11) or in [2^13, 2^14) moves the result by less than 1e-3 bars
     (so no test copies the kernels' scale rule).
A dgrad's bar is taken in units of its dY magnitude (dY ~ 1e-6 or 1e3: the range of dx / magnitude), which is what the GPU file
does too: against the literal max(1, range) a 1e-6 gradient would be held to nothing.

The weight-gradient cases of tests/test_wgrad_f16x3_ops_gpu.py follow further down, with their own bar and thresholds.
"""
import pytest

from tests import f16x3_ref as R


def _bar(truth, unit=1.0):
    return R.BAR * max(1.0, R.out_range(truth) / unit) * unit


def _check(get, unit=1.0):
    truth, e1, e2, e3, e3b = get(0), get(1), get(2), get(3), get(3, 11)
    rng, bar = R.out_range(truth), _bar(truth, unit)
    d3, d1, d23, dtop = [float(v.abs().max()) for v in (e3 - truth, e1 - truth, e2 - e3, e3b - e3)]
    print(f"range {rng:.3e} bar {bar:.3e}: |emu3-truth| {d3:.3e} |emu1-truth| {d1 / bar:.1f} bars |emu2-emu3| {d23 / bar:.1f} bars "
          f"|top 11 - top 14| {dtop / bar:.2e} bars")
    assert d3 < 1e-6 * rng
    assert d1 > 10 * bar
    assert d23 > 3 * bar
    assert dtop < 1e-3 * bar


@pytest.mark.parametrize("shape,form", R.fwd_cases())
def test_forward_operands(shape, form):
    _check(lambda nprod, top=14: R.fwd_ref(shape, form, nprod, top))


@pytest.mark.parametrize("shape", list(R.DGRAD_SHAPES))
@pytest.mark.parametrize("form", R.DGRAD_FORMS)
def test_dgrad_operands(shape, form):
    _check(lambda nprod, top=14: R.dgrad_ref(shape, form, nprod, R.DY_SMALL, top), R.DY_SMALL)


def test_dgrad_operands_large_dy():
    _check(lambda nprod, top=14: R.dgrad_ref("96from32", "addmask", nprod, R.DY_LARGE, top), R.DY_LARGE)


# ------------------------------------------------------------------------------------------------------------ weight gradient
# tests/test_wgrad_f16x3_ops_gpu.py holds wgrad_f16x3.hip to WGRAD_BAR * range of the true gradient (test_wgrad_f16x3_direct's bar,
# relative to the range with no max(1, .): a 1e-6 gradient would otherwise be held to nothing).  The same four conditions, with the
# thresholds measured for this kernel's operands (one product misses by >= 7.9 bars, two and three differ by >= 5.9 bars on
# test_wgrad_f16x3_direct-like sets): 1e-6 of the range, 5 bars, 3 bars; and what a test would have to copy from the kernel is the
# window xs puts max|dY| into: [2^10, 2^11) instead of [2^13, 2^14) moves the result by less than 1e-3 bars.
def _wgrad_check(shape, form, mag, xmag, d3_bound=None):
    import torch
    get = lambda nprod, top=14: R.wgrad_ref(shape, form, nprod, mag, xmag, top)
    truth, e1, e2, e3, e3b = get(0), get(1), get(2), get(3), get(3, 11)
    rng = R.out_range(truth)
    bar = R.WGRAD_BAR * rng
    d3, d1, d23, dtop = [float(v.abs().max()) for v in (e3 - truth, e1 - truth, e2 - e3, e3b - e3)]
    print(f"wgrad {shape}/{form} dy {mag:g} x {xmag:g}: range {rng:.3e} bar {bar:.3e}: |emu3-truth| {d3 / rng:.3e} of range "
          f"|emu1-truth| {d1 / bar:.1f} bars |emu2-emu3| {d23 / bar:.1f} bars |top 11 - top 14| {dtop / bar:.2e} bars")
    assert torch.isfinite(truth).all() and rng > 0
    assert d3 < (1e-6 * rng if d3_bound is None else d3_bound(rng))
    assert d1 > 5 * bar
    assert d23 > 3 * bar
    assert dtop < 1e-3 * bar


@pytest.mark.parametrize("shape,form", R.wgrad_cases())
def test_wgrad_operands(shape, form):
    _wgrad_check(shape, form, R.DY_SMALL, 1.0)


@pytest.mark.parametrize("shape,form,mag,xmag", R.WGRAD_RANGES)
def test_wgrad_operands_ranges(shape, form, mag, xmag):
    """dY ~ 1e3, X ~ 300 and X ~ 1e-3.  Below fp16's normal range the low half of X has an absolute step of 2^-24: |X - hi - lo| <=
    2^-25 per element there, whatever X is, so at X ~ 1e-3 the three products miss the truth by up to 2^-25 * the largest
    sum over pixels of |dY| of a row — that, on top of the 1e-6 of the range, is condition 1 there (the GPU file holds that case
    to the emulation alone)."""
    bound = None
    if xmag < 0.01:
        dy = R.wgrad_case(shape, form, mag, xmag)["dy"].double()
        bound = lambda rng: 1e-6 * rng + 2.0 ** -25 * float(dy.abs().sum((0, 2, 3)).max())
    _wgrad_check(shape, form, mag, xmag, bound)


def test_wgrad_zero_dy():
    """dY all zero: xs stays 1 and every product count gives exactly zero"""
    assert float(R.pow2_scale(R.wgrad_case("halo", "lazy", 0.0)["dy"].abs().max().reshape(1))[0]) == 1.0
    for nprod in (0, 1, 2, 3):
        assert float(R.wgrad_ref("halo", "lazy", nprod, 0.0).abs().max()) == 0.0


def test_wgrad_case_table():
    """every case reaches the branch its table comment names on any card: the same (stage width, workgroups, splits, stages per
    split) for 64, 256 and 304 CUs, and the last split of `uneven` is the shorter one"""
    names = [s if s in R.WGRAD_SHAPES else f"{s}/{f}" for s, f in R.wgrad_cases() if s not in R.WGRAD_SHAPES or f == "plain"]
    assert sorted(names) == sorted(R.WGRAD_CLAIMS)
    for name in names:
        shape, _, form = name.partition("/")
        cin, wrows, coutp, n, h, w = R.wgrad_dims(shape, form or "plain")
        assert wrows <= coutp and coutp % 4 == 0 and cin % 32 == 0
        wx, pairs, nstages = R.wgrad_geometry(cin, wrows, h, w, n)
        for cus in (64, 256, 304):
            nsplit, sps = R.wgrad_splits(pairs, nstages, cus)
            print(f"{name}: WX {wx} pairs {pairs} stages {nstages} cus {cus}: {nsplit} splits of {sps}")
            assert (wx, pairs * nsplit, nsplit, sps) == R.WGRAD_CLAIMS[name], (name, cus)
            assert (nsplit - 1) * sps < nstages <= nsplit * sps
    nsplit, sps = R.wgrad_splits(2, 9, 256)
    assert 9 - (nsplit - 1) * sps == 4                      # uneven: 5 + 4


def test_split_halves():
    """hi + lo carries 22 bits: |v - hi - lo| <= 2^-22 |v| where lo stays a normal fp16, and the scales are exact powers of two"""
    import torch
    g = torch.Generator().manual_seed(1)
    v = ((torch.rand(4096, generator=g) + 1.0) * 4096.0 * (torch.randint(0, 2, (4096,), generator=g) * 2 - 1)).double()
    assert float(((v - R.hi(v) - R.lo(v)).abs() / v.abs()).max()) <= 2.0 ** -22
    s = R.pow2_scale(torch.tensor([3e-7, 1.0, 8191.9, 8192.0, 5e4]), 14)
    assert all(float(x) == 2.0 ** round(float(torch.log2(x))) for x in s)
    assert bool(((torch.tensor([3e-7, 1.0, 8191.9, 8192.0, 5e4]).double() * s >= 2.0 ** 13) & (torch.tensor([3e-7, 1.0, 8191.9, 8192.0, 5e4]).double() * s < 2.0 ** 14)).all())
    assert float(R.pow2_scale(torch.zeros(1))[0]) == 1.0
