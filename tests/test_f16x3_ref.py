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
