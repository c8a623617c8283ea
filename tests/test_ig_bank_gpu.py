"""Pre-split weight banks of the fp16x3 implicit GEMM (conv_igemm.hip, ConvArgs::wbank): the weight operand of the stride-2 layers is
scaled by 2^12, clamped and split into hi / lo fp16 halves ONCE per step, into the kernel's LDS row image (ig_bank_unit, a job of
the fp16x3 bank launch), and the kernel copies 16 bytes per thread where it used to split the panel in every workgroup.  Same
arithmetic, same layout: every product is bit-identical, so forward, dgrad and the whole model must equal the split-while-staging
form bit for bit (uwm_op_set_igemm_f16x3(2) on the operators; UWM_DEBUG=1 UWM_NO_IG_BANK=1, read once per process, on the model)."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, cin, cout, h, w, k, pad): forward Kpad / dgrad KpadD = 288 / 576, 64 / 32, 96 / 96 — both remainders of 64 on either side
OPS = [(1, 32, 64, 10, 10, 3, 1), (1, 64, 32, 8, 8, 1, 0), (1, 96, 96, 12, 8, 1, 0)]


@pytest.mark.parametrize("n,cin,cout,h,w,k,pad", OPS, ids=[f"{k}x{k}s2-{ci}to{co}-{h}x{w}" for _, ci, co, h, w, k, _p in OPS])
def test_banked_operand_is_bit_identical_to_the_staged_split(cuda, n, cin, cout, h, w, k, pad):
    import ctypes as C
    from tests.util import P, nhwc, pack_w, rup, src, stream
    from unet_watermark_amd import _lib as L
    g = torch.Generator().manual_seed(77 + cin)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    wt[0, 0] = 30.0                                           # beyond the 2^12 scale's fp16 range: the clamp is part of the image
    sc = torch.rand(cin, generator=g) + 0.5; sh = torch.randn(cin, generator=g) * 0.2
    ho, wo = (h + 2 * pad - k) // 2 + 1, (w + 2 * pad - k) // 2 + 1
    xd, scd, shd = nhwc(x).to(cuda), sc.to(cuda), sh.to(cuda)
    wp, kpad = pack_w(wt)
    wp = wp.to(cuda)
    kpadd = rup(k * k * cout, 32)
    assert kpad % 64 != 0 or kpadd % 64 != 0
    wd = torch.empty(cin, kpadd, device=cuda)
    L.check(L.lib().uwm_op_pack_dgrad(P(wp), cout, kpad, k * k, cin, P(wd), kpadd, cout, stream()))
    dy = (torch.randn(n, ho, wo, cout, generator=g) * 1e-6).to(cuda)
    addend = (torch.randn(n, h, w, cin, generator=g) * 1e-6).to(cuda)
    mask = torch.randn(n, h, w, cin, generator=g).to(cuda)
    got = {}
    for on in (2, 1):                                          # 2: split while staging; 1: through the bank
        L.lib().uwm_op_set_igemm_f16x3(on)
        try:
            y = torch.full((n, ho, wo, cout), float("nan"), device=cuda)
            stats = torch.zeros(2 * cout, dtype=torch.float64, device=cuda)
            s0 = src(xd, scd, shd, relu=1)
            L.check(L.lib().uwm_op_conv(C.byref(s0), None, P(wp), cout, kpad, k, k, 2, pad, n, cout, None, P(y), P(stats), -1, stream()))
            dx = torch.full((n, h, w, cin), float("nan"), device=cuda)
            L.check(L.lib().uwm_op_dgrad(P(dy), n, ho, wo, cout, P(wd), cin, kpadd, k, k, 2, pad, h, w, P(addend), P(mask), None, None,
                                         P(dx), stream()))
            torch.cuda.synchronize()
        finally:
            L.lib().uwm_op_set_igemm_f16x3(0)
        got[on] = (y.cpu(), dx.cpu())
    assert torch.isfinite(got[1][0]).all() and torch.isfinite(got[1][1]).all()
    assert float(got[1][0].abs().max()) > 0 and float(got[1][1].abs().max()) > 0
    assert torch.equal(got[1][0], got[2][0]), float((got[1][0] - got[2][0]).abs().max())
    assert torch.equal(got[1][1], got[2][1]), float((got[1][1] - got[2][1]).abs().max())


def _model_run():
    """Small resnet34 Unet, 64 x 64, batch 2, f16x3_all: logits, every gradient, and the eval logits of the frozen model."""
    import unet_watermark_amd as U
    from oracle import unet_oracle as O
    from tests.test_model_gpu import _pair
    cuda = torch.device("cuda:0")
    m, _ = _pair("resnet34", dev=cuda)
    x, t = O.synthetic_batch(2, 64, 64, seed=11)
    crit = U.CombinedLoss([U.BCEWithLogitsLoss(), U.DiceLoss(smooth=1e-5)], [0.5, 0.5])
    m.train()
    m.set_precision("f16x3_all", min_workgroups=1)
    out = m(x.to(cuda))
    crit(out, t.unsqueeze(1).to(cuda)).backward()
    torch.cuda.synchronize()
    grads = m.flat_grads().clone()
    m.eval()
    with torch.no_grad():
        ev = m(x.to(cuda)).clone()
        m.freeze(batch_shape=(2, 64, 64))
        p0 = m.prep_launches()
        fz = m(x.to(cuda)).clone()
        frozen_prep = m.prep_launches() - p0
    return out.detach().cpu(), grads.cpu(), ev.cpu(), fz.cpu(), frozen_prep


def test_model_through_the_banks_equals_the_unbanked_build(cuda, tmp_path):
    out, grads, ev, fz, frozen_prep = _model_run()
    assert frozen_prep == 0                                    # the banks sit in the frozen arena: no bank kernel per call
    assert torch.equal(ev, fz)
    ref = tmp_path / "unbanked.pt"
    env = dict(os.environ, UWM_DEBUG="1", UWM_NO_IG_BANK="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, os.path.abspath(__file__), str(ref)], check=True, cwd=ROOT, env=env, timeout=300)
    base = torch.load(ref)
    assert torch.equal(out, base["out"]), float((out - base["out"]).abs().max())
    assert torch.equal(grads, base["grads"]), float((grads - base["grads"]).abs().max())
    assert torch.equal(fz, base["fz"])


if __name__ == "__main__":          # the unbanked build's tensors (environment set by the test above)
    o_, g_, e_, f_, _n = _model_run()
    torch.save({"out": o_, "grads": g_, "ev": e_, "fz": f_}, sys.argv[1])
