"""The EfficientNet-b0..b7 encoders against the CPU reference of tests/effnet_family_ref.py, fused AdamW against
torch.optim.AdamW, and the text-watermark recipe (UnetPlusPlus-b3, CombinedLoss, AdamW, CosineAnnealingWarmRestarts, gradient
clipping) end to end."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import effnet_family_ref as R
from tests.test_grad_scale_gpu import _is_f16
from tests.test_model_gpu import LOGIT_TOL, _effb4_grad_check

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fpair(enc, seed, dev, arch="Unet"):
    import unet_watermark_amd as U
    ref = R.build(enc, seed=seed, arch=arch)
    m = getattr(U, arch)(enc).to(dev)
    m.load_state_dict(ref.state_dict())
    return m, ref


def _crits():
    import unet_watermark_amd as U
    from oracle import unet_oracle as O
    return (U.CombinedLoss([U.BCEWithLogitsLoss(), U.DiceLoss(smooth=1e-5)], [0.5, 0.5]),
            O.CombinedLoss([O.BCEWithLogits(), O.DiceLoss(smooth=1e-5)], [0.5, 0.5]))


@pytest.mark.parametrize("mode", ["default", "f16x3_all"])
@pytest.mark.parametrize("arch,n,h,w,drop", [("Unet", 4, 128, 128, True), ("UnetPlusPlus", 2, 128, 160, True)])
def test_efficientnet_b3_parity(cuda, arch, n, h, w, drop, mode):
    """Unet / UnetPlusPlus over EfficientNet-b3 (the text-watermark encoder): train forward with drop-connect masks, loss,
    every gradient, running statistics, eval forward — the bars of test_efficientnet_b4_encoder_parity."""
    from oracle import unet_oracle as O
    m, ref = _fpair("efficientnet-b3", 3, cuda, arch)
    if mode != "default":
        m.set_precision(mode, min_workgroups=1)
    x, t = O.synthetic_batch(n, h, w, seed=13)
    nb = len(ref.encoder._blocks)
    assert nb == 26
    keep = (torch.rand(nb, n, generator=torch.Generator().manual_seed(1)) > 0.3).float()
    m.train(); ref.train()
    m.drop_connect = drop
    m._keep_override = keep if drop else None
    crit, crit_ref = _crits()
    out_ref = ref(x, [keep[i] for i in range(nb)] if drop else None)
    loss_ref = crit_ref(out_ref, t.unsqueeze(1)); loss_ref.backward()
    out = m(x.to(cuda)); loss = crit(out, t.unsqueeze(1).to(cuda)); loss.backward()
    assert (out.detach().cpu() - out_ref.detach()).abs().max() < LOGIT_TOL
    assert abs(loss.item() - loss_ref.item()) < 1e-5
    _effb4_grad_check(m, ref)
    bref = dict(ref.named_buffers())
    for k, b in m.named_buffers():
        assert (b.detach().cpu().double() - bref[k].double()).abs().max() < 1e-4, k
    m.eval(); ref.eval()
    with torch.no_grad():
        assert (m(x.to(cuda)).cpu() - ref(x)).abs().max() < LOGIT_TOL


@pytest.mark.parametrize("enc", ["efficientnet-b0", "efficientnet-b1", "efficientnet-b2", "efficientnet-b5", "efficientnet-b6",
                                 "efficientnet-b7"])
def test_efficientnet_variant_train_step(cuda, enc):
    """One Unet train step at 2 x 3 x 64 x 64 per remaining variant: forward and every gradient.  b2 / b5 / b7 carry the
    stride-2 k-3 depthwise with pad (1, 1); b7 the widest mids (3840).

    The deep variants at this size sit at the noise floor of the fp32 bars: with 2 x 2 x 2 values per deepest BatchNorm, the
    reference's own fp32 gradients are up to 3.3 % (relative L2) from an fp64 run of the same net (b6, _blocks.3._se_reduce).
    So both runs are held against the fp64 reference: every gradient of ours within max(3e-2, 2 x torch fp32's own error) of it
    (the `_bn2.bias` gradients of the blocks measured against their `_bn2.weight` partner, as in _effb4_grad_check)."""
    from oracle import unet_oracle as O
    m, ref = _fpair(enc, 4, cuda)
    m.drop_connect = False
    x, t = O.synthetic_batch(2, 64, 64, seed=7)
    m.train(); ref.train()
    crit, crit_ref = _crits()
    out_ref = ref(x); loss_ref = crit_ref(out_ref, t.unsqueeze(1)); loss_ref.backward()
    g32 = {n: p.grad.double() for n, p in ref.named_parameters()}
    ref.zero_grad(set_to_none=True)
    ref = ref.double()
    out64 = ref(x.double()); loss64 = crit_ref(out64, t.unsqueeze(1)); loss64.backward()
    out = m(x.to(cuda)); loss = crit(out, t.unsqueeze(1).to(cuda)); loss.backward()
    assert float((out.detach().cpu().double() - out64.detach()).abs().max()) < LOGIT_TOL
    assert abs(loss.item() - loss64.item()) < 1e-5
    g64 = {n: p.grad for n, p in ref.named_parameters()}
    worst = (0.0, None)
    for n, p in m.named_parameters():
        g, r = p.grad.detach().cpu().double(), g64[n]
        scale = g64[n[:-4] + "weight"].norm() if (n.endswith("_bn2.bias") and "_blocks" in n) else r.norm()
        if scale == 0:
            assert g.norm() == 0, n
            continue
        e, e32 = float((g - r).norm() / scale), float((g32[n] - r).norm() / scale)
        worst = max(worst, (e, n))
        assert e <= max(3e-2, 2 * e32), f"{n}: relative L2 error {e} (torch fp32: {e32})"
    print(f"\n[{enc}] worst gradient error vs fp64 {worst[0]:.3e} ({worst[1]})")


def test_efficientnet_b3_f16x3_all_at_full_size_magnitudes(cuda):
    """f16x3_all with dlogits at the 4 x 1024^2 magnitude (as test_f16x3_all_gradients_at_full_size_magnitudes does for b4):
    the gradients times 2^6 hold the oracle-parity bars, and the expand convs with whole 32-channel chunks run their dgrads on
    an fp16x3 GEMM form (range-scaled: a form without a max|dY| producer fails the backward) and their wgrads on wgrad_igemm's
    fp16x3 form or on the exact wgrad_gemm."""
    from oracle import unet_oracle as O
    m, ref = _fpair("efficientnet-b3", 3, cuda)
    m.drop_connect = False
    x, t = O.synthetic_batch(4, 128, 128, seed=13)
    m.train(); ref.train()
    crit, crit_ref = _crits()
    out_ref = ref(x); loss_ref = crit_ref(out_ref, t.unsqueeze(1)); loss_ref.backward()
    m.set_precision("f16x3_all", min_workgroups=1)
    m.routing(enable=True)
    out = m(x.to(cuda))
    dmax = []
    out.register_hook(lambda g: dmax.append(float(g.abs().max())))
    loss = crit(out, t.unsqueeze(1).to(cuda))
    (loss * 2.0 ** -6).backward()
    rec = m.routing()
    m.routing(enable=False)
    assert dmax and dmax[0] < 2e-6, dmax
    assert float((out.detach().cpu() - out_ref.detach()).abs().max()) < LOGIT_TOL
    with torch.no_grad():
        for p in m.parameters():
            p.grad.mul_(2.0 ** 6)
    _effb4_grad_check(m, ref)
    by = {}
    for pas, layer, kern in rec:
        if pas != "fwd":
            by.setdefault(pas, {}).setdefault(layer, set()).add(kern)
    n, wg16 = 0, 0
    for pname, kind, arena, off, shp, strd in m._infos:
        if arena == 0 and pname.endswith("_expand_conv.weight") and shp[1] % 32 == 0:
            layer = pname[: -len(".weight")]
            assert any(_is_f16(k) for k in by["dgrad"].get(layer, ())), (layer, by["dgrad"].get(layer))
            assert all(_is_f16(k) or k.startswith("wgrad_gemm_kernel") for k in by["wgrad"].get(layer, ())), by["wgrad"].get(layer)
            assert by["wgrad"].get(layer)
            wg16 += any(_is_f16(k) for k in by["wgrad"][layer])
            n += 1
    assert n == 9 and wg16 >= 1, (n, wg16)
    m.set_precision("f32", min_workgroups=0)


def test_efficientnet_b3_unetplusplus_recipe_size_eval(cuda):
    """UnetPlusPlus-b3 at the recipe's 512 x 512: eval logits within 1e-3 of the reference in f32 and in f16x3_all."""
    m, ref = _fpair("efficientnet-b3", 5, cuda, "UnetPlusPlus")
    x = torch.randn(1, 3, 512, 512, generator=torch.Generator().manual_seed(2))
    m.eval(); ref.eval()
    with torch.no_grad():
        r = ref(x)
        for mode in ("f32", "f16x3_all"):
            m.set_precision(mode)
            d = float((m(x.to(cuda)).cpu() - r).abs().max())
            assert d < 1e-3, (mode, d)
    m.set_precision("f32")


# ------------------------------------------------------------------------------ AdamW
def _adamw_call(fn, p, gd, mm, vv, n, lr, wd, step, gscale, clip=None, scr=None):
    from unet_watermark_amd import _lib as L
    args = [C.c_void_p(p.data_ptr()), C.c_void_p(gd.data_ptr()), C.c_void_p(mm.data_ptr()), C.c_void_p(vv.data_ptr()), n, lr,
            0.9, 0.999, 1e-8, wd, step, gscale]
    if clip:
        args += [clip, C.c_void_p(scr.data_ptr())]
    L.check(getattr(L.lib(), fn)(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream)))


@pytest.mark.parametrize("n", [100003, 4097 * 3 + 2])
@pytest.mark.parametrize("wd", [1e-4, 1e-2])
@pytest.mark.parametrize("clip", [None, 1.0])
def test_adamw_kernel_matches_torch_optim(cuda, n, wd, clip):
    """uwm_adamw / uwm_adamw_clip == torch.optim.AdamW (decoupled weight decay) over 3 steps with a gradient scale != 1."""
    g = torch.Generator().manual_seed(0)
    gscale = 0.5
    p0 = torch.randn(n, generator=g)
    pr = p0.clone().requires_grad_()
    opt = torch.optim.AdamW([pr], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    p = p0.to(cuda); mm = torch.zeros_like(p); vv = torch.zeros_like(p)
    scr = torch.zeros(2, dtype=torch.float64, device=cuda)
    for step in range(1, 4):
        gr = torch.randn(n, generator=g) * 10 ** float(torch.randint(-4, 1, (), generator=g))
        pr.grad = gr.clone() * gscale
        if clip:
            torch.nn.utils.clip_grad_norm_([pr], clip)
        opt.step()
        _adamw_call("uwm_adamw_clip" if clip else "uwm_adamw", p, gr.to(cuda), mm, vv, n, 1e-3, wd, step, gscale, clip, scr)
        assert (p.cpu() - pr.detach()).abs().max() < 2e-6, step
    st = opt.state[pr]
    # (the kernel forms 1 - beta2 in fp32 from the fp32 beta2, as uwm_adam does: 0.999f leaves 1.3e-5 relative in exp_avg_sq)
    for ours, theirs in ((mm, st["exp_avg"]), (vv, st["exp_avg_sq"])):
        assert float((ours.cpu() - theirs).abs().max()) <= 3e-5 * float(theirs.abs().max())


@pytest.mark.parametrize("clip", [False, True])
def test_adamw_graph_replay_equals_eager(cuda, clip):
    """uwm_adamw_graph captured once and replayed three times == three direct calls, bit for bit (hyper-parameters and the
    step counter in device memory), and both follow torch.optim.AdamW."""
    from unet_watermark_amd import _lib as L
    n = 50001
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * 0.1 for _ in range(3)]
    hyper = [1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.5, 0.7 if clip else 0.0, 0.0, 0.0, 0.0]

    def state():
        return (p0.to(cuda), torch.zeros(n, device=cuda), torch.zeros(n, device=cuda), torch.tensor(hyper, device=cuda),
                torch.zeros(2, dtype=torch.float64, device=cuda) if clip else None)

    def call(p, gd, mm, vv, hy, scr):
        L.check(L.lib().uwm_adamw_graph(C.c_void_p(p.data_ptr()), C.c_void_p(gd.data_ptr()), C.c_void_p(mm.data_ptr()),
                                        C.c_void_p(vv.data_ptr()), n, C.c_void_p(hy.data_ptr()),
                                        C.c_void_p(scr.data_ptr()) if scr is not None else None,
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    a = state()
    ga = torch.zeros(n, device=cuda)
    for gr in grads:
        ga.copy_(gr.to(cuda)); call(a[0], ga, a[1], a[2], a[3], a[4])
    b = state()
    gb = torch.zeros(n, device=cuda)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        call(b[0], gb, b[1], b[2], b[3], b[4])
    torch.cuda.synchronize()
    assert torch.equal(b[0].cpu(), p0) and float(b[3][7]) == 0.0        # capture alone runs nothing
    for gr in grads:
        gb.copy_(gr.to(cuda)); graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    assert float(b[3][7]) == 3.0
    pr = p0.clone().requires_grad_()
    opt = torch.optim.AdamW([pr], lr=1e-3, weight_decay=1e-2)
    for gr in grads:
        pr.grad = gr * 0.5
        if clip:
            torch.nn.utils.clip_grad_norm_([pr], 0.7)
        opt.step()
    assert (a[0].cpu() - pr.detach()).abs().max() < 2e-6


def test_trainer_adamw_graph_matches_eager(cuda):
    """Trainer(optimizer="AdamW", use_graph=True) follows the eager AdamW trainer over 3 steps (the bars of
    test_trainer_hipgraph_step_matches_eager), and the eager AdamW step differs from Adam's (the decay is decoupled)."""
    import unet_watermark_amd as U
    from unet_watermark_amd.train import FusedAdamW, Trainer
    from oracle import unet_oracle as O
    torch.manual_seed(3)
    a = U.Unet("resnet18").to(cuda)
    b = U.Unet("resnet18").to(cuda)
    c = U.Unet("resnet18").to(cuda)
    b.load_state_dict(a.state_dict()); c.load_state_dict(a.state_dict())
    kw = dict(w_dice=0.5, w_bce=0.5, lr=1e-3, adam_eps=1e-2, weight_decay=0.5, max_grad_norm=0.5)
    ta = Trainer(a, optimizer="AdamW", **kw)
    tb = Trainer(b, optimizer="AdamW", use_graph=True, **kw)
    tc = Trainer(c, optimizer="Adam", **kw)
    assert isinstance(ta.opt, FusedAdamW) and isinstance(tb.opt, FusedAdamW)
    for k in range(3):
        x, t = O.synthetic_batch(4, 64, 96, seed=20 + k)
        la = ta.step(x.to(cuda), t.to(cuda)).clone()
        lb = tb.step(x.to(cuda), t.to(cuda)).clone()
        tc.step(x.to(cuda), t.to(cuda))
        assert torch.allclose(la, lb, rtol=0, atol=5e-4), (k, la, lb)
    assert tb.opt._step == ta.opt._step == 3 and len(tb._graphs) == 1
    assert float((a.flat_parameters() - b.flat_parameters()).abs().max()) < 2e-3
    assert float((a.flat_parameters() - c.flat_parameters()).abs().max()) > 1e-4


# ------------------------------------------------------------------------------ the text-watermark recipe
TEXT_CONFIG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unet_text_watermark.yaml")


def _train(args, cwd):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "train"] + args, cwd=cwd, capture_output=True, text=True,
                       timeout=400)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{") and '"epoch"' in l]


def test_text_watermark_recipe_end_to_end(cuda, tmp_path):
    """main.py train --config <the text-watermark config>: UnetPlusPlus-b3, CombinedLoss (Dice 0.5, BCE 0.3), AdamW, warm
    restarts and --grad-clip.  Exits 0, the loss falls, the checkpoint names efficientnet-b3, the per-epoch LRs are torch's
    CosineAnnealingWarmRestarts sequence (here T_0 = 1, T_mult = 2: a restart inside the run), and a resume continues it."""
    from unet_watermark_amd.config import get_cfg_defaults, update_config
    cfg_text = open(TEXT_CONFIG, encoding="utf-8").read()
    assert cfg_text.count("SCHEDULER_T_0: 50 ") == 1
    cfg_text = cfg_text.replace("SCHEDULER_T_0: 50 ", "SCHEDULER_T_0: 1 ")
    cfg_path = tmp_path / "text.yaml"
    cfg_path.write_text(cfg_text, encoding="utf-8")
    cfg = update_config(get_cfg_defaults(), str(cfg_path))
    assert cfg.MODEL.ENCODER_NAME == "efficientnet-b3" and cfg.OPTIMIZER.NAME == "AdamW" and cfg.OPTIMIZER.SCHEDULER_T_0 == 1
    common = ["--config", str(cfg_path), "--synthetic", "16", "--img-size", "64", "--grad-clip", "--workers", "0",
              "--no-early-stopping", "--model-save-path", str(tmp_path / "text.pth"), "--checkpoint-dir", str(tmp_path / "ck")]
    hist = _train(common + ["--epochs", "3"], tmp_path)
    assert len(hist) == 3 and hist[-1]["train_loss"] < hist[0]["train_loss"], hist
    ref = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(
        torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=float(cfg.TRAIN.LR)), T_0=1, T_mult=2,
        eta_min=float(cfg.OPTIMIZER.SCHEDULER_ETA_MIN))
    want = []
    for _ in range(5):
        ref.step()
        want.append(ref.optimizer.param_groups[0]["lr"])
    assert [h["lr"] for h in hist] == pytest.approx(want[:3], rel=1e-12, abs=0), (hist, want)
    from unet_watermark_amd.checkpoint import load_checkpoint
    ck = load_checkpoint(str(tmp_path / "ck" / "checkpoint_epoch_003.pth"))
    assert ck["config"]["MODEL"]["ENCODER_NAME"] == "efficientnet-b3" and ck["config"]["MODEL"]["NAME"] == "UnetPlusPlus"
    assert "encoder._blocks.25._project_conv.weight" in ck["model_state_dict"]
    assert ck["scheduler_state_dict"]["T_0"] == 1 and "exp_avg" in ck["optimizer_state_dict"]["state"][0]
    assert ck["optimizer_state_dict"]["param_groups"][0]["weight_decay"] == pytest.approx(1e-4)
    more = _train(common + ["--epochs", "5", "--resume", str(tmp_path / "ck" / "checkpoint_epoch_003.pth")], tmp_path)
    assert [h["epoch"] for h in more] == [4, 5]
    assert [h["lr"] for h in more] == pytest.approx(want[3:], rel=1e-12, abs=0), (more, want)
