"""The fp16x3 backward's range-scaling contract, tested where unscaled fp16 would fail.

Every fp16x3 data or weight gradient splits dY into fp16 hi / lo halves after multiplying it by 2^(14-e), e the exponent of
max|dY|; it reads that maximum from the 32 "xmax" floats of the layer's BatchNorm, which the BatchNorm backward that produced
dY writes (bn_bwd_apply_kernel, bn_bwd_apply_act_kernel).  A consumer whose slot nobody wrote falls back to scale 1 without
a word: dY loses mantissa below ~6e-5, flushes to zero below ~6e-8 and overflows above 65504.  The oracle-parity tests run at
gradient magnitudes where that still passes, and the op tests hand each kernel a correct xmax of their own.

So here: (1) for one fixed forward the backward is linear in dlogits, and with correct range scaling a power-of-two factor s
on dlogits multiplies every gradient by EXACTLY s in every precision mode (exact fp32; split bf16, which has fp32's exponent
range; fp16x3 / fp16x3_bwd2 / fp16x1, whose staged value dY * 2^(14-e) does not depend on s).  Only run-to-run reordering of
atomics departs from it, and that is measured per case.  (2) EfficientNet-b4 and resnet50 in f16x3_all against the CPU oracle
with dlogits at the magnitude of the benched 4 x 1024^2 step (~2e-7)."""
import pytest
import torch

from tests.test_model_gpu import LOGIT_TOL, _effb4_grad_check, _expect_f16x3_headline_routing, _grad_check, _pair

pytestmark = pytest.mark.gpu

SCALES = (2.0 ** -30, 2.0 ** -10, 2.0 ** 10, 2.0 ** 30)
MODES = ["f32", "bf16x3_all", "f16x3", "f16x3_all", "f16x3_bwd2", "f16x1"]
F16_BWD = ("f16x3_all", "f16x3_bwd2", "f16x1")          # the modes whose backward runs fp16x3 (or fp16) dgrads and wgrads
MODELS = [("Unet", "resnet18", 4, 128, 160), ("Unet", "resnet34", 2, 256, 192), ("UnetPlusPlus", "resnet34", 2, 128, 192),
          ("Unet", "resnet50", 4, 128, 160), ("Unet", "efficientnet-b4", 4, 128, 128)]
CASES = [(arch, enc, n, h, w, mode, 0) for arch, enc, n, h, w in MODELS for mode in MODES]
CASES.append(("Unet", "resnet34", 2, 512, 512, "f16x3_all", 16))      # the headline step's exact kernel routing
CASES.append(("Unet", "resnet50", 4, 128, 160, "f16x3_all", 16))      # kernels chosen as for 16 images: the 1x1 dgrads on conv_gemm
STAGED = {("Unet", "efficientnet-b4", "f16x3_all"), ("Unet", "resnet34", "f16x3_all")}      # + the backward one stage at a time


# backward kernels of the fp16x3 forms.  The implicit-GEMM / 1x1-GEMM kernels carry the F16 form as their last template
# argument: the routing record names it "<..., true>"
_F16_NAMES = ("conv_f16x3", "conv_up2_dgrad_f16", "conv_c16_f16", "conv_c32_f16", "wgrad_f16x3", "wgrad_stem_f16",
              "wgrad_c16_f16", "wgrad_up2_f16")


def _is_f16(kern):
    return kern.startswith(_F16_NAMES) or (kern.startswith(("conv_igemm_kernel", "conv_gemm_kernel", "wgrad_igemm_kernel"))
                                           and kern.endswith(", true>"))


def _expect_f16_backward(m, arch, enc, rb, rec):
    """Non-vacuity: the backward of this case really ran on the fp16x3 forms this file is about (explicit per case; together
    the cases cover every fp16x3 dgrad and wgrad kernel)."""
    by = {}
    for pas, layer, kern in rec:
        if pas != "fwd":
            by.setdefault(pas, {}).setdefault(layer, set()).add(kern)

    def has(pas, pred, layer=None):
        ks = [k for l_, s in by.get(pas, {}).items() if layer is None or l_ == layer for k in s]
        assert any(pred(k) for k in ks), (pas, layer, sorted(set(ks)))

    def name(prefix):
        return lambda k: k.startswith(prefix)

    def f16(prefix):
        return lambda k: k.startswith(prefix) and _is_f16(k)

    has("dgrad", name("conv_f16x3"))
    has("wgrad", name("wgrad_f16x3"))
    if enc.startswith("resnet"):
        has("dgrad", f16("conv_igemm_kernel"))                     # stride-2 3x3 and 1x1 downsample layers
        has("wgrad", f16("wgrad_igemm_kernel"))
    if enc == "resnet34":
        has("wgrad", name("wgrad_stem_f16"), "encoder.conv1")      # (the 160-pixel-wide cases keep it on the fp32 implicit GEMM)
    if enc == "resnet50":
        for layer in ("encoder.layer1.0.conv1", "encoder.layer1.0.conv3", "encoder.layer3.2.conv3"):      # Bottleneck 1x1 / stride 1
            has("dgrad", _is_f16, layer)
        if rb == 16:
            has("dgrad", f16("conv_gemm_kernel"))                  # (large launches only: conv_gemm_preferred)
    if arch == "Unet" and enc == "resnet34":                       # (the 160-pixel-wide cases route decoder block 4 otherwise)
        has("dgrad", name("conv_up2_dgrad_f16"), "decoder.blocks.4.conv1.0")
        has("wgrad", name("wgrad_up2_f16"), "decoder.blocks.4.conv1.0")
        has("dgrad", name("conv_c16_f16"), "decoder.blocks.4.conv2.0")
        has("wgrad", name("wgrad_c16_f16"), "decoder.blocks.4.conv2.0")
    if enc == "efficientnet-b4":
        # the MBConv expand convs with channels % 32 == 0 (1x1 / stride 1): their dY comes out of the swish BatchNorm backward.
        # Every dgrad runs on an fp16x3 GEMM form; the weight gradient on wgrad_igemm's fp16x3 form (the 448-channel blocks at
        # 4 x 4 pixels) or on wgrad_gemm (exact fp32, no fp16x3 form: it ignores the slot)
        n, wg16 = 0, 0
        for pname, kind, arena, off, shp, strd in m._infos:
            if arena == 0 and pname.endswith("_expand_conv.weight") and shp[1] % 32 == 0:
                layer = pname[: -len(".weight")]
                has("dgrad", _is_f16, layer)
                has("wgrad", lambda k: _is_f16(k) or k.startswith("wgrad_gemm_kernel"), layer)
                wg16 += any(_is_f16(k) for k in by["wgrad"].get(layer, ()))
                n += 1
        assert n >= 10 and wg16 >= 1, (n, wg16)


def _param_grads(m, flat):
    return {name: flat.as_strided(shp, strd, off).double() for name, kind, arena, off, shp, strd in m._infos if arena == 0}


def _norms_of(g1):
    """||g1|| per tensor; EfficientNet's `_blocks.*._bn2.bias` gradients are rounding noise around zero (_effb4_grad_check):
    they are held against their `_bn2.weight` partner's norm."""
    out = {}
    for name, v in g1.items():
        ref = g1[name[:-4] + "weight"] if (name.endswith("_bn2.bias") and "_blocks" in name) else v
        out[name] = float(ref.norm())
    return out


@pytest.mark.parametrize("arch,enc,n,h,w,mode,rb", CASES,
                         ids=[f"{a}-{e}-{n}x{h}x{w}-{md}" + (f"-rb{rb}" if rb else "") for a, e, n, h, w, md, rb in CASES])
def test_backward_is_scale_equivariant(cuda, arch, enc, n, h, w, mode, rb):
    """g(s * dlogits) == s * g(dlogits) per parameter tensor, s in {2^-30, 2^-10, 2^10, 2^30}, within 4x the run-to-run
    noise of two unscaled backwards over the same forward (+1e-6).  A missing, stale or wrong max|dY| slot breaks this by
    orders of magnitude more (at s = 2^-30 an unscaled fp16 dY flushes to zero).

    Range: dlogits = randn * 2^-17 in channel 0, so s * dlogits stays within 2^-52 .. 2^16 in magnitude, and the gradients of
    these nets stay within 2^+-40 of it (BatchNorm 1/sigma factors, sums over <= 2^18 pixels): between 2^-92 and 2^56, inside
    fp32's normal range (2^-126 .. 2^128) and fp64's; fp32 can neither underflow nor overflow at these extremes, and the test
    checks that every scaled gradient is finite and that a non-zero tensor stays non-zero."""
    from oracle import unet_oracle as O
    m, _ = _pair(enc, seed=3 if enc == "efficientnet-b4" else 42, dev=cuda, arch=arch)
    m.drop_connect = False
    m.set_precision(mode, min_workgroups=0 if rb else 1, routing_batch=rb)      # (the headline case: bench.py's own fill rule)
    m.routing(enable=True)
    m.train()
    x, _ = O.synthetic_batch(n, h, w, seed=5)
    logits = m._forward_raw(x.to(cuda), training=True)
    dl = torch.zeros_like(logits)
    dl[..., 0] = torch.randn(logits.shape[:-1], device=cuda, generator=torch.Generator(device="cuda").manual_seed(6)) * 2.0 ** -17

    staged = (arch, enc, mode) in STAGED

    def backward(d, by_stage=False):
        if by_stage:
            for k in range(len(m.stages)):
                m._backward_raw(d, k, k + 1)
        else:
            m._backward_raw(d)
        torch.cuda.synchronize()
        return _param_grads(m, m.flat_grads().clone())

    g1 = backward(dl)
    g1b = backward(dl)
    norms = _norms_of(g1)
    noise = {k: (float((g1b[k] - v).norm()) / norms[k] if norms[k] > 0 else 0.0) for k, v in g1.items()}
    runs = [(s, False, g1) for s in SCALES]
    if staged:
        g1s = backward(dl, True)
        runs += [(s, True, g1s) for s in SCALES]
    worst_e, worst = 0.0, None
    for s, by_stage, base in runs:
        gs = backward(dl * s, by_stage)
        for k, v in base.items():
            t = gs[k]
            assert torch.isfinite(t).all(), f"{k}: non-finite gradient at s = {s:g}"
            if norms[k] == 0:
                assert float(t.abs().max()) == 0, f"{k}: zero at s = 1, non-zero at s = {s:g}"
                continue
            assert float(t.abs().max()) > 0 or float(v.abs().max()) == 0, f"{k}: all zero at s = {s:g}"
            e = float((t / s - v).norm()) / norms[k]
            n_t = noise[k]
            if e > worst_e:
                worst_e, worst = e, (k, s, by_stage)
            assert e <= 4 * n_t + 1e-6, (f"{k}: s = {s:g}{' (staged)' if by_stage else ''}: ||g_s/s - g_1|| / ||g_1|| = {e:.3e}, "
                                         f"run-to-run noise n_t = {n_t:.3e}")
    print(f"\n[grad-scale] {arch}-{enc} {n}x{h}x{w} {mode}{' rb' + str(rb) if rb else ''}: max n_t {max(noise.values()):.3e} "
          f"({max(noise, key=noise.get)}), max e_t {worst_e:.3e} ({worst})")
    if rb == 16 and enc == "resnet34":
        m._forward_raw(x.to(cuda), training=True)          # (the headline expectations count the two forwards of the bs16 test's record)
    rec = m.routing()
    m.routing(enable=False)
    if mode in F16_BWD:
        _expect_f16_backward(m, arch, enc, rb, rec)
        if rb == 16 and enc == "resnet34":
            _expect_f16x3_headline_routing(rec)
    else:
        assert not any(_is_f16(k) for p_, l_, k in rec if p_ != "fwd"), mode       # the fp32-backward modes stay off them


@pytest.mark.parametrize("arch,enc,n,h,w", [("Unet", "efficientnet-b4", 4, 128, 128), ("Unet", "resnet50", 4, 128, 160)])
def test_f16x3_all_gradients_at_full_size_magnitudes(cuda, arch, enc, n, h, w):
    """f16x3_all against the CPU oracle with dlogits at the magnitude of the benched 4 x 1024^2 step: the loss gradient is taken
    times 2^-6 (dlogits ~2e-7 instead of ~1e-5 at 4 x 128^2), the model's gradients times 2^6 are held against the oracle's
    under the oracle-parity bars of these encoders (test_efficientnet_b4_encoder_parity, test_resnet50_bottleneck_encoder_parity).
    The oracle is linear in its loss gradient: one oracle run serves.  resnet50 covers the Bottleneck 1x1 layers' fp16x3 forms;
    EfficientNet-b4 the MBConv expand convs, whose dY comes out of the swish BatchNorm backward."""
    import unet_watermark_amd as U
    from oracle import unet_oracle as O
    effb4 = enc == "efficientnet-b4"
    m, ref = _pair(enc, seed=3 if effb4 else 42, dev=cuda, arch=arch)
    m.drop_connect = False
    x, t = O.synthetic_batch(n, h, w, seed=13)
    m.train(); ref.train()
    crit_ref = O.CombinedLoss([O.BCEWithLogits(), O.DiceLoss(smooth=1e-5)], [0.5, 0.5])
    crit = U.CombinedLoss([U.BCEWithLogitsLoss(), U.DiceLoss(smooth=1e-5)], [0.5, 0.5])
    out_ref = ref(x); loss_ref = crit_ref(out_ref, t.unsqueeze(1)); loss_ref.backward()
    m.set_precision("f16x3_all", min_workgroups=1)
    out = m(x.to(cuda))
    dmax = []
    out.register_hook(lambda g: dmax.append(float(g.abs().max())))
    loss = crit(out, t.unsqueeze(1).to(cuda))
    (loss * 2.0 ** -6).backward()
    assert dmax and dmax[0] < 2e-6, dmax            # dlogits really at the full-size magnitude
    assert float((out.detach().cpu() - out_ref.detach()).abs().max()) < LOGIT_TOL
    assert abs(loss.item() - loss_ref.item()) < 1e-5
    with torch.no_grad():
        for p in m.parameters():
            p.grad.mul_(2.0 ** 6)
    if effb4:
        _effb4_grad_check(m, ref)
    else:
        _grad_check(m, ref, l2_rel=7e-2, cos_min=0.9975)
    m.set_precision("f32", min_workgroups=0)
