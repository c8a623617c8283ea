"""Frozen-weight inference on the device: model.freeze() / uwm_freeze make the eval forward's parameter-derived items (BatchNorm
scale / shift, forward filter banks, stem bank) once, into an arena; frozen forwards read it and launch no preparation kernel.
The acceptance criterion is bit-equality with the unfrozen eval forward — torch.equal everywhere, no tolerance.

Weights come from oracle.unet_oracle.build(..., seed=...) (efficientnet-b0, which that oracle does not build, from
tests/effnet_family_ref.build, the reference of its own tests); the running statistics are made representative by a few
train-mode forwards, as test_config5_bs64_512_hipgraph does."""
import ctypes as C

import pytest
import torch

from tests import effnet_family_ref as R
from tests.util import nhwc

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _lib():
    from unet_watermark_amd import _lib as L
    return L, L.lib()


def _model(arch, enc, dev, prec, seed=3, min_workgroups="pin"):
    import unet_watermark_amd as U
    from oracle import unet_oracle as O
    ref = R.build(enc, seed=seed, arch=arch) if enc.startswith("efficientnet") else O.build(enc, seed=seed, arch=arch)
    m = getattr(U, arch)(enc).to(dev)
    m.load_state_dict(ref.state_dict())
    m.drop_connect = False
    if min_workgroups == "pin":              # fp16x3: every eligible layer on the fp16x3 kernels, whatever the launch size
        min_workgroups = 1 if prec != "f32" else None
    m.set_precision(prec, min_workgroups=min_workgroups)
    return m


def _warm_stats(m, n, h, w, dev, seed=5):
    """representative running statistics (a fresh net's 0 / 1 do not normalise)"""
    from oracle import unet_oracle as O
    xs, _ = O.synthetic_batch(n, h, w, seed=seed)
    m.train()
    with torch.no_grad():
        for k in range(3):
            m(xs.to(dev) * (1.0 + 0.1 * k))
    m.eval()
    return m


def _x(n, h, w, dev, seed=9):
    return torch.randn(n, 3, h, w, generator=torch.Generator().manual_seed(seed)).to(dev)


def _names(L, m):
    bns = [n[:-len(".running_mean")] for n, kind, *_ in m._infos if kind == L.KIND_BN_MEAN]
    convs = [n[:-len(".weight")] for n, kind, *_ in m._infos if kind == L.KIND_CONV_W]
    return bns, convs


def _fwd_kernels(m):
    return {layer: kern for pas, layer, kern in m.routing() if pas == "fwd"}


CASES = [("Unet", "resnet18", 2, 128, 128), ("Unet", "resnet34", 2, 128, 128), ("Unet", "resnet50", 2, 128, 128),
         ("UnetPlusPlus", "resnet34", 2, 128, 128), ("Unet", "efficientnet-b0", 2, 64, 64)]


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("arch,enc,n,h,w", CASES)
def test_frozen_logits_equal_unfrozen_bitwise(cuda, arch, enc, n, h, w, prec):
    L, lib = _lib()
    m = _warm_stats(_model(arch, enc, cuda, prec), n, h, w, cuda)
    x = _x(n, h, w, cuda)
    with torch.no_grad():
        base = m(x).clone()
        m.routing(True)
        m(x)
        unfrozen_route = m.routing()
        m.freeze()
        assert m.frozen and not lib.uwm_is_frozen(m._h)          # batch_shape=None: the first forward fixes the forms
        out = m(x).clone()
        assert lib.uwm_is_frozen(m._h) and m.frozen_serves(n, h, w)
        m.routing()
        p0 = m.prep_launches()
        out2 = m(x).clone()
        assert m.prep_launches() == p0                           # served from the arena
        assert m.routing() == unfrozen_route                     # the same kernels, layer by layer
    assert torch.equal(out, base) and torch.equal(out2, base)
    assert bool(torch.isfinite(out).all())
    if prec == "f16x3" and enc.startswith("resnet"):
        assert any("f16x3" in k for p_, l_, k in unfrozen_route if p_ == "fwd"), sorted({k for _, _, k in unfrozen_route})


def test_frozen_resnet34_bs8_512_f16x3_banks(cuda):
    """The fp16x3 banks at the predictor's size: 8 x 3 x 512 x 512, f16x3 with the fill rule at 1.  The routing record of the
    FROZEN forward shows the fp16x3 forward kernels, so the cached banks are the fp16x3 ones."""
    m = _warm_stats(_model("Unet", "resnet34", cuda, "f16x3"), 4, 256, 256, cuda)
    x = _x(8, 512, 512, cuda)
    with torch.no_grad():
        base = m(x).clone()
        m.freeze(batch_shape=(8, 512, 512))
        m.routing(True)
        p0 = m.prep_launches()
        out = m(x).clone()
        assert m.prep_launches() == p0
        by = _fwd_kernels(m)
    assert torch.equal(out, base)
    for layer in ("encoder.layer1.0.conv1", "encoder.layer2.1.conv2", "encoder.layer3.2.conv1", "encoder.layer4.1.conv1",
                  "decoder.blocks.0.conv1.0", "decoder.blocks.2.conv2.0"):
        assert "conv_f16x3" in by[layer], (layer, by[layer])
    assert "conv_stem_f16x3" in by["encoder.conv1"], by["encoder.conv1"]
    assert sum(1 for k in by.values() if "conv_f16x3" in k) >= 30, sorted(by.items())


def test_cache_is_used_and_freeze_is_cheap(cuda):
    m = _warm_stats(_model("Unet", "resnet34", cuda, "f16x3"), 2, 128, 128, cuda)
    x = _x(2, 128, 128, cuda)
    with torch.no_grad():
        p0 = m.prep_launches()
        base = m(x).clone()
        per_forward = m.prep_launches() - p0
        assert per_forward >= 46                                 # one BatchNorm launch per layer + the bank builders
        p0 = m.prep_launches()
        m.freeze(batch_shape=(2, 128, 128))
        freeze_cost = m.prep_launches() - p0
        assert 0 < freeze_cost < per_forward, (freeze_cost, per_forward)       # bn_eval_multi: every BatchNorm in one launch
        assert freeze_cost <= 8, freeze_cost
        for _ in range(5):
            p = m.prep_launches()
            assert torch.equal(m(x), base)
            assert m.prep_launches() == p
        m.unfreeze()
        assert not m.frozen
        for _ in range(3):
            p = m.prep_launches()
            assert torch.equal(m(x), base)
            assert m.prep_launches() == p + per_forward


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_frozen_items_are_read_from_the_arena(cuda, prec):
    """NaN over exactly the workspace copies of what the arena replaces — every BatchNorm's scale / shift and every forward bank
    slot of the fixed region: the frozen logits do not change."""
    L, lib = _lib()
    m = _warm_stats(_model("Unet", "resnet34", cuda, prec), 2, 128, 128, cuda)
    x = _x(2, 128, 128, cuda)
    with torch.no_grad():
        base = m(x).clone()
        m.freeze()
        assert torch.equal(m(x), base)
        bns, convs = _names(L, m)
        poisoned = 0
        for key in ["bnf:" + b for b in bns] + ["wu:" + c for c in convs]:
            buf = m.debug_buffer(key)
            buf.fill_(float("nan"))
            poisoned += buf.numel()
        assert poisoned >= lib.uwm_frozen_bytes(m._h) // 4 - 64 * (len(convs) + 1)
        out = m(x).clone()
    assert bool(torch.isfinite(out).all())
    assert torch.equal(out, base)


def test_form_mismatch_takes_the_unfrozen_path(cuda):
    """Default fill rule (one workgroup per two CUs = 128 on this part), resnet34, f16x3.  At 2 x 128 x 128 layer1's 3x3 convs would
    launch 2 * 2 * 2 * 1 = 8 workgroups on the fp16x3 kernel: they stay on the Winograd banks.  At 32 x 128 x 128 they launch
    32 * 2 * 2 * 1 = 128: the fp16x3 bank.  An arena frozen at the first shape cannot serve the second."""
    L, lib = _lib()
    m = _warm_stats(_model("Unet", "resnet34", cuda, "f16x3", min_workgroups=0), 2, 128, 128, cuda)
    x2, x32 = _x(2, 128, 128, cuda), _x(32, 128, 128, cuda, seed=10)
    with torch.no_grad():
        m.routing(True)
        base2 = m(x2).clone()
        r2 = _fwd_kernels(m)
        base32 = m(x32).clone()
        r32 = _fwd_kernels(m)
        assert "f16x3" not in r2["encoder.layer1.0.conv1"], r2["encoder.layer1.0.conv1"]
        assert "conv_f16x3" in r32["encoder.layer1.0.conv1"], r32["encoder.layer1.0.conv1"]
        m.routing(False)
        m.freeze(batch_shape=(2, 128, 128))
        assert m.frozen_serves(2, 128, 128) and not m.frozen_serves(32, 128, 128)
        torch.cuda.synchronize()
        arena = m._fz_arena.clone()
        p = m.prep_launches()
        out32 = m(x32).clone()
        assert m.prep_launches() > p                             # prepared in the workspace, as an unfrozen forward does
        assert torch.equal(out32, base32)
        assert torch.equal(m._fz_arena, arena)
        assert lib.uwm_is_frozen(m._h)
        p = m.prep_launches()
        assert torch.equal(m(x2), base2)                         # and the arena still serves its own shape
        assert m.prep_launches() == p


def test_pinned_routing_serves_other_batches(cuda):
    m = _warm_stats(_model("Unet", "resnet34", cuda, "f16x3"), 2, 128, 128, cuda)
    x8 = _x(8, 128, 128, cuda)
    with torch.no_grad():
        base1 = m(x8[3:4]).clone()
        base8 = m(x8).clone()
        m.freeze(batch_shape=(8, 128, 128))
        p = m.prep_launches()
        out1 = m(x8[3:4]).clone()
        out8 = m(x8).clone()
        assert m.prep_launches() == p
    assert torch.equal(out1, base1) and torch.equal(out8, base8)
    assert torch.equal(out1[0], out8[3])


def test_library_unfreezes_on_training_forward_and_bind(cuda):
    import unet_watermark_amd as U
    L, lib = _lib()
    m = _warm_stats(_model("Unet", "resnet18", cuda, "f32"), 2, 128, 128, cuda)
    x = _x(2, 128, 128, cuda)
    with torch.no_grad():
        m.freeze()
        frozen_out = m(x).clone()
        assert lib.uwm_is_frozen(m._h)
        # a training forward straight on the ABI (model.train() would already unfreeze on the Python side)
        m._forward_raw(x * 3.0 + 1.0, training=True)
        assert not lib.uwm_is_frozen(m._h)
        after = m(x).clone()                                     # (the model re-freezes itself from the moved statistics)
        assert lib.uwm_is_frozen(m._h)
        fresh = U.Unet("resnet18").to(cuda)
        fresh.load_state_dict(m.state_dict())
        fresh.eval()
        expect = fresh(x).clone()
        assert not torch.equal(after, frozen_out)
        assert torch.equal(after, expect)
        # uwm_bind
        key = m._bound
        L.check(lib.uwm_bind(m._h, C.c_void_p(key[0]), C.c_void_p(key[1]), C.c_void_p(key[2])))
        assert not lib.uwm_is_frozen(m._h)
        assert lib.uwm_unfreeze(m._h) == 0


def test_python_unfreeze_triggers(cuda):
    m = _warm_stats(_model("Unet", "resnet18", cuda, "f32"), 2, 128, 128, cuda)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    for trigger in (lambda: m.train(True), lambda: m.load_state_dict(sd), lambda: m.to(cuda), lambda: m.float(),
                    lambda: m.set_precision("f16x3"), lambda: m.set_precision("f16x3", min_workgroups=1),
                    lambda: m.set_precision("f32", routing_batch=0), lambda: m.unfreeze()):
        m.eval()
        m.freeze(batch_shape=(2, 128, 128))
        assert m.frozen
        trigger()
        assert not m.frozen
    m.eval()
    assert not m.frozen                                          # eval() alone freezes nothing


@pytest.mark.parametrize("prec", [None, "f16x3"])
def test_graph_replay_survives_an_eager_forward_of_another_shape(cuda, prec):
    from unet_watermark_amd.predict import WatermarkPredictor
    from unet_watermark_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults(); cfg.MODEL.NAME = "Unet"
    m = _warm_stats(_model("Unet", "resnet34", cuda, "f32"), 2, 128, 128, cuda)
    plain = _model("Unet", "resnet34", cuda, "f32")
    plain.load_state_dict(m.state_dict())
    pred = WatermarkPredictor(model=m, config=cfg, device=cuda, precision=prec, freeze=True)
    ref = WatermarkPredictor(model=plain, config=cfg, device=cuda, precision=prec)
    assert pred.model.frozen and not ref.model.frozen
    x, y = _x(4, 128, 128, cuda), _x(2, 256, 256, cuda, seed=11)
    first = pred.logits(x, use_graph=True).clone()
    torch.cuda.synchronize()
    arena = m._fz_arena.clone()
    other = pred.logits(y, use_graph=False).clone()
    again = pred.logits(x, use_graph=True).clone()
    assert torch.equal(again, first)
    assert torch.equal(first, ref.logits(x, use_graph=True))
    assert torch.equal(other, ref.logits(y, use_graph=False))
    assert torch.equal(m._fz_arena, arena)


@pytest.mark.parametrize("frozen", [False, True])
def test_predict_u8_equals_the_three_call_sequence(cuda, frozen):
    import unet_watermark_amd as U
    from unet_watermark_amd.predict import WatermarkPredictor
    from unet_watermark_amd.config import get_cfg_defaults
    m = _warm_stats(_model("Unet", "resnet18", cuda, "f16x3"), 2, 128, 128, cuda)
    img = torch.randint(0, 256, (4, 128, 128, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(21)).to(cuda)
    with torch.no_grad():
        x = U.device_preprocess(img, mean=MEAN, std=STD)
        lg = m(x).clone()
        thr = float(lg.median())
        if frozen:
            m.freeze()
        for size in ((128, 128), (96, 160)):
            want_mask, want_resized = U.resize_threshold(lg, size, thr, return_resized=True)
            p0 = m.prep_launches()
            mask, logits = m.predict_u8(img, MEAN, STD, thr, out_size=size, return_logits=True)
            if frozen and size != (128, 128):
                assert m.prep_launches() == p0
            assert torch.equal(logits, lg)
            assert mask.shape == (4,) + size and torch.equal(mask, want_mask)
            assert torch.equal(m.predict_u8(img, MEAN, STD, thr, out_size=size), want_mask)      # logits kept in the workspace
            assert 0.2 < float((mask > 0).float().mean()) < 0.8
        # the forward's input buffer: the three normalised channels, and zero in the padding channel
        x4 = m.debug_buffer("x4").view(4, 128, 128, 4)
        assert torch.equal(x4[..., :3], x.permute(0, 2, 3, 1))
        assert float(x4[..., 3].abs().max()) == 0.0
        # graph-replayed, through the predictor
        cfg = get_cfg_defaults(); cfg.MODEL.NAME = "Unet"
        pred = WatermarkPredictor(model=m, config=cfg, device=cuda, freeze=frozen)
        pred.threshold = thr
        assert pred.model.frozen == frozen
        for size in (None, (96, 160)):
            want = U.resize_threshold(lg, size or (128, 128), thr)
            assert torch.equal(pred.predict_mask_u8(img, out_size=size, use_graph=False), want)
            assert torch.equal(pred.predict_mask_u8(img, out_size=size, use_graph=True), want)
            img2 = torch.roll(img, 1, 0)
            assert torch.equal(pred.predict_mask_u8(img2, out_size=size, use_graph=True), torch.roll(want, 1, 0))


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_preprocess_u8_nhwc4_equals_preprocess_u8(cuda, c):
    """The input kernel alone, at pixel counts that are and are not multiples of the 4 pixels a thread takes."""
    import unet_watermark_amd as U
    L, lib = _lib()
    mean, std = (0.485, 0.456, 0.406, 0.5)[:c], (0.229, 0.224, 0.225, 0.25)[:c]
    g = torch.Generator().manual_seed(100 + c)
    for n, h, w in ((1, 1, 1), (1, 5, 7), (2, 3, 33), (1, 32, 32), (3, 17, 129), (2, 256, 256)):
        img = torch.randint(0, 256, (n, h, w, c), dtype=torch.uint8, generator=g).to(cuda)
        want = nhwc(U.device_preprocess(img, mean=mean, std=std), 4)
        out = torch.full((n, h, w, 4), float("nan"), device=cuda)
        guard = torch.full((64,), 7.0, device=cuda)               # (allocated next: a write past the end would be seen on most layouts)
        mc, sc = (C.c_float * c)(*mean), (C.c_float * c)(*std)
        L.check(lib.uwm_op_preprocess_u8_nhwc4(C.c_void_p(img.data_ptr()), n * h * w, c, mc, sc, C.c_void_p(out.data_ptr()),
                                               C.c_void_p(L.stream_ptr(cuda))))
        assert torch.equal(out, want), (n, h, w, c)
        assert bool((guard == 7.0).all())
