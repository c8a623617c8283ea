"""CPU tests of the EfficientNet-b0..b7 encoder family, AdamW and the text-watermark recipe's plumbing
(the b3 / AdamW / CosineAnnealingWarmRestarts config, src/configs/unet_text_watermark.yaml).  No GPU compute here."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import effnet_family_ref as R  # noqa: E402

# efficientnet_pytorch's published structure: stem, stage outputs, repeats, smp feature taps, encoder parameters (no
# classifier head), and the published total with the head (_conv_head, _bn1, _fc) added back
TABLE = {
    "efficientnet-b0": (32, (16, 24, 40, 80, 112, 192, 320), (1, 2, 2, 3, 3, 4, 1), (3, 5, 11, 16), 3_595_388, 5_288_548),
    "efficientnet-b1": (32, (16, 24, 40, 80, 112, 192, 320), (2, 3, 3, 4, 4, 5, 2), (5, 8, 16, 23), 6_101_024, 7_794_184),
    "efficientnet-b2": (32, (16, 24, 48, 88, 120, 208, 352), (2, 3, 3, 4, 4, 5, 2), (5, 8, 16, 23), 7_202_562, 9_109_994),
    "efficientnet-b3": (40, (24, 32, 48, 96, 136, 232, 384), (2, 3, 3, 5, 5, 6, 2), (5, 8, 18, 26), 10_103_336, 12_233_232),
    "efficientnet-b4": (48, (24, 32, 56, 112, 160, 272, 448), (2, 4, 4, 6, 6, 8, 2), (6, 10, 22, 32), 16_742_216, 19_341_616),
    "efficientnet-b5": (48, (24, 40, 64, 128, 176, 304, 512), (3, 5, 5, 7, 7, 9, 3), (8, 13, 27, 39), 27_288_112, 30_389_784),
    "efficientnet-b6": (56, (32, 40, 72, 144, 200, 344, 576), (3, 6, 6, 8, 8, 11, 3), (9, 15, 31, 45), 39_403_992, 43_040_704),
    "efficientnet-b7": (64, (32, 48, 80, 160, 224, 384, 640), (4, 7, 7, 10, 10, 13, 4), (11, 18, 38, 55), 62_143_440, 66_347_960),
}


@pytest.fixture(scope="module")
def U():
    import __graft_entry__ as g
    g.build()
    import unet_watermark_amd as U
    return U


@pytest.mark.parametrize("name", list(TABLE))
def test_reference_reproduces_published_structure(name):
    stem, outs, reps, taps, enc_params, total = TABLE[name]
    ref = R.build(name)
    enc = ref.encoder
    assert enc._conv_stem.out_channels == stem
    assert tuple(st[5] for st in R.stages(name)) == outs and tuple(st[0] for st in R.stages(name)) == reps
    assert enc.stage_idxs == taps and len(enc._blocks) == sum(reps) == taps[-1]
    assert enc.out_channels == (3, stem, outs[1], outs[2], outs[4], outs[6])
    assert R.encoder_params(ref) == enc_params
    assert enc_params + R.head_params(name) == total
    nb = len(enc._blocks)
    assert [b.drop_rate for b in enc._blocks] == [0.2 * i / nb for i in range(nb)]
    feats = enc(torch.zeros(1, 3, 64, 64))
    assert [f.shape[1] for f in feats] == list(enc.out_channels)
    assert [f.shape[-1] for f in feats] == [64, 32, 16, 8, 4, 2]


def test_b3_smp_out_channels():
    assert R.out_channels("efficientnet-b3") == (3, 40, 32, 48, 136, 384)


@pytest.mark.parametrize("arch", ["Unet", "UnetPlusPlus"])
def test_reference_b4_equals_oracle(arch):
    from oracle import unet_oracle as O
    ref, fam = O.build("efficientnet-b4", seed=5, arch=arch), R.build("efficientnet-b4", seed=5, arch=arch)
    so, sf = ref.state_dict(), fam.state_dict()
    assert list(so) == list(sf) and all(torch.equal(so[k], sf[k]) for k in so)
    x, _ = O.synthetic_batch(2, 64, 64, seed=3)
    keep = [torch.tensor([1.0, 0.0]) for _ in ref.encoder._blocks]
    ref.train(); fam.train()
    assert torch.equal(ref(x, keep), fam(x, keep))
    ref.eval(); fam.eval()
    with torch.no_grad():
        assert torch.equal(ref(x), fam(x))


@pytest.mark.parametrize("name", list(TABLE))
def test_library_matches_reference(U, name):
    """The planner's model for every variant under both decoders: smp state_dict keys / shapes, parameter count, drop-connect
    ramp, and conv FLOPs equal to the reference's own count."""
    from unet_watermark_amd import _lib as L
    for arch in ("Unet", "UnetPlusPlus"):
        ref = R.build(name, arch=arch)
        m = getattr(U, arch)(name)
        sd, so = m.state_dict(), ref.state_dict()
        assert list(sd) == list(so)
        assert all(sd[k].shape == so[k].shape for k in so)
        assert m.num_parameters() == sum(p.numel() for p in ref.parameters())
        nb = len(ref.encoder._blocks)
        assert m._n_mb == nb
        for i, b in enumerate(ref.encoder._blocks):
            want = b.drop_rate if (b.stride == 1 and b.cin == b.cout) else 0.0
            assert abs(m._mb_drop[i] - want) < 1e-7, (i, m._mb_drop[i], want)
        for h, w in ((64, 64), (128, 96)):
            f, fb = m.conv_flops(h, w)
            rf, rfb = R.conv_flops(ref, h, w)
            assert abs(f - rf) <= 1e-9 * rf and abs(fb - rfb) <= 1e-9 * rfb, (arch, h, w, f, rf, fb, rfb)
        if name == "efficientnet-b3":
            m.load_state_dict(so)
            assert all(torch.equal(m.state_dict()[k], so[k]) for k in so)
    assert L.ENC[name] == 100 + int(name[-1])
    assert name in U.Unet.SUPPORTED_ENCODERS


def test_b3_unetplusplus_workspace_bound(U):
    """UnetPlusPlus-b3 at the recipe's 6 x 512^2 plans its training workspace within 10 GiB (8.7 GiB; b4: 10.8)."""
    from unet_watermark_amd import _lib as L
    m = U.UnetPlusPlus("efficientnet-b3")
    ws = L.lib().uwm_workspace_bytes(m._h, 6, 512, 512, 1)
    assert 0 < ws <= 10 * 2 ** 30, ws
    m4 = U.UnetPlusPlus("efficientnet-b4")
    assert ws < L.lib().uwm_workspace_bytes(m4._h, 6, 512, 512, 1)


def test_unknown_efficientnet_rejected(U):
    with pytest.raises(ValueError, match="Unsupported encoder"):
        U.Unet("efficientnet-b8")
    from unet_watermark_amd import _lib as L
    d = L.uwm_unet_desc(108, 3, 1, (C.c_int * 5)(256, 128, 64, 32, 16), 1e-5, 0.1, 0)
    h = C.c_void_p()
    assert L.lib().uwm_create(C.byref(d), C.byref(h)) != 0
    assert b"unsupported encoder" in L.lib().uwm_last_error()


# ------------------------------------------------------------------------------ recipe plumbing
TEXT_YAML = """
DEVICE: "cpu"
MODEL:
  NAME: "UnetPlusPlus"
  ENCODER_NAME: "efficientnet-b3"
  ENCODER_WEIGHTS: "imagenet"
  ENCODER_DEPTH: 5
  DECODER_CHANNELS: [256, 128, 64, 32, 16]
  IN_CHANNELS: 3
  CLASSES: 1
  ACTIVATION: null
TRAIN:
  BATCH_SIZE: 6
  EPOCHS: 1500
  LR: 0.003
  WEIGHT_DECAY: 0.0001
  GRADIENT_CLIP: 0.8
LOSS:
  NAME: "CombinedLoss"
  SMOOTH: 1e-6
  BCE_WEIGHT: 0.3
  DICE_WEIGHT: 0.5
  FOCAL_WEIGHT: 0.2
OPTIMIZER:
  NAME: "AdamW"
  LR_SCHEDULER: "CosineAnnealingWarmRestarts"
  SCHEDULER_T_0: 50
  SCHEDULER_T_MULT: 2
  SCHEDULER_ETA_MIN: 1e-6
"""


def _text_cfg(tmp_path, drop=None):
    from unet_watermark_amd.config import get_cfg_defaults, update_config
    text = TEXT_YAML if drop is None else "\n".join(l for l in TEXT_YAML.splitlines() if drop not in l)
    p = tmp_path / "text.yaml"
    p.write_text(text)
    return update_config(get_cfg_defaults(), str(p))


def test_text_config_builds_model_optimizer_and_scheduler(U, tmp_path):
    from unet_watermark_amd import cli
    from unet_watermark_amd.model import create_model_from_config
    from unet_watermark_amd.train import FusedAdamW
    cfg = _text_cfg(tmp_path)
    cfg.MODEL.ENCODER_WEIGHTS = None
    m = create_model_from_config(cfg)
    assert isinstance(m, U.UnetPlusPlus) and m.encoder_name == "efficientnet-b3"
    assert cli._loss_weights(cfg) == (0.5, 0.3)
    opt = FusedAdamW(m, lr=float(cfg.TRAIN.LR), weight_decay=float(cfg.TRAIN.WEIGHT_DECAY))
    s = cli._make_scheduler(cfg, opt)
    assert isinstance(s, torch.optim.lr_scheduler.CosineAnnealingWarmRestarts)
    assert (s.T_0, s.T_mult, s.eta_min) == (50, 2, 1e-6)
    # torch's own sequence over a fake optimizer with the same base LR
    ref = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(
        torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=0.003), T_0=50, T_mult=2, eta_min=1e-6)
    for _ in range(160):
        assert opt.param_groups[0]["lr"] == ref.optimizer.param_groups[0]["lr"]
        s.step(); ref.step()


def test_warm_restarts_defaults_and_missing_t0(U, tmp_path):
    from unet_watermark_amd import cli
    from unet_watermark_amd.train import FusedAdamW
    m = U.Unet("resnet18")
    opt = FusedAdamW(m, lr=0.01)
    cfg = _text_cfg(tmp_path, drop="SCHEDULER_T_MULT")
    del cfg.OPTIMIZER["SCHEDULER_ETA_MIN"]
    s = cli._make_scheduler(cfg, opt)
    assert (s.T_0, s.T_mult, s.eta_min) == (50, 1, 0.0)
    cfg = _text_cfg(tmp_path, drop="SCHEDULER_T_0")
    with pytest.raises(ValueError, match="SCHEDULER_T_0"):
        cli._make_scheduler(cfg, opt)


def test_cli_accepts_adamw_and_warm_restarts(U, monkeypatch):
    """The parser takes --optimizer AdamW / --lr-scheduler CosineAnnealingWarmRestarts; training itself stops for lack of a
    device here (after the config has been validated)."""
    from unet_watermark_amd import cli
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="HIP device"):
        cli.main(["train", "--optimizer", "AdamW", "--lr-scheduler", "CosineAnnealingWarmRestarts", "--encoder", "efficientnet-b3",
                  "--synthetic", "4", "--epochs", "1"])
    with pytest.raises(SystemExit):
        cli.main(["train", "--optimizer", "RMSprop"])


def test_fused_adamw_defaults_and_state_interchange(U):
    from unet_watermark_amd.train import FusedAdam, FusedAdamW
    import unet_watermark_amd as pkg
    assert pkg.FusedAdamW is FusedAdamW and issubclass(FusedAdamW, FusedAdam)
    m = U.Unet("resnet18")
    opt = FusedAdamW(m)
    g = opt.param_groups[0]
    ref = torch.optim.AdamW([torch.zeros(1, requires_grad=True)])
    for k in ("lr", "betas", "eps", "weight_decay"):
        assert g[k] == ref.param_groups[0][k], k
    with pytest.raises(ValueError, match="amsgrad"):
        FusedAdamW(m, amsgrad=True)
    # torch.optim.AdamW state over the same parameters loads into FusedAdamW and comes back out unchanged
    params = [torch.nn.Parameter(p.detach().clone()) for p in m.parameters()]
    topt = torch.optim.AdamW(params, lr=1e-3, weight_decay=1e-2)
    gen = torch.Generator().manual_seed(0)
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen)
    topt.step(); topt.step()
    sd = topt.state_dict()
    opt.load_state_dict(sd)
    assert opt._step == 2 and opt.param_groups[0]["weight_decay"] == 1e-2
    back = opt.state_dict()
    assert set(back["state"]) == set(sd["state"])
    for i, ent in sd["state"].items():
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(back["state"][i][k], ent[k]), (i, k)
        assert float(back["state"][i]["step"]) == float(ent["step"])
    topt2 = torch.optim.AdamW([torch.nn.Parameter(p.detach().clone()) for p in params], lr=1e-3)
    topt2.load_state_dict(back)
    assert topt2.param_groups[0]["weight_decay"] == 1e-2
