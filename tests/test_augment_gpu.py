"""Train-time augmentation on the device (csrc/augment_u8.hip) against the numpy restatement of its rule (tests/augment_ref.py), and
the training path built on it (`main.py train --augment basic`).  The rule is integral: every comparison is bit-equal, there is no
tolerance and no case is exempted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as A  # noqa: E402

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)
HSVS = [(10, 20, 10), (-10, -20, -10), (179, 255, -255)]


def _D():
    from unet_watermark_amd import data
    return data


def _batch(n, h, w, c, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
    img[0, : h // 2] = (img[0, : h // 2] // 32) * 32 + 7          # flat patches too: greys and saturated colours for the HSV stage
    mask = rng.integers(0, 256, size=(n, h, w), dtype=np.uint8)
    return img, mask


def _descs(h, w, flag_list, c=3):
    """one descriptor per entry of flag_list, all different: identity first, then every flag word with the 15 degree / 0.9 /
    (0.1, -0.1) affine, and over them a shear, the shift of several image sizes, the 90 degree matrix (square only), a steep and an
    identity table and the three HSV triples"""
    D = _D()
    p = D.identity_aug_params(len(flag_list))
    steep = D.brightness_contrast_lut(1.2, -0.2)
    for i, fl in enumerate(flag_list):
        p["flags"][i] = fl
        if i == 0:
            continue                                                # identity
        p["minv"][i] = D.affine_inverse(h, w, 15.0, 0.9, 0.1, -0.1)
        if i % 6 == 2:
            p["minv"][i] = D.affine_inverse(h, w, -7.0, 1.05, 0.0, 0.05, shear=8.0)
        if i % 6 == 3:
            p["minv"][i] = (1.0, 0.0, int(2.5 * w) + 0.375, 0.0, 1.0, -(int(3.25 * h) + 0.625))
        if i % 6 == 4 and h == w:
            p["minv"][i] = D.affine_inverse(h, w, 90.0, 1.0, 0.0, 0.0)
        if i % 2 == 1:
            p["lut"][i] = steep
        if c == 3 and i % 6 in (1, 3, 5):
            p["hue"][i], p["sat"][i], p["val"][i] = HSVS[(i % 6) // 2]
    return p


CASES = {
    "24x40x3": (24, 40, 3, [0, 1, 2, 3, 1, 2]),
    "32x32x3_a": (32, 32, 3, [0, 1, 2, 3, 4, 5]),
    "32x32x3_b": (32, 32, 3, [6, 7, 8, 9, 10, 11]),
    "32x32x3_c": (32, 32, 3, [12, 13, 14, 15, 4, 8]),
    "8x8x1": (8, 8, 1, [5]),
    "8x8x1_affine": (8, 8, 1, [0, 6]),
    "1x7x3": (1, 7, 3, [0, 1, 2, 3]),
    "5x300x4": (5, 300, 4, [3, 1]),                                 # more than one lane stride per row (W > 256), four channels
}
_REF = {}


def _case(name):
    """(images, masks, descriptors, expected uint8 images, expected masks): the reference is computed once per case"""
    if name not in _REF:
        h, w, c, flag_list = CASES[name]
        img, mask = _batch(len(flag_list), h, w, c, seed=len(name) + h)
        p = _descs(h, w, flag_list, c)
        want = [A.augment_desc(img[i], mask[i], p[i]) for i in range(len(flag_list))]
        _REF[name] = (img, mask, p, np.stack([a for a, _ in want]), np.stack([m for _, m in want]))
    return _REF[name]


@pytest.mark.parametrize("name", list(CASES))
def test_augment_equals_the_restatement(cuda, name):
    D = _D()
    img, mask, p, want_u8, want_m = _case(name)
    c = img.shape[3]
    x, m = torch.from_numpy(img).to(cuda), torch.from_numpy(mask).to(cuda)
    out, mo, u8 = D.device_augment(x, m, p, MEAN, STD, return_u8=True)
    got_u8, got_m = u8.cpu().numpy(), mo.cpu().numpy()
    for i in range(len(p)):
        diff = int(np.abs(got_u8[i].astype(int) - want_u8[i]).max())
        print(name, "image", i, "flags", int(p["flags"][i]), "max |diff|", diff, "mask mismatches", int((got_m[i] != want_m[i]).sum()))
        assert np.array_equal(got_u8[i], want_u8[i]), (name, i, diff)
        assert np.array_equal(got_m[i], want_m[i]), (name, i)
    if name != "1x7x3":
        assert 0 < want_m.mean() < 1 and len(np.unique(want_u8)) > 8
    # Normalize is uwm_preprocess_u8's, bit for bit
    norm = D.device_preprocess(u8, None, None, MEAN, STD)
    assert out.shape == (len(p), c, img.shape[1], img.shape[2]) and out.dtype == torch.float32
    assert torch.equal(out.view(torch.int32), norm.view(torch.int32))
    # without masks / without the uint8 copy: the same values
    only = D.device_augment(x, None, p, MEAN, STD)
    assert isinstance(only, torch.Tensor) and torch.equal(only.view(torch.int32), out.view(torch.int32))


@pytest.mark.parametrize("h,w,c", [(32, 32, 3), (24, 40, 3), (8, 8, 1), (1, 7, 3)])
def test_identity_descriptors_equal_device_preprocess_for_every_flag_word(cuda, h, w, c):
    D = _D()
    flag_list = list(range(16 if h == w else 4))
    img, mask = _batch(len(flag_list), h, w, c, seed=11)
    p = D.identity_aug_params(len(flag_list))
    p["flags"] = flag_list
    x, m = torch.from_numpy(img).to(cuda), torch.from_numpy(mask).to(cuda)
    out, mo = D.device_augment(x, m, p, MEAN, STD)
    want, want_m = D.device_preprocess(x, m, torch.tensor(flag_list, dtype=torch.int32), MEAN, STD)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32)) and torch.equal(mo, want_m)


def test_rejected_inputs_raise_before_any_launch(cuda):
    D = _D()
    x = torch.zeros((2, 8, 12, 3), dtype=torch.uint8, device=cuda)
    x1 = torch.zeros((2, 8, 12, 1), dtype=torch.uint8, device=cuda)
    ok = D.identity_aug_params(2)
    bad = ok.copy(); bad["flags"][0] = D.aug_flags(rot90=2)
    with pytest.raises(ValueError, match="square"):
        D.device_augment(x, None, bad)
    bad = ok.copy(); bad["hue"][1] = 3
    with pytest.raises(ValueError, match="3-channel"):
        D.device_augment(x1, None, bad, MEAN[:1], STD[:1])
    bad = ok.copy(); bad["minv"][1, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        D.device_augment(x, None, bad)
    bad = ok.copy(); bad["minv"][0, 5] = -np.inf
    with pytest.raises(ValueError, match="non-finite"):
        D.device_augment(x, None, bad)
    with pytest.raises(ValueError, match="one descriptor per image"):
        D.device_augment(x, None, D.identity_aug_params(3))
    with pytest.raises(ValueError, match="masks"):
        D.device_augment(x, torch.zeros((2, 8, 8), dtype=torch.uint8, device=cuda), ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.device_augment(x.cpu(), None, ok)
    assert D.device_augment(x, None, ok).shape == (2, 3, 8, 12)


def test_sampled_parameters_run_through_the_kernel(cuda):
    """what `--augment basic` feeds the kernel: a sampled batch equals the restatement as well"""
    D = _D()
    img, mask = _batch(12, 32, 32, 3, seed=21)
    p = D.sample_aug_params(12, 32, 32, torch.Generator().manual_seed(3))
    _, mo, u8 = D.device_augment(torch.from_numpy(img).to(cuda), torch.from_numpy(mask).to(cuda), p, return_u8=True)
    for i in range(12):
        a, m = A.augment_desc(img[i], mask[i], p[i])
        assert np.array_equal(u8[i].cpu().numpy(), a) and np.array_equal(mo[i].cpu().numpy(), m), i


# ------------------------------------------------------------------------------------------------ main.py train --augment basic
def _write_folder(root):
    from PIL import Image
    rng = np.random.default_rng(8)
    os.makedirs(root / "watermarked"); os.makedirs(root / "masks")
    for i, (h, w) in enumerate([(64, 64), (50, 70), (90, 61), (64, 96), (33, 47), (128, 128), (71, 71), (40, 100)]):
        base = rng.integers(0, 256, size=(h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8)
        img = np.asarray(Image.fromarray(base).resize((w, h), Image.BILINEAR)).copy()
        m = np.zeros((h, w), dtype=np.uint8)
        y0, x0 = h // 4 + i, w // 5 + i
        m[y0: y0 + h // 3, x0: x0 + w // 2] = 255
        img[m > 0] = (img[m > 0].astype(int) * 6 // 10 + 100).astype(np.uint8)
        Image.fromarray(img).save(root / "watermarked" / f"im{i}.png")
        Image.fromarray(m).save(root / "masks" / f"im{i}.png")


def _train(root, tmp, tag, augment):
    from unet_watermark_amd import cli
    return cli.main(["train", "--data-dir", str(root), "--epochs", "1", "--batch-size", "2", "--lr", "0.002", "--no-early-stopping",
                     "--img-size", "64", "--encoder", "resnet18", "--model", "Unet", "--workers", "0", "--augment", augment,
                     "--model-save-path", str(tmp / f"{tag}.pth"), "--checkpoint-dir", str(tmp / f"ck_{tag}")])


def _parent_path_epoch_loss(root):
    """the epoch loss of the host input path as it was before --augment existed: FolderDataset -> DataLoader -> Trainer.step, with
    train_command's seeding, split and loader arguments"""
    from torch.utils.data import DataLoader, Subset
    from unet_watermark_amd import cli
    from unet_watermark_amd.config import get_cfg_defaults
    from unet_watermark_amd.data import FolderDataset
    from unet_watermark_amd.model import create_model_from_config
    from unet_watermark_amd.train import Trainer
    cfg = get_cfg_defaults()
    cfg.MODEL.NAME, cfg.MODEL.ENCODER_NAME, cfg.MODEL.ENCODER_WEIGHTS = "Unet", "resnet18", None
    cfg.DATA.IMG_SIZE, cfg.TRAIN.BATCH_SIZE, cfg.TRAIN.LR = 64, 2, 0.002
    dev = torch.device("cuda", 0)
    torch.manual_seed(int(cfg.DATA.SEED))
    model = create_model_from_config(cfg).to(dev)
    wd, wb = cli._loss_weights(cfg)
    trainer = Trainer(model, w_dice=wd, w_bce=wb, smooth=float(cfg.LOSS.SMOOTH), lr=0.002, weight_decay=float(cfg.TRAIN.WEIGHT_DECAY),
                      optimizer=cfg.OPTIMIZER.NAME, max_grad_norm=None, global_dice=False)
    full = FolderDataset(str(root), 64)
    perm = torch.randperm(len(full), generator=torch.Generator().manual_seed(int(cfg.DATA.SEED))).tolist() if cfg.DATA.SHUFFLE else list(range(len(full)))
    ntr = max(1, int(len(full) * float(cfg.DATA.TRAIN_RATIO)))
    tr = DataLoader(Subset(full, perm[:ntr]), 2, shuffle=True, sampler=None, num_workers=0, drop_last=True, pin_memory=True)
    model.train()
    acc = torch.zeros(3, device=dev)
    for x, t in tr:
        acc += trainer.step(x.to(dev, non_blocking=True), t.to(dev, non_blocking=True))
    torch.cuda.synchronize(dev)
    return float(acc[0]) / max(1, len(tr))


def test_train_on_a_folder_of_mixed_sizes_with_and_without_augmentation(cuda, tmp_path, capsys):
    root = tmp_path / "data"
    _write_folder(root)
    a = _train(root, tmp_path, "a", "basic")
    assert "serving the 'basic' recipe" in capsys.readouterr().out
    b = _train(root, tmp_path, "b", "basic")
    assert len(a) == 1 and np.isfinite(a[0]["train_loss"]) and np.isfinite(a[0]["val_loss"])
    print("basic:", a[0]["train_loss"], a[0]["val_loss"], "rerun:", b[0]["train_loss"], b[0]["val_loss"])
    assert a[0]["train_loss"] == b[0]["train_loss"] and a[0]["val_loss"] == b[0]["val_loss"]
    none = _train(root, tmp_path, "n", "none")
    want = _parent_path_epoch_loss(root)
    print("none:", none[0]["train_loss"], "direct FolderDataset run:", want)
    assert np.isfinite(want) and none[0]["train_loss"] == want
    assert none[0]["train_loss"] != a[0]["train_loss"]


def test_train_on_synthetic_images_takes_the_device_path(cuda, tmp_path):
    from unet_watermark_amd import cli
    hist = cli.main(["train", "--epochs", "2", "--batch-size", "4", "--lr", "0.002", "--no-early-stopping", "--synthetic", "16",
                     "--img-size", "64", "--encoder", "resnet18", "--model", "Unet", "--workers", "0", "--augment", "basic",
                     "--model-save-path", str(tmp_path / "s.pth"), "--checkpoint-dir", str(tmp_path / "ck")])
    assert len(hist) == 2 and all(np.isfinite(h["train_loss"]) and np.isfinite(h["val_loss"]) for h in hist)
