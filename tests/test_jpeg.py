"""ImageCompression of the transparent_watermark recipe, the parts that need no device: the numpy restatement of the rule
(tests/jpeg_ref.py) against Pillow's libjpeg-turbo, bit for bit and with no exempted case; its int32 operand bound; the recipe's
sampler; the refusals of device_jpeg, of the C ABI and of the command line."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_ref as J  # noqa: E402

SIZES = [(16, 16), (16, 48), (48, 16), (32, 32), (64, 96)]
QUALITIES = [1, 2, 5, 10, 25, 49, 50, 51, 60, 77, 95, 100]


def _pillow():
    PIL = pytest.importorskip("PIL")
    from PIL import Image, features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("Pillow without libjpeg-turbo")
    return Image


def _pillow_roundtrip(Image, img, q):
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=q)          # Pillow's defaults: baseline, 4:2:0, islow DCT; decode: fancy up-sampling
    b.seek(0)
    im = Image.open(b)
    return np.asarray(im.convert("RGB")), im.quantization


def test_reference_equals_pillow_bit_for_bit():
    Image = _pillow()
    wrong = []
    for h, w in SIZES:
        for kind, img in J.sample_images(h, w).items():
            for q in QUALITIES:
                got, _ = _pillow_roundtrip(Image, img, q)
                ref = J.roundtrip(img, q)
                if not np.array_equal(got, ref):
                    wrong.append((h, w, kind, q, int(np.abs(got.astype(int) - ref).max())))
    assert not wrong, wrong


def test_quality_tables_equal_the_tables_of_a_written_file():
    """Pillow hands a file's tables out in natural order (it undoes the file's zigzag order itself)"""
    Image = _pillow()
    img = J.sample_images(16, 16)["noise"]
    for q in (1, 49, 50, 60, 100):
        _, tables = _pillow_roundtrip(Image, img, q)
        lum, chrom = J.quant_tables(q)
        assert list(tables[0]) == lum.tolist() and list(tables[1]) == chrom.tolist(), q
    assert J.quant_tables(100)[0].tolist() == [1] * 64 and J.quant_tables(1)[1].max() == 255
    with pytest.raises(ValueError):
        J.quant_tables(0)


def test_every_dct_operand_stays_inside_int32():
    """the reference asserts the bound on every product, sum and shift operand as it goes; these are the extreme inputs"""
    J.STATS["max_abs"] = 0
    for kind in ("noise01", "noise", "stripes", "checker8"):
        img = J.sample_images(32, 32)[kind]
        for q in (1, 50, 100):
            J.roundtrip(img, q)
    for v in (0, 255):                                             # the largest DC term
        J.roundtrip(np.full((16, 16, 3), v, dtype=np.uint8), 100)
    print("largest DCT operand:", J.STATS["max_abs"])
    assert 0 < J.STATS["max_abs"] < 1 << 31
    with pytest.raises(AssertionError):
        J._c(np.array([1 << 31]))


def test_reference_passes_quality_zero_through_and_refuses_other_shapes():
    img = J.sample_images(16, 32)["noise"]
    assert np.array_equal(J.roundtrip(img, 0), img)
    assert not np.array_equal(J.roundtrip(img, 100), img)
    for bad in (img[:8], img[:, :24], img[..., :1], img.astype(np.int32)):
        with pytest.raises(ValueError):
            J.roundtrip(bad, 50)
    flat = np.full((16, 16, 3), 128, dtype=np.uint8)               # a grey survives every quality
    assert np.array_equal(J.roundtrip(flat, 1), flat)


# ------------------------------------------------------------------------------------------------ the recipe's sampler
def test_transparent_recipe_sampler():
    from unet_watermark_amd import data as D
    n = 4000
    p, e, q = D.sample_transparent_recipe(n, 32, 32, torch.Generator().manual_seed(3))
    p2, e2, q2 = D.sample_transparent_recipe(n, 32, 32, torch.Generator().manual_seed(3))
    assert p.tobytes() == p2.tobytes() and e.tobytes() == e2.tobytes() and q.tobytes() == q2.tobytes()
    p3, e3, q3 = D.sample_transparent_recipe(n, 32, 32, torch.Generator().manual_seed(4))
    assert p.tobytes() != p3.tobytes() and q.tobytes() != q3.tobytes()
    assert q.dtype == np.int32 and q.shape == (n,)
    drawn = q[q != 0]
    assert drawn.min() == 60 and drawn.max() == 100 and set(np.unique(drawn)) == set(range(60, 101))
    assert D._check_aug_params(p, n, 32, 32, 3) is not None and D._check_aug_ext_params(e, n, 32, 32, 3) is not None
    ident = D.identity_aug_params(1)
    rates = {
        "hflip": ((p["flags"] & 1) != 0, 0.5), "vflip": ((p["flags"] & 2) != 0, 0.2), "rot90": (((p["flags"] >> 2) & 3) != 0, 0.3),
        "affine": ((p["minv"] != ident["minv"][0]).any(1), 0.3), "brightness": ((p["lut"] != ident["lut"][0]).any(1), 0.7),
        "hsv": ((p["hue"] != 0) | (p["sat"] != 0) | (p["val"] != 0), 0.5), "noise": (e["noise_sigma"] != 0, 0.3),
        "blur": (e["blur"] != 0, 0.2), "jpeg": (q != 0, 0.3),
    }
    for name, (hit, prob) in rates.items():
        rate, sd = float(np.mean(hit)), np.sqrt(prob * (1 - prob) / n)
        print(f"{name}: {rate:.4f} (p = {prob}, 4 sd = {4 * sd:.4f})")
        assert abs(rate - prob) <= 4 * sd, (name, rate, prob)
    assert (e["tone"] == 0).all()                                  # no CLAHE / gamma in this recipe
    sig = e["noise_sigma"][e["noise_sigma"] != 0] / 256.0
    assert sig.min() >= np.sqrt(10.0) - 0.01 and sig.max() <= np.sqrt(50.0) + 0.01
    assert (e["blur"] == D.BLUR_MOTION).any() and (e["blur"] == D.BLUR_GAUSS).any()
    # rectangular images: no rot90
    pr, _, _ = D.sample_transparent_recipe(64, 32, 48, torch.Generator().manual_seed(3))
    assert not ((pr["flags"] >> 2) & 3).any()
    with pytest.raises(ValueError, match="sample_transparent_recipe"):
        D.sample_aug_recipe(4, 32, 32, recipe="transparent_watermark")


def test_device_jpeg_refusals_on_the_host():
    from unet_watermark_amd import data as D
    z = lambda *s: torch.zeros(s, dtype=torch.uint8)      # noqa: E731
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.device_jpeg(z(2, 16, 16, 3), [60, 0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.device_jpeg(z(2, 16, 16, 3).float(), [60, 0])
    with pytest.raises(ValueError, match="C must be 3"):
        D.device_jpeg(z(2, 16, 16, 1), [60, 0])
    with pytest.raises(ValueError, match="multiples of 16"):
        D.device_jpeg(z(2, 24, 16, 3), [60, 0])
    with pytest.raises(ValueError, match="multiples of 16"):
        D.device_jpeg(z(2, 16, 8, 3), [60, 0])
    with pytest.raises(ValueError, match=r"0 \(pass through\) or 1\.\.100"):
        D.device_jpeg(z(2, 16, 16, 3), [60, 101])
    with pytest.raises(ValueError, match=r"0 \(pass through\) or 1\.\.100"):
        D.device_jpeg(z(2, 16, 16, 3), [-1, 60])
    with pytest.raises(ValueError, match="one per image"):
        D.device_jpeg(z(2, 16, 16, 3), [60])
    with pytest.raises(ValueError, match="one per image"):
        D.device_jpeg(z(2, 16, 16, 3), [60.0, 70.0])


# ------------------------------------------------------------------------------------------------ the C ABI
def _lib():
    import __graft_entry__ as g
    g.build()
    from unet_watermark_amd import _lib
    return _lib.lib()


def test_abi_entry_checks_arguments_before_any_launch():
    """uwm_jpeg_u8's refusals, in the words of uwm_augment_ext_u8's.  The pointers are host memory, so no launch is reached."""
    lib = _lib()
    buf = (C.c_uint8 * 8192)()
    p = C.c_void_p(C.addressof(buf) + (-C.addressof(buf)) % 16)
    odd4, odd1 = C.c_void_p(p.value + 4), C.c_void_p(p.value + 1)
    mean = (C.c_float * 3)(0.5, 0.5, 0.5); std = (C.c_float * 3)(0.25, 0.25, 0.25); std0 = (C.c_float * 3)(0.25, 0.25, 0.0)

    def bad(rc, word):
        assert rc != 0
        assert word in lib.uwm_last_error().decode(), lib.uwm_last_error().decode()

    need = lib.uwm_jpeg_workspace_bytes(1, 16, 16)
    assert need == 16 * 16 * 3 // 2 and lib.uwm_jpeg_workspace_bytes(5, 64, 96) == 5 * 64 * 96 * 3 // 2
    for shape in ((0, 16, 16), (1, 0, 16), (1, 16, 0), (1, 24, 16), (1, 16, 8), (-1, 16, 16)):
        assert lib.uwm_jpeg_workspace_bytes(*shape) == 0
        assert "bad shape" in lib.uwm_last_error().decode()
    f = lib.uwm_jpeg_u8
    bad(f(None, p, 1, 16, 16, mean, std, p, need, p, p, None), "null")
    bad(f(p, None, 1, 16, 16, mean, std, p, need, p, p, None), "null")
    bad(f(p, p, 1, 16, 16, None, std, p, need, p, p, None), "null")
    bad(f(p, p, 1, 16, 16, mean, None, p, need, p, p, None), "null")
    bad(f(p, p, 1, 16, 16, mean, std, p, need, None, None, None), "both null")
    bad(f(p, p, 0, 16, 16, mean, std, p, need, p, p, None), ">= 1")
    bad(f(p, p, 1, 0, 16, mean, std, p, need, p, p, None), ">= 1")
    bad(f(p, p, 1, 16, -16, mean, std, p, need, p, p, None), ">= 1")
    bad(f(p, p, 1, 24, 16, mean, std, p, need, p, p, None), "multiples of 16")
    bad(f(p, p, 1, 16, 40, mean, std, p, need, p, p, None), "multiples of 16")
    bad(f(p, p, 1, 16, 16, mean, std0, p, need, p, p, None), "positive")
    bad(f(p, odd1, 1, 16, 16, mean, std, p, need, p, p, None), "quality must be 4-byte aligned")
    bad(f(odd1, p, 1, 16, 16, mean, std, p, need, p, p, None), "images and out_u8 must be 4-byte aligned")
    bad(f(p, p, 1, 16, 16, mean, std, p, need, p, odd1, None), "images and out_u8 must be 4-byte aligned")
    bad(f(p, p, 1, 16, 16, mean, std, p, need, odd4, p, None), "out_nchw must be 16-byte aligned")
    bad(f(p, p, 1, 16, 16, mean, std, None, need, p, p, None), "null workspace")
    bad(f(p, p, 1, 16, 16, mean, std, p, need - 1, p, p, None), "too small")
    bad(f(p, p, 1, 16, 16, mean, std, odd4, need, p, p, None), "16-byte aligned")


# ------------------------------------------------------------------------------------------------ the command line
def test_parser_takes_the_jpeg_flag_and_the_recipe_is_served_only_with_it():
    from unet_watermark_amd import cli
    from unet_watermark_amd.config import get_cfg_defaults
    a = cli.build_parser().parse_args(["train", "--augment", "config", "--jpeg", "device"])
    assert a.jpeg == "device" and cli.build_parser().parse_args(["train"]).jpeg == "refuse"
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["train", "--jpeg", "host"])
    cfg = get_cfg_defaults()
    assert cfg.DATA.AUGMENTATION_TYPE == "transparent_watermark"
    recipe, note = cli._served_recipe("config", cfg, "device")
    assert recipe == "transparent_watermark" and "ImageCompression" in note and "libjpeg" in note and "reflect" in note
    with pytest.raises(ValueError, match="ImageCompression") as err:
        cli._served_recipe("config", cfg)
    assert "--jpeg device" in str(err.value)
    with pytest.raises(ValueError, match="ImageCompression"):
        cli._served_recipe("config", cfg, "refuse")
    # the flag changes nothing for the other recipes
    assert cli._served_recipe("basic", cfg, "device") == cli._served_recipe("basic", cfg)
    assert cli._served_recipe("none", cfg, "device") == ("none", "")
    cfg.DATA.AUGMENTATION_TYPE = "enhanced"
    assert cli._served_recipe("config", cfg, "device") == cli._served_recipe("config", cfg)
