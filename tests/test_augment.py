"""Train-time augmentation, host side: properties of the rule itself (tests/augment_ref.py, which csrc/augment_u8.hip must equal
bit for bit — tests/test_augment_gpu.py), float sanity of its integer arithmetic, and the parameter sampler / descriptor layout of
unet_watermark_amd.data.  No GPU."""
import colorsys
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as A  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data():
    from unet_watermark_amd import data
    return data


def _image(h, w, c=3, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, c), dtype=np.uint8)


def _smooth(h, w, seed=0):
    """a smooth image: a few low-frequency waves per channel"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ch = []
    for _ in range(3):
        a, b, p, q = rng.uniform(0.02, 0.12, 2).tolist() + rng.uniform(0, 6.28, 2).tolist()
        ch.append(127.5 + 60 * np.sin(a * x + p) + 60 * np.cos(b * y + q))
    return np.clip(np.rint(np.stack(ch, -1)), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the rule
def test_identity_map_returns_image_and_mask_unchanged():
    for h, w in ((24, 40), (1, 7), (8, 8)):
        img = _image(h, w)
        assert np.array_equal(A.augment_image(img), img)
        assert np.array_equal(A.warp_nearest(img[..., 0], A.IDENTITY_MINV), img[..., 0])
        assert np.array_equal(A.augment_mask(img[..., 0]), (img[..., 0] > 127).astype(np.uint8))


@pytest.mark.parametrize("tx,ty", [(3, 0), (-5, 2), (0, -7), (11, 9)])
def test_integer_translation_is_a_slice_of_a_reflect_pad(tx, ty):
    h, w = 24, 40
    img = _image(h, w, seed=1)
    pad = 12
    big = np.pad(img, ((pad, pad), (pad, pad), (0, 0)), mode="reflect")
    minv = (1.0, 0.0, float(tx), 0.0, 1.0, float(ty))             # src = dst + (tx, ty)
    want = big[pad + ty: pad + ty + h, pad + tx: pad + tx + w]
    assert np.array_equal(A.warp_linear(img, minv), want)
    assert np.array_equal(A.warp_nearest(img[..., 1], minv), want[..., 1])


def test_a_shift_of_several_image_sizes_reflects_several_times():
    h, w = 20, 24
    img = _image(h, w, seed=2)
    tx, ty = int(2.5 * w), int(3.25 * h)
    for sgn in (1, -1):
        minv = (1.0, 0.0, float(sgn * tx), 0.0, 1.0, float(sgn * ty))
        iy = np.array([A.brute_reflect(y + sgn * ty, h) for y in range(h)])
        ix = np.array([A.brute_reflect(x + sgn * tx, w) for x in range(w)])
        assert 0 <= iy.min() and iy.max() < h and 0 <= ix.min() and ix.max() < w
        assert np.array_equal(A.reflect101(np.arange(h) + sgn * ty, h), iy) and np.array_equal(A.reflect101(np.arange(w) + sgn * tx, w), ix)
        assert np.array_equal(A.warp_linear(img, minv), img[iy][:, ix])
        assert np.array_equal(A.warp_nearest(img[..., 0], minv), img[iy][:, ix][..., 0])
    assert np.array_equal(A.reflect101(np.arange(-9, 9), 1), np.zeros(18, dtype=np.int64))


@pytest.mark.parametrize("n", [8, 33])
def test_right_angle_matrices_equal_rot90(n):
    D = _data()
    img = _image(n, n, seed=3)
    for k, angle in ((1, 90.0), (2, 180.0), (3, 270.0)):
        minv = D.affine_inverse(n, n, angle, 1.0, 0.0, 0.0)
        assert np.array_equal(A.warp_linear(img, minv), np.rot90(img, k)), angle
        assert np.array_equal(A.warp_nearest(img[..., 2], minv), np.rot90(img[..., 2], k)), angle


def test_flags_equal_flip_then_rot90():
    img = _image(16, 16, seed=4)
    for flags in range(16):
        want = np.rot90(img[:, ::-1] if flags & 1 else img, 0)
        want = want[::-1] if flags & 2 else want
        want = np.rot90(want, flags >> 2)
        assert np.array_equal(A.augment_image(img, flags=flags), want), flags


def _grid(step=3):
    v = np.arange(0, 256, step, dtype=np.uint8)
    return np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)


def test_hsv_forward_on_primaries_and_grey():
    px = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [90, 90, 90], [0, 0, 0], [255, 255, 255]], dtype=np.uint8)
    h, s, v = A.rgb_to_hsv(px)
    assert (h[:3].tolist(), s[:3].tolist(), v[:3].tolist()) == ([0, 60, 120], [255] * 3, [255] * 3)
    assert s[3:].tolist() == [0, 0, 0] and v[3:].tolist() == [90, 0, 255]


def test_hue_stays_in_range_over_the_grid():
    h, s, v = A.rgb_to_hsv(_grid())
    assert h.min() >= 0 and h.max() <= 179 and s.min() >= 0 and s.max() <= 255


# ------------------------------------------------------------------------------------------------ float sanity of the integer rules
def test_fixed_point_warp_is_within_one_lsb_of_a_float_warp():
    """200 draws of the basic recipe's ShiftScaleRotate ranges on a smooth 64 x 64 image"""
    D = _data()
    img = _smooth(64, 64)
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(200):
        minv = D.affine_inverse(64, 64, rng.uniform(-15, 15), rng.uniform(0.9, 1.1), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1))
        worst = max(worst, float(np.abs(A.warp_linear(img, minv) - A.float_warp(img, minv)).max()))
    print("fixed-point warp vs float64 bilinear: max", worst)
    assert worst <= 1.0


def test_hsv_round_trip_without_shifts_is_within_five_lsb():
    g = _grid()
    back = A.hsv_to_rgb(*A.rgb_to_hsv(g))
    err = int(np.abs(back.astype(int) - g.astype(int)).max())
    print("HSV round trip: max", err)
    assert err <= 5


def _colorsys_shift(rgb, hue, sat, val):
    out = np.empty(rgb.shape, dtype=np.float64)
    for i, (r, g, b) in enumerate(rgb.tolist()):
        h, s, v = colorsys.rgb_to_hsv(r / 255.0, g / 255.0, b / 255.0)
        h = ((h * 180.0 + hue) % 180.0) / 180.0
        s = min(max(s * 255.0 + sat, 0.0), 255.0) / 255.0
        v = min(max(v * 255.0 + val, 0.0), 255.0) / 255.0
        out[i] = [c * 255.0 for c in colorsys.hsv_to_rgb(h, s, v)]
    return out


@pytest.mark.parametrize("shifts", [(10, 20, 10), (-10, -20, -10), (7, -13, 4), (-3, 20, -10)])
def test_shifted_hsv_is_within_six_lsb_of_colorsys(shifts):
    """5 000 sampled colours per shift triple: 20 000 in all"""
    rgb = np.random.default_rng(sum(shifts) + 100).integers(0, 256, size=(5000, 3), dtype=np.uint8)
    got = A.hsv_shift(rgb, *shifts).astype(np.float64)
    err = float(np.abs(got - _colorsys_shift(rgb, *shifts)).max())
    print("shifted HSV vs colorsys", shifts, ": max", err)
    assert err <= 6.0


# ------------------------------------------------------------------------------------------------ host helpers and the sampler
def test_brightness_contrast_lut():
    D = _data()
    assert np.array_equal(D.brightness_contrast_lut(1.0, 0.0), np.arange(256, dtype=np.uint8))
    lut = D.brightness_contrast_lut(1.2, -0.2)
    want = [int(min(max(np.float32(v) * np.float32(1.2) + np.float32(-0.2 * 255), 0), 255)) for v in range(256)]
    assert lut.dtype == np.uint8 and lut.tolist() == want
    assert lut[0] == 0 and lut[42] == 0 and lut[255] == 255 and (np.diff(lut.astype(int)) >= 0).all()


def test_affine_inverse_inverts_the_forward_matrix():
    D = _data()
    h, w, angle, scale, dx, dy = 48, 64, 15.0, 0.9, 0.1, -0.1
    minv = D.affine_inverse(h, w, angle, scale, dx, dy)
    a = np.deg2rad(angle); al, be = scale * np.cos(a), scale * np.sin(a)
    cx, cy = w / 2 - 0.5, h / 2 - 0.5
    M = np.array([[al, be, (1 - al) * cx - be * cy + dx * w], [-be, al, be * cx + (1 - al) * cy + dy * h], [0, 0, 1]])
    assert np.allclose(np.vstack([minv.reshape(2, 3), [0, 0, 1]]) @ M, np.eye(3), atol=1e-12)
    assert np.array_equal(D.affine_inverse(h, w, 0.0, 1.0, 0.0, 0.0), np.array(D.IDENTITY_MINV))
    sh = D.affine_inverse(h, w, 0.0, 1.0, 0.0, 0.0, shear=10.0).reshape(2, 3)
    assert np.allclose(sh[:, :2], [[1, -np.tan(np.deg2rad(10.0))], [0, 1]]) and np.allclose(sh @ [cx, cy, 1], [cx, cy])


def _stages(p):
    D = _data()
    return ((p["minv"] != np.array(D.IDENTITY_MINV)).any(1), (p["lut"] != np.arange(256)).any(1),
            (p["hue"] != 0) | (p["sat"] != 0) | (p["val"] != 0))


def test_sampler_is_deterministic_for_a_seed():
    D = _data()
    a = D.sample_aug_params(64, 32, 32, torch.Generator().manual_seed(7))
    b = D.sample_aug_params(64, 32, 32, torch.Generator().manual_seed(7))
    c = D.sample_aug_params(64, 32, 32, torch.Generator().manual_seed(8))
    assert a.dtype == D.AUG_DESC_DTYPE and a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes()
    with pytest.raises(ValueError):
        D.sample_aug_params(4, 32, 32, recipe="enhanced")


def test_sampler_frequencies_ranges_and_skipped_stages():
    D = _data()
    n, h, w = 4000, 48, 64
    p = D.sample_aug_params(n, h, w, torch.Generator().manual_seed(0))
    aff, lut, hsv = _stages(p)
    for name, on, prob in (("affine", aff, 0.3), ("lut", lut, 0.3), ("hsv", hsv, 0.3), ("hflip", (p["flags"] & 1) != 0, 0.5),
                           ("vflip", (p["flags"] & 2) != 0, 0.2)):
        assert abs(on.mean() - prob) <= 5 * np.sqrt(prob * (1 - prob) / n), (name, on.mean())
    assert not (p["flags"] >> 2).any()                              # 48 x 64 is not square: no rot90
    q = D.sample_aug_params(n, 64, 64, torch.Generator().manual_seed(0))
    rot = (q["flags"] >> 2) & 3
    assert abs((rot != 0).mean() - 0.3) <= 5 * np.sqrt(0.21 / n) and set(np.unique(rot)) == {0, 1, 2, 3}
    # ranges: hsv limits; the forward map's scale, angle and shift recovered from the inverse
    assert np.abs(p["hue"]).max() <= 10 and np.abs(p["sat"]).max() <= 20 and np.abs(p["val"]).max() <= 10
    assert np.abs(p["hue"]).max() == 10 and np.abs(p["sat"]).max() == 20
    m = p["minv"][aff].reshape(-1, 2, 3)
    scale = 1.0 / np.sqrt(np.abs(np.linalg.det(m[:, :, :2])))
    angle = np.degrees(np.arctan2(-m[:, 0, 1], m[:, 0, 0]))         # the inverse rotates by -angle
    cx, cy = w / 2 - 0.5, h / 2 - 0.5
    fwd = np.linalg.inv(np.concatenate([m, np.tile([[[0, 0, 1]]], (len(m), 1, 1))], 1))
    shift = (fwd @ [cx, cy, 1])[:, :2] - [cx, cy]
    assert scale.min() >= 0.9 - 1e-9 and scale.max() <= 1.1 + 1e-9 and scale.max() - scale.min() > 0.15
    assert np.abs(angle).max() <= 15 + 1e-9 and np.abs(angle).max() > 12
    assert np.abs(shift[:, 0]).max() <= 0.1 * w + 1e-9 and np.abs(shift[:, 1]).max() <= 0.1 * h + 1e-9
    # brightness / contrast: every table is the table of some (alpha, beta) within the limits -> bounded by the extreme ones
    lo, hi = D.brightness_contrast_lut(0.8, -0.2).astype(int), D.brightness_contrast_lut(1.2, 0.2).astype(int)
    t = p["lut"][lut].astype(int)
    assert (t >= np.minimum(lo, hi)[None] - 0).all() and (t <= hi[None]).all()
    # skipped stages are exact identities
    assert (p["minv"][~aff] == np.array(D.IDENTITY_MINV)).all() and (p["lut"][~lut] == np.arange(256)).all()
    assert not p["hue"][~hsv].any() and not p["sat"][~hsv].any() and not p["val"][~hsv].any()
    ident = D.identity_aug_params(3)
    assert not any(s.any() for s in _stages(ident)) and not ident["flags"].any()


def test_descriptor_layout_equals_the_header():
    D = _data()
    text = open(os.path.join(ROOT, "include", "uwm.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} uwm_aug_desc;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = {"int": 4, "double": 8, "unsigned char": 1}
    off, fields, align = 0, {}, 1
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.match(r"(unsigned char|int|double)\s+(.*)", decl)
        for name in (s.strip() for s in m.group(2).split(",")):
            cnt = re.match(r"(\w+)(?:\[(\d+)\])?$", name)
            a = size[m.group(1)]
            off = (off + a - 1) // a * a
            fields[cnt.group(1)] = (off, m.group(1), int(cnt.group(2) or 1))
            off += a * int(cnt.group(2) or 1)
            align = max(align, a)
    total = (off + align - 1) // align * align
    assert total == 320 == D.AUG_DESC_DTYPE.itemsize
    assert {k: v[0] for k, v in fields.items()} == {"flags": 0, "hue": 4, "sat": 8, "val": 12, "minv": 16, "lut": 64}
    for name, (o, _, cnt) in fields.items():
        dt, fo = D.AUG_DESC_DTYPE.fields[name][:2]
        assert fo == o and dt.itemsize == cnt * size[fields[name][1]], name


def test_host_validation_needs_no_device():
    """what device_augment refuses is decided on the host, before anything is uploaded"""
    D = _data()
    ok = D.identity_aug_params(2)
    assert D._check_aug_params(ok, 2, 8, 12, 3) is not None
    bad = ok.copy(); bad["flags"][1] = D.aug_flags(rot90=1)
    with pytest.raises(ValueError, match="square"):
        D._check_aug_params(bad, 2, 8, 12, 3)
    assert D._check_aug_params(bad, 2, 8, 8, 3) is not None
    bad = ok.copy(); bad["sat"][0] = 5
    with pytest.raises(ValueError, match="3-channel"):
        D._check_aug_params(bad, 2, 8, 12, 1)
    for v in (np.nan, np.inf):
        bad = ok.copy(); bad["minv"][1, 4] = v
        with pytest.raises(ValueError, match="non-finite"):
            D._check_aug_params(bad, 2, 8, 12, 3)
    bad = ok.copy(); bad["minv"][0, 2] = 1e7
    with pytest.raises(ValueError, match="range"):
        D._check_aug_params(bad, 2, 8, 12, 3)
    with pytest.raises(ValueError, match="one descriptor per image"):
        D._check_aug_params(ok, 3, 8, 12, 3)


def test_abi_entry_checks_arguments_before_any_launch():
    """a null pointer, masks without out_masks, C = 5, H = 0, misaligned descriptors, std = 0: non-zero with a message, and no
    launch is reached (the pointers are host memory); the --augment switch parses and defaults to today's path"""
    import ctypes as C
    import __graft_entry__ as g
    g.build()
    from unet_watermark_amd import _lib, cli
    lib = _lib.lib()
    buf = (C.c_uint8 * 4096)()
    p = C.c_void_p(C.addressof(buf) + (-C.addressof(buf)) % 16)
    odd = C.c_void_p(p.value + 4)
    mean = (C.c_float * 4)(0.5, 0.5, 0.5, 0.5); std = (C.c_float * 4)(0.25, 0.25, 0.25, 0.25); std0 = (C.c_float * 4)(0.25, 0.0, 0.25, 0.25)

    def bad(rc, word):
        assert rc != 0
        assert word in lib.uwm_last_error().decode(), lib.uwm_last_error().decode()

    f = lib.uwm_augment_u8
    bad(f(None, None, p, 1, 8, 8, 3, mean, std, 127, p, None, None, None), "null")
    bad(f(p, None, None, 1, 8, 8, 3, mean, std, 127, p, None, None, None), "null")
    bad(f(p, None, p, 1, 8, 8, 3, mean, std, 127, None, None, None, None), "null")
    bad(f(p, None, p, 1, 8, 8, 3, None, std, 127, p, None, None, None), "null")
    bad(f(p, p, p, 1, 8, 8, 3, mean, std, 127, p, None, None, None), "together")
    bad(f(p, None, p, 1, 8, 8, 3, mean, std, 127, p, p, None, None), "together")
    bad(f(p, None, p, 1, 8, 8, 5, mean, std, 127, p, None, None, None), "1..4")
    bad(f(p, None, p, 1, 0, 8, 3, mean, std, 127, p, None, None, None), ">= 1")
    bad(f(p, None, p, 0, 8, 8, 3, mean, std, 127, p, None, None, None), ">= 1")
    bad(f(p, None, odd, 1, 8, 8, 3, mean, std, 127, p, None, None, None), "aligned")
    bad(f(p, None, p, 1, 8, 8, 3, mean, std0, 127, p, None, None, None), "positive")
    assert cli.build_parser().parse_args(["train"]).augment == "none"
    assert cli.build_parser().parse_args(["train", "--augment", "basic"]).augment == "basic"
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["train", "--augment", "enhanced"])
