"""Train-time augmentation on the device: Normalize with flips / rot90 (uwm_preprocess_u8), the basic recipe's stages
(uwm_augment_u8, csrc/augment_u8.hip), the enhanced recipe's (uwm_augment_ext_u8, csrc/augment_ext_u8.hip) and ImageCompression
(uwm_jpeg_u8, csrc/jpeg_u8.hip); the descriptors, the host tables they carry, and the sampler that draws them from a recipe's numbers
(RECIPES)."""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from ..constants import IMAGENET_MEAN, IMAGENET_STD
from .._device import device_u8, norm_arrays, ptr, upload_records, workspace

AUG_HFLIP, AUG_VFLIP = 1, 2


def aug_flags(hflip=False, vflip=False, rot90=0) -> int:
    """flag word of one image: HorizontalFlip, VerticalFlip, RandomRotate90(k) — applied in that order."""
    return (AUG_HFLIP if hflip else 0) | (AUG_VFLIP if vflip else 0) | ((int(rot90) & 3) << 2)


def random_aug_flags(n: int, generator=None, p_hflip=0.5, p_vflip=0.2, p_rot90=0.3) -> torch.Tensor:
    """The geometric part of the reference's get_train_transform (dataset.py:378-384 probabilities)."""
    r = torch.rand(n, 3, generator=generator)
    k = torch.randint(1, 4, (n,), generator=generator)
    f = (r[:, 0] < p_hflip).int() | ((r[:, 1] < p_vflip).int() << 1) | (torch.where(r[:, 2] < p_rot90, k, 0).int() << 2)
    return f.to(torch.int32)


def _checked_masks(masks_u8, x):
    """masks_u8 (or None), contiguous, after the check that it goes with the (N,H,W,C) images x"""
    if masks_u8 is None:
        return None
    m = masks_u8.contiguous()
    if m.dtype != torch.uint8 or m.shape != x.shape[:3] or m.device != x.device:
        raise ValueError("masks must be uint8 (N,H,W) on the same device")
    return m


def device_preprocess(images_u8: torch.Tensor, masks_u8=None, flags=None, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                      mask_threshold: int = 127):
    """uint8 (N,H,W,C) images [+ uint8 (N,H,W) masks] on the HIP device -> (N,C,H,W) fp32 normalised images
    [+ uint8 {0,1} masks], optional per-image flip/rot90 flags (int32 tensor, see aug_flags): one kernel each —
    the tail of every get_*_transform of the reference (Normalize + ToTensorV2) and its exact geometric
    augmentations, without a host round trip or an fp32 upload."""
    x = device_u8(images_u8, 4, "device_preprocess needs a uint8 (N,H,W,C) tensor on a HIP device (no CPU fallback)")
    n, h, w, c = x.shape
    fl = None
    if flags is not None:
        fl = flags.to(device=x.device, dtype=torch.int32).contiguous()
        if fl.numel() != n:
            raise ValueError("flags must have one entry per image")
        if h != w and bool(((fl >> 2) & 3).any()):
            raise ValueError("rot90 needs square images")
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    mean_c, std_c = norm_arrays(mean, std, c)
    st = C.c_void_p(L.stream_ptr(x.device))
    L.check(L.lib().uwm_preprocess_u8(ptr(x), n, h, w, c, mean_c, std_c, ptr(fl), ptr(out), st))
    if masks_u8 is None:
        return out
    m = _checked_masks(masks_u8, x)
    mo = torch.empty((n, h, w), dtype=torch.uint8, device=x.device)
    L.check(L.lib().uwm_preprocess_mask_u8(ptr(m), n, h, w, int(mask_threshold), ptr(fl), ptr(mo), st))
    return out, mo


# ---------------------------------------------------------------------------- the descriptors and their host tables
AUG_DESC_DTYPE = np.dtype({"names": ["flags", "hue", "sat", "val", "minv", "lut"],
                           "formats": ["<i4", "<i4", "<i4", "<i4", ("<f8", (6,)), ("u1", (256,))],
                           "offsets": [0, 4, 8, 12, 16, 64], "itemsize": 320})      # = uwm_aug_desc (include/uwm.h)
AUG_EXT_DTYPE = np.dtype({"names": ["tone", "clahe_clip", "noise_sigma", "blur", "blur_w", "seed", "lut2"],
                          "formats": ["<i4", "<i4", "<i4", "<i4", ("u1", (9,)), "<u8", ("u1", (256,))],
                          "offsets": [0, 4, 8, 12, 16, 32, 40], "itemsize": 296})      # = uwm_aug_ext_desc (include/uwm.h)
IDENTITY_MINV = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
TONE_NONE, TONE_CLAHE, TONE_TABLE = 0, 1, 2
BLUR_NONE, BLUR_MOTION, BLUR_GAUSS = 0, 1, 2
NOISE_SIGMA_MAX = 16383                   # noise_sigma is sigma * 256; the kernel clamps to this
JPEG_QUALITY_RANGE = (60, 100)            # A.ImageCompression(quality_range=(60, 100)) of the transparent_watermark recipe
_AUG_COORD_LIMIT = float(1 << 29)         # fixed-point units (1/1024 pixel): half of what the kernel clamps to


def affine_inverse(h, w, angle, scale, dx, dy, shear=0.0):
    """The inverse map (6 float64, dst -> src) of ShiftScaleRotate on an h x w image: the forward matrix is
    cv2.getRotationMatrix2D((w/2 - 0.5, h/2 - 0.5), angle, scale) (degrees, counter-clockwise) with dx*w, dy*h added to its
    translations, inverted in float64 in the order of cv2.invertAffineTransform.  shear (degrees) multiplies the linear part by an
    x-shear [[1, tan(shear)], [0, 1]] about the same centre (0 leaves getRotationMatrix2D's entries as they are)."""
    cx, cy = w / 2.0 - 0.5, h / 2.0 - 0.5
    a = np.float64(angle) * (np.pi / 180.0)
    alpha, beta = np.cos(a) * np.float64(scale), np.sin(a) * np.float64(scale)
    m00, m01, m10, m11 = alpha, beta, -beta, alpha
    if shear:
        t = np.tan(np.float64(shear) * (np.pi / 180.0))
        m01, m11 = m00 * t + m01, m10 * t + m11
        m02, m12 = cx - m00 * cx - m01 * cy, cy - m10 * cx - m11 * cy
    else:
        m02, m12 = (1.0 - alpha) * cx - beta * cy, beta * cx + (1.0 - alpha) * cy
    m02, m12 = m02 + np.float64(dx) * w, m12 + np.float64(dy) * h
    det = m00 * m11 - m01 * m10
    det = 1.0 / det if det != 0.0 else 0.0
    a11, a22, a12, a21 = m11 * det, m00 * det, -m01 * det, -m10 * det
    b1, b2 = -a11 * m02 - a12 * m12, -a21 * m02 - a22 * m12
    return np.array([a11, a12, b1, a21, a22, b2], dtype=np.float64)


def brightness_contrast_lut(alpha, beta):
    """RandomBrightnessContrast's table for uint8 with brightness_by_max (the reference's transform leaves that default):
    clip(float32(v) * float32(alpha) + float32(beta * 255), 0, 255), truncated."""
    v = np.arange(256, dtype=np.float32) * np.float32(alpha) + np.float32(float(beta) * 255.0)
    return np.clip(v, 0, 255).astype(np.uint8)


def gamma_lut(gamma):
    """RandomGamma's table for uint8: trunc(((i / 255) ** gamma) * 255) in float64 (gamma = gamma_limit / 100)"""
    return ((np.arange(256, dtype=np.float64) / 255.0) ** np.float64(gamma) * 255.0).astype(np.uint8)


def motion_kernel(p0, p1) -> np.ndarray:
    """MotionBlur(blur_limit=3): the 0/1 taps (9 bytes, row by row) of the line between two DISTINCT points (x, y) of the 3 x 3
    grid: both end points and, between end points two apart, the middle point, a half rounded up (2 or 3 taps)."""
    (x0, y0), (x1, y1) = (int(p0[0]), int(p0[1])), (int(p1[0]), int(p1[1]))
    if (x0, y0) == (x1, y1) or not all(0 <= v <= 2 for v in (x0, y0, x1, y1)):
        raise ValueError("motion_kernel needs two distinct points of the 3 x 3 grid")
    k = np.zeros(9, dtype=np.uint8)
    k[3 * y0 + x0] = k[3 * y1 + x1] = 1
    if max(abs(x1 - x0), abs(y1 - y0)) == 2:
        k[3 * ((y0 + y1 + 1) // 2) + (x0 + x1 + 1) // 2] = 1
    return k


def clahe_clip_limit(clip, h, w) -> int:
    """OpenCV's integer clip limit per histogram bin for an h x w plane on 8 x 8 tiles: max(1, int(clip * tileArea / 256)), the
    tiles those of the plane padded to multiples of 8"""
    area = ((int(h) + 7) // 8) * ((int(w) + 7) // 8)
    return max(1, int(float(clip) * area / 256.0))


def identity_aug_params(n: int) -> np.ndarray:
    """n descriptors that change nothing: no flags, identity map, identity table, zero shifts"""
    p = np.zeros(int(n), AUG_DESC_DTYPE)
    p["minv"] = IDENTITY_MINV
    p["lut"] = np.arange(256, dtype=np.uint8)
    return p


def identity_aug_ext_params(n: int) -> np.ndarray:
    """n ext descriptors that change nothing: no tone stage, no noise, no blur (clahe_clip 1 and an identity lut2, both unused)"""
    e = np.zeros(int(n), AUG_EXT_DTYPE)
    e["clahe_clip"] = 1
    e["lut2"] = np.arange(256, dtype=np.uint8)
    return e


# ---------------------------------------------------------------------------- the recipes: their numbers, and the one sampler
# One entry per recipe of the reference's dataset.py, numbers only.  width: columns of the uniform block u (n, width) in [0, 1);
# draws: the integer side draws the recipe makes, in this order, after u.  A stage is (column of its probability draw, p) and then,
# per value, (column, limit) for a uniform in [-limit, limit) or (column, low, width) for one in [low, low + width); a stage a
# recipe lacks is never drawn.  hsv's limits bound the three integer shifts; a OneOf's `pick` column chooses its first member below 1/2.
_SSR = dict(p=(0, 0.3), angle=(1, 15.0), scale=(2, 0.1), shift=((3, 0.1), (4, 0.1)))       # ShiftScaleRotate, in both train transforms
RECIPES = {
    # get_train_transform (dataset.py:375-387)
    "basic": dict(width=9, draws=("hsv",), affine=_SSR,
                  brightness_contrast=dict(p=(5, 0.3), alpha=(6, 0.2), beta=(7, 0.2)),
                  hsv=dict(p=(8, 0.3), limits=(10, 20, 10))),
    # get_enhanced_train_transform (dataset.py:336-373)
    "enhanced": dict(width=17, draws=("hsv", "seeds", "ends"), affine=_SSR,
                     brightness_contrast=dict(p=(5, 0.6), alpha=(6, 0.25), beta=(7, 0.25)),
                     hsv=dict(p=(8, 0.4), limits=(12, 25, 15)),
                     tone=dict(p=(9, 0.3), pick=10, clahe_clip=(11, 1.0, 1.0), gamma=(12, 0.8, 0.4)),
                     noise=dict(p=(13, 0.2), var=(14, 5.0, 25.0)),
                     blur=dict(p=(15, 0.15), pick=16)),
    # get_transparent_watermark_transform (dataset.py:298-334); GaussNoise at albumentations 1.3's default variance
    "transparent_watermark": dict(width=13, draws=("hsv", "seeds", "ends", "quality"),
                                  affine=dict(p=(0, 0.3), angle=(1, 15.0), scale=(2, 0.1), shear=(3, 5.0)),
                                  brightness_contrast=dict(p=(4, 0.7), alpha=(5, 0.3), beta=(6, 0.3)),
                                  hsv=dict(p=(7, 0.5), limits=(15, 30, 20)),
                                  noise=dict(p=(8, 0.3), var=(9, 10.0, 40.0)),
                                  blur=dict(p=(10, 0.2), pick=11),
                                  jpeg=dict(p=(12, 0.3), quality=JPEG_QUALITY_RANGE)),
}
AUG_RECIPES = ("basic",)                  # what sample_aug_params serves
AUG_RECIPES_EXT = ("basic", "enhanced")   # what sample_aug_recipe serves


def sample_recipe(recipe, n, h, w, generator=None):
    """-> (params, ext, quality) of n h x w images drawn with the numbers of RECIPES[recipe]: one uwm_aug_desc per image, one
    uwm_aug_ext_desc (None for a recipe without tone / noise / blur stages) and one JPEG quality (int32; 0 = not drawn; None for a
    recipe without ImageCompression).  The generator is asked for random_aug_flags, then the uniform block, then the recipe's side
    draws (the three HSV shifts, the noise seeds, the two motion-blur end draws, the qualities), always in that order; each stage
    then fills in the images that drew it.  A stage that is not drawn is an exact identity.  Deterministic for a seeded torch.Generator."""
    if recipe not in RECIPES:
        raise ValueError(f"unknown augmentation recipe {recipe!r} (served: {', '.join(RECIPES)})")
    r, n = RECIPES[recipe], int(n)
    p = identity_aug_params(n)
    e = identity_aug_ext_params(n) if {"tone", "noise", "blur"} & r.keys() else None
    flags = random_aug_flags(n, generator)
    if h != w:
        flags = flags & 3                                       # RandomRotate90 needs a square image
    p["flags"] = flags.numpy()
    u = torch.rand(n, r["width"], generator=generator, dtype=torch.float64).numpy()
    randint = lambda lo, hi: torch.randint(lo, hi, (n,), generator=generator)      # noqa: E731
    quality = None
    if "hsv" in r["draws"]:
        hsv = torch.stack([randint(-lim, lim + 1) for lim in r["hsv"]["limits"]], 1).numpy()
    if "seeds" in r["draws"]:
        seeds = randint(0, 1 << 62).numpy().astype(np.uint64)
    if "ends" in r["draws"]:
        ends = torch.stack([randint(0, 9), randint(1, 9)], 1).numpy()
    if "quality" in r["draws"]:
        qual = randint(r["jpeg"]["quality"][0], r["jpeg"]["quality"][1] + 1).numpy()
        quality = np.zeros(n, dtype=np.int32)
    span = lambda i, cl: (2.0 * u[i, cl[0]] - 1.0) * cl[1] if cl else 0.0      # noqa: E731   uniform in [-limit, limit); no entry: 0
    ramp = lambda i, clw: clw[1] + clw[2] * u[i, clw[0]]                        # noqa: E731   uniform in [low, low + width)

    def drawn(stage):
        """the images that drew `stage` (none where the recipe lacks it)"""
        return np.flatnonzero(u[:, r[stage]["p"][0]] < r[stage]["p"][1]) if stage in r else ()

    a, bc = r["affine"], r["brightness_contrast"]
    for i in drawn("affine"):
        dx, dy = (span(i, cl) for cl in a.get("shift", (None, None)))
        p["minv"][i] = affine_inverse(h, w, span(i, a["angle"]), 1.0 + span(i, a["scale"]), dx, dy, shear=span(i, a.get("shear")))
    for i in drawn("brightness_contrast"):
        p["lut"][i] = brightness_contrast_lut(1.0 + span(i, bc["alpha"]), span(i, bc["beta"]))
    i = drawn("hsv")
    p["hue"][i], p["sat"][i], p["val"][i] = hsv[i].T
    for i in drawn("tone"):                                     # OneOf(CLAHE, RandomGamma)
        if u[i, r["tone"]["pick"]] < 0.5:
            e["tone"][i] = TONE_CLAHE
            e["clahe_clip"][i] = clahe_clip_limit(ramp(i, r["tone"]["clahe_clip"]), h, w)
        else:
            e["tone"][i] = TONE_TABLE
            e["lut2"][i] = gamma_lut(ramp(i, r["tone"]["gamma"]))
    for i in drawn("noise"):                                    # GaussNoise
        e["noise_sigma"][i] = int(round(np.sqrt(ramp(i, r["noise"]["var"])) * 256.0))
        e["seed"][i] = seeds[i]
    for i in drawn("blur"):                                     # OneOf(MotionBlur 3, GaussianBlur 3)
        if u[i, r["blur"]["pick"]] < 0.5:
            c0, c1 = int(ends[i, 0]), int((ends[i, 0] + ends[i, 1]) % 9)      # two distinct cells of the grid
            e["blur"][i] = BLUR_MOTION
            e["blur_w"][i] = motion_kernel((c0 % 3, c0 // 3), (c1 % 3, c1 // 3))
        else:
            e["blur"][i] = BLUR_GAUSS
    if quality is not None:                                     # ImageCompression
        i = drawn("jpeg")
        quality[i] = qual[i]
    return p, e, quality


def sample_aug_params(n, h, w, generator=None, recipe="basic") -> np.ndarray:
    """One uwm_aug_desc per image, drawn independently with the numbers of the reference's get_train_transform
    (dataset.py:379-384): flips / rot90 as random_aug_flags; ShiftScaleRotate p = 0.3 (shift +-0.1, scale 1 +- 0.1, angle +-15
    degrees); RandomBrightnessContrast p = 0.3 (limits 0.2); HueSaturationValue p = 0.3 (integer limits 10 / 20 / 10).  A stage
    that is not drawn leaves the identity map / identity table / zero shifts.  Deterministic for a seeded torch.Generator."""
    if recipe not in AUG_RECIPES:
        raise ValueError(f"unknown augmentation recipe {recipe!r} (served: {', '.join(AUG_RECIPES)})")
    return sample_recipe(recipe, n, h, w, generator)[0]


def sample_aug_recipe(n, h, w, generator=None, recipe="basic"):
    """-> (params, ext): one uwm_aug_desc and (for 'enhanced') one uwm_aug_ext_desc per image.  'basic' is sample_aug_params, byte for
    byte, with ext = None.  'enhanced' carries the numbers of the reference's get_enhanced_train_transform (dataset.py:336-373):
    flips / rot90 as random_aug_flags; ShiftScaleRotate p = 0.3 (shift +-0.1, scale 1 +- 0.1, angle +-15 degrees), as basic;
    RandomBrightnessContrast p = 0.6 (limits 0.25); HueSaturationValue p = 0.4 (12 / 25 / 15); OneOf(CLAHE clip 1..2, RandomGamma
    0.8..1.2) p = 0.3; GaussNoise var 5..30 p = 0.2; OneOf(MotionBlur 3, GaussianBlur 3) p = 0.15.  A OneOf picks one member with
    probability 1/2 each and always applies it.  A stage that is not drawn is an exact identity.  Deterministic for a seeded
    torch.Generator."""
    if recipe == "transparent_watermark":
        raise ValueError("the 'transparent_watermark' recipe has a third part, the JPEG qualities: draw it with sample_transparent_recipe")
    if recipe not in AUG_RECIPES_EXT:
        raise ValueError(f"unknown augmentation recipe {recipe!r} (served: {', '.join(AUG_RECIPES_EXT)})")
    return sample_recipe(recipe, n, h, w, generator)[:2]


def sample_transparent_recipe(n, h, w, generator=None):
    """-> (params, ext, quality): one uwm_aug_desc, one uwm_aug_ext_desc and one JPEG quality (int32) per image, with the numbers of
    the reference's get_transparent_watermark_transform (dataset.py:298-334): flips / rot90 as random_aug_flags; Affine p = 0.3
    (scale 0.9..1.1, rotate +-15 degrees, shear +-5 degrees, no translation); RandomBrightnessContrast p = 0.7 (limits 0.3);
    HueSaturationValue p = 0.5 (15 / 30 / 20); GaussNoise p = 0.3 (albumentations 1.3's default variance 10..50);
    OneOf(MotionBlur 3, GaussianBlur 3) p = 0.2; ImageCompression p = 0.3, quality an integer uniform in 60..100 inclusive, else 0
    (= not drawn: device_jpeg passes the image through).  A stage that is not drawn is an exact identity.  Deterministic for a seeded
    torch.Generator.
      Two deviations: albumentations' Affine fills the border with zeros and draws the x and y scale (and shear) separately; here the
    stage runs through the warp of uwm_augment_u8 and affine_inverse(..., shear=...), so the border is reflect-101, as for
    ShiftScaleRotate, there is one scale, and the shear is an x-shear.  Image and mask stay consistent either way."""
    return sample_recipe("transparent_watermark", n, h, w, generator)


# ---------------------------------------------------------------------------- the device calls
def _check_aug_params(params, n, h, w, c):
    p = np.ascontiguousarray(params)
    if p.dtype != AUG_DESC_DTYPE or p.ndim != 1:
        raise TypeError("params must be a 1-D array of data.AUG_DESC_DTYPE")
    if p.shape[0] != n:
        raise ValueError(f"params must have one descriptor per image ({p.shape[0]} for {n} images)")
    if h != w and bool(((p["flags"] >> 2) & 3).any()):
        raise ValueError("rot90 needs square images")
    if c != 3 and bool((p["hue"] != 0).any() or (p["sat"] != 0).any() or (p["val"] != 0).any()):
        raise ValueError("HueSaturationValue shifts need 3-channel images")
    m = p["minv"]
    if not np.isfinite(m).all():
        raise ValueError("affine matrix with a non-finite entry")
    # every fixed-point term the kernel forms is largest at a corner of the image
    reach = np.stack([np.abs(m[:, 0]) * (w - 1), np.abs(m[:, 3]) * (w - 1), np.abs(m[:, 2]), np.abs(m[:, 5]),
                      np.abs(m[:, 1] * (h - 1) + m[:, 2]), np.abs(m[:, 4] * (h - 1) + m[:, 5])])
    if not (reach * 1024.0 < _AUG_COORD_LIMIT).all():
        raise ValueError("affine matrix maps the image outside the int32 fixed-point coordinate range")
    return p


def _check_aug_ext_params(ext, n, h, w, c):
    """the host's refusals for an ext descriptor array: what the kernels would only clamp or skip"""
    e = np.ascontiguousarray(ext)
    if e.dtype != AUG_EXT_DTYPE or e.ndim != 1:
        raise TypeError("ext must be a 1-D array of data.AUG_EXT_DTYPE")
    if e.shape[0] != n:
        raise ValueError(f"ext must have one descriptor per image ({e.shape[0]} for {n} images)")
    if not np.isin(e["tone"], (TONE_NONE, TONE_CLAHE, TONE_TABLE)).all():
        raise ValueError("unknown tone stage (0 none, 1 CLAHE, 2 table)")
    if not np.isin(e["blur"], (BLUR_NONE, BLUR_MOTION, BLUR_GAUSS)).all():
        raise ValueError("unknown blur stage (0 none, 1 motion, 2 gaussian)")
    clahe = e["tone"] == TONE_CLAHE
    if clahe.any():
        if c not in (1, 3):
            raise ValueError("CLAHE needs 1-channel or 3-channel images")
        if h < 8 or w < 8:
            raise ValueError("CLAHE needs H and W >= 8 (8 x 8 tiles)")
        if (e["clahe_clip"][clahe] < 1).any():
            raise ValueError("CLAHE clip limit must be >= 1")
    if ((e["noise_sigma"] < 0) | (e["noise_sigma"] > NOISE_SIGMA_MAX)).any():
        raise ValueError(f"noise_sigma (sigma * 256) must be 0..{NOISE_SIGMA_MAX}")
    motion = e["blur"] == BLUR_MOTION
    if motion.any() and (e["blur_w"][motion] != 0).sum(1).min() == 0:
        raise ValueError("empty motion kernel (no tap set)")
    return e


def device_augment(images_u8: torch.Tensor, masks_u8, params, mean=IMAGENET_MEAN, std=IMAGENET_STD, return_u8=False,
                   mask_threshold: int = 127, ext=None):
    """uint8 (N,H,W,C) images [+ uint8 (N,H,W) masks] on the HIP device, one AUG_DESC_DTYPE record per image (sample_aug_params) ->
    (N,C,H,W) fp32 normalised images [, uint8 {0,1} masks] [, the augmented uint8 (N,H,W,C) images when return_u8]: flips / rot90 ->
    affine warp (reflect-101 border) -> brightness / contrast table -> HueSaturationValue -> Normalize in one kernel, the mask's
    nearest warp in a second (uwm_augment_u8; the rule is in include/uwm.h).  ext: one AUG_EXT_DTYPE record per image
    (sample_aug_recipe) adds tone (CLAHE / gamma) -> noise -> blur in front of Normalize (uwm_augment_ext_u8; its workspace is
    allocated once per device and reused); None (default) is the call as it was.  The descriptors are validated here, on the host:
    the kernels only clamp.  No CPU fallback."""
    x = device_u8(images_u8, 4, "device_augment needs a uint8 (N,H,W,C) tensor on a HIP device (no CPU fallback)")
    n, h, w, c = x.shape
    if not 1 <= c <= 4:
        raise ValueError(f"device_augment: C must be 1..4 (got {c})")
    p = _check_aug_params(params, n, h, w, c)
    ex = _check_aug_ext_params(ext, n, h, w, c) if ext is not None else None
    m = _checked_masks(masks_u8, x)
    dd = upload_records(p, x.device)
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    mo = torch.empty((n, h, w), dtype=torch.uint8, device=x.device) if m is not None else None
    u8 = torch.empty((n, h, w, c), dtype=torch.uint8, device=x.device) if return_u8 else None
    mean_c, std_c = norm_arrays(mean, std, c)
    with L.on_device(x):
        st = C.c_void_p(L.stream_ptr(x.device))
        if ex is None:
            L.check(L.lib().uwm_augment_u8(ptr(x), ptr(m), ptr(dd), n, h, w, c, mean_c, std_c, int(mask_threshold), ptr(out), ptr(mo),
                                           ptr(u8), st), ValueError)
        else:
            ed = upload_records(ex, x.device)
            ws = workspace("augment_ext", x.device, L.lib().uwm_augment_ext_workspace_bytes(n, h, w, c), ValueError)
            L.check(L.lib().uwm_augment_ext_u8(ptr(x), ptr(m), ptr(dd), ptr(ed), n, h, w, c, mean_c, std_c, int(mask_threshold), ptr(ws),
                                               ws.numel(), ptr(out), ptr(mo), ptr(u8), st), ValueError)
    res = (out,) + ((mo,) if m is not None else ()) + ((u8,) if return_u8 else ())
    return res[0] if len(res) == 1 else res


def device_jpeg(images_u8: torch.Tensor, quality, mean=IMAGENET_MEAN, std=IMAGENET_STD, return_u8=False):
    """A.ImageCompression on the HIP device: uint8 (N,H,W,3) RGB images, H and W multiples of 16, and one integer quality per image
    (0 = the image passes through unchanged, else 1..100; a host array, or an int32 tensor already on the device, which is then not
    checked) -> (N,3,H,W) fp32 normalised images [, the uint8 (N,H,W,3) images when return_u8]: what a baseline 4:2:0 JPEG encode +
    decode at that quality does to the pixels, bit-equal to libjpeg's default path (Pillow, cv2.imencode / imdecode), then Normalize
    (uwm_jpeg_u8; the rule is in include/uwm.h).  The workspace is allocated once per device and reused.  No CPU fallback."""
    refusal = "device_jpeg needs a uint8 (N,H,W,3) tensor on a HIP device (no CPU fallback)"
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4:
        raise RuntimeError(refusal)
    n, h, w, c = images_u8.shape
    if c != 3:
        raise ValueError(f"device_jpeg: C must be 3 (got {c})")
    if n < 1 or h < 16 or w < 16 or h % 16 or w % 16:
        raise ValueError(f"device_jpeg: H and W must be multiples of 16 (got {h} x {w})")
    on_device = isinstance(quality, torch.Tensor) and quality.device.type == "cuda"
    if on_device:
        if quality.dtype != torch.int32 or quality.numel() != n or quality.device != images_u8.device:
            raise ValueError("a device quality tensor must be int32, on the images' device, with one entry per image")
    else:
        q = np.asarray(quality)
        if q.ndim != 1 or q.shape[0] != n or not np.issubdtype(q.dtype, np.integer):
            raise ValueError(f"quality must be {n} integers, one per image")
        if ((q < 0) | (q > 100)).any():
            raise ValueError("quality must be 0 (pass through) or 1..100")
    x = device_u8(images_u8, 4, refusal)                      # (the device is looked at last: a host caller hears of its numbers first)
    qd = quality.contiguous() if on_device else upload_records(q.astype(np.int32), x.device)
    out = torch.empty((n, 3, h, w), dtype=torch.float32, device=x.device)
    u8 = torch.empty((n, h, w, 3), dtype=torch.uint8, device=x.device) if return_u8 else None
    mean_c, std_c = norm_arrays(mean, std, 3)
    with L.on_device(x):
        ws = workspace("jpeg", x.device, L.lib().uwm_jpeg_workspace_bytes(n, h, w), ValueError)
        L.check(L.lib().uwm_jpeg_u8(ptr(x), ptr(qd), n, h, w, mean_c, std_c, ptr(ws), ws.numel(), ptr(out), ptr(u8),
                                    C.c_void_p(L.stream_ptr(x.device))), ValueError)
    return (out, u8) if return_u8 else out
