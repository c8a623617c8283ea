"""Minimal data side of the boundary: tensors with the contract of the reference's dataset
(/root/reference/src/utils/dataset.py:113-122,332-333,389-395) — image fp32 NCHW normalised with the
ImageNet mean/std, mask int64 {0,1} (H,W).  A synthetic generator and a plain PIL folder reader are provided; the reference's
basic and enhanced albumentations recipes run on the device (device_augment, DeviceInputPipeline: `main.py train --augment basic` /
`--augment config`), and so does the transparent_watermark recipe, whose ImageCompression is a baseline JPEG round trip on the device
(device_jpeg, sample_transparent_recipe; `--augment config --jpeg device`).  An image without a mask file gets the
mask the reference derives from its clean counterpart, also on the device (RawPairDataset, device_pair_mask)."""
from __future__ import annotations

import os

import numpy as np
import torch
from torch.utils.data import Dataset

from .predict import IMAGENET_MEAN, IMAGENET_STD


class SyntheticWatermarkDataset(Dataset):
    """Smooth random backgrounds with a semi-transparent rectangular 'watermark'; mask = its footprint."""

    def __init__(self, length=256, img_size=512, seed=42):
        self.length, self.size, self.seed = int(length), int(img_size), int(seed)

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed * 100003 + i)
        s = self.size
        base = torch.rand(3, s // 16, s // 16, generator=g)
        img = torch.nn.functional.interpolate(base[None], size=(s, s), mode="bilinear", align_corners=False)[0]
        rh = int(torch.randint(s // 8, s // 2, (), generator=g)); rw = int(torch.randint(s // 8, s // 2, (), generator=g))
        y0 = int(torch.randint(0, s - rh, (), generator=g)); x0 = int(torch.randint(0, s - rw, (), generator=g))
        alpha = 0.3 + 0.4 * float(torch.rand((), generator=g))
        img[:, y0:y0 + rh, x0:x0 + rw] = (1 - alpha) * img[:, y0:y0 + rh, x0:x0 + rw] + alpha
        mask = torch.zeros(s, s, dtype=torch.int64)
        mask[y0:y0 + rh, x0:x0 + rw] = 1
        mean = torch.tensor(IMAGENET_MEAN).view(3, 1, 1); std = torch.tensor(IMAGENET_STD).view(3, 1, 1)
        return (img - mean) / std, mask


class FolderDataset(Dataset):
    """<root>/watermarked/*.{png,jpg} + <root>/masks/<same stem>.png (the reference's layout, dataset.py:60-84)."""

    def __init__(self, root, img_size=512):
        from PIL import Image  # noqa: F401
        self.root, self.size = root, int(img_size)
        wd = os.path.join(root, "watermarked")
        self.files = sorted(f for f in os.listdir(wd) if f.lower().endswith((".png", ".jpg", ".jpeg")))

    def __len__(self):
        return len(self.files)

    def __getitem__(self, i):
        from PIL import Image
        f = self.files[i]
        img = Image.open(os.path.join(self.root, "watermarked", f)).convert("RGB").resize((self.size, self.size), Image.BILINEAR)
        mpath = os.path.join(self.root, "masks", os.path.splitext(f)[0] + ".png")
        m = Image.open(mpath).convert("L").resize((self.size, self.size), Image.NEAREST)
        x = torch.from_numpy(np.asarray(img, dtype=np.float32) / 255.0).permute(2, 0, 1)
        mean = torch.tensor(IMAGENET_MEAN).view(3, 1, 1); std = torch.tensor(IMAGENET_STD).view(3, 1, 1)
        return (x - mean) / std, torch.from_numpy((np.asarray(m) > 127).astype(np.int64))


# ---------------------------------------------------------------------------- device-side input pipeline
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


def device_preprocess(images_u8: torch.Tensor, masks_u8=None, flags=None, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                      mask_threshold: int = 127):
    """uint8 (N,H,W,C) images [+ uint8 (N,H,W) masks] on the HIP device -> (N,C,H,W) fp32 normalised images
    [+ uint8 {0,1} masks], optional per-image flip/rot90 flags (int32 tensor, see aug_flags): one kernel each —
    the tail of every get_*_transform of the reference (Normalize + ToTensorV2) and its exact geometric
    augmentations, without a host round trip or an fp32 upload."""
    import ctypes as C
    from . import _lib as L
    if images_u8.device.type != "cuda" or images_u8.dtype != torch.uint8 or images_u8.dim() != 4:
        raise RuntimeError("device_preprocess needs a uint8 (N,H,W,C) tensor on a HIP device (no CPU fallback)")
    x = images_u8.contiguous()
    n, h, w, c = x.shape
    fl = None
    if flags is not None:
        fl = flags.to(device=x.device, dtype=torch.int32).contiguous()
        if fl.numel() != n:
            raise ValueError("flags must have one entry per image")
        if h != w and bool(((fl >> 2) & 3).any()):
            raise ValueError("rot90 needs square images")
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    mean_c = (C.c_float * c)(*[float(v) for v in mean[:c]]); std_c = (C.c_float * c)(*[float(v) for v in std[:c]])
    st = C.c_void_p(L.stream_ptr(x.device))
    L.check(L.lib().uwm_preprocess_u8(C.c_void_p(x.data_ptr()), n, h, w, c, mean_c, std_c,
                                      C.c_void_p(fl.data_ptr() if fl is not None else 0), C.c_void_p(out.data_ptr()), st))
    if masks_u8 is None:
        return out
    m = masks_u8.contiguous()
    if m.dtype != torch.uint8 or m.shape != (n, h, w) or m.device != x.device:
        raise ValueError("masks must be uint8 (N,H,W) on the same device")
    mo = torch.empty((n, h, w), dtype=torch.uint8, device=x.device)
    L.check(L.lib().uwm_preprocess_mask_u8(C.c_void_p(m.data_ptr()), n, h, w, int(mask_threshold),
                                           C.c_void_p(fl.data_ptr() if fl is not None else 0), C.c_void_p(mo.data_ptr()), st))
    return out, mo


# ---------------------------------------------------------------------------- images of any size (uwm_resize_u8, csrc/resize_u8.hip)
DESC_DTYPE = np.dtype([("offset", "<i8"), ("h", "<i4"), ("w", "<i4")])      # = uwm_image_desc (include/uwm.h), 16 bytes
INTERP = {"nearest": 0, "linear": 1}                                        # UWM_INTER_* = cv2's values


def pack_images(images, out=None):
    """A sequence of uint8 (h, w, C) arrays or tensors of ANY sizes (one C) -> (packed, descs, mask_descs): `packed` a flat uint8
    host tensor (pinned where a HIP device is present) holding the images back to back, each at a 4-byte-aligned offset; `descs`
    the uwm_image_desc array (numpy, DESC_DTYPE) of those offsets and sizes; `mask_descs` the same sizes with offsets that pack one
    h*w-byte mask per image back to back (what uwm_resize_threshold_ragged / uwm_predict_images_u8 write).  Validation is done here,
    on the host: the device kernels only clamp.  out: a flat uint8 host tensor to pack into (a caller's persistent pinned buffer);
    `packed` is then its leading slice, or a fresh tensor when `out` is too small."""
    if len(images) == 0:
        raise ValueError("pack_images: no images")
    arrs = []
    for i, im in enumerate(images):
        a = im.detach().cpu().numpy() if isinstance(im, torch.Tensor) else np.asarray(im)
        if a.dtype != np.uint8:
            raise TypeError(f"pack_images: image {i} has dtype {a.dtype}, expected uint8")
        if a.ndim != 3:
            raise ValueError(f"pack_images: image {i} has shape {a.shape}, expected (h, w, C)")
        if a.shape[0] < 1 or a.shape[1] < 1 or not 1 <= a.shape[2] <= 4:
            raise ValueError(f"pack_images: image {i} has shape {a.shape}: h, w must be >= 1 and C in 1..4")
        if arrs and a.shape[2] != arrs[0].shape[2]:
            raise ValueError(f"pack_images: image {i} has {a.shape[2]} channels, image 0 has {arrs[0].shape[2]}")
        arrs.append(a)
    descs = np.zeros(len(arrs), DESC_DTYPE)
    mask_descs = np.zeros(len(arrs), DESC_DTYPE)
    off = moff = 0
    for i, a in enumerate(arrs):
        descs[i] = (off, a.shape[0], a.shape[1])
        mask_descs[i] = (moff, a.shape[0], a.shape[1])
        off += (a.size + 3) // 4 * 4
        moff += a.shape[0] * a.shape[1]
    if out is not None and out.dtype == torch.uint8 and out.dim() == 1 and out.device.type == "cpu" and out.numel() >= off:
        packed = out[:off]
    else:
        packed = torch.empty(off, dtype=torch.uint8, pin_memory=torch.cuda.is_available())      # (the <= 3 padding bytes behind an image are never used)
    flat = packed.numpy()
    for a, d in zip(arrs, descs):
        flat[int(d["offset"]): int(d["offset"]) + a.size] = a.reshape(-1)
    return packed, descs, mask_descs


def descs_tensor(descs, device=None) -> torch.Tensor:
    """uwm_image_desc array (numpy, DESC_DTYPE) -> its bytes as a uint8 tensor (on `device` when given)."""
    d = np.ascontiguousarray(descs)
    if d.dtype != DESC_DTYPE or d.ndim != 1:
        raise TypeError("expected a 1-D array of data.DESC_DTYPE")
    t = torch.from_numpy(d.view(np.uint8).copy())
    return t if device is None else t.to(device)


def device_resize(packed: torch.Tensor, descs, size, channels: int, interp: str = "linear") -> torch.Tensor:
    """cv2.resize(image, (W, H), interpolation=INTER_LINEAR | INTER_NEAREST) of every image of a packed ragged batch
    (pack_images) on the HIP device -> uint8 (N, H, W, C): the reference's A.Resize(IMG_SIZE, IMG_SIZE) on image ('linear') and mask
    ('nearest').  The rule is the restatement in include/uwm.h (not run against cv2).  No CPU fallback."""
    import ctypes as C
    from . import _lib as L
    if interp not in INTERP:
        raise ValueError(f"interp must be 'linear' or 'nearest', got {interp!r}")
    H, W = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    src = packed if packed.device.type == "cuda" else (packed.cuda(non_blocking=True) if torch.cuda.is_available() else packed)
    if src.device.type != "cuda" or src.dtype != torch.uint8 or src.dim() != 1:
        raise RuntimeError("device_resize needs a flat uint8 tensor and a HIP device (no CPU fallback)")
    src = src.contiguous()
    dd = descs_tensor(descs, src.device) if not isinstance(descs, torch.Tensor) else descs.to(src.device)
    n = dd.numel() // DESC_DTYPE.itemsize
    out = torch.empty((n, H, W, int(channels)), dtype=torch.uint8, device=src.device)
    with L.on_device(src):
        L.check(L.lib().uwm_resize_u8(C.c_void_p(src.data_ptr()), src.numel(), C.c_void_p(dd.data_ptr()), n, int(channels), H, W,
                                      INTERP[interp], C.c_void_p(out.data_ptr()), C.c_void_p(L.stream_ptr(src.device))), ValueError)
    return out


# ---------------------------------------------------------------------------- train-time augmentation (uwm_augment_u8, csrc/augment_u8.hip)
AUG_DESC_DTYPE = np.dtype({"names": ["flags", "hue", "sat", "val", "minv", "lut"],
                           "formats": ["<i4", "<i4", "<i4", "<i4", ("<f8", (6,)), ("u1", (256,))],
                           "offsets": [0, 4, 8, 12, 16, 64], "itemsize": 320})      # = uwm_aug_desc (include/uwm.h)
IDENTITY_MINV = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
AUG_RECIPES = ("basic",)                  # the reference's get_train_transform (dataset.py:375-387)
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


def identity_aug_params(n: int) -> np.ndarray:
    """n descriptors that change nothing: no flags, identity map, identity table, zero shifts"""
    p = np.zeros(int(n), AUG_DESC_DTYPE)
    p["minv"] = IDENTITY_MINV
    p["lut"] = np.arange(256, dtype=np.uint8)
    return p


def sample_aug_params(n, h, w, generator=None, recipe="basic") -> np.ndarray:
    """One uwm_aug_desc per image, drawn independently with the numbers of the reference's get_train_transform
    (dataset.py:379-384): flips / rot90 as random_aug_flags; ShiftScaleRotate p = 0.3 (shift +-0.1, scale 1 +- 0.1, angle +-15
    degrees); RandomBrightnessContrast p = 0.3 (limits 0.2); HueSaturationValue p = 0.3 (integer limits 10 / 20 / 10).  A stage
    that is not drawn leaves the identity map / identity table / zero shifts.  Deterministic for a seeded torch.Generator."""
    if recipe not in AUG_RECIPES:
        raise ValueError(f"unknown augmentation recipe {recipe!r} (served: {', '.join(AUG_RECIPES)})")
    n = int(n)
    p = identity_aug_params(n)
    flags = random_aug_flags(n, generator)
    if h != w:
        flags = flags & 3                                       # RandomRotate90 needs a square image
    p["flags"] = flags.numpy()
    u = torch.rand(n, 9, generator=generator, dtype=torch.float64).numpy()
    hsv = torch.stack([torch.randint(-lim, lim + 1, (n,), generator=generator) for lim in (10, 20, 10)], 1).numpy()
    span = lambda col, lim: (2.0 * u[:, col] - 1.0) * lim      # noqa: E731   uniform in [-lim, lim)
    angle, scale, dx, dy = span(1, 15.0), 1.0 + span(2, 0.1), span(3, 0.1), span(4, 0.1)
    alpha, beta = 1.0 + span(6, 0.2), span(7, 0.2)
    for i in range(n):
        if u[i, 0] < 0.3:
            p["minv"][i] = affine_inverse(h, w, angle[i], scale[i], dx[i], dy[i])
        if u[i, 5] < 0.3:
            p["lut"][i] = brightness_contrast_lut(alpha[i], beta[i])
        if u[i, 8] < 0.3:
            p["hue"][i], p["sat"][i], p["val"][i] = hsv[i]
    return p


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


def device_augment(images_u8: torch.Tensor, masks_u8, params, mean=IMAGENET_MEAN, std=IMAGENET_STD, return_u8=False,
                   mask_threshold: int = 127, ext=None):
    """uint8 (N,H,W,C) images [+ uint8 (N,H,W) masks] on the HIP device, one AUG_DESC_DTYPE record per image (sample_aug_params) ->
    (N,C,H,W) fp32 normalised images [, uint8 {0,1} masks] [, the augmented uint8 (N,H,W,C) images when return_u8]: flips / rot90 ->
    affine warp (reflect-101 border) -> brightness / contrast table -> HueSaturationValue -> Normalize in one kernel, the mask's
    nearest warp in a second (uwm_augment_u8; the rule is in include/uwm.h).  ext: one AUG_EXT_DTYPE record per image
    (sample_aug_recipe) adds tone (CLAHE / gamma) -> noise -> blur in front of Normalize (uwm_augment_ext_u8; its workspace is
    allocated once per device and reused); None (default) is the call as it was.  The descriptors are validated here, on the host:
    the kernels only clamp.  No CPU fallback."""
    import ctypes as C
    from . import _lib as L
    if images_u8.device.type != "cuda" or images_u8.dtype != torch.uint8 or images_u8.dim() != 4:
        raise RuntimeError("device_augment needs a uint8 (N,H,W,C) tensor on a HIP device (no CPU fallback)")
    x = images_u8.contiguous()
    n, h, w, c = x.shape
    if not 1 <= c <= 4:
        raise ValueError(f"device_augment: C must be 1..4 (got {c})")
    p = _check_aug_params(params, n, h, w, c)
    ex = _check_aug_ext_params(ext, n, h, w, c) if ext is not None else None
    m = None
    if masks_u8 is not None:
        m = masks_u8.contiguous()
        if m.dtype != torch.uint8 or m.shape != (n, h, w) or m.device != x.device:
            raise ValueError("masks must be uint8 (N,H,W) on the same device")
    host = torch.from_numpy(p.view(np.uint8).reshape(-1).copy())
    dd = (host.pin_memory() if torch.cuda.is_available() else host).to(x.device, non_blocking=True)
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    mo = torch.empty((n, h, w), dtype=torch.uint8, device=x.device) if m is not None else None
    u8 = torch.empty((n, h, w, c), dtype=torch.uint8, device=x.device) if return_u8 else None
    mean_c = (C.c_float * c)(*[float(v) for v in mean[:c]]); std_c = (C.c_float * c)(*[float(v) for v in std[:c]])
    ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)      # noqa: E731
    with L.on_device(x):
        if ex is None:
            L.check(L.lib().uwm_augment_u8(ptr(x), ptr(m), ptr(dd), n, h, w, c, mean_c, std_c, int(mask_threshold), ptr(out), ptr(mo),
                                           ptr(u8), C.c_void_p(L.stream_ptr(x.device))), ValueError)
        else:
            ehost = torch.from_numpy(ex.view(np.uint8).reshape(-1).copy())
            ed = (ehost.pin_memory() if torch.cuda.is_available() else ehost).to(x.device, non_blocking=True)
            need = int(L.lib().uwm_augment_ext_workspace_bytes(n, h, w, c))
            ws = _ext_workspace(x.device, need)
            L.check(L.lib().uwm_augment_ext_u8(ptr(x), ptr(m), ptr(dd), ptr(ed), n, h, w, c, mean_c, std_c, int(mask_threshold), ptr(ws),
                                               ws.numel(), ptr(out), ptr(mo), ptr(u8), C.c_void_p(L.stream_ptr(x.device))), ValueError)
    res = (out,) + ((mo,) if m is not None else ()) + ((u8,) if return_u8 else ())
    return res[0] if len(res) == 1 else res


# ---------------------------------------------------------------------------- the enhanced recipe's stages (uwm_augment_ext_u8, csrc/augment_ext_u8.hip)
AUG_EXT_DTYPE = np.dtype({"names": ["tone", "clahe_clip", "noise_sigma", "blur", "blur_w", "seed", "lut2"],
                          "formats": ["<i4", "<i4", "<i4", "<i4", ("u1", (9,)), "<u8", ("u1", (256,))],
                          "offsets": [0, 4, 8, 12, 16, 32, 40], "itemsize": 296})      # = uwm_aug_ext_desc (include/uwm.h)
TONE_NONE, TONE_CLAHE, TONE_TABLE = 0, 1, 2
BLUR_NONE, BLUR_MOTION, BLUR_GAUSS = 0, 1, 2
NOISE_SIGMA_MAX = 16383                   # noise_sigma is sigma * 256; the kernel clamps to this
AUG_RECIPES_EXT = ("basic", "enhanced")   # what sample_aug_recipe serves (get_train_transform, get_enhanced_train_transform)


def identity_aug_ext_params(n: int) -> np.ndarray:
    """n ext descriptors that change nothing: no tone stage, no noise, no blur (clahe_clip 1 and an identity lut2, both unused)"""
    e = np.zeros(int(n), AUG_EXT_DTYPE)
    e["clahe_clip"] = 1
    e["lut2"] = np.arange(256, dtype=np.uint8)
    return e


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


def sample_aug_recipe(n, h, w, generator=None, recipe="basic"):
    """-> (params, ext): one uwm_aug_desc and (for 'enhanced') one uwm_aug_ext_desc per image.  'basic' is sample_aug_params, byte for
    byte, with ext = None.  'enhanced' carries the numbers of the reference's get_enhanced_train_transform (dataset.py:336-373):
    flips / rot90 as random_aug_flags; ShiftScaleRotate p = 0.3 (shift +-0.1, scale 1 +- 0.1, angle +-15 degrees), as basic;
    RandomBrightnessContrast p = 0.6 (limits 0.25); HueSaturationValue p = 0.4 (12 / 25 / 15); OneOf(CLAHE clip 1..2, RandomGamma
    0.8..1.2) p = 0.3; GaussNoise var 5..30 p = 0.2; OneOf(MotionBlur 3, GaussianBlur 3) p = 0.15.  A OneOf picks one member with
    probability 1/2 each and always applies it.  A stage that is not drawn is an exact identity.  Deterministic for a seeded
    torch.Generator."""
    if recipe == "basic":
        return sample_aug_params(n, h, w, generator, "basic"), None
    if recipe == "transparent_watermark":
        raise ValueError("the 'transparent_watermark' recipe has a third part, the JPEG qualities: draw it with sample_transparent_recipe")
    if recipe != "enhanced":
        raise ValueError(f"unknown augmentation recipe {recipe!r} (served: {', '.join(AUG_RECIPES_EXT)})")
    n = int(n)
    p, e = identity_aug_params(n), identity_aug_ext_params(n)
    flags = random_aug_flags(n, generator)
    if h != w:
        flags = flags & 3
    p["flags"] = flags.numpy()
    u = torch.rand(n, 17, generator=generator, dtype=torch.float64).numpy()
    hsv = torch.stack([torch.randint(-lim, lim + 1, (n,), generator=generator) for lim in (12, 25, 15)], 1).numpy()
    seeds = torch.randint(0, 1 << 62, (n,), generator=generator).numpy().astype(np.uint64)
    ends = torch.stack([torch.randint(0, 9, (n,), generator=generator), torch.randint(1, 9, (n,), generator=generator)], 1).numpy()
    span = lambda col, lim: (2.0 * u[:, col] - 1.0) * lim      # noqa: E731   uniform in [-lim, lim)
    angle, scale, dx, dy = span(1, 15.0), 1.0 + span(2, 0.1), span(3, 0.1), span(4, 0.1)
    alpha, beta = 1.0 + span(6, 0.25), span(7, 0.25)
    for i in range(n):
        if u[i, 0] < 0.3:
            p["minv"][i] = affine_inverse(h, w, angle[i], scale[i], dx[i], dy[i])
        if u[i, 5] < 0.6:
            p["lut"][i] = brightness_contrast_lut(alpha[i], beta[i])
        if u[i, 8] < 0.4:
            p["hue"][i], p["sat"][i], p["val"][i] = hsv[i]
        if u[i, 9] < 0.3:
            if u[i, 10] < 0.5:
                e["tone"][i] = TONE_CLAHE
                e["clahe_clip"][i] = clahe_clip_limit(1.0 + u[i, 11], h, w)
            else:
                e["tone"][i] = TONE_TABLE
                e["lut2"][i] = gamma_lut(0.8 + 0.4 * u[i, 12])
        if u[i, 13] < 0.2:
            e["noise_sigma"][i] = int(round(np.sqrt(5.0 + 25.0 * u[i, 14]) * 256.0))
            e["seed"][i] = seeds[i]
        if u[i, 15] < 0.15:
            if u[i, 16] < 0.5:
                a, b = int(ends[i, 0]), int((ends[i, 0] + ends[i, 1]) % 9)      # two distinct cells of the grid
                e["blur"][i] = BLUR_MOTION
                e["blur_w"][i] = motion_kernel((a % 3, a // 3), (b % 3, b // 3))
            else:
                e["blur"][i] = BLUR_GAUSS
    return p, e


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


_EXT_WORKSPACE = {}


def _ext_workspace(device, nbytes):
    """one workspace per device, grown when a larger one is needed (calls on one stream are ordered, so it is reused)"""
    ws = _EXT_WORKSPACE.get(device)
    if ws is None or ws.numel() < nbytes:
        ws = _EXT_WORKSPACE[device] = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    return ws


# ---------------------------------------------------------------------------- ImageCompression (uwm_jpeg_u8, csrc/jpeg_u8.hip)
JPEG_QUALITY_RANGE = (60, 100)            # A.ImageCompression(quality_range=(60, 100)) of the transparent_watermark recipe
_JPEG_WORKSPACE = {}


def _jpeg_workspace(device, nbytes):
    """as _ext_workspace: one per device, grown when a larger one is needed"""
    ws = _JPEG_WORKSPACE.get(device)
    if ws is None or ws.numel() < nbytes:
        ws = _JPEG_WORKSPACE[device] = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    return ws


def device_jpeg(images_u8: torch.Tensor, quality, mean=IMAGENET_MEAN, std=IMAGENET_STD, return_u8=False):
    """A.ImageCompression on the HIP device: uint8 (N,H,W,3) RGB images, H and W multiples of 16, and one integer quality per image
    (0 = the image passes through unchanged, else 1..100; a host array, or an int32 tensor already on the device, which is then not
    checked) -> (N,3,H,W) fp32 normalised images [, the uint8 (N,H,W,3) images when return_u8]: what a baseline 4:2:0 JPEG encode +
    decode at that quality does to the pixels, bit-equal to libjpeg's default path (Pillow, cv2.imencode / imdecode), then Normalize
    (uwm_jpeg_u8; the rule is in include/uwm.h).  The workspace is allocated once per device and reused.  No CPU fallback."""
    import ctypes as C
    from . import _lib as L
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4:
        raise RuntimeError("device_jpeg needs a uint8 (N,H,W,3) tensor on a HIP device (no CPU fallback)")
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
    if images_u8.device.type != "cuda":
        raise RuntimeError("device_jpeg needs a uint8 (N,H,W,3) tensor on a HIP device (no CPU fallback)")
    x = images_u8.contiguous()
    if on_device:
        qd = quality.contiguous()
    else:
        host = torch.from_numpy(q.astype(np.int32))
        qd = host.pin_memory().to(x.device, non_blocking=True)
    out = torch.empty((n, 3, h, w), dtype=torch.float32, device=x.device)
    u8 = torch.empty((n, h, w, 3), dtype=torch.uint8, device=x.device) if return_u8 else None
    mean_c = (C.c_float * 3)(*[float(v) for v in mean[:3]]); std_c = (C.c_float * 3)(*[float(v) for v in std[:3]])
    with L.on_device(x):
        ws = _jpeg_workspace(x.device, int(L.lib().uwm_jpeg_workspace_bytes(n, h, w)))
        L.check(L.lib().uwm_jpeg_u8(C.c_void_p(x.data_ptr()), C.c_void_p(qd.data_ptr()), n, h, w, mean_c, std_c, C.c_void_p(ws.data_ptr()),
                                    ws.numel(), C.c_void_p(out.data_ptr()), C.c_void_p(u8.data_ptr() if u8 is not None else 0),
                                    C.c_void_p(L.stream_ptr(x.device))), ValueError)
    return (out, u8) if return_u8 else out


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
    n = int(n)
    p, e = identity_aug_params(n), identity_aug_ext_params(n)
    flags = random_aug_flags(n, generator)
    if h != w:
        flags = flags & 3
    p["flags"] = flags.numpy()
    u = torch.rand(n, 13, generator=generator, dtype=torch.float64).numpy()
    hsv = torch.stack([torch.randint(-lim, lim + 1, (n,), generator=generator) for lim in (15, 30, 20)], 1).numpy()
    seeds = torch.randint(0, 1 << 62, (n,), generator=generator).numpy().astype(np.uint64)
    ends = torch.stack([torch.randint(0, 9, (n,), generator=generator), torch.randint(1, 9, (n,), generator=generator)], 1).numpy()
    qual = torch.randint(JPEG_QUALITY_RANGE[0], JPEG_QUALITY_RANGE[1] + 1, (n,), generator=generator).numpy()
    span = lambda col, lim: (2.0 * u[:, col] - 1.0) * lim      # noqa: E731   uniform in [-lim, lim)
    angle, scale, shear = span(1, 15.0), 1.0 + span(2, 0.1), span(3, 5.0)
    alpha, beta = 1.0 + span(5, 0.3), span(6, 0.3)
    quality = np.zeros(n, dtype=np.int32)
    for i in range(n):
        if u[i, 0] < 0.3:
            p["minv"][i] = affine_inverse(h, w, angle[i], scale[i], 0.0, 0.0, shear=shear[i])
        if u[i, 4] < 0.7:
            p["lut"][i] = brightness_contrast_lut(alpha[i], beta[i])
        if u[i, 7] < 0.5:
            p["hue"][i], p["sat"][i], p["val"][i] = hsv[i]
        if u[i, 8] < 0.3:
            e["noise_sigma"][i] = int(round(np.sqrt(10.0 + 40.0 * u[i, 9]) * 256.0))
            e["seed"][i] = seeds[i]
        if u[i, 10] < 0.2:
            if u[i, 11] < 0.5:
                a, b = int(ends[i, 0]), int((ends[i, 0] + ends[i, 1]) % 9)      # two distinct cells of the grid
                e["blur"][i] = BLUR_MOTION
                e["blur_w"][i] = motion_kernel((a % 3, a // 3), (b % 3, b // 3))
            else:
                e["blur"][i] = BLUR_GAUSS
        if u[i, 12] < 0.3:
            quality[i] = qual[i]
    return p, e, quality


# ---------------------------------------------------------------------------- the device input path of `main.py train --augment basic`
class RawFolderDataset(Dataset):
    """FolderDataset's files, decoded and nothing else: (image uint8 (h, w, 3) RGB, mask uint8 (h, w)) numpy arrays at the file's
    own size.  Resize, augmentation and Normalize happen on the device (DeviceInputPipeline)."""

    def __init__(self, root):
        from PIL import Image  # noqa: F401
        self.root = root
        wd = os.path.join(root, "watermarked")
        self.files = sorted(f for f in os.listdir(wd) if f.lower().endswith((".png", ".jpg", ".jpeg")))

    def __len__(self):
        return len(self.files)

    def __getitem__(self, i):
        from PIL import Image
        f = self.files[i]
        img = np.asarray(Image.open(os.path.join(self.root, "watermarked", f)).convert("RGB"), dtype=np.uint8)
        m = np.asarray(Image.open(os.path.join(self.root, "masks", os.path.splitext(f)[0] + ".png")).convert("L"), dtype=np.uint8)
        return img, m


# ---------------------------------------------------------------------------- masks from watermarked / clean pairs (uwm_pair_mask_u8, csrc/pair_mask_u8.hip)
def mask_descs_for(descs) -> np.ndarray:
    """uwm_image_desc array of images -> the same sizes with offsets that pack one h*w-byte mask per image back to back
    (pack_images' third result)"""
    m = np.zeros(len(descs), DESC_DTYPE)
    m["h"], m["w"] = descs["h"], descs["w"]
    sizes = descs["h"].astype(np.int64) * descs["w"].astype(np.int64)
    m["offset"] = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    return m


def device_pair_mask(packed_wm, wm_descs, packed_clean, clean_descs, threshold, open=True, mask=None, mask_descs=None) -> torch.Tensor:
    """The reference's WatermarkDataset._generate_mask (use_blurred_mask = False) for every pair of a ragged batch on the HIP device:
    mask_i = open3(gray(|wm_i - clean_i|) > threshold) at the image's own size, {0, 255} (uwm_pair_mask_u8; the rule is in
    include/uwm.h).  packed_wm / packed_clean: flat uint8 tensors of RGB images (pack_images) with their uwm_image_desc arrays; a
    clean descriptor with h == 0 skips that image (its mask bytes stay), a pair whose sizes differ gets a zero mask — bring such a
    clean image to the watermarked size with uwm_resize_u8 first.  mask / mask_descs: a packed mask buffer on the device to write
    into (e.g. one that already holds the masks read from files); absent, one is made, zero-filled, with the layout of
    mask_descs_for(wm_descs).  -> the packed mask (flat uint8, on the device).  No CPU fallback."""
    import ctypes as C
    from . import _lib as L
    t = int(threshold)
    if not 0 <= t <= 255:
        raise ValueError(f"device_pair_mask: threshold must be 0..255 (got {threshold})")
    wd, cd = np.ascontiguousarray(wm_descs), np.ascontiguousarray(clean_descs)
    if wd.dtype != DESC_DTYPE or cd.dtype != DESC_DTYPE or wd.ndim != 1 or wd.shape != cd.shape or len(wd) == 0:
        raise ValueError("device_pair_mask: wm_descs and clean_descs must be 1-D data.DESC_DTYPE arrays of one length")
    if (mask is None) != (mask_descs is None):
        raise ValueError("device_pair_mask: mask and mask_descs come together")
    md = mask_descs_for(wd) if mask_descs is None else np.ascontiguousarray(mask_descs)
    if md.dtype != DESC_DTYPE or md.shape != wd.shape:
        raise ValueError("device_pair_mask: mask_descs must be a data.DESC_DTYPE array with one entry per image")
    wm = packed_wm if packed_wm.device.type == "cuda" else (packed_wm.cuda(non_blocking=True) if torch.cuda.is_available() else packed_wm)
    if wm.device.type != "cuda" or wm.dtype != torch.uint8 or wm.dim() != 1:
        raise RuntimeError("device_pair_mask needs flat uint8 tensors and a HIP device (no CPU fallback)")
    cl = packed_clean.to(wm.device, non_blocking=True)
    if cl.dtype != torch.uint8 or cl.dim() != 1:
        raise RuntimeError("device_pair_mask needs flat uint8 tensors and a HIP device (no CPU fallback)")
    if mask is None:
        mask = torch.zeros(max(1, int((md["h"].astype(np.int64) * md["w"]).sum())), dtype=torch.uint8, device=wm.device)
    elif mask.device != wm.device or mask.dtype != torch.uint8 or mask.dim() != 1 or not mask.is_contiguous():
        raise ValueError("device_pair_mask: mask must be a flat contiguous uint8 tensor on the images' device")
    wm, cl = wm.contiguous(), cl.contiguous()
    dd = descs_tensor(np.concatenate([wd, cd, md]), wm.device)                 # one upload; 16-byte records keep every part 8-byte aligned
    n, step = len(wd), len(wd) * DESC_DTYPE.itemsize
    with L.on_device(wm):
        L.check(L.lib().uwm_pair_mask_u8(C.c_void_p(wm.data_ptr()), wm.numel(), C.c_void_p(dd.data_ptr()), C.c_void_p(cl.data_ptr()), cl.numel(),
                                         C.c_void_p(dd.data_ptr() + step), n, 3, t, int(bool(open)), C.c_void_p(mask.data_ptr()), mask.numel(),
                                         C.c_void_p(dd.data_ptr() + 2 * step), C.c_void_p(L.stream_ptr(wm.device))), ValueError)
    return mask


def stage_clean(cleans, wm_descs, device, upload=None):
    """The clean images of a batch on the device, each at its watermarked image's size: cleans holds a uint8 (h, w, 3) array or None
    per image, wm_descs the watermarked images' descriptors.  The arrays are packed and uploaded (upload(arrays, extra_bytes) ->
    (flat device tensor with extra_bytes spare bytes behind the packed images, descs); default: pack_images + a fresh tensor); a clean
    image of another size is then resized by uwm_resize_u8 (LINEAR: cv2.resize's default, as the reference calls it) into the spare
    bytes, one launch per such image.  -> (flat device tensor, clean_descs) for device_pair_mask: h == 0 where cleans[i] is None;
    (None, None) when every entry is None."""
    import ctypes as C
    from . import _lib as L
    have = [i for i, c in enumerate(cleans) if c is not None]
    if not have:
        return None, None
    arrays = [np.ascontiguousarray(cleans[i]) for i in have]
    for i, a in zip(have, arrays):
        if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
            raise ValueError(f"clean image {i} has shape {a.shape}, dtype {a.dtype}: expected uint8 (h, w, 3)")
    odd = [(k, i) for k, i in enumerate(have) if arrays[k].shape[:2] != (int(wm_descs[i]["h"]), int(wm_descs[i]["w"]))]
    spare = [(int(wm_descs[i]["h"]) * int(wm_descs[i]["w"]) * 3 + 3) // 4 * 4 for _, i in odd]
    if upload is None:
        def upload(arrs, extra):
            packed, d, _ = pack_images(arrs)
            dev = torch.empty(packed.numel() + extra, dtype=torch.uint8, device=device)
            dev[:packed.numel()].copy_(packed, non_blocking=True)
            return dev, d
    dev, d = upload(arrays, sum(spare))
    used = dev.numel() - sum(spare)
    cd = np.zeros(len(cleans), DESC_DTYPE)
    for k, i in enumerate(have):
        cd[i] = d[k]
    if odd:
        dd = descs_tensor(d, dev.device)
        off = used
        with L.on_device(dev):
            for (k, i), nbytes in zip(odd, spare):
                h, w = int(wm_descs[i]["h"]), int(wm_descs[i]["w"])
                L.check(L.lib().uwm_resize_u8(C.c_void_p(dev.data_ptr()), used, C.c_void_p(dd.data_ptr() + k * DESC_DTYPE.itemsize), 1, 3, h, w,
                                              INTERP["linear"], C.c_void_p(dev.data_ptr() + off), C.c_void_p(L.stream_ptr(dev.device))),
                        ValueError)
                cd[i] = (off, h, w)
                off += nbytes
    return dev, cd


PAIR_IMAGE_EXTENSIONS = (".jpg", ".jpeg", ".png", ".bmp", ".tiff", ".tif")      # the reference's _collect_image_files


class RawPairDataset(Dataset):
    """The reference's dataset contract, decoded and nothing else: roots = [DATA.ROOT_DIR] + DATA.ADDITIONAL_ROOT_DIRS, each with
    watermarked/, clean/ and masks/.  The file list is every image file of every watermarked/ directory, sorted by path
    (dataset.py:57-69).  An image's mask is <stem>.png in the FIRST masks/ directory (in root order) that has a readable one; failing
    that, its clean counterpart is the file of the SAME NAME in the first clean/ directory that has a readable one
    (dataset.py:158-195).  Items are (image uint8 (h, w, 3) RGB, mask uint8 (h, w) or None, clean uint8 (h', w', 3) or None); the
    clean image is only read when there is no mask.  DeviceInputPipeline derives the missing masks on the device with
    `mask_threshold` (DATA.GENERATE_MASK_THRESHOLD); an image with neither gets a zero mask."""

    def __init__(self, roots, mask_threshold):
        from PIL import Image  # noqa: F401
        self.roots = [roots] if isinstance(roots, (str, os.PathLike)) else list(roots)
        if not self.roots:
            raise ValueError("RawPairDataset: no root directory")
        self.mask_threshold = int(mask_threshold)
        if not 0 <= self.mask_threshold <= 255:
            raise ValueError(f"RawPairDataset: mask_threshold must be 0..255 (got {mask_threshold})")
        files = []
        for root in self.roots:
            wd = os.path.join(root, "watermarked")
            if os.path.isdir(wd):
                files += [os.path.join(wd, f) for f in os.listdir(wd) if f.lower().endswith(PAIR_IMAGE_EXTENSIONS)]
        self.files = sorted(files)
        self.mask_dirs = [os.path.join(r, "masks") for r in self.roots]
        self.clean_dirs = [os.path.join(r, "clean") for r in self.roots]

    def __len__(self):
        return len(self.files)

    def mask_paths(self, i):
        """the existing mask files of image i, in lookup order"""
        name = os.path.splitext(os.path.basename(self.files[i]))[0] + ".png"
        return [p for p in (os.path.join(d, name) for d in self.mask_dirs) if os.path.exists(p)]

    def clean_paths(self, i):
        name = os.path.basename(self.files[i])
        return [p for p in (os.path.join(d, name) for d in self.clean_dirs) if os.path.exists(p)]

    def missing_masks(self):
        """indices of the images without a mask file"""
        return [i for i in range(len(self.files)) if not self.mask_paths(i)]

    @staticmethod
    def _read(paths, mode):
        from PIL import Image
        for p in paths:
            try:
                return np.asarray(Image.open(p).convert(mode), dtype=np.uint8)
            except (OSError, ValueError):          # unreadable: the reference goes on to the next directory
                continue
        return None

    def __getitem__(self, i):
        from PIL import Image
        img = np.asarray(Image.open(self.files[i]).convert("RGB"), dtype=np.uint8)
        m = self._read(self.mask_paths(i), "L")
        clean = self._read(self.clean_paths(i), "RGB") if m is None else None
        return img, m, clean


class DeviceU8Dataset(Dataset):
    """A dataset of (normalised fp32 image, {0,1} mask) pairs (SyntheticWatermarkDataset) converted ONCE to uint8 tensors on the
    device: images (n, S, S, C), masks (n, S, S) in {0, 255}.  Items are indices; DeviceInputPipeline gathers them on the device."""

    def __init__(self, base, device, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        xs, ms = zip(*(base[i] for i in range(len(base))))
        x = torch.stack(xs).to(device)
        c = x.shape[1]
        mean_t = torch.tensor(mean[:c], device=device).view(1, c, 1, 1); std_t = torch.tensor(std[:c], device=device).view(1, c, 1, 1)
        self.images = ((x * std_t + mean_t) * 255.0).round_().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        self.masks = (torch.stack(ms).to(device) > 0).to(torch.uint8) * 255

    def __len__(self):
        return self.images.shape[0]

    def __getitem__(self, i):
        return int(i)


# ---------------------------------------------------------------------------- logo-watermarked samples (uwm_synth_u8, csrc/synth_u8.hip)
SYNTH_JOB_DTYPE = np.dtype([("enabled", "<i4"), ("logo", "<i4"), ("w1", "<i4"), ("h1", "<i4"), ("rotate", "<i4"), ("w2", "<i4"), ("h2", "<i4"),
                            ("stretch", "<i4"), ("w3", "<i4"), ("h3", "<i4"), ("shear", "<i4"), ("blur", "<i4"), ("blur_r", "<i4"),
                            ("blur_ww", "<u4"), ("blur_fw", "<u4"), ("ndefects", "<i4"), ("defects", "<i4", (3, 4)), ("enhance", "<i4"),
                            ("brightness", "<f4"), ("contrast", "<f4"), ("color", "<f4"), ("x", "<i4"), ("y", "<i4"),
                            ("rot", "<f8", (6,)), ("shear_minv", "<f8", (6,)), ("opacity", "u1", (256,))])      # = uwm_synth_job, 488 bytes
assert SYNTH_JOB_DTYPE.itemsize == 488
SYNTH_SLOTS = 3                           # K: the reference pastes one to three logos
SYNTH_MAX_SLOTS = 8                       # what the kernels serve
SYNTH_MAX_SIDE = 32767
LOGO_SUBDIRS = ("combined", "independent", "car_logo")        # gen_data.py's load_watermarks
LOGO_EXTENSIONS = (".png", ".jpg", ".jpeg")


def empty_synth_jobs(*shape) -> np.ndarray:
    """job records with every stage off, every slot empty and the identity opacity table"""
    j = np.zeros(shape, SYNTH_JOB_DTYPE)
    j["opacity"] = np.arange(256, dtype=np.uint8)
    j["rot"] = IDENTITY_MINV; j["shear_minv"] = IDENTITY_MINV
    return j


def synth_rotate_setup(w, h, angle):
    """Image.rotate(angle, expand=True)'s host arithmetic -> (matrix of 6 floats, expanded width, expanded height)"""
    import math
    angle = angle % 360.0
    cx, cy = w / 2.0, h / 2.0
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]

    def tr(x, y):
        return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]

    m[2], m[5] = tr(-cx, -cy)
    m[2] += cx; m[5] += cy
    xs, ys = zip(*(tr(x, y) for x, y in ((0, 0), (w, 0), (w, h), (0, h))))
    nw = math.ceil(max(xs)) - math.floor(min(xs)); nh = math.ceil(max(ys)) - math.floor(min(ys))
    m[2], m[5] = tr(-(nw - w) / 2.0, -(nh - h) / 2.0)
    return m, int(nw), int(nh)


def synth_shear_inverse(sx, sy):
    """cv2.warpAffine's float64 inverse of M = [[1, sx, 0], [sy, 1, 0]] held as float32 (restated, not run against cv2)"""
    M = [1.0, float(np.float32(sx)), 0.0, float(np.float32(sy)), 1.0, 0.0]
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[4] * D, M[0] * D
    M[0] = A11; M[1] *= -D; M[3] *= -D; M[4] = A22
    return [M[0], M[1], -M[0] * M[2] - M[1] * M[5], M[3], M[4], -M[3] * M[2] - M[4] * M[5]]


def synth_blur_params(radius):
    """Pillow's _gaussian_blur_radius (3 passes) and ImagingHorizontalBoxBlur's weights, in C's float / double mix -> (R, ww, fw)"""
    import math
    f32 = np.float32
    r = f32(radius)
    sigma2 = f32(f32(r * r) / f32(3))
    L = f32(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = f32(math.floor((float(L) - 1.0) / 2.0))
    a = f32(f32(f32(2) * l + f32(1)) * f32(f32(l * f32(l + f32(1))) - f32(f32(3) * sigma2)))
    a = f32(a / f32(f32(6) * f32(sigma2 - f32(f32(l + f32(1)) * f32(l + f32(1))))))
    fr = f32(l + a)
    R = int(fr)
    ww = int(f32(f32(1 << 24) / f32(f32(fr * f32(2)) + f32(1))))
    return R, ww, (((1 << 24) - (2 * R + 1) * ww) & 0xFFFFFFFF) // 2


def synth_opacity_lut(alpha):
    return (np.arange(256, dtype=np.uint8) * float(alpha)).astype(np.uint8)


def _overlap_area(r1, r2):
    x1, y1, x2, y2 = max(r1[0], r2[0]), max(r1[1], r2[1]), min(r1[2], r2[2]), min(r1[3], r2[3])
    return (x2 - x1) * (y2 - y1) if x2 > x1 and y2 > y1 else 0


def _sample_effects(rng, jobs, k, lw, lh, W, H, enhance_transparent):
    """apply_watermark_effects' draws, in its order, into job record k -> the processed patch's (w, h), or None when a size reaches 0
    (Pillow's resize raises there and the reference goes on to the next logo; no further number is drawn)"""
    scale = rng.uniform(0.03, 0.35)
    w = int(W * scale)
    h = int(lh * w / lw)
    if h > H * 0.35:
        h = int(H * 0.35)
        w = int(lw * h / lh)
    if w < 1 or h < 1:
        return None
    jobs["w1"][k], jobs["h1"][k] = w, h
    if rng.random() < 0.8:
        angle = rng.uniform(0, 360)
        if angle % 360.0 != 0.0:
            m, w, h = synth_rotate_setup(w, h, angle)
            jobs["rotate"][k], jobs["rot"][k], jobs["w2"][k], jobs["h2"][k] = 1, m, w, h
    if rng.random() < 0.75:
        hs, vs = rng.uniform(0.6, 1.6), rng.uniform(0.6, 1.6)
        w, h = int(w * hs), int(h * vs)
        if w < 1 or h < 1:
            return None
        jobs["stretch"][k], jobs["w3"][k], jobs["h3"][k] = 1, w, h
        if rng.random() < 0.6:
            sx, sy = rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4)
            jobs["shear"][k], jobs["shear_minv"][k] = 1, synth_shear_inverse(sx, sy)
    if rng.random() < 0.4:
        jobs["blur"][k] = 1
        jobs["blur_r"][k], jobs["blur_ww"][k], jobs["blur_fw"][k] = synth_blur_params(rng.uniform(0.5, 2.5))
    if rng.random() < 0.3:
        n = rng.randint(1, 3)
        for d in range(n):
            dw, dh = rng.randint(int(w * 0.05), int(w * 0.2)), rng.randint(int(h * 0.05), int(h * 0.2))
            jobs["defects"][k, d] = (rng.randint(0, max(0, w - dw)), rng.randint(0, max(0, h - dh)), dw, dh)
        jobs["ndefects"][k] = n
    alpha = rng.uniform(0.08, 0.45) if enhance_transparent else rng.uniform(0.25, 0.85)
    jobs["enhance"][k] = 1
    jobs["brightness"][k], jobs["contrast"][k], jobs["color"][k] = rng.uniform(0.4, 1.8), rng.uniform(0.5, 1.6), rng.uniform(0.5, 1.5)
    jobs["opacity"][k] = synth_opacity_lut(alpha)
    return w, h


def _plain_job(rng, jobs, k, lw, lh, W, H):
    """resize_watermark(original, size, 0.02, 0.12): job record k becomes stage 1 only -> (w, h) or None"""
    jobs[k] = empty_synth_jobs(1)[0]
    jobs["logo"][k] = k
    scale = rng.uniform(0.02, 0.12)
    w = int(W * scale)
    h = int(lh * w / lw)
    if h > H * 0.12:
        h = int(H * 0.12)
        w = int(lw * h / lh)
    if w < 1 or h < 1:
        return None
    jobs["w1"][k], jobs["h1"][k] = w, h
    return w, h


def sample_synth_jobs(rng, image_size, logo_sizes, enhance_transparent=True, slots=SYNTH_SLOTS):
    """The host side of generate_multiple_watermarks_image for ONE image: `rng` a seeded random.Random (the script's own generator
    type, so uniform / randint / random mean what they mean there), image_size = (W, H), logo_sizes = [(w, h), ...] the chosen logos
    in paste order (at most `slots`).  Draws every effect parameter in the script's order, derives every size, runs the placement
    loop (20 attempts; accepted when the overlap with every placed rectangle is under 30 % of the patch, or when it is the first; an
    oversized patch falls back to the plain resize_watermark(.., 0.02, 0.12); a first logo that never fitted is placed anyway) and
    returns `slots` records of SYNTH_JOB_DTYPE whose `logo` is the index into logo_sizes.  A logo whose size reaches 0 is dropped
    (enabled = 0), as the reference's `except: continue` does."""
    W, H = int(image_size[0]), int(image_size[1])
    if len(logo_sizes) > slots:
        raise ValueError(f"sample_synth_jobs: {len(logo_sizes)} logos for {slots} slots")
    jobs = empty_synth_jobs(slots)
    placed = []
    for k, (lw, lh) in enumerate(logo_sizes):
        jobs["logo"][k] = k
        size = _sample_effects(rng, jobs, k, int(lw), int(lh), W, H, enhance_transparent)
        if size is None:
            continue
        done = False
        max_x = max_y = 0
        for _ in range(20):
            max_x, max_y = W - size[0], H - size[1]
            if max_x <= 0 or max_y <= 0:
                size = _plain_job(rng, jobs, k, int(lw), int(lh), W, H)
                if size is None:
                    break
                max_x, max_y = W - size[0], H - size[1]
            if max_x <= 0 or max_y <= 0:
                break
            x, y = rng.randint(0, max_x), rng.randint(0, max_y)
            region = (x, y, x + size[0], y + size[1])
            ratio = max([_overlap_area(region, r) / (size[0] * size[1]) for r in placed], default=0)
            if ratio < 0.3 or not placed:
                jobs["x"][k], jobs["y"][k], jobs["enabled"][k] = x, y, 1
                placed.append(region)
                done = True
                break
        if size is None:
            continue
        if not done and not placed:
            jobs["x"][k], jobs["y"][k], jobs["enabled"][k] = rng.randint(0, max(0, max_x)), rng.randint(0, max(0, max_y)), 1
    return jobs


def sample_synth_choice(rng, num_logos, transparent_ratio=0.6, multi_watermark_ratio=0.4, max_watermarks=3):
    """gen_data.py main()'s choices for one sample, logo branch only -> (enhance_transparent, [indices of the logos to paste]).  One
    departure: main() also makes the first count*ratio samples transparent whatever the draw; that quota needs the run's state, so
    here the draw alone decides."""
    transparent = rng.random() < transparent_ratio
    single = rng.randrange(num_logos)
    if rng.random() < multi_watermark_ratio and num_logos > 1 and max_watermarks >= 2:
        chosen = rng.sample(range(num_logos), min(rng.randint(2, max_watermarks), num_logos))
        limit = max_watermarks
    else:
        chosen, limit = [single], 1
    n = rng.randint(1, limit)                                  # generate_multiple_watermarks_image's own count
    if len(chosen) == 1:
        picked = chosen * n
    else:
        picked = rng.sample(chosen, min(n, len(chosen)))
        while len(picked) < n:
            picked.append(rng.choice(chosen))
    return transparent, picked


def synth_job_needs(jobs, logo_descs):
    """-> (max_patch_pixels, max_taps) that uwm_synth_u8 needs to run every enabled job: the largest logo, intermediate or final patch
    and the largest coefficient table (out * (ksize + 2)), both at least 1"""
    import math
    need = [1, 1]

    def table(n_in, n_out):
        return n_out * (int(math.ceil(3.0 * max(n_in / n_out, 1.0))) * 2 + 1 + 2)

    for j in np.asarray(jobs).reshape(-1):
        if not j["enabled"] or not 0 <= int(j["logo"]) < len(logo_descs):
            continue
        w, h = int(logo_descs[int(j["logo"])]["w"]), int(logo_descs[int(j["logo"])]["h"])
        sizes = [(int(j["w1"]), int(j["h1"])), (int(j["w2"]), int(j["h2"])) if j["rotate"] else None,
                 (int(j["w3"]), int(j["h3"])) if j["stretch"] else None]
        if w < 1 or h < 1 or any(s is not None and min(s) < 1 for s in sizes):
            continue                                             # the device skips it
        need[0] = max(need[0], w * h)
        for step, s in enumerate(sizes):
            if s is None:
                continue
            if step != 1:                                        # a resize: the horizontal pass first
                if s[0] != w:
                    need[1] = max(need[1], table(w, s[0])); need[0] = max(need[0], s[0] * h)
                if s[1] != h:
                    need[1] = max(need[1], table(h, s[1]))
            need[0] = max(need[0], s[0] * s[1])
            w, h = s
    return need[0], need[1]


_SYNTH_WORKSPACE = {}


def device_synth(packed_images, image_descs, packed_logos, logo_descs, jobs, with_mask=False, inplace=False):
    """Paste the logos of `jobs` onto a ragged batch on the HIP device (uwm_synth_u8; the rule is in include/uwm.h).
    packed_images / image_descs: flat uint8 RGB images (pack_images); packed_logos / logo_descs: flat uint8 RGBA logos; jobs: an
    (N, K) array of SYNTH_JOB_DTYPE (sample_synth_jobs), K <= 8, whose `logo` indexes logo_descs.  -> (the synthesized batch — a copy
    unless inplace — in the layout of image_descs, the pasted alpha planes in the layout of mask_descs_for(image_descs) or None).
    The workspace is sized for this batch's jobs, allocated once per device and grown when needed.  No CPU fallback."""
    import ctypes as C
    from . import _lib as L
    idesc, ldesc = np.ascontiguousarray(image_descs), np.ascontiguousarray(logo_descs)
    if idesc.dtype != DESC_DTYPE or ldesc.dtype != DESC_DTYPE or idesc.ndim != 1 or ldesc.ndim != 1 or len(idesc) == 0 or len(ldesc) == 0:
        raise ValueError("device_synth: image_descs and logo_descs must be non-empty 1-D data.DESC_DTYPE arrays")
    j = np.ascontiguousarray(jobs)
    if j.dtype != SYNTH_JOB_DTYPE or j.ndim != 2 or j.shape[0] != len(idesc) or not 1 <= j.shape[1] <= SYNTH_MAX_SLOTS:
        raise ValueError(f"device_synth: jobs must be an (N, K) array of data.SYNTH_JOB_DTYPE with N = {len(idesc)} images and K in 1..{SYNTH_MAX_SLOTS}")
    on = j["enabled"] != 0
    if ((j["logo"][on] < 0) | (j["logo"][on] >= len(ldesc))).any():
        raise ValueError(f"device_synth: an enabled job names a logo outside 0..{len(ldesc) - 1}")
    if (ldesc["offset"] % 4).any():
        raise ValueError("device_synth: every logo must start at a multiple of 4 bytes (pack_images does that)")
    if (j["ndefects"][on] < 0).any() or (j["ndefects"][on] > 3).any():
        raise ValueError("device_synth: ndefects must be 0..3")
    for name, t in (("packed_images", packed_images), ("packed_logos", packed_logos)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 1:
            raise RuntimeError(f"device_synth: {name} must be a flat uint8 tensor (no CPU fallback)")
    img = packed_images if packed_images.device.type == "cuda" else (packed_images.cuda(non_blocking=True) if torch.cuda.is_available() else packed_images)
    if img.device.type != "cuda":
        raise RuntimeError("device_synth needs a HIP device (no CPU fallback)")
    if int((idesc["offset"] + idesc["h"].astype(np.int64) * idesc["w"] * 3).max()) > img.numel():
        raise ValueError("device_synth: an image descriptor leaves packed_images")
    if int((ldesc["offset"] + ldesc["h"].astype(np.int64) * ldesc["w"] * 4).max()) > packed_logos.numel():
        raise ValueError("device_synth: a logo descriptor leaves packed_logos")
    out = img.contiguous() if inplace or img is not packed_images else img.clone()
    logos = packed_logos.to(out.device, non_blocking=True).contiguous()
    n, k = j.shape
    P, T = synth_job_needs(j, ldesc)
    md = mask_descs_for(idesc)
    mask = torch.empty(max(1, int((md["h"].astype(np.int64) * md["w"]).sum())), dtype=torch.uint8, device=out.device) if with_mask else None
    dd = descs_tensor(np.concatenate([idesc, md, ldesc]), out.device)
    jd = torch.from_numpy(j.reshape(-1).view(np.uint8).copy()).to(out.device, non_blocking=True)
    step = DESC_DTYPE.itemsize
    with L.on_device(out):
        need = int(L.lib().uwm_synth_workspace_bytes(n, k, P, T))
        if need == 0:
            L.check(1, ValueError)
        ws = _SYNTH_WORKSPACE.get(out.device)
        if ws is None or ws.numel() < need:
            ws = _SYNTH_WORKSPACE[out.device] = torch.empty(need, dtype=torch.uint8, device=out.device)
        L.check(L.lib().uwm_synth_u8(C.c_void_p(out.data_ptr()), out.numel(), C.c_void_p(dd.data_ptr()),
                                     C.c_void_p(mask.data_ptr() if with_mask else 0), mask.numel() if with_mask else 0,
                                     C.c_void_p(dd.data_ptr() + n * step), C.c_void_p(logos.data_ptr()), logos.numel(),
                                     C.c_void_p(dd.data_ptr() + 2 * n * step), len(ldesc), C.c_void_p(jd.data_ptr()), n, k, P, T,
                                     C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(L.stream_ptr(out.device))), ValueError)
    return out, mask


def list_logos(logos_dir):
    """gen_data.py's load_watermarks: the image files of combined/, independent/ and car_logo/; a flat directory of logos also works"""
    files = []
    for sub in LOGO_SUBDIRS:
        d = os.path.join(logos_dir, sub)
        if os.path.isdir(d):
            files += [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.lower().endswith(LOGO_EXTENSIONS)]
    if not files and os.path.isdir(logos_dir):
        files = [os.path.join(logos_dir, f) for f in sorted(os.listdir(logos_dir)) if f.lower().endswith(LOGO_EXTENSIONS)]
    return files


class RawSynthDataset(Dataset):
    """Clean photographs + a directory of logos -> the items the device turns into training pairs: (clean uint8 (h, w, 3) RGB,
    [logo uint8 (h', w', 4) RGBA, ...], jobs [SYNTH_SLOTS] of SYNTH_JOB_DTYPE).  Workers only decode and draw numbers
    (sample_synth_choice, sample_synth_jobs); DeviceInputPipeline pastes the logos with uwm_synth_u8 and derives the masks.  The
    draws of item i are a function of (seed, epoch, i): set_epoch(e) before an epoch's loader is made gives that epoch new samples,
    and a dataset that is never told the epoch (a validation split) reproduces its samples every time.  Decoded logos are kept in a
    per-process LRU of `cache` entries."""

    def __init__(self, clean_dir, logos_dir, seed=42, transparent_ratio=0.6, multi_watermark_ratio=0.4, max_watermarks=3,
                 mask_threshold=None, mask_source="pair", cache=64):
        from PIL import Image  # noqa: F401
        if not os.path.isdir(clean_dir):
            raise ValueError(f"RawSynthDataset: clean directory not found: {clean_dir}")
        self.files = sorted(os.path.join(clean_dir, f) for f in os.listdir(clean_dir) if f.lower().endswith(LOGO_EXTENSIONS))
        self.logos = list_logos(logos_dir)
        if not self.files or not self.logos:
            raise ValueError(f"RawSynthDataset: {len(self.files)} clean images in {clean_dir}, {len(self.logos)} logos in {logos_dir}: need both")
        if not 1 <= int(max_watermarks) <= SYNTH_SLOTS:
            raise ValueError(f"RawSynthDataset: max_watermarks must be 1..{SYNTH_SLOTS} (got {max_watermarks})")
        if mask_source not in ("pair", "alpha"):
            raise ValueError(f"RawSynthDataset: mask_source must be 'pair' or 'alpha' (got {mask_source!r})")
        self.seed, self.epoch = int(seed), 0
        self.transparent_ratio, self.multi_watermark_ratio = float(transparent_ratio), float(multi_watermark_ratio)
        self.max_watermarks, self.mask_threshold, self.mask_source = int(max_watermarks), mask_threshold, mask_source
        self.cache = int(cache)
        self._lru = {}

    def __len__(self):
        return len(self.files)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def _logo(self, i):
        from PIL import Image
        a = self._lru.pop(i, None)
        if a is None:
            a = np.asarray(Image.open(self.logos[i]).convert("RGBA"), dtype=np.uint8)
            if len(self._lru) >= self.cache:
                self._lru.pop(next(iter(self._lru)))
        self._lru[i] = a                                     # most recently used last
        return a

    def draw(self, i, image_size):
        """-> (enhance_transparent, logo indices, decoded logos, jobs) of item i at this epoch"""
        import random
        rng = random.Random(f"uwm-synth:{self.seed}:{self.epoch}:{int(i)}")
        transparent, picked = sample_synth_choice(rng, len(self.logos), self.transparent_ratio, self.multi_watermark_ratio, self.max_watermarks)
        logos = [self._logo(k) for k in picked]
        jobs = sample_synth_jobs(rng, image_size, [(a.shape[1], a.shape[0]) for a in logos], transparent)
        return transparent, picked, logos, jobs

    def __getitem__(self, i):
        from PIL import Image
        clean = np.asarray(Image.open(self.files[i]).convert("RGB"), dtype=np.uint8)
        _, _, logos, jobs = self.draw(i, (clean.shape[1], clean.shape[0]))
        return clean, logos, jobs


def list_collate(batch):
    """keeps the items as they are: raw images differ in size, so there is nothing to stack"""
    return list(batch)


class DeviceInputPipeline:
    """Batches of a raw dataset -> what Trainer.step takes, on the device.  Raw folder items (uint8 arrays of any size) are packed
    into persistent pinned buffers (pack_images), uploaded and resized to size x size by uwm_resize_u8 — linear for the image,
    nearest for the mask (the reference's A.Resize); RawPairDataset items (image, mask or None, clean or None) get their missing masks
    from uwm_pair_mask_u8 at the image's own size first; DeviceU8Dataset items are gathered.  Training batches then go through
    device_augment with parameters drawn from `generator`, validation batches through device_preprocess (get_val_transform).
    recipe 'transparent_watermark' (sample_transparent_recipe) sends the augmented uint8 images through device_jpeg, which normalises."""

    def __init__(self, size, device, source=None, recipe="basic", mean=IMAGENET_MEAN, std=IMAGENET_STD, mask_threshold=None):
        self.size, self.device, self.source, self.recipe = int(size), torch.device(device), source, recipe
        self.mean, self.std = mean, std
        self.mask_threshold = mask_threshold if mask_threshold is not None else getattr(source, "mask_threshold", None)
        self._pin, self._sent = [None, None, None], [None, None, None]

    def _upload(self, arrays, slot, extra=0):
        """extra: spare bytes behind the packed images in the device tensor"""
        need = sum((a.size + 3) // 4 * 4 for a in arrays)
        buf = self._pin[slot]
        if buf is None or buf.numel() < need:
            buf = self._pin[slot] = torch.empty(max(need, 1 << 20), dtype=torch.uint8, pin_memory=True)
            self._sent[slot] = torch.cuda.Event()
        else:
            self._sent[slot].synchronize()                   # the previous batch's upload has left the buffer
        packed, descs, _ = pack_images(arrays, out=buf)
        if extra:
            dev = torch.empty(packed.numel() + extra, dtype=torch.uint8, device=self.device)
            dev[:packed.numel()].copy_(packed, non_blocking=True)
        else:
            dev = packed.to(self.device, non_blocking=True)
        self._sent[slot].record(torch.cuda.current_stream(self.device))
        return dev, descs

    def to_u8(self, items):
        """-> (images uint8 (N, S, S, C), masks uint8 (N, S, S)) on the device"""
        if isinstance(self.source, DeviceU8Dataset):
            idx = torch.as_tensor([int(i) for i in items], device=self.device)
            return self.source.images[idx], self.source.masks[idx]
        if isinstance(self.source, RawSynthDataset):
            return self._synth_u8(items)
        imgs = [np.ascontiguousarray(it[0]) for it in items]
        cleans = [(it[2] if it[1] is None else None) if len(it) > 2 else None for it in items]      # (a file mask wins over a clean image)
        # an image without a mask file uploads zeros: they stay where there is no clean image either
        masks = [np.ascontiguousarray(it[1])[..., None] if it[1] is not None else np.zeros(a.shape[:2] + (1,), np.uint8)
                 for it, a in zip(items, imgs)]
        for i, (a, m) in enumerate(zip(imgs, masks)):
            if a.shape[:2] != m.shape[:2]:
                raise ValueError(f"image {i} is {a.shape[:2]}, its mask {m.shape[:2]}")
        generate = any(c is not None for c in cleans)
        if generate and self.mask_threshold is None:
            raise ValueError("items with a clean image and no mask need mask_threshold (DATA.GENERATE_MASK_THRESHOLD)")
        with torch.cuda.device(self.device):
            pi, di = self._upload(imgs, 0)
            pm, dm = self._upload(masks, 1)
            if generate:
                pc, dc = stage_clean(cleans, di, self.device, lambda arrs, extra: self._upload(arrs, 2, extra))
                device_pair_mask(pi, di, pc, dc, self.mask_threshold, True, pm, dm)
            x = device_resize(pi, di, self.size, imgs[0].shape[2], "linear")
            m = device_resize(pm, dm, self.size, 1, "nearest")
        return x, m.view(len(items), self.size, self.size)

    def _synth_u8(self, items):
        """RawSynthDataset items (clean, logos, jobs): upload the clean images and the logos the batch uses, paste the logos into a copy
        of the clean batch (uwm_synth_u8), take the masks from (synthesized, clean) with uwm_pair_mask_u8 — the reference's default
        flow, gen_data.py writes no masks unless asked — or, mask_source 'alpha', from the pasted alpha planes; then resize as ever"""
        cleans = [np.ascontiguousarray(it[0]) for it in items]
        logos, jobs = [], []
        for it in items:
            j = np.array(it[2], copy=True)
            j["logo"] += len(logos)                              # item-local logo index -> index into the batch's logos
            logos += [np.ascontiguousarray(a) for a in it[1]]
            jobs.append(j)
        alpha = self.source.mask_source == "alpha"
        if not alpha and self.mask_threshold is None:
            raise ValueError("synthesized samples with masks from pairs need mask_threshold (DATA.GENERATE_MASK_THRESHOLD)")
        with torch.cuda.device(self.device):
            pc, dc = self._upload(cleans, 0)
            pl, dl = self._upload(logos, 2)
            synth, pm = device_synth(pc, dc, pl, dl, np.stack(jobs), with_mask=alpha)
            if not alpha:
                pm = device_pair_mask(synth, dc, pc, dc, self.mask_threshold)
            x = device_resize(synth, dc, self.size, 3, "linear")
            m = device_resize(pm, mask_descs_for(dc), self.size, 1, "nearest")
        return x, m.view(len(items), self.size, self.size)

    def train_batch(self, items, generator=None):
        x, m = self.to_u8(items)
        if self.recipe == "transparent_watermark":
            params, ext, quality = sample_transparent_recipe(x.shape[0], x.shape[1], x.shape[2], generator)
            _, mo, u8 = device_augment(x, m, params, self.mean, self.std, return_u8=True, ext=ext)
            return device_jpeg(u8, quality, self.mean, self.std), mo
        params, ext = sample_aug_recipe(x.shape[0], x.shape[1], x.shape[2], generator, self.recipe)
        return device_augment(x, m, params, self.mean, self.std, ext=ext)

    def val_batch(self, items):
        x, m = self.to_u8(items)
        return device_preprocess(x, m, None, self.mean, self.std)
