"""Minimal data side of the boundary: tensors with the contract of the reference's dataset
(/root/reference/src/utils/dataset.py:113-122,332-333,389-395) — image fp32 NCHW normalised with the
ImageNet mean/std, mask int64 {0,1} (H,W).  The reference's OpenCV/albumentations pipeline is out of scope
(SURVEY.md §2 row 8); a synthetic generator and a plain PIL folder reader are provided."""
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
