"""Images of any size: a ragged batch packed into one flat buffer with a descriptor per image, and its resize on the device
(uwm_resize_u8, csrc/resize_u8.hip)."""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from .._device import device_u8, ptr

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
    off = 0
    for i, a in enumerate(arrs):
        descs[i] = (off, a.shape[0], a.shape[1])
        off += (a.size + 3) // 4 * 4
    if out is not None and out.dtype == torch.uint8 and out.dim() == 1 and out.device.type == "cpu" and out.numel() >= off:
        packed = out[:off]
    else:
        packed = torch.empty(off, dtype=torch.uint8, pin_memory=torch.cuda.is_available())      # (the <= 3 padding bytes behind an image are never used)
    flat = packed.numpy()
    for a, d in zip(arrs, descs):
        flat[int(d["offset"]): int(d["offset"]) + a.size] = a.reshape(-1)
    return packed, descs, mask_descs_for(descs)


def mask_descs_for(descs) -> np.ndarray:
    """uwm_image_desc array of images -> the same sizes with offsets that pack one h*w-byte mask per image back to back
    (pack_images' third result)"""
    m = np.zeros(len(descs), DESC_DTYPE)
    m["h"], m["w"] = descs["h"], descs["w"]
    sizes = descs["h"].astype(np.int64) * descs["w"].astype(np.int64)
    m["offset"] = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    return m


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
    if interp not in INTERP:
        raise ValueError(f"interp must be 'linear' or 'nearest', got {interp!r}")
    H, W = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    src = device_u8(packed, 1, "device_resize needs a flat uint8 tensor and a HIP device (no CPU fallback)", upload=True)
    dd = descs_tensor(descs, src.device) if not isinstance(descs, torch.Tensor) else descs.to(src.device)
    n = dd.numel() // DESC_DTYPE.itemsize
    out = torch.empty((n, H, W, int(channels)), dtype=torch.uint8, device=src.device)
    with L.on_device(src):
        L.check(L.lib().uwm_resize_u8(ptr(src), src.numel(), ptr(dd), n, int(channels), H, W, INTERP[interp], ptr(out),
                                      C.c_void_p(L.stream_ptr(src.device))), ValueError)
    return out
