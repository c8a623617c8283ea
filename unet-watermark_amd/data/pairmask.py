"""Masks from watermarked / clean pairs on the device (uwm_pair_mask_u8, csrc/pair_mask_u8.hip)."""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from .._device import device_u8, ptr
from .ragged import DESC_DTYPE, INTERP, descs_tensor, mask_descs_for, pack_images


def device_pair_mask(packed_wm, wm_descs, packed_clean, clean_descs, threshold, open=True, mask=None, mask_descs=None) -> torch.Tensor:
    """The reference's WatermarkDataset._generate_mask (use_blurred_mask = False) for every pair of a ragged batch on the HIP device:
    mask_i = open3(gray(|wm_i - clean_i|) > threshold) at the image's own size, {0, 255} (uwm_pair_mask_u8; the rule is in
    include/uwm.h).  packed_wm / packed_clean: flat uint8 tensors of RGB images (pack_images) with their uwm_image_desc arrays; a
    clean descriptor with h == 0 skips that image (its mask bytes stay), a pair whose sizes differ gets a zero mask — bring such a
    clean image to the watermarked size with uwm_resize_u8 first.  mask / mask_descs: a packed mask buffer on the device to write
    into (e.g. one that already holds the masks read from files); absent, one is made, zero-filled, with the layout of
    mask_descs_for(wm_descs).  -> the packed mask (flat uint8, on the device).  No CPU fallback."""
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
    refusal = "device_pair_mask needs flat uint8 tensors and a HIP device (no CPU fallback)"
    wm = device_u8(packed_wm, 1, refusal, upload=True)
    cl = device_u8(packed_clean.to(wm.device, non_blocking=True), 1, refusal)
    if mask is None:
        mask = torch.zeros(max(1, int((md["h"].astype(np.int64) * md["w"]).sum())), dtype=torch.uint8, device=wm.device)
    elif mask.device != wm.device or mask.dtype != torch.uint8 or mask.dim() != 1 or not mask.is_contiguous():
        raise ValueError("device_pair_mask: mask must be a flat contiguous uint8 tensor on the images' device")
    dd = descs_tensor(np.concatenate([wd, cd, md]), wm.device)                 # one upload; 16-byte records keep every part 8-byte aligned
    n, step = len(wd), len(wd) * DESC_DTYPE.itemsize
    with L.on_device(wm):
        L.check(L.lib().uwm_pair_mask_u8(ptr(wm), wm.numel(), ptr(dd), ptr(cl), cl.numel(), C.c_void_p(dd.data_ptr() + step), n, 3, t,
                                         int(bool(open)), ptr(mask), mask.numel(), C.c_void_p(dd.data_ptr() + 2 * step),
                                         C.c_void_p(L.stream_ptr(wm.device))), ValueError)
    return mask


def stage_clean(cleans, wm_descs, device, upload=None):
    """The clean images of a batch on the device, each at its watermarked image's size: cleans holds a uint8 (h, w, 3) array or None
    per image, wm_descs the watermarked images' descriptors.  The arrays are packed and uploaded (upload(arrays, extra_bytes) ->
    (flat device tensor with extra_bytes spare bytes behind the packed images, descs); default: pack_images + a fresh tensor); a clean
    image of another size is then resized by uwm_resize_u8 (LINEAR: cv2.resize's default, as the reference calls it) into the spare
    bytes, one launch per such image.  -> (flat device tensor, clean_descs) for device_pair_mask: h == 0 where cleans[i] is None;
    (None, None) when every entry is None."""
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
                L.check(L.lib().uwm_resize_u8(ptr(dev), used, C.c_void_p(dd.data_ptr() + k * DESC_DTYPE.itemsize), 1, 3, h, w,
                                              INTERP["linear"], C.c_void_p(dev.data_ptr() + off), C.c_void_p(L.stream_ptr(dev.device))),
                        ValueError)
                cd[i] = (off, h, w)
                off += nbytes
    return dev, cd
