"""The JPEG save of the synthesis chain on the device (uwm_jpeg_ragged_u8, csrc/jpeg_ragged_u8.hip): a baseline 4:2:0
round trip of every image of a packed ragged batch at its own size — the reference's gen_data.py saves every sample at quality 95."""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from .._device import device_u8, ptr, upload_records, workspace
from .ragged import DESC_DTYPE, descs_tensor

SYNTH_JPEG_QUALITY = 95                   # gen_data.py:908 (and the temporary file of a mixed sample, gen_data.py:402-410)


def check_jpeg_quality(q, what="jpeg quality") -> int:
    """-> q as an int when it is 0 (no round trip) or 1..100; ValueError otherwise"""
    if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or not 0 <= int(q) <= 100:
        raise ValueError(f"{what} must be 0 (no round trip) or an integer 1..100 (got {q!r})")
    return int(q)


def device_jpeg_ragged(packed: torch.Tensor, descs, quality, inplace=False) -> torch.Tensor:
    """What Image.save(quality=q) and a reload do to the pixels of every RGB image of a packed ragged batch (pack_images) on the HIP
    device, each at its own size, any h and w >= 1: a baseline 4:2:0 JPEG encode + decode, bit-equal to Pillow's (libjpeg-turbo)
    (uwm_jpeg_ragged_u8; the rule, with libjpeg's edge handling, is in include/uwm.h).  descs: the uwm_image_desc array (numpy,
    DESC_DTYPE); quality: one integer per image, 0 = the image is left as it is, else 1..100.  Everything is validated here, on the
    host: the kernels only clamp and skip.  -> the packed result (flat uint8, on the device): `packed` itself when inplace (and
    already there), else a new tensor (whose <= 3 padding bytes behind an image are not written).  The workspace is allocated once per device and reused.  No CPU fallback."""
    d = np.ascontiguousarray(descs)
    if d.dtype != DESC_DTYPE or d.ndim != 1 or len(d) == 0:
        raise ValueError("device_jpeg_ragged: descs must be a non-empty 1-D data.DESC_DTYPE array")
    n = len(d)
    q = np.asarray(quality)
    if q.ndim != 1 or q.shape[0] != n or not np.issubdtype(q.dtype, np.integer):
        raise ValueError(f"device_jpeg_ragged: quality must be {n} integers, one per image")
    if ((q < 0) | (q > 100)).any():
        raise ValueError("device_jpeg_ragged: quality must be 0 (the image stays) or 1..100")
    refusal = "device_jpeg_ragged needs a flat uint8 tensor and a HIP device (no CPU fallback)"
    if not isinstance(packed, torch.Tensor) or packed.dtype != torch.uint8 or packed.dim() != 1:
        raise RuntimeError(refusal)
    pixels = d["h"].astype(np.int64) * d["w"]
    if (d["h"] < 1).any() or (d["w"] < 1).any() or (d["offset"] < 0).any() or (d["offset"] % 4).any():
        raise ValueError("device_jpeg_ragged: every image needs h, w >= 1 and an offset that is a non-negative multiple of 4 (pack_images does that)")
    if int((d["offset"] + pixels * 3).max()) > packed.numel():
        raise ValueError("device_jpeg_ragged: an image descriptor leaves the packed buffer")
    if int(pixels.max()) >= (1 << 31) - 1:
        raise ValueError("device_jpeg_ragged: an image has 2^31 - 1 pixels or more")
    src = device_u8(packed, 1, refusal, upload=True)
    out = src if inplace else torch.empty_like(src)
    dd = descs_tensor(d, src.device)
    qd = upload_records(q.astype(np.int32), src.device)
    with L.on_device(src):
        ws = workspace("jpeg_ragged", src.device, L.lib().uwm_jpeg_ragged_workspace_bytes(n, src.numel()), ValueError)
        L.check(L.lib().uwm_jpeg_ragged_u8(ptr(src), ptr(out), src.numel(), ptr(dd), ptr(qd), n, 3, int(pixels.max()), ptr(ws), ws.numel(),
                                           C.c_void_p(L.stream_ptr(src.device))), ValueError)
    return out
