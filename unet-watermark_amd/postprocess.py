"""Mask post-processing on the device — counterpart of WatermarkPredictor._optimize_mask
(/root/reference/src/predict.py:161-301): binary morphology (open / close / dilate with elliptical and line elements), an
8-connected component analysis and a selection by area, for the three mask types `watermark`, `text`, `mixed`.  The reference
does this with OpenCV on the host; here it is HIP (csrc/mask_post.hip: uwm_optimize_mask and its building blocks), exact integer
work whose results equal the specification in DESIGN.md §8b bit for bit.  No CPU fallback.  optimize_masks_ragged is the same on
a ragged batch of masks of any sizes in ONE call (uwm_optimize_masks_ragged), with eight statistics per image.
enhance_masks_ragged / enhance_mask are the reference's scripts/enhance_masks.py::enhance_mask (grey close and dilate, Gaussian blur,
threshold, smoothing: csrc/mask_enhance.hip) on a ragged batch, again in one call.

The reference's _enhance_text_features (the image enhancement in front of the network for text watermarks) is served by textenh.py
(csrc/text_enhance.hip); its automatic type detection (_detect_watermark_type: Canny / Sobel on the image) stays out."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _device as D, _lib as L

MASK_TYPES = {"watermark": 0, "text": 1, "mixed": 2}
SHAPES = {"rect": 0, "ellipse": 2, 0: 0, 2: 2}          # cv2.MORPH_RECT / cv2.MORPH_ELLIPSE
_OPS = {"dilate": 1, "erode": 0}


def mask_type_code(mask_type) -> int:
    if mask_type not in MASK_TYPES:
        raise ValueError(f"mask_type must be one of 'watermark', 'text', 'mixed', got {mask_type!r}")
    return MASK_TYPES[mask_type]


def _shape_code(shape) -> int:
    if shape not in SHAPES:
        raise ValueError(f"shape must be 'rect' or 'ellipse' (or cv2's 0 / 2), got {shape!r}")
    return SHAPES[shape]


def _ksize(ksize):
    kw, kh = (ksize, ksize) if isinstance(ksize, int) else ksize        # (w, h), as cv2.getStructuringElement takes it
    return int(kw), int(kh)


def structuring_element(shape, ksize) -> np.ndarray:
    """cv2.getStructuringElement(shape, (w, h)) as a uint8 (h, w) array of 0/1 (host; 1 <= w, h <= 15)."""
    kw, kh = _ksize(ksize)
    out = np.zeros((max(kh, 1), max(kw, 1)), np.uint8)
    rc = L.lib().uwm_mask_element(_shape_code(shape), kw, kh, C.c_void_p(out.ctypes.data))
    if rc:
        raise ValueError(L.lib().uwm_last_error().decode(errors="replace"))
    return out


def _masks(mask_u8: torch.Tensor, what: str):
    if not isinstance(mask_u8, torch.Tensor) or mask_u8.device.type != "cuda":
        raise RuntimeError(f"uwm {what} runs only on a HIP device (no CPU fallback)")
    if mask_u8.dtype != torch.uint8 or mask_u8.dim() not in (2, 3) or mask_u8.numel() == 0:
        raise RuntimeError(f"expected a non-empty uint8 mask of shape (H,W) or (N,H,W), got {mask_u8.dtype} {tuple(mask_u8.shape)}")
    m = mask_u8.contiguous()
    return (m[None] if m.dim() == 2 else m), m.dim() == 2


def workspace(device, n: int, h: int, w: int) -> torch.Tensor:
    """The calls' scratch (bit planes, labels, areas): one buffer per device, kept and grown on demand like the model's workspace.
    A captured graph holds the buffer it was captured with (WatermarkPredictor keeps that reference), so growing it later for a
    larger shape leaves the graph valid."""
    return D.workspace("mask", device, L.lib().uwm_mask_workspace_bytes(n, h, w))


def optimize_mask(mask_u8: torch.Tensor, mask_type: str = "watermark", return_summary: bool = False, out=None):
    """uint8 (H,W) | (N,H,W) masks on the HIP device (foreground > 127) -> the reference's optimised masks, uint8 {0,255} of the
    same shape.  return_summary: also an int64 (N,4) | (4,) device tensor {components found, area of the largest, foreground
    pixels of the output, id of the largest or -1} — the reference's watermark_ratio and its "no watermark found" test without
    copying the mask back.  out: a uint8 tensor of the same shape to write into (may be the input)."""
    code = mask_type_code(mask_type)
    m, squeeze = _masks(mask_u8, "optimize_mask")
    n, h, w = m.shape
    if out is None:
        o = torch.empty_like(m)
    else:
        if out.dtype != torch.uint8 or out.device != m.device or out.numel() != m.numel() or not out.is_contiguous():
            raise RuntimeError("optimize_mask: out must be a contiguous uint8 tensor of the input's shape on the same device")
        o = out
    summary = torch.empty((n, 4), dtype=torch.int64, device=m.device) if return_summary else None
    with L.on_device(m):
        ws = workspace(m.device, n, h, w)
        L.check(L.lib().uwm_optimize_mask(C.c_void_p(m.data_ptr()), C.c_void_p(o.data_ptr()), n, h, w, code,
                                          C.c_void_p(summary.data_ptr() if summary is not None else 0),
                                          C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(L.stream_ptr(m.device))))
    res = o.view(mask_u8.shape) if out is None else out
    if return_summary:
        return res, (summary[0] if squeeze else summary)
    return res


RAGGED_TYPES = {**MASK_TYPES, "none": 3}                 # 'none' (UWM_MASK_NONE): binarise, no morphology, every component kept
STATS_FIELDS = ("components", "largest_area", "foreground", "largest_id", "kept_components", "largest_kept_area", "pixels", "status")


def ragged_workspace(device, n: int, mask_bytes: int, rows: int) -> torch.Tensor:
    """The ragged call's scratch for the capacities (n, mask_bytes, rows): one buffer per device, kept and grown like `workspace`; a
    captured graph holds the buffer it was captured with."""
    return D.workspace("mask_ragged", device, L.lib().uwm_mask_ragged_workspace_bytes(int(n), int(mask_bytes), int(rows)))


def optimize_masks_ragged(buf: torch.Tensor, descs, mask_type: str = "watermark", return_stats: bool = False, out=None, *,
                          n: Optional[int] = None, max_pixels: Optional[int] = None, rows: Optional[int] = None, stats=None):
    """A ragged batch of masks through ONE library call (uwm_optimize_masks_ragged), whatever their sizes.  buf: uint8 1-d device
    tensor; image i is descs[i]'s (h, w), one byte per pixel, at buf[descs[i].offset:].  descs: a host record array with the fields
    offset / h / w (uploaded here), or a device tensor of uwm_image_desc bytes — then n, max_pixels and rows must be given, nothing
    about the batch is read on the host, and the call can be captured.  -> the uint8 buffer of the results at the same offsets
    (`out`, which may be buf itself, or a new tensor; bytes outside the images are then zero), with return_stats also the int64
    (n, 8) device tensor STATS_FIELDS (`stats`: a tensor to write them into).  mask_type: 'watermark' | 'text' | 'mixed' | 'none'.
    max_pixels / rows: capacities, at least the largest h*w and the sum of h; an image beyond a capacity is a misfit (status 1)."""
    if mask_type not in RAGGED_TYPES:
        raise ValueError(f"mask_type must be one of 'watermark', 'text', 'mixed', 'none', got {mask_type!r}")
    d, n, caps = D.ragged_args("optimize_masks_ragged", (buf,), descs, n, max_pixels=max_pixels, rows=rows)
    o = D.out_like("optimize_masks_ragged", out, buf)
    if return_stats:
        stats = D.stats_like("optimize_masks_ragged", stats, n, 8, buf.device)
    with L.on_device(buf):
        ws = ragged_workspace(buf.device, n, buf.numel(), caps["rows"])
        L.check(L.lib().uwm_optimize_masks_ragged(D.ptr(buf), D.ptr(o), buf.numel(), D.ptr(d), n, RAGGED_TYPES[mask_type], caps["max_pixels"],
                                                  caps["rows"], D.ptr(stats if return_stats else None), D.ptr(ws), ws.numel(),
                                                  C.c_void_p(L.stream_ptr(buf.device))))
    return (o, stats) if return_stats else o


ENHANCE_STATS_FIELDS = ("foreground_in", "foreground_out", "pixels", "status")


def enhance_workspace(device, n: int, mask_bytes: int) -> torch.Tensor:
    """uwm_enhance_masks_ragged's scratch for the capacities (n, mask_bytes): one buffer per device, kept and grown like `workspace`;
    a captured graph holds the buffer it was captured with."""
    return D.workspace("enhance", device, L.lib().uwm_enhance_masks_workspace_bytes(int(n), int(mask_bytes)))


def _enhance_params(expand_pixels, blur_kernel, smooth_iterations):
    e, k, s = int(expand_pixels), int(blur_kernel), int(smooth_iterations)
    if not 0 <= e <= 31:
        raise ValueError(f"expand_pixels must be in 0..31, got {expand_pixels!r}")
    if not 0 <= k <= 63:
        raise ValueError(f"blur_kernel must be in 0..63, got {blur_kernel!r}")
    if not 0 <= s <= 8:
        raise ValueError(f"smooth_iterations must be in 0..8, got {smooth_iterations!r}")
    return e, k, s


def enhance_masks_ragged(buf: torch.Tensor, descs, expand_pixels: int = 10, blur_kernel: int = 15, smooth_iterations: int = 2,
                         return_stats: bool = False, out=None, *, n: Optional[int] = None, max_pixels: Optional[int] = None, stats=None):
    """The reference's enhance_mask (scripts/enhance_masks.py) on a ragged batch of 8-bit grey masks through ONE library call
    (uwm_enhance_masks_ragged): close E(7,7), dilate by expand_pixels, Gaussian blur of side blur_kernel (0: none; even: + 1),
    threshold at 127, smooth_iterations rounds of open / close E(5,5) -> masks in {0,255}.  buf, descs, out, n, max_pixels as
    optimize_masks_ragged takes them (device descriptors need n and max_pixels; the call can then be captured).  return_stats: also
    the int64 (n, 4) device tensor ENHANCE_STATS_FIELDS (`stats`: a tensor to write them into).  The rules are restated from
    OpenCV's documented behaviour, not run against it (include/uwm.h)."""
    e, k, s = _enhance_params(expand_pixels, blur_kernel, smooth_iterations)
    d, n, caps = D.ragged_args("enhance_masks_ragged", (buf,), descs, n, max_pixels=max_pixels)
    o = D.out_like("enhance_masks_ragged", out, buf)
    if return_stats:
        stats = D.stats_like("enhance_masks_ragged", stats, n, 4, buf.device)
    with L.on_device(buf):
        ws = enhance_workspace(buf.device, n, buf.numel())
        L.check(L.lib().uwm_enhance_masks_ragged(D.ptr(buf), D.ptr(o), buf.numel(), D.ptr(d), n, e, k, s, caps["max_pixels"],
                                                 D.ptr(stats if return_stats else None), D.ptr(ws), ws.numel(),
                                                 C.c_void_p(L.stream_ptr(buf.device))))
    return (o, stats) if return_stats else o


def enhance_mask(mask_u8: torch.Tensor, expand_pixels: int = 10, blur_kernel: int = 15, smooth_iterations: int = 2,
                 return_stats: bool = False, out=None):
    """enhance_masks_ragged for uint8 (H,W) | (N,H,W) masks on the HIP device -> the enhanced masks, uint8 {0,255} of the same shape
    (`out`: a contiguous uint8 tensor of that shape to write into, which may be the input); return_stats: also the int64 (N,4) | (4,)
    device tensor ENHANCE_STATS_FIELDS."""
    import numpy as np
    from .data import DESC_DTYPE
    _enhance_params(expand_pixels, blur_kernel, smooth_iterations)
    m, squeeze = _masks(mask_u8, "enhance_mask")
    n, h, w = m.shape
    if out is not None and (out.dtype != torch.uint8 or out.device != m.device or out.numel() != m.numel() or not out.is_contiguous()):
        raise RuntimeError("enhance_mask: out must be a contiguous uint8 tensor of the input's shape on the same device")
    descs = np.zeros(n, DESC_DTYPE)
    descs["offset"], descs["h"], descs["w"] = np.arange(n, dtype=np.int64) * (h * w), h, w
    o = torch.empty_like(m) if out is None else out
    res = enhance_masks_ragged(m.view(-1), descs, expand_pixels, blur_kernel, smooth_iterations, return_stats, o.view(-1))
    o = o.view(mask_u8.shape) if out is None else out
    if return_stats:
        return o, (res[1][0] if squeeze else res[1])
    return o


def morphology(mask_u8: torch.Tensor, op: str, shape, ksize, iterations: int = 1) -> torch.Tensor:
    """`iterations` passes of cv2.dilate / cv2.erode (op 'dilate' | 'erode') with getStructuringElement(shape, ksize)."""
    if op not in _OPS:
        raise ValueError(f"op must be 'dilate' or 'erode', got {op!r}")
    m, _ = _masks(mask_u8, "morphology")
    n, h, w = m.shape
    kw, kh = _ksize(ksize)
    o = torch.empty_like(m)
    with L.on_device(m):
        ws = workspace(m.device, n, h, w)
        L.check(L.lib().uwm_op_morph(C.c_void_p(m.data_ptr()), C.c_void_p(o.data_ptr()), n, h, w, _OPS[op], _shape_code(shape),
                                     kw, kh, int(iterations), C.c_void_p(ws.data_ptr()), ws.numel(),
                                     C.c_void_p(L.stream_ptr(m.device))), ValueError)
    return o.view(mask_u8.shape)


def connected_components(mask_u8: torch.Tensor):
    """-> (labels, areas), int32 tensors of the mask's shape: labels = component id + 1 (0 = background), the id being the linear
    index y*W + x of the component's first pixel in raster order; areas = the pixel count at the id pixel, 0 elsewhere."""
    m, _ = _masks(mask_u8, "connected_components")
    n, h, w = m.shape
    labels = torch.empty((n, h, w), dtype=torch.int32, device=m.device)
    areas = torch.empty((n, h, w), dtype=torch.int32, device=m.device)
    with L.on_device(m):
        ws = workspace(m.device, n, h, w)
        L.check(L.lib().uwm_op_components(C.c_void_p(m.data_ptr()), C.c_void_p(labels.data_ptr()), C.c_void_p(areas.data_ptr()),
                                          n, h, w, C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(L.stream_ptr(m.device))))
    return labels.view(mask_u8.shape), areas.view(mask_u8.shape)
