"""Text-feature enhancement on the device — counterpart of WatermarkPredictor._enhance_text_features
(the reference's src/predict.py:370-404): the OpenCV chain the reference runs on an image before the network sees it when the mask
type is `text` or `mixed` — grey, CLAHE(2.0, 8 x 8), Canny(50, 150), dilation with the 2 x 2 ellipse, x 1.2 on the edge pixels, the
3 x 3 sharpening filter.  Here it is HIP (csrc/text_enhance.hip: uwm_text_enhance_ragged) on a ragged batch of images
at their own sizes in ONE call of eleven launches, byte-exact against tests/textenh_ref.py and the same on every run.  No CPU
fallback.  WatermarkPredictor.predict_images(text_enhance=True) puts the call in front of the forward inside the captured graph."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _device as D, _lib as L

STATUS = {"done": 0, "misfit": 1, "copied": 2}            # UWM_TEXT_ENHANCE_*: per image; `copied`: a side below MIN_SIDE, left unchanged
MIN_SIDE = 16


def text_enhance_workspace(device, total_pixels: int, n: int) -> torch.Tensor:
    """uwm_text_enhance_ragged's scratch for the capacities (total_pixels, n): one buffer per device, kept and grown on demand; a
    captured graph holds the buffer it was captured with.  Its first n int32 are the per-image status after a call."""
    return D.workspace("text_enhance", device, L.lib().uwm_text_enhance_workspace_bytes(int(total_pixels), int(n)))


def text_enhance_ragged(buf: torch.Tensor, descs, out=None, *, n: Optional[int] = None, max_pixels: Optional[int] = None,
                        total_pixels: Optional[int] = None, edges=None, edge_descs=None, return_status: bool = False):
    """A ragged batch of RGB images through ONE library call (uwm_text_enhance_ragged).  buf: uint8 1-d device tensor; image i is
    descs[i]'s (h, w, 3) interleaved bytes at buf[descs[i].offset:].  descs: a host record array with the fields offset / h / w
    (uploaded here), or a device tensor of uwm_image_desc bytes — then n, max_pixels and total_pixels must be given, nothing about
    the batch is read on the host, and the call can be captured.  -> the uint8 buffer of the results at the same offsets (`out`, which
    must not be buf, or a new tensor; bytes outside the images are then zero).  edges + edge_descs (both or neither, as buf + descs):
    a flat uint8 device buffer that receives every image's dilated edge plane, one byte per pixel in {0, 255}.  return_status: also
    the int32 (n,) device tensor of STATUS values (a view of the workspace: read it before the next call).  max_pixels /
    total_pixels: capacities, at least the largest h*w and the sum of h*w; an image beyond one is a misfit (status 1)."""
    if (edges is None) != (edge_descs is None):
        raise ValueError("text_enhance_ragged: edges and edge_descs go together")
    d, n, caps = D.ragged_args("text_enhance_ragged", (buf,), descs, n, max_pixels=max_pixels, total_pixels=total_pixels)
    ed = None
    if edges is not None:
        ed = D.ragged_args("text_enhance_ragged", (buf, edges), edge_descs, n, **caps)[0]
    o = D.out_like("text_enhance_ragged", out, buf)
    with L.on_device(buf):
        ws = text_enhance_workspace(buf.device, caps["total_pixels"], n)
        L.check(L.lib().uwm_text_enhance_ragged(D.ptr(buf), D.ptr(o), buf.numel(), D.ptr(d), n, 3, caps["max_pixels"], caps["total_pixels"],
                                                D.ptr(edges), edges.numel() if edges is not None else 0, D.ptr(ed), D.ptr(ws), ws.numel(),
                                                C.c_void_p(L.stream_ptr(buf.device))))
    return (o, ws[:4 * n].view(torch.int32)) if return_status else o


def enhance_text_features(images, device="cuda", return_edges: bool = False, return_status: bool = False):
    """A list of uint8 (h_i, w_i, 3) images (arrays or tensors) of ANY sizes -> the list of their enhanced images as uint8 (h_i, w_i,
    3) tensors on the HIP device: the reference's _enhance_text_features for each, in one library call.  An image with a side below
    MIN_SIDE comes back unchanged (status 'copied').  return_edges: also the list of uint8 (h_i, w_i) dilated edge planes in {0, 255};
    return_status: also the int32 (n,) HOST array of STATUS values."""
    from .data import pack_images
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("uwm enhance_text_features runs only on a HIP device (no CPU fallback)")
    packed, descs, mdescs = pack_images(images)
    if int(images[0].shape[2]) != 3:
        raise ValueError("enhance_text_features takes 3-channel RGB images")
    buf = packed.to(dev, non_blocking=True)
    areas = descs["h"].astype("int64") * descs["w"]
    edges = torch.zeros(int(areas.sum()), dtype=torch.uint8, device=dev) if return_edges else None
    out, status = text_enhance_ragged(buf, descs, edges=edges, edge_descs=mdescs if return_edges else None, return_status=True)
    ret = [D.ragged_views(out, descs, 3)]
    if return_edges:
        ret.append(D.ragged_views(edges, mdescs))
    if return_status:
        ret.append(status.cpu().numpy().copy())
    return ret[0] if len(ret) == 1 else tuple(ret)
