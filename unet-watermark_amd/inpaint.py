"""Membrane fill on the device — what `main.py repair` puts in the place of a predicted watermark.  The reference hands image and
mask to IOPaint's LaMa (src/predict.py, steps 2-4), whose weights do not ship; this is the weight-free fill every inpainting toolbox
carries beside its models: inside the hole every channel satisfies the discrete Laplace equation with the known pixels as boundary
values (the membrane, or harmonic, interpolant).  It is a SMOOTH fill: it removes a logo from sky, wall, paper or skin and it smears
texture.  The solver is a geometric multigrid on the hole with the pull-push pyramid as its initial guess (csrc/inpaint.hip:
uwm_inpaint_ragged), a ragged batch of images at their own sizes in ONE capturable call, byte-exact against
tests/inpaint_ref.py and the same on every run.  No CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _device as D, _lib as L

# the smallest count at which every case of tests/test_inpaint.py's convergence table is within 0.5 grey levels of the exact membrane
# before rounding (the corner hole at 97 x 131 is the slowest, 0.51 after six cycles, 0.26 after seven)
DEFAULT_CYCLES = 7
MAX_CYCLES = 32
MAX_SIDE = 32768
INPAINT_STATS_FIELDS = ("hole_pixels", "status", "levels", "reserved")
STATUS = {"filled": 0, "no_hole": 1, "no_known": 2, "misfit": 3}          # UWM_INPAINT_*


def check_cycles(cycles) -> int:
    if isinstance(cycles, bool) or int(cycles) != cycles or not 0 <= int(cycles) <= MAX_CYCLES:
        raise ValueError(f"cycles must be an integer in 0..{MAX_CYCLES}, got {cycles!r}")
    return int(cycles)


def inpaint_workspace(device, n: int, image_bytes: int, channels: int, max_side: int) -> torch.Tensor:
    """uwm_inpaint_ragged's scratch for the capacities (n, image_bytes, channels, max_side): one buffer per device, kept and grown on
    demand; a captured graph holds the buffer it was captured with"""
    return D.workspace("inpaint", device, L.lib().uwm_inpaint_workspace_bytes(int(n), int(image_bytes), int(channels), int(max_side)))


def launch_count(cycles: int, max_side: int) -> int:
    """the number of kernel launches of one call: it follows `cycles` and the capacity max_side alone"""
    k = L.lib().uwm_inpaint_launch_count(int(cycles), int(max_side))
    if k == 0:
        raise ValueError(L.lib().uwm_last_error().decode(errors="replace"))
    return k


def inpaint_buffers(buf: torch.Tensor, descs: torch.Tensor, mbuf: torch.Tensor, mdescs: torch.Tensor, n: int, channels: int, *,
                    max_pixels: int, rows: int, max_side: int, cycles: int = DEFAULT_CYCLES, out: Optional[torch.Tensor] = None,
                    stats: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The library call on device buffers: buf / mbuf flat uint8 tensors of packed images / masks, descs / mdescs uint8 tensors of
    uwm_image_desc bytes on the same device.  Nothing about the batch is read on the host, so the call can be captured; max_pixels,
    rows and max_side are capacities (the largest h*w, the sum of h, the largest side).  out: buf itself (in place) or a tensor of
    its size (default: a new one; bytes outside the images are zero); stats: an int64 (n, 4) device tensor (INPAINT_STATS_FIELDS)"""
    descs, n, caps = D.ragged_args("inpaint", (buf, mbuf), descs, n, max_pixels=max_pixels, rows=rows)
    if not isinstance(mdescs, torch.Tensor) or mdescs.device != buf.device or mdescs.dtype != torch.uint8 or mdescs.numel() < 16 * n:
        raise RuntimeError("inpaint: mdescs must be a uint8 tensor of 16 n bytes on the images' device")
    cycles = check_cycles(cycles)
    out = D.out_like("inpaint", out, buf)
    if stats is not None:
        stats = D.stats_like("inpaint", stats, n, 4, buf.device)
    with L.on_device(buf):
        ws = workspace if workspace is not None else inpaint_workspace(buf.device, n, buf.numel(), channels, max_side)
        L.check(L.lib().uwm_inpaint_ragged(D.ptr(buf), D.ptr(out), buf.numel(), D.ptr(descs), D.ptr(mbuf), mbuf.numel(), D.ptr(mdescs), n,
                                           int(channels), cycles, caps["max_pixels"], caps["rows"], int(max_side), D.ptr(stats), D.ptr(ws),
                                           ws.numel(), C.c_void_p(L.stream_ptr(buf.device))), ValueError)
    return out


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def inpaint_ragged(images, masks, cycles: int = DEFAULT_CYCLES, return_stats: bool = False, device="cuda"):
    """Lists of uint8 (h_i, w_i, C) images and (h_i, w_i) masks (arrays or tensors; a mask byte != 0 is a hole pixel) of ANY sizes ->
    the list of filled uint8 (h_i, w_i, C) tensors on the HIP device, in one library call.  An image without a hole pixel or without
    a known pixel comes back as it is.  return_stats: also the int64 (n, 4) HOST array of INPAINT_STATS_FIELDS"""
    from .data import descs_tensor, pack_images
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("uwm inpaint runs only on a HIP device (no CPU fallback)")
    cycles = check_cycles(cycles)
    images, masks = list(images), [_host(m) for m in masks]
    if len(images) != len(masks):
        raise ValueError(f"{len(images)} images but {len(masks)} masks")
    for i, (im, m) in enumerate(zip(images, masks)):
        if m.ndim == 3 and m.shape[2] == 1:
            masks[i] = m = m[:, :, 0]
        if m.ndim != 2 or m.dtype != np.uint8 or tuple(m.shape) != tuple(im.shape[:2]):
            raise ValueError(f"mask {i} is {m.dtype} {tuple(m.shape)}: it must be a uint8 mask of its image's size {tuple(im.shape[:2])}")
    packed, descs, mdescs = pack_images(images)
    channels = int(images[0].shape[2])
    hs, ws_ = descs["h"].astype("int64"), descs["w"].astype("int64")
    areas = hs * ws_
    if int(max(hs.max(), ws_.max())) > MAX_SIDE or int(areas.max()) > 2 ** 30:
        raise ValueError(f"inpaint: an image with a side above {MAX_SIDE} or more than 2^30 pixels")
    mhost = np.zeros(int(mdescs["offset"][-1] + areas[-1]), np.uint8)
    for m, o, a in zip(masks, mdescs["offset"], areas):
        mhost[int(o): int(o) + int(a)] = m.reshape(-1)
    buf, mbuf = packed.to(dev, non_blocking=True), torch.from_numpy(mhost).to(dev)
    n = len(descs)
    stats = torch.empty((n, 4), dtype=torch.int64, device=dev) if return_stats else None
    out = inpaint_buffers(buf, descs_tensor(descs).to(dev), mbuf, descs_tensor(mdescs).to(dev), n, channels, max_pixels=int(areas.max()),
                          rows=int(hs.sum()), max_side=int(max(hs.max(), ws_.max())), cycles=cycles, stats=stats)
    res = D.ragged_views(out, descs, channels)
    return (res, stats.cpu().numpy()) if return_stats else res


def inpaint(image, mask, cycles: int = DEFAULT_CYCLES, return_stats: bool = False, device="cuda"):
    """one uint8 (h, w, C) or (h, w) image and its (h, w) mask -> the filled image as a device tensor of the image's shape"""
    a = image if isinstance(image, torch.Tensor) else np.asarray(image)
    grey = a.ndim == 2
    res = inpaint_ragged([a[:, :, None] if grey else a], [mask], cycles, return_stats, device)
    imgs, stats = res if return_stats else (res, None)
    o = imgs[0][:, :, 0] if grey else imgs[0]
    return (o, stats[0]) if return_stats else o
