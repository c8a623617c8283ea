"""What every wrapper of this package needs around its library call: the tensor checks, the uploads, the ctypes arguments, the
per-device workspaces (one store for the whole package, with a recorder for the owner of a captured graph) and, for the calls on
a ragged batch (a flat uint8 buffer + uwm_image_desc records), their capacities, argument checks and per-image views."""
import ctypes as C
from contextlib import contextmanager

import numpy as np
import torch

from . import _lib as L

_WORKSPACE = {}
_RECORDERS = []


def resolve(device) -> torch.device:
    """`device` as a torch.device with its index: an index-less 'cuda' is the current device, so 'cuda' and 'cuda:0' are one key"""
    d = device if isinstance(device, torch.device) else torch.device(device)
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


def workspace(name, device, nbytes, exc=RuntimeError) -> torch.Tensor:
    """one uint8 workspace per (name, device), grown when a larger one is needed (calls on one stream are ordered, so it is reused).
    nbytes: what the call's uwm_*_workspace_bytes query returned; 0 is its refusal, raised as `exc` with the library's message.
    A captured graph holds the buffer it was captured with: its owner pins that buffer (`recording`), so growing the store's entry
    later for a larger call leaves the graph valid."""
    if nbytes == 0:
        L.check(1, exc)
    key = (name, resolve(device))
    ws = _WORKSPACE.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _WORKSPACE[key] = torch.empty(int(nbytes), dtype=torch.uint8, device=key[1])
    for seen in _RECORDERS:
        seen.append(ws)
    return ws


@contextmanager
def recording():
    """-> the list of every tensor `workspace` hands out while the context is active, in call order"""
    seen = []
    _RECORDERS.append(seen)
    try:
        yield seen
    finally:
        _RECORDERS.remove(seen)


def device_u8(t: torch.Tensor, ndim: int, refusal: str, upload=False) -> torch.Tensor:
    """t, contiguous, when it is a uint8 tensor of `ndim` dimensions on a HIP device (upload: a host tensor is brought there first,
    where there is a device); RuntimeError(refusal) otherwise"""
    if upload and t.device.type != "cuda" and torch.cuda.is_available():
        t = t.cuda(non_blocking=True)
    if t.device.type != "cuda" or t.dtype != torch.uint8 or t.dim() != ndim:
        raise RuntimeError(refusal)
    return t.contiguous()


def norm_arrays(mean, std, c):
    """-> the first c entries of mean and of std as ctypes float arrays"""
    return (C.c_float * c)(*[float(v) for v in mean[:c]]), (C.c_float * c)(*[float(v) for v in std[:c]])


def upload_records(records: np.ndarray, device) -> torch.Tensor:
    """the bytes of a numpy array (of any dtype, structured ones included) -> a pinned copy -> a non-blocking upload to `device`"""
    host = torch.from_numpy(np.ascontiguousarray(records).reshape(-1).view(np.uint8).copy())
    return (host.pin_memory() if torch.cuda.is_available() else host).to(device, non_blocking=True)


def ptr(t) -> C.c_void_p:
    """a tensor's address, NULL for None"""
    return C.c_void_p(t.data_ptr() if t is not None else 0)


# ---------------------------------------------------------------- ragged batches
def ragged_capacities(descs) -> dict:
    """host uwm_image_desc records -> the capacities a ragged call may ask for: max_pixels (the largest h*w), rows (the sum of h),
    total_pixels (the sum of h*w); negative sides count as 0 and every capacity is at least 1.  Pure numpy."""
    if len(descs) == 0:
        raise ValueError("ragged_capacities: empty batch")
    h, w = descs["h"].astype("int64").clip(min=0), descs["w"].astype("int64").clip(min=0)
    areas = h * w
    return {"max_pixels": max(1, int(areas.max())), "rows": max(1, int(h.sum())), "total_pixels": max(1, int(areas.sum()))}


def ragged_args(name, buffers, descs, n, **caps):
    """The checks every ragged wrapper makes before its library call.  buffers: the call's flat uint8 device tensors; descs: a host
    record array with the fields offset / h / w (uploaded here; n and the capacities left None are derived from it), or a device tensor
    of uwm_image_desc bytes — then n and every capacity in `caps` must be given, and nothing about the batch is read on the host.
    -> (descs tensor, n, capacities)"""
    first = buffers[0]
    if any(not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.device != first.device for t in buffers):
        raise RuntimeError(f"uwm {name} runs only on a HIP device (no CPU fallback)")
    for t in buffers:
        if t.dtype != torch.uint8 or t.dim() != 1 or t.numel() == 0 or not t.is_contiguous():
            raise RuntimeError(f"expected a non-empty contiguous 1-d uint8 buffer, got {t.dtype} {tuple(t.shape)}")
    if isinstance(descs, torch.Tensor):
        if n is None or None in caps.values():
            names = ["n", *caps]
            raise ValueError(f"{name}: device descriptors need {', '.join(names[:-1])} and {names[-1]}")
        if descs.device != first.device or descs.dtype != torch.uint8 or descs.numel() < 16 * int(n):
            raise RuntimeError(f"{name}: descs must be a uint8 tensor of 16 n bytes on the buffers' device")
        d = descs
    else:
        from .data.ragged import descs_tensor
        n = len(descs) if n is None else int(n)
        if n < 1:
            raise ValueError(f"{name}: empty batch")
        if None in caps.values():
            derived = ragged_capacities(descs)
            caps = {k: derived[k] if v is None else v for k, v in caps.items()}
        d = descs_tensor(descs).to(first.device)
    return d, int(n), {k: int(v) for k, v in caps.items()}


def out_like(name, out, buf) -> torch.Tensor:
    """the call's output buffer: `out` when it is a contiguous uint8 tensor of buf's size on its device, a zero-filled one for None"""
    if out is None:
        return torch.zeros_like(buf)
    if out.dtype != torch.uint8 or out.device != buf.device or out.numel() != buf.numel() or not out.is_contiguous():
        raise RuntimeError(f"{name}: out must be a contiguous uint8 tensor of the buffer's size on the same device")
    return out


def stats_like(name, stats, n, fields, device, dtype=torch.int64, what="stats") -> torch.Tensor:
    """the call's per-image records: `stats` when it is a contiguous `dtype` tensor of at least n * fields entries on `device`, a new
    (n, fields) one for None"""
    if stats is None:
        return torch.empty((n, fields), dtype=dtype, device=device)
    if stats.dtype != dtype or stats.device != device or stats.numel() < fields * n or not stats.is_contiguous():
        raise RuntimeError(f"{name}: {what} must be a contiguous {str(dtype).split('.')[-1]} tensor of {fields} n entries on the buffers' device")
    return stats


def ragged_views(buf, descs, channels=None) -> list:
    """a flat buffer and the host records of its images -> the per-image views: (h, w, channels), or (h, w) of one element per pixel
    when channels is None"""
    c = 1 if channels is None else int(channels)
    return [buf[int(o): int(o) + c * int(h) * int(w)].view((int(h), int(w)) if channels is None else (int(h), int(w), c))
            for o, h, w in zip(descs["offset"], descs["h"], descs["w"])]
