"""What every device_* wrapper of this package needs around its library call: the tensor checks, the uploads, the ctypes arguments
and the per-device workspaces."""
import ctypes as C

import numpy as np
import torch

_WORKSPACE = {}


def workspace(name, device, nbytes) -> torch.Tensor:
    """one uint8 workspace per (name, device), grown when a larger one is needed (calls on one stream are ordered, so it is reused)"""
    ws = _WORKSPACE.get((name, device))
    if ws is None or ws.numel() < nbytes:
        ws = _WORKSPACE[(name, device)] = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    return ws


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
