"""Test-time augmentation, the part that needs no device: the view codes and sets of include/uwm.h, their torch
restatements, the slot table of a batch, and the merge restated on the host in float32, operation by operation.

A view is a code c = r + 4 f: view_c(x) = rot90^r(hflip^f(x)) — the horizontal flip first, then r counter-clockwise quarter turns
(torch.rot90).  A view set is a bitmask in 1..255; the network input of item i under the j-th view of the set (ascending code order) is
slot i * k + j.  The merge is the mean of the LOGIT planes mapped back, summed in ascending code order — not of the probabilities."""
from __future__ import annotations

import numpy as np
import torch

VIEW_SETS = {"none": 0x01, "hflip": 0x11, "flips": 0x55, "d4": 0xFF}


def view_mask(name_or_int) -> int:
    """'none' | 'hflip' | 'flips' | 'd4' or a bitmask in 1..255 (None: 'none') -> the bitmask"""
    if name_or_int is None:
        return VIEW_SETS["none"]
    if isinstance(name_or_int, str):
        if name_or_int not in VIEW_SETS:
            raise ValueError(f"tta must be one of {', '.join(VIEW_SETS)} or a view mask in 1..255, got {name_or_int!r}")
        return VIEW_SETS[name_or_int]
    if isinstance(name_or_int, bool) or not isinstance(name_or_int, (int, np.integer)) or not 1 <= int(name_or_int) <= 255:
        raise ValueError(f"a view mask must be an integer in 1..255, got {name_or_int!r}")
    return int(name_or_int)


def view_codes(mask) -> list:
    """the codes of the set, ascending"""
    mask = view_mask(mask)
    return [c for c in range(8) if (mask >> c) & 1]


def _check(x, code: int):
    if isinstance(code, bool) or not 0 <= int(code) <= 7:
        raise ValueError(f"a view code must be in 0..7, got {code!r}")
    if x.dim() < 2:
        raise ValueError("a view takes a tensor whose last two dimensions are (H, W)")
    if (int(code) & 1) and x.shape[-2] != x.shape[-1]:
        raise ValueError(f"view {code} (a quarter turn) needs H == W, got {x.shape[-2]} x {x.shape[-1]}")


def apply_view(x: torch.Tensor, code: int) -> torch.Tensor:
    """view_code of the (H, W) plane(s) in the last two dimensions of x"""
    _check(x, code)
    r, f = int(code) & 3, int(code) >> 2
    if f:
        x = torch.flip(x, (-1,))
    return torch.rot90(x, r, (-2, -1)).contiguous()


def invert_view(x: torch.Tensor, code: int) -> torch.Tensor:
    """view_code^-1: invert_view(apply_view(x, c), c) == x"""
    _check(x, code)
    r, f = int(code) & 3, int(code) >> 2
    x = torch.rot90(x, -r, (-2, -1))
    if f:
        x = torch.flip(x, (-1,))
    return x.contiguous()


def plan_slots(num: int, mask, batch: int):
    """the slot table of `num` items under the view set, run `batch` at a time -> (table, chunks): table an int32 (chunks * batch, 2)
    array of (item, code) per slot, slot i * k + j = the j-th view of item i, padding slots (-1, 0); chunks = ceil(num * k / batch)"""
    num, batch = int(num), int(batch)
    if num < 1 or batch < 1:
        raise ValueError(f"plan_slots needs at least one item and a batch of at least 1, got {num}, {batch}")
    codes = view_codes(mask)
    k = len(codes)
    chunks = -(-num * k // batch)
    table = np.zeros((chunks * batch, 2), np.int32)
    table[:, 0] = -1
    table[: num * k, 0] = np.repeat(np.arange(num, dtype=np.int32), k)
    table[: num * k, 1] = np.tile(np.asarray(codes, np.int32), num)
    return table, chunks


def merge_views(planes: torch.Tensor, mask) -> torch.Tensor:
    """planes (k, H, W) or (B, k, H, W) float32: the logit planes of the set's views, ascending code order, each still in its view ->
    the merged plane(s): acc = l'_0; acc += l'_j in order; acc / float32(k) (k > 1), l'_j = invert_view(l_j, c_j), every operation
    a float32 operation of its own.  The arithmetic runs on the host, whatever device the planes live on; the result goes back there"""
    codes = view_codes(mask)
    k = len(codes)
    if planes.dtype != torch.float32 or planes.dim() not in (3, 4) or planes.shape[-3] != k:
        raise ValueError(f"merge_views takes float32 planes (k, H, W) or (B, k, H, W) with k = {k}, got {planes.dtype} {tuple(planes.shape)}")
    host = planes.detach().cpu()
    acc = invert_view(host[..., 0, :, :], codes[0]).clone()
    for j in range(1, k):
        acc = acc + invert_view(host[..., j, :, :], codes[j])
    if k > 1:
        acc = acc / torch.tensor(float(k), dtype=torch.float32)
    return acc.to(planes.device)
