"""Prediction at native resolution: the tile plan of WatermarkPredictor.predict_images_tiled (csrc/tile_u8.hip; the rule:
include/uwm.h).  An image is cut into model-sized tiles that overlap, every tile goes through the eval forward, and
the tile logits are blended back into one plane at the image's own size.  All of this module is host arithmetic on integers; the
device derives the tiles that cover a pixel from the same formula, so the table below and the blend cannot disagree.

One axis of length `len`, tile side T, S = T - overlap:
    len <= T : one tile at origin 0 (the part of the tile outside the image is filled by reflection on the device)
    len >  T : n = ceil((len - T) / S) + 1 tiles at o_j = min(j * S, len - T): the last tile ends at the border
Tiles of an image are ordered row-major (jy outer, jx inner)."""
from __future__ import annotations

import numpy as np

TILE_DTYPE = np.dtype([("image", "<i4"), ("y0", "<i4"), ("x0", "<i4"), ("first", "<i4")])          # = uwm_tile_desc, 16 bytes
TILE_IMAGE_DTYPE = np.dtype([("first", "<i4"), ("ny", "<i4"), ("nx", "<i4"), ("reserved", "<i4")])  # = uwm_tile_image, 16 bytes
MAX_TILE = 1024                           # the blend's integer weights and their sums are exact in fp32 up to this side


def check_overlap(T_h: int, T_w: int, overlap) -> int:
    """`overlap` as an int, or ValueError: an integer in [0, T / 2] on both axes"""
    if isinstance(overlap, bool) or not isinstance(overlap, (int, np.integer)):
        raise ValueError(f"overlap must be an integer, got {overlap!r}")
    for T in (T_h, T_w):
        if isinstance(T, bool) or not isinstance(T, (int, np.integer)) or not 1 <= T <= MAX_TILE:
            raise ValueError(f"a tile side must be an integer in 1..{MAX_TILE}, got {T!r}")
    if overlap < 0 or 2 * overlap > min(T_h, T_w):
        raise ValueError(f"overlap must lie in [0, T / 2] on both axes (tile {T_h} x {T_w}), got {overlap}")
    return int(overlap)


def axis_count(length: int, T: int, overlap: int) -> int:
    """tiles along one axis"""
    if length < 1:
        raise ValueError(f"a side must be >= 1, got {length}")
    if length <= T:
        return 1
    S = T - overlap
    return -(-(length - T) // S) + 1


def axis_origins(length: int, T: int, overlap: int) -> list:
    """the tile origins along one axis, ascending"""
    n = axis_count(length, T, overlap)
    if n == 1:
        return [0]
    S = T - overlap
    return [min(j * S, length - T) for j in range(n)]


def plan_tiles(h: int, w: int, T_h: int, T_w: int, overlap: int) -> list:
    """the (y0, x0) of every tile of an h x w image, row-major"""
    overlap = check_overlap(T_h, T_w, overlap)
    ys, xs = axis_origins(int(h), int(T_h), overlap), axis_origins(int(w), int(T_w), overlap)
    return [(y0, x0) for y0 in ys for x0 in xs]


def plan_batch(sizes, T_h: int, T_w: int, overlap: int, N: int):
    """[(h, w), ...] -> (tiles, images): `tiles` the uwm_tile_desc table (TILE_DTYPE) of all images' plans back to back, padded to a
    multiple of the forward batch N with image = -1 entries; `images` one uwm_tile_image (TILE_IMAGE_DTYPE) per image: the index of
    its first tile in the table and its tile counts along y and x"""
    overlap = check_overlap(T_h, T_w, overlap)
    if int(N) < 1:
        raise ValueError(f"the forward batch must be >= 1, got {N}")
    if len(sizes) == 0:
        raise ValueError("plan_batch: no images")
    images = np.zeros(len(sizes), TILE_IMAGE_DTYPE)
    rows = []
    for i, (h, w) in enumerate(sizes):
        ys, xs = axis_origins(int(h), int(T_h), overlap), axis_origins(int(w), int(T_w), overlap)
        first = len(rows)
        images[i] = (first, len(ys), len(xs), 0)
        rows.extend((i, y0, x0, first) for y0 in ys for x0 in xs)
        if len(rows) > 2 ** 31 - 1 - int(N):
            raise ValueError("plan_batch: more than 2^31 tiles")
    K = -(-len(rows) // int(N)) * int(N)
    tiles = np.zeros(K, TILE_DTYPE)
    tiles["image"] = -1
    if rows:
        tiles[:len(rows)] = np.array(rows, dtype=np.int32).view(TILE_DTYPE).reshape(-1)
    return tiles, images


def table_tensor(table, device=None):
    """a TILE_DTYPE / TILE_IMAGE_DTYPE array -> its bytes as a uint8 tensor (on `device` when given)"""
    import torch
    d = np.ascontiguousarray(table)
    if d.dtype not in (TILE_DTYPE, TILE_IMAGE_DTYPE) or d.ndim != 1:
        raise TypeError("expected a 1-D array of tiling.TILE_DTYPE or tiling.TILE_IMAGE_DTYPE")
    t = torch.from_numpy(d.view(np.uint8).copy())
    return t if device is None else t.to(device)
