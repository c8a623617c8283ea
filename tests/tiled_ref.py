"""numpy restatement of the tiled prediction's rule (csrc/tile_u8.hip; include/uwm.h): the tile plan of one axis, the
reflected crop that the gather makes, and the blend of tile logits into one plane, in np.float32 operations in the stated order.
Written from the rule, not from unet_watermark_amd/tiling.py, which tests/test_tiled.py holds against it.  A helper of
tests/test_tiled.py and tests/test_tiled_gpu.py, not itself a test."""
import numpy as np

F = np.float32


def axis_origins(length, T, overlap):
    """len <= T: [0]; else n = ceil((len - T) / S) + 1 origins min(j * S, len - T), S = T - overlap"""
    if length <= T:
        return [0]
    S = T - overlap
    n = (length - T + S - 1) // S + 1
    return [min(j * S, length - T) for j in range(n)]


def plan(h, w, T_h, T_w, overlap):
    """(y0, x0) of every tile, row-major"""
    return [(y0, x0) for y0 in axis_origins(h, T_h, overlap) for x0 in axis_origins(w, T_w, overlap)]


def reflect101(c, n):
    """cv2.borderInterpolate(BORDER_REFLECT_101) of integer coordinates (an array) into [0, n): period 2 (n - 1); n = 1 gives 0"""
    c = np.asarray(c, np.int64)
    if n == 1:
        return np.zeros_like(c)
    p = 2 * (n - 1)
    m = np.mod(c, p)
    return np.where(m < n, m, p - m)


def crop(img, y0, x0, T_h, T_w):
    """the T_h x T_w tile of img (h, w, C) at (y0, x0), reflected where it leaves the image"""
    iy = reflect101(y0 + np.arange(T_h), img.shape[0])
    ix = reflect101(x0 + np.arange(T_w), img.shape[1])
    return img[iy][:, ix]


def w1(T):
    """the weight along one axis: min(t + 1, T - t), integers"""
    t = np.arange(T, dtype=np.int64)
    return np.minimum(t + 1, T - t)


def blend(tile_logits, h, w, T_h, T_w, overlap):
    """tile_logits: float32 (tiles, T_h, T_w) in plan order -> float32 (h, w).  A pixel under one tile takes that tile's logit
    unchanged; otherwise acc = w_0 * l_0, acc += w_k * l_k in plan order, v = acc / sum(w), every operation rounded to float32"""
    tile_logits = np.asarray(tile_logits, F)
    origins = plan(h, w, T_h, T_w, overlap)
    assert tile_logits.shape == (len(origins), T_h, T_w)
    wy, wx = w1(T_h), w1(T_w)
    wt = (wy[:, None] * wx[None, :])                       # integers <= 2^18: exact in float32
    acc = np.zeros((h, w), F)
    wsum = np.zeros((h, w), np.int64)
    count = np.zeros((h, w), np.int64)
    single = np.zeros((h, w), F)
    for lg, (y0, x0) in zip(tile_logits, origins):
        th, tw = min(T_h, h - y0), min(T_w, w - x0)        # (the padded part of a tile is never output)
        sl = (slice(y0, y0 + th), slice(x0, x0 + tw))
        term = wt[:th, :tw].astype(F) * lg[:th, :tw]       # float32 product, rounded
        fresh = count[sl] == 0
        acc[sl] = np.where(fresh, term, acc[sl] + term)    # the first term is taken as it is, the others are float32 additions
        single[sl] = np.where(fresh, lg[:th, :tw], single[sl])
        wsum[sl] += wt[:th, :tw]
        count[sl] += 1
    assert (count >= 1).all()
    return np.where(count == 1, single, acc / wsum.astype(F)).astype(F)


def predict_mask(v, threshold, apply_sigmoid, sigmoid32=None):
    """blended plane -> uint8 {0, 255}; sigmoid32: the project's float32 sigmoid restatement (tests/filter_ref.sigmoid32)"""
    p = sigmoid32(v) if apply_sigmoid else np.asarray(v, F)
    return ((p > F(threshold)).astype(np.uint8)) * 255
