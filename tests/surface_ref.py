"""The restatement of uwm_edt_ragged and uwm_surface_distances_ragged (include/uwm.h) in numpy and scipy, for the tests:
the border is scipy's binary_erosion with the 4-neighbour cross (MedPy's convention), D2 comes from the nearest-pixel indices of
scipy's exact distance_transform_edt in integer arithmetic, and the record is the definition written out."""
import numpy as np
from scipy import ndimage

EDT_NONE = 2 ** 31 - 1
MISFIT = np.array([0] * 9 + [1], dtype=np.int64)
CROSS = ndimage.generate_binary_structure(2, 1)


def binary(mask):
    return np.asarray(mask) > 127


def border(m):
    """m & ~erode(m), m boolean; everything outside the image is unset"""
    return m & ~ndimage.binary_erosion(m, CROSS, border_value=0)


def d2(m):
    """the squared Euclidean distance of every pixel to the nearest set pixel of the boolean m, int64; EDT_NONE without one"""
    if not m.any():
        return np.full(m.shape, EDT_NONE, np.int64)
    idx = ndimage.distance_transform_edt(~m, return_distances=False, return_indices=True)
    yy, xx = np.indices(m.shape)
    return (yy - idx[0]).astype(np.int64) ** 2 + (xx - idx[1]).astype(np.int64) ** 2


def lists(pred, truth):
    """-> (a, b): D2(border of truth) at the prediction's border pixels, D2(border of prediction) at the truth's, int64"""
    bp, bg = border(binary(pred)), border(binary(truth))
    return d2(bg)[bp], d2(bp)[bg]


def record(pred, truth):
    """-> (int64 [10] record, float64 [2] sums) of one pair"""
    p, g = binary(pred), binary(truth)
    a, b = lists(pred, truth)
    out = np.zeros(10, np.int64)
    out[0], out[1] = a.size, b.size
    out[7] = 0 if not g.any() else -1 if not p.any() else int(d2(p)[g].max())
    if not p.any() and not g.any():
        out[8] = 1
        return out, np.zeros(2)
    if not p.any() or not g.any():
        out[2:6] = -1
        return out, np.zeros(2)
    v = np.sort(np.concatenate([a, b]))
    lo, rem = divmod(95 * (v.size - 1), 100)
    out[2], out[3], out[4], out[5], out[6], out[8] = a.max(), b.max(), v[lo], v[lo + (rem > 0)], rem, 1
    return out, np.array([np.sqrt(a.astype(np.float64)).sum(), np.sqrt(b.astype(np.float64)).sum()])


def records(preds, truths):
    got = [record(p, t) for p, t in zip(preds, truths)]
    return np.stack([r for r, _ in got]), np.stack([s for _, s in got])
