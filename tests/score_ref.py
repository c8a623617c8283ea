"""numpy / scipy restatement of uwm_score_masks_ragged (include/uwm.h): the eight counts per mask pair.  The test
side's oracle; the library never imports it."""
import numpy as np
from scipy import ndimage

_SQUARE = np.ones((3, 3), dtype=bool)


def binarise(mask_u8):
    return np.asarray(mask_u8) > 127


def erode(m, d):
    """E_d: the 3 x 3 square erosion iterated d times, everything outside the image unset"""
    m = np.asarray(m, dtype=bool)
    if d <= 0:
        return m.copy()
    return ndimage.binary_erosion(m, _SQUARE, iterations=int(d), border_value=0)


def erode_brute(m, d):
    """E_d by its definition: the whole (2d+1) x (2d+1) window centred on the pixel lies inside the image and is set"""
    m = np.asarray(m, dtype=bool)
    h, w = m.shape
    out = np.zeros_like(m)
    for y in range(d, h - d):
        for x in range(d, w - d):
            out[y, x] = m[y - d: y + d + 1, x - d: x + d + 1].all()
    return out


def boundary(m, d, erosion=erode):
    return m & ~erosion(m, d)


def counts(pred_u8, truth_u8, d, erosion=erode):
    """the int64 [8] row of one pair: tp, fp, fn, tn, |B(P) & B(G)|, |B(P)|, |B(G)|, status 0"""
    p, g = binarise(pred_u8), binarise(truth_u8)
    row = [int((p & g).sum()), int((p & ~g).sum()), int((~p & g).sum()), int((~p & ~g).sum()), 0, 0, 0, 0]
    if d > 0:
        bp, bg = boundary(p, d, erosion), boundary(g, d, erosion)
        row[4:7] = [int((bp & bg).sum()), int(bp.sum()), int(bg.sum())]
    return np.array(row, dtype=np.int64)


def counts_batch(preds, truths, radii, erosion=erode):
    return np.stack([counts(p, g, int(d), erosion) for p, g, d in zip(preds, truths, radii)])


MISFIT = np.array([0, 0, 0, 0, 0, 0, 0, 1], dtype=np.int64)
