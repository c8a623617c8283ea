"""numpy / scipy / Pillow restatement of the watermark extraction (include/uwm.h), written from the stated rules: what
the device calls are compared with, plus the literal checks of those rules (a border follower with the shoelace formulas, scipy's
binary_fill_holes, Pillow's ImageEnhance / ImageFilter run as they are)."""
import math
import os

import numpy as np
from PIL import Image, ImageEnhance
from scipy import ndimage

import resize_ref

RECT3 = np.ones((3, 3), bool)
MAX_REGIONS = 254


# ------------------------------------------------------------------------------------------------ stage 1
def binary_mask(wm, clean, threshold):
    """gray(|wm - clean|) > threshold, then close and open with the 3 x 3 RECT element (outside pixels ignored)"""
    d = np.abs(wm.astype(np.int64) - clean.astype(np.int64))
    g = (d[..., 0] * 9798 + d[..., 1] * 19235 + d[..., 2] * 3735 + 16384) >> 15
    m = g > int(threshold)
    m = ndimage.binary_erosion(ndimage.binary_dilation(m, RECT3, border_value=0), RECT3, border_value=1)
    return ndimage.binary_dilation(ndimage.binary_erosion(m, RECT3, border_value=1), RECT3, border_value=0)


def fill(m):
    """B2 by its own words: m plus every background pixel that is not 4-connected through background to the outside"""
    h, w = m.shape
    pad = np.zeros((h + 2, w + 2), bool)
    pad[1:-1, 1:-1] = m
    lab, _ = ndimage.label(~pad)                            # 4-connected (the default cross)
    return m | (lab[1:-1, 1:-1] != lab[0, 0]) & ~m


def label_regions(F):
    """8-connected components -> (labels 1.., ids): scipy numbers components by their raster-first pixel, ids[k-1] = y*w + x of it"""
    lab, n = ndimage.label(F, np.ones((3, 3), int))
    flat = lab.reshape(-1)
    ids = np.zeros(n, np.int64)
    if n:
        idx = np.flatnonzero(flat)
        first = np.full(n + 1, flat.size, np.int64)
        np.minimum.at(first, flat[idx], idx)
        ids = first[1:]
        assert np.all(np.diff(ids) > 0)
    return lab, ids


def window_sums(F, lab, n):
    """B4: (a00, a10, a01) per label 1..n over every 2 x 2 window of neighbouring pixels (a window that reaches outside the image has at
    most two corners in F)"""
    a = np.zeros((n + 1, 3), np.int64)
    f = F.astype(np.int64)
    c = [f[:-1, :-1], f[:-1, 1:], f[1:, :-1], f[1:, 1:]]
    cnt = c[0] + c[1] + c[2] + c[3]
    who = np.maximum(np.maximum(lab[:-1, :-1], lab[:-1, 1:]), np.maximum(lab[1:, :-1], lab[1:, 1:]))
    y, x = np.mgrid[0:F.shape[0] - 1, 0:F.shape[1] - 1]
    four = cnt == 4
    np.add.at(a, (who[four], 0), 2); np.add.at(a, (who[four], 1), 6 * x[four] + 3); np.add.at(a, (who[four], 2), 6 * y[four] + 3)
    three = cnt == 3
    sx = c[0] * x + c[1] * (x + 1) + c[2] * x + c[3] * (x + 1)
    sy = c[0] * y + c[1] * y + c[2] * (y + 1) + c[3] * (y + 1)
    np.add.at(a, (who[three], 0), 1); np.add.at(a, (who[three], 1), sx[three]); np.add.at(a, (who[three], 2), sy[three])
    return a[1:]


def regions(wm, clean, threshold, min_area):
    """-> dict(status, found, kept, rows (kept, 9) int64, plane uint8): what uwm_extract_regions_ragged returns for one pair"""
    h, w = wm.shape[:2]
    if wm.shape != clean.shape or h < 3 or w < 3:
        return dict(status=1, found=0, kept=0, rows=np.zeros((0, 9), np.int64), plane=None)
    F = fill(binary_mask(wm, clean, threshold))
    lab, ids = label_regions(F)
    sums = window_sums(F, lab, len(ids))
    keep = [k for k in range(len(ids)) if sums[k, 0] > 2 * int(min_area)]
    plane = np.full((h, w), 255, np.uint8)
    if len(keep) > MAX_REGIONS:
        return dict(status=2, found=len(ids), kept=len(keep), rows=np.zeros((0, 9), np.int64), plane=plane)
    rows = np.zeros((len(keep), 9), np.int64)
    for r, k in enumerate(keep):
        ys, xs = np.nonzero(lab == k + 1)
        rows[r] = (ids[k], sums[k, 0], sums[k, 1], sums[k, 2], xs.min(), ys.min(), xs.max(), ys.max(), len(xs))
        plane[lab == k + 1] = r
    return dict(status=0, found=len(ids), kept=len(keep), rows=rows, plane=plane)


# ------------------------------------------------------------------------------------------------ the literal contour rule
N8 = [(0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1)]      # (dy, dx): E NE N NW W SW S SE, counter-clockwise on screen


def outer_border(comp):
    """Border following (Suzuki and Abe 1985, step 3) of the outer border of one 8-connected component: the (x, y) sequence
    cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_NONE) would give.  comp: bool array holding that component alone"""
    h, w = comp.shape

    def at(y, x):
        return 0 <= y < h and 0 <= x < w and comp[y, x]
    y0, x0 = divmod(int(np.flatnonzero(comp)[0]), w)
    first = None
    for k in range(8):                                      # clockwise from west
        d = (4 - k) % 8
        if at(y0 + N8[d][0], x0 + N8[d][1]):
            first = d
            break
    if first is None:
        return [(x0, y0)]
    y1, x1 = y0 + N8[first][0], x0 + N8[first][1]
    pts = []
    y2, x2, y3, x3 = y1, x1, y0, x0
    while True:
        d2 = N8.index((y2 - y3, x2 - x3))
        for k in range(1, 9):                               # counter-clockwise from the element after (y2, x2)
            d = (d2 + k) % 8
            if at(y3 + N8[d][0], x3 + N8[d][1]):
                y4, x4 = y3 + N8[d][0], x3 + N8[d][1]
                break
        pts.append((x3, y3))
        if (y4, x4) == (y0, x0) and (y3, x3) == (y1, x1):
            return pts
        y2, x2, y3, x3 = y3, x3, y4, x4


def shoelace(pts):
    """(a00, a10, a01) of the closed polygon: 2 * area and 6 * the first moments, as cv2.contourArea / cv2.moments sum them"""
    a00 = a10 = a01 = 0
    for (xa, ya), (xb, yb) in zip(pts, pts[1:] + pts[:1]):
        cr = xa * yb - xb * ya
        a00 += cr; a10 += cr * (xa + xb); a01 += cr * (ya + yb)
    return (-a00, -a10, -a01) if a00 < 0 else (a00, a10, a01)


def random_mask(rng, smooth):
    h, w = (int(v) for v in rng.integers(5, 41, 2))
    if smooth:
        f = ndimage.gaussian_filter(rng.standard_normal((h, w)), float(rng.uniform(0.8, 3.0)))
        return f > np.quantile(f, float(rng.uniform(0.3, 0.8)))
    return rng.random((h, w)) < float(rng.uniform(0.2, 0.7))


# ------------------------------------------------------------------------------------------------ stage 2
def cutout(wm, plane, job):
    """one cut-out, Pillow run literally: RGBA crop, alpha on the member regions, Contrast 1.3, Sharpness 1.4, Brightness 1.1"""
    x, y, w, h = job["x"], job["y"], job["w"], job["h"]
    member = np.zeros(256, bool)
    member[list(job["members"])] = True
    member[255] = False
    rgba = np.dstack([wm[y:y + h, x:x + w], np.where(member[plane[y:y + h, x:x + w]], 255, 0).astype(np.uint8)])
    im = Image.fromarray(np.ascontiguousarray(rgba))
    assert im.mode == "RGBA"
    im = ImageEnhance.Contrast(im).enhance(1.3)
    im = ImageEnhance.Sharpness(im).enhance(1.4)
    im = ImageEnhance.Brightness(im).enhance(1.1)
    return np.asarray(im)


def blend8(d, v, f):
    """Image.blend(degenerate, image, f) for f > 1, in float32"""
    f = np.float32(f)
    t = d.astype(np.float32) + f * (v.astype(np.float32) - d.astype(np.float32))
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t)).astype(np.uint8)


def enhance_restated(rgba):
    """the enhancement as the device computes it (include/uwm.h), in numpy: held to Pillow by tests/test_extract.py"""
    rgb = rgba[..., :3].astype(np.int64)
    L = (19595 * rgb[..., 0] + 38470 * rgb[..., 1] + 7471 * rgb[..., 2] + 0x8000) >> 16
    mean = int(float(L.sum()) / float(L.size) + 0.5)
    c = blend8(np.full(rgb.shape, mean, np.uint8), rgba[..., :3], 1.3)
    k1, k5 = np.float32(1) / np.float32(13), np.float32(5) / np.float32(13)
    x = c.astype(np.float32)
    d = c.copy()
    if c.shape[0] >= 3 and c.shape[1] >= 3:
        ss = np.full(x[1:-1, 1:-1].shape, 0.5, np.float32)
        for rows, kc in ((x[2:], k1), (x[1:-1], k5), (x[:-2], k1)):
            ss = ss + ((rows[:, :-2] * k1 + rows[:, 1:-1] * kc) + rows[:, 2:] * k1)
        d[1:-1, 1:-1] = np.where(ss <= 0, 0, np.where(ss >= 255, 255, ss)).astype(np.uint8)
    s = blend8(d, c, 1.4)
    b = blend8(np.zeros_like(s), s, 1.1)
    return np.dstack([b, rgba[..., 3]])


# ------------------------------------------------------------------------------------------------ the whole tool
def predict_folder(pairs, threshold, min_area, plan_cutouts):
    """pairs: [(stem, clean array or None, wm array or None)] -> (files {name: RGBA array}, counts) as `main.py extract` must write
    them; plan_cutouts: the package's host plan (checked on its own in tests/test_extract.py)"""
    files, counts = {}, dict(processed=0, extracted=0, written=0, errors=0)
    for stem, clean, wm in pairs:
        if clean is None or wm is None:
            counts["errors"] += 1
            continue
        if clean.shape != wm.shape:
            h, w = min(clean.shape[0], wm.shape[0]), min(clean.shape[1], wm.shape[1])
            clean, wm = resize_ref.resize_u8_linear(clean, h, w), resize_ref.resize_u8_linear(wm, h, w)
        counts["processed"] += 1
        r = regions(wm, clean, threshold, min_area)
        if r["status"] != 0:
            counts["errors"] += 1
            continue
        cuts = plan_cutouts([(0, r["rows"])], [wm.shape[:2]], [stem])[0]
        counts["extracted"] += bool(cuts)
        for c in cuts:
            files[c["name"]] = cutout(wm, r["plane"], c)
            counts["written"] += 1
    return files, counts


def reference_dbscan_eps(h, w):
    return math.sqrt(h * h + w * w) * 0.25


def read_rgba(path):
    with Image.open(os.fspath(path)) as im:
        assert im.mode == "RGBA", im.mode
        return np.asarray(im)
