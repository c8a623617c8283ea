"""CPU restatement of the mask post-processing specification (test-side only, numpy only).

The reference passes every predicted mask through WatermarkPredictor._optimize_mask (OpenCV morphology, an 8-connected
component analysis, a selection by area).  DESIGN.md §8b states what that chain computes; this module is that statement in
numpy, and the device kernels (csrc/mask_post.hip) must equal it bit for bit.  It also builds the case list of
tests/golden/maskpost.npz (`python tests/maskpost_ref.py` rewrites that file).

Masks are bool (H, W) here; foreground of a uint8 mask is `> 127`.
"""
from __future__ import annotations

import os

import numpy as np

RECT, ELLIPSE = 0, 2                     # cv2.MORPH_RECT / cv2.MORPH_ELLIPSE
MASK_TYPES = ("watermark", "text", "mixed")


# ------------------------------------------------------------------ structuring elements (cv2.getStructuringElement)
def ellipse(w, h):
    r, c = h // 2, w // 2
    inv_r2 = 1.0 / (r * r) if r else 0.0
    k = np.zeros((h, w), np.uint8)
    for i in range(h):
        dy = i - r
        if abs(dy) <= r:
            dx = int(np.rint(c * np.sqrt((r * r - dy * dy) * inv_r2)))       # round half to even
            k[i, max(c - dx, 0):min(c + dx + 1, w)] = 1
    return k


def rect(w, h):
    return np.ones((h, w), np.uint8)


def element(shape, w, h):
    if shape == RECT:
        return rect(w, h)
    if shape == ELLIPSE:
        return ellipse(w, h)
    raise ValueError(f"unknown element shape {shape}")


# ------------------------------------------------------------------ morphology
def _morph(m, k, dilate):
    """dst(y,x) = OR / AND over k[i,j] != 0 of src(y+i-ay, x+j-ax), anchor (kw//2, kh//2); pixels outside are ignored"""
    H, W = m.shape
    kh, kw = k.shape
    ay, ax = kh // 2, kw // 2
    pad = np.zeros((H + kh, W + kw), bool) if dilate else np.ones((H + kh, W + kw), bool)
    pad[ay:ay + H, ax:ax + W] = m
    out = np.zeros((H, W), bool) if dilate else np.ones((H, W), bool)
    for i in range(kh):
        for j in range(kw):
            if k[i, j]:
                s = pad[i:i + H, j:j + W]
                out = (out | s) if dilate else (out & s)
    return out


def dilate(m, k, it=1):
    for _ in range(it):
        m = _morph(m, k, True)
    return m


def erode(m, k, it=1):
    for _ in range(it):
        m = _morph(m, k, False)
    return m


def opening(m, k, it=1):
    return dilate(erode(m, k, it), k, it)


def closing(m, k, it=1):
    return erode(dilate(m, k, it), k, it)


# ------------------------------------------------------------------ 8-connected components
def components(m):
    """-> (labels int32 (H,W): id + 1, 0 = background; areas int32 (H,W): area at the id pixel, 0 elsewhere).
    A component's id is the linear index y*W + x of its first pixel in raster order.  Union-find over horizontal runs."""
    H, W = m.shape
    labels = np.zeros((H, W), np.int32)
    areas = np.zeros((H, W), np.int32)
    if not m.any():
        return labels, areas
    p = np.zeros((H, W + 2), np.int8)
    p[:, 1:-1] = m
    d = np.diff(p, axis=1)
    ry, rs = np.nonzero(d == 1)                    # run starts (raster order)
    _, re = np.nonzero(d == -1)                    # run ends, exclusive (same order)
    nrun = len(ry)
    parent = list(range(nrun))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    row_first = np.searchsorted(ry, np.arange(H + 1))
    rs_l, re_l = rs.tolist(), re.tolist()
    for y in range(1, H):
        a, a_end = int(row_first[y - 1]), int(row_first[y])
        b, b_end = a_end, int(row_first[y + 1])
        while a < a_end and b < b_end:
            # 8-connectivity: runs [s,e) of adjacent rows touch when s_a <= e_b and s_b <= e_a
            if rs_l[a] <= re_l[b] and rs_l[b] <= re_l[a]:
                ra, rb = find(a), find(b)
                if ra != rb:
                    if ra < rb:
                        parent[rb] = ra
                    else:
                        parent[ra] = rb
            if re_l[a] < re_l[b]:
                a += 1
            else:
                b += 1
    root = np.array([find(i) for i in range(nrun)], np.int64)
    ids = (ry.astype(np.int64) * W + rs)[root]     # id of the run's component = start pixel of its root (= minimum) run
    length = (re - rs).astype(np.int64)
    labels[m] = np.repeat(ids + 1, length).astype(np.int32)
    np.add.at(areas.reshape(-1), ids, length.astype(np.int32))
    return labels, areas


def _select(m, mask_type):
    """-> (selected mask, summary [components, largest area, foreground of the output, id of the largest or -1])"""
    labels, areas = components(m)
    flat = areas.reshape(-1)
    ids = np.nonzero(flat)[0]
    n = len(ids)
    if n == 0:
        return m.copy(), [0, 0, int(m.sum()), -1]
    big = int(ids[np.argmax(flat[ids])])           # greatest area, ties to the smallest id (argmax takes the first)
    big_area = int(flat[big])
    area_of = np.concatenate([[0], flat])[labels]  # area of each pixel's component (labels index flat shifted by one)
    if mask_type == "watermark":
        out = (area_of > 200) if big_area < 500 else (labels == big + 1)
    elif mask_type == "text":
        out = area_of > 50
    elif mask_type == "mixed":
        out = area_of > 100
    else:
        raise ValueError(f"mask_type must be one of {MASK_TYPES}")
    return out, [n, big_area, int(out.sum()), big]


def _chain(m, mask_type):
    E = ellipse
    if mask_type == "watermark":
        m = opening(m, E(3, 3))
        m = closing(m, E(7, 7), 3)
        m = closing(m, E(11, 11), 2)
        return dilate(m, E(9, 9), 2)
    if mask_type == "text":
        m = opening(m, E(2, 2))
        m = closing(m, E(3, 3), 2)
        m = closing(m, rect(5, 1)) | closing(m, rect(1, 5))
        return dilate(m, E(4, 4))
    if mask_type == "mixed":
        m = opening(m, E(2, 2))
        m = closing(m, E(5, 5), 2)
        return dilate(m, E(6, 6))
    raise ValueError(f"mask_type must be one of {MASK_TYPES}")


def optimize_mask(mask_u8, mask_type="watermark"):
    """uint8 (H,W) -> (uint8 {0,255} (H,W), summary list of 4 ints).  The reference's trailing GaussianBlur((3,3), 0.5) +
    threshold 127 of the watermark type is the identity on a {0,255} image and is not restated."""
    out, summary = _select(_chain(np.asarray(mask_u8) > 127, mask_type), mask_type)
    return out.astype(np.uint8) * 255, summary


# ------------------------------------------------------------------ the golden case list
def synth(h, w, seed):
    """blobs + strokes + 1 % salt-and-pepper noise, some touching the border"""
    g = np.random.default_rng(seed)
    m = np.zeros((h, w), bool)
    yy, xx = np.mgrid[:h, :w]
    for _ in range(int(g.integers(1, 5))):
        cy, cx = g.integers(0, h), g.integers(0, w)
        ry, rx = g.integers(3, max(4, h // 5)), g.integers(3, max(4, w // 5))
        m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
    for _ in range(int(g.integers(0, 12))):
        y, x = g.integers(0, h), g.integers(0, w)
        if g.random() < .5:
            m[y:y + 2, x:x + int(g.integers(4, 30))] = True
        else:
            m[y:y + int(g.integers(4, 30)), x:x + 2] = True
    m ^= g.random((h, w)) < 0.01
    return m


def _squares(h, w, *sq):
    m = np.zeros((h, w), bool)
    for y, x, s in sq:
        m[y:y + s, x:x + s] = True
    return m


SEEDED_SIZES = ((64, 64), (37, 200), (333, 517), (480, 640), (768, 1024))


def cases():
    """-> list of (name, bool (N,H,W)).  The named cases are the ones DESIGN.md §8b lists with their pixel counts."""
    c = [("empty", np.zeros((1, 96, 160), bool)),
         ("full", np.ones((1, 96, 160), bool)),
         ("sq3", _squares(96, 160, (40, 40, 3))[None]),
         ("sq3x2", _squares(96, 160, (20, 20, 3), (60, 120, 3))[None]),
         ("sq2", _squares(96, 160, (40, 40, 2))[None]),
         ("tie", _squares(200, 300, (30, 30, 20), (120, 200, 20))[None]),
         ("tie_corner", _squares(200, 300, (0, 0, 20), (180, 280, 20))[None]),
         ("sq3_sq30", _squares(200, 300, (30, 30, 3), (100, 150, 30))[None]),
         ("one_pixel", np.ones((1, 1, 1), bool)),
         ("row130", np.ones((1, 1, 130), bool))]
    for i, (h, w) in enumerate(SEEDED_SIZES):
        c.append((f"seeded_{h}x{w}_n1", synth(h, w, 10 * i)[None]))
        c.append((f"seeded_{h}x{w}_n3", np.stack([synth(h, w, 10 * i + s) for s in (1, 2, 3)])))
    return c


# foreground pixel counts of the watermark / text / mixed outputs of the named cases
EXPECTED_COUNTS = {"empty": (0, 0, 0), "full": (15360, 15360, 15360), "sq3": (265, 0, 0), "sq3x2": (530, 0, 0),
                   "sq2": (0, 0, 0), "tie": (1200, 1048, 1230), "tie_corner": (760, 925, 1010),
                   "sq3_sq30": (2020, 1084, 1215), "one_pixel": (0, 0, 0), "row130": (0, 130, 130)}

GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maskpost.npz")


def build_golden():
    """-> dict of arrays: per case `<name>/shape`, `<name>/in` (packed bits), and per type `<name>/<type>` (packed bits of the
    expected output) and `<name>/<type>_summary` int64 (N,4)"""
    d = {}
    for name, batch in cases():
        d[f"{name}/shape"] = np.array(batch.shape, np.int64)
        d[f"{name}/in"] = np.packbits(batch)
        for t in MASK_TYPES:
            outs, sums = zip(*(optimize_mask(img.astype(np.uint8) * 255, t) for img in batch))
            d[f"{name}/{t}"] = np.packbits(np.stack(outs) > 127)
            d[f"{name}/{t}_summary"] = np.array(sums, np.int64)
    return d


def load_golden(path=GOLDEN_PATH):
    """-> list of (name, uint8 {0,255} (N,H,W) input, {type: (uint8 (N,H,W) expected, int64 (N,4) summary)})"""
    z = np.load(path)
    names = [k[:-len("/shape")] for k in z.files if k.endswith("/shape")]
    out = []
    for name in names:
        shape = tuple(int(v) for v in z[f"{name}/shape"])
        cnt = int(np.prod(shape))
        unpack = lambda a: (np.unpackbits(a, count=cnt).reshape(shape) * 255).astype(np.uint8)
        out.append((name, unpack(z[f"{name}/in"]),
                    {t: (unpack(z[f"{name}/{t}"]), z[f"{name}/{t}_summary"]) for t in MASK_TYPES}))
    return out


if __name__ == "__main__":
    np.savez_compressed(GOLDEN_PATH, **build_golden())
    print(GOLDEN_PATH, os.path.getsize(GOLDEN_PATH), "bytes")
