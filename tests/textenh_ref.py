"""Restatement of the reference's _enhance_text_features (src/predict.py:370-404) in numpy, in the LITERAL form: what
uwm_text_enhance_ragged (csrc/text_enhance.hip) is held to byte for byte.

    gray = cvtColor(RGB2GRAY) -> createCLAHE(2.0, (8, 8)).apply -> Canny(50, 150) -> dilate(MORPH_ELLIPSE (2, 2)) ->
    channel[edge] = clip(channel[edge] * 1.2, 0, 255) per channel in float32 -> filter2D with the 3 x 3 sharpening kernel

OpenCV is not available to this project, so every cv2 rule is restated here from its documented behaviour and its source, not run:
CLAHE pads with copyMakeBorder only when a side is no multiple of the tile count (then both sides grow); Canny is written as cv2's
loop writes it (row scan with prev_flag, an explicit stack, the 0 / 1 / 2 map); the even-sided ellipse has its anchor at (1, 1);
filter2D's default border is BORDER_REFLECT_101.  The kernels compute the hysteresis as a component property instead;
tests/test_textenh.py holds the two forms together."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maskpost_ref as M  # noqa: E402
import pairmask_ref as PM  # noqa: E402

MIN_SIDE = 16
LOW, HIGH = 50, 150
TG22 = 13573
SHARPEN = np.array([[-1, -1, -1], [-1, 9, -1], [-1, -1, -1]], dtype=np.int64)
DONE, MISFIT, COPIED = 0, 1, 2


def gray(img):
    """cv2.cvtColor(RGB2GRAY) on uint8 (h, w, 3): pairmask_ref.diff_gray's rule against a zero image"""
    return PM.diff_gray(img, np.zeros_like(img)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ CLAHE(2.0, (8, 8))
def border_reflect101(plane, bottom, right):
    """copyMakeBorder(plane, 0, bottom, 0, right, BORDER_REFLECT_101) as an explicit copy, row by row and column by column"""
    H, W = plane.shape
    out = np.zeros((H + bottom, W + right), dtype=plane.dtype)
    out[:H, :W] = plane
    for k in range(right):
        out[:H, W + k] = plane[:, W - 2 - k]
    for k in range(bottom):
        out[H + k, :] = out[H - 2 - k, :]
    return out


def clahe_geometry(H, W):
    """-> (rows added, columns added, tile height, tile width): cv2 pads only when a side is no multiple of 8, and then BOTH"""
    if H % 8 == 0 and W % 8 == 0:
        return 0, 0, H // 8, W // 8
    bottom, right = 8 - H % 8, 8 - W % 8
    return bottom, right, (H + bottom) // 8, (W + right) // 8


def clahe_clip(th, tw):
    return max(int(2.0 * th * tw / 256), 1)


def clahe_luts(plane):
    """uint8 (H, W) -> the 64 tables, uint8 (8, 8, 256)"""
    H, W = plane.shape
    bottom, right, th, tw = clahe_geometry(H, W)
    pad = border_reflect101(plane, bottom, right) if bottom or right else plane
    clip = clahe_clip(th, tw)
    scale = np.float32(255.0) / np.float32(th * tw)
    luts = np.zeros((8, 8, 256), dtype=np.uint8)
    for ty in range(8):
        for tx in range(8):
            hist = np.bincount(pad[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].ravel(), minlength=256).astype(np.int64)
            clipped = 0
            for i in range(256):
                if hist[i] > clip:
                    clipped += int(hist[i]) - clip
                    hist[i] = clip
            batch = clipped // 256
            residual = clipped - batch * 256
            hist += batch
            if residual:
                step = max(256 // residual, 1)
                i = 0
                while i < 256 and residual > 0:
                    hist[i] += 1
                    i += step
                    residual -= 1
            v = np.cumsum(hist).astype(np.float32) * scale
            luts[ty, tx] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return luts


def clahe_apply(plane, luts, th, tw):
    H, W = plane.shape
    one, half = np.float32(1.0), np.float32(0.5)

    def axis(n, t):
        f = np.arange(n, dtype=np.float32) * (one / np.float32(t)) - half
        t1 = np.floor(f)
        a = f - t1
        t1 = t1.astype(np.int64)
        return np.clip(t1, 0, 7), np.clip(t1 + 1, 0, 7), a, one - a

    y1, y2, ya, ya1 = axis(H, th)
    x1, x2, xa, xa1 = axis(W, tw)
    v = plane.astype(np.int64)
    tap = lambda ty, tx: luts[ty[:, None], tx[None, :], v].astype(np.float32)      # noqa: E731
    xa, xa1, ya, ya1 = xa[None, :], xa1[None, :], ya[:, None], ya1[:, None]
    res = (tap(y1, x1) * xa1 + tap(y1, x2) * xa) * ya1 + (tap(y2, x1) * xa1 + tap(y2, x2) * xa) * ya
    assert res.dtype == np.float32
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)


def clahe(plane):
    _, _, th, tw = clahe_geometry(*plane.shape)
    return clahe_apply(plane, clahe_luts(plane), th, tw)


# ------------------------------------------------------------------------------------------------ Canny(50, 150), aperture 3, L1
def sobel(plane):
    """-> (dx, dy), int64: the 3 x 3 Sobel derivatives as correlations over a BORDER_REPLICATE copy"""
    H, W = plane.shape
    p = np.zeros((H + 2, W + 2), dtype=np.int64)
    p[1:-1, 1:-1] = plane
    p[0, 1:-1], p[-1, 1:-1] = plane[0], plane[-1]
    p[:, 0], p[:, -1] = p[:, 1], p[:, -2]
    kx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], dtype=np.int64)
    dx = np.zeros((H, W), dtype=np.int64)
    dy = np.zeros((H, W), dtype=np.int64)
    for i in range(3):
        for j in range(3):
            win = p[i:i + H, j:j + W]
            dx += kx[i, j] * win
            dy += kx[j, i] * win
    return dx, dy


def _survives(mag, dx, dy, i, j):
    """cv2's non-maximum suppression at (i, j); mag carries a zero frame of one pixel"""
    m = mag[i + 1, j + 1]
    xs, ys = int(dx[i, j]), int(dy[i, j])
    x, y = abs(xs), abs(ys) << 15
    tg22x = x * TG22
    if y < tg22x:
        return m > mag[i + 1, j] and m >= mag[i + 1, j + 2]
    tg67x = tg22x + (x << 16)
    if y > tg67x:
        return m > mag[i, j + 1] and m >= mag[i + 2, j + 1]
    s = -1 if (xs ^ ys) < 0 else 1
    return m > mag[i, j + 1 - s] and m > mag[i + 2, j + 1 + s]


def canny(plane, low=LOW, high=HIGH):
    """cv2.Canny(plane, low, high) as its loop writes it -> uint8 {0, 255}.  map: 1 = no edge, 0 = may be one, 2 = edge."""
    H, W = plane.shape
    dx, dy = sobel(plane)
    mag = np.zeros((H + 2, W + 2), dtype=np.int64)
    mag[1:-1, 1:-1] = np.abs(dx) + np.abs(dy)
    mp = np.ones((H + 2, W + 2), dtype=np.uint8)
    stack = []
    for i in range(H):
        prev_flag = False
        for j in range(W):
            m = mag[i + 1, j + 1]
            if m > low and _survives(mag, dx, dy, i, j):
                if not prev_flag and m > high and mp[i, j + 1] != 2:
                    mp[i + 1, j + 1] = 2
                    stack.append((i + 1, j + 1))
                    prev_flag = True
                else:
                    mp[i + 1, j + 1] = 0
                continue
            prev_flag = False
            mp[i + 1, j + 1] = 1
    while stack:
        y, x = stack.pop()
        for ny, nx in ((y - 1, x - 1), (y - 1, x), (y - 1, x + 1), (y, x - 1), (y, x + 1), (y + 1, x - 1), (y + 1, x), (y + 1, x + 1)):
            if mp[ny, nx] == 0:
                mp[ny, nx] = 2
                stack.append((ny, nx))
    return ((mp[1:-1, 1:-1] >> 1) * 255).astype(np.uint8)


def candidates(plane, low=LOW, high=HIGH):
    """-> (candidate, strong) bool planes: what survives the suppression above `low`, and those of them above `high`"""
    H, W = plane.shape
    dx, dy = sobel(plane)
    mag = np.zeros((H + 2, W + 2), dtype=np.int64)
    mag[1:-1, 1:-1] = np.abs(dx) + np.abs(dy)
    cand = np.zeros((H, W), dtype=bool)
    for i in range(H):
        for j in range(W):
            cand[i, j] = mag[i + 1, j + 1] > low and _survives(mag, dx, dy, i, j)
    return cand, cand & (mag[1:-1, 1:-1] > high)


# ------------------------------------------------------------------------------------------------ dilate, boost, sharpen
def dilate2(edges):
    """cv2.dilate(edges, getStructuringElement(MORPH_ELLIPSE, (2, 2))): [[0,1],[1,1]], anchor (1, 1), written out"""
    H, W = edges.shape
    out = edges.copy()
    out[1:, :] = np.maximum(out[1:, :], edges[:-1, :])
    out[:, 1:] = np.maximum(out[:, 1:], edges[:, :-1])
    return out


def boost(img, edges_dilated):
    """the reference's per-channel float code"""
    enhanced = img.copy()
    for i in range(3):
        channel = enhanced[:, :, i].astype(np.float32)
        edge_mask = edges_dilated > 0
        channel[edge_mask] = np.clip(channel[edge_mask] * 1.2, 0, 255)
        assert channel.dtype == np.float32
        enhanced[:, :, i] = channel.astype(np.uint8)
    return enhanced


def sharpen(img):
    """cv2.filter2D(img, -1, SHARPEN): a correlation per channel over a BORDER_REFLECT_101 copy, saturated"""
    H, W = img.shape[:2]
    p = np.pad(img.astype(np.int64), ((1, 1), (1, 1), (0, 0)), mode="reflect")
    acc = np.zeros(img.shape, dtype=np.int64)
    for i in range(3):
        for j in range(3):
            acc += SHARPEN[i, j] * p[i:i + H, j:j + W]
    return np.clip(acc, 0, 255).astype(np.uint8)


def text_enhance(img):
    """uint8 (h, w, 3) -> (enhanced uint8 (h, w, 3), dilated edges uint8 (h, w) in {0, 255}, status)"""
    img = np.ascontiguousarray(img)
    if min(img.shape[:2]) < MIN_SIDE:
        return img.copy(), np.zeros(img.shape[:2], dtype=np.uint8), COPIED
    edges = dilate2(canny(clahe(gray(img))))
    return sharpen(boost(img, edges)), edges, DONE


assert np.array_equal(M.ellipse(2, 2), [[0, 1], [1, 1]])


# ------------------------------------------------------------------------------------------------ the cases of the GPU test
def _blocks(rng, h, w, step=5):
    """random flat blocks with a little noise: step edges of every strength and direction"""
    coarse = rng.integers(0, 256, (-(-h // step), -(-w // step), 3))
    img = np.repeat(np.repeat(coarse, step, axis=0), step, axis=1)[:h, :w]
    return np.clip(img + rng.integers(-6, 7, (h, w, 3)), 0, 255).astype(np.uint8)


def spiral(strong, h=96, w=200, base=90, step=22, extra=18):
    """A rectangular spiral band, 4 pixels wide, `step` grey levels above a flat ground: its outline is ONE closed one-pixel-wide
    ridge of weak candidates (50 < magnitude <= 150) that winds through all 64 CLAHE tiles.  strong: one pixel at the band's inner end
    is raised by `extra`, which lifts exactly one candidate above the high threshold (tests/test_textenh.py checks both claims)."""
    g = np.full((h, w), base, dtype=np.int64)
    x0, y0, x1, y1 = 4, 4, w - 5, h - 5
    pts = []
    while x1 - x0 > 16 and y1 - y0 > 8:
        pts += [(y0, x0), (y0, x1), (y1, x1), (y1, x0 + 12)]
        x0, y0, x1, y1 = x0 + 12, y0 + 12, x1 - 12, y1 - 12
    pts.append((y0, x0))
    for (ya, xa), (yb, xb) in zip(pts[:-1], pts[1:]):
        g[min(ya, yb):max(ya, yb) + 4, min(xa, xb):max(xa, xb) + 4] = base + step
    if strong:
        ye, xe = pts[-1]
        g[ye + 1, xe + 1] += extra
    return np.repeat(g[:, :, None], 3, axis=2).astype(np.uint8), pts[-1]


def images():
    """the ragged batch of tests/test_textenh_gpu.py: [(name, uint8 (h, w, 3))]"""
    rng = np.random.default_rng(20240607)
    cross = np.full((40, 48, 3), 60, dtype=np.uint8)
    cross[:, 20:27] = 200
    cross[17:24, :] = (30, 220, 140)
    return [("least 16x16", _blocks(rng, 16, 16)),
            ("17x23", _blocks(rng, 17, 23)),
            ("16x20", _blocks(rng, 16, 20)),
            ("40x64", _blocks(rng, 40, 64)),
            ("33x130", _blocks(rng, 33, 130)),
            ("constant", np.full((24, 40, 3), (70, 130, 200), dtype=np.uint8)),
            ("borders", cross),
            ("spiral strong", spiral(True)[0]),
            ("spiral weak", spiral(False)[0]),
            ("small 12x40", _blocks(rng, 12, 40))]
