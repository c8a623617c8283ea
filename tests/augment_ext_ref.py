"""numpy restatement of the rule that csrc/augment_ext_u8.hip implements behind the basic stages (include/uwm.h):
tone (CLAHE on the plane or on a lightness plane, or a gamma table) -> noise (integer Gaussian from a counter hash) -> 3x3 blur
(motion or Gaussian, reflect-101) -> Normalize's input.  CLAHE restates OpenCV 4.x's algorithm from knowledge of the source, NOT run
against cv2; the lightness chain, the noise generator and the motion rasterisation are the project's own integer rules.  Everything
is integer work or float32 with every operation rounded on its own.  The tables are built here from the stated formulae with exact
integer comparisons (Python integers), independently of the library's.  A helper of tests/test_augment_ext*.py, not itself a test."""
import numpy as np

import augment_ref as A

EXT_DTYPE = np.dtype({"names": ["tone", "clahe_clip", "noise_sigma", "blur", "blur_w", "seed", "lut2"],
                      "formats": ["<i4", "<i4", "<i4", "<i4", ("u1", (9,)), "<u8", ("u1", (256,))],
                      "offsets": [0, 4, 8, 12, 16, 32, 40], "itemsize": 296})
TONE_NONE, TONE_CLAHE, TONE_TABLE = 0, 1, 2
BLUR_NONE, BLUR_MOTION, BLUR_GAUSS = 0, 1, 2
GAUSS_W = np.array([1, 2, 1, 2, 4, 2, 1, 2, 1], dtype=np.int64)
SIGMA_MAX = 16383                      # noise_sigma is sigma * 256; the kernel clamps to this (sigma < 64 grey levels)


# ------------------------------------------------------------------------------------------------ gamma
def gamma_lut(gamma):
    """RandomGamma's table for uint8: trunc(((i / 255) ** gamma) * 255) in float64"""
    return ((np.arange(256, dtype=np.float64) / 255.0) ** np.float64(gamma) * 255.0).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ blur
def _div_rne(a, b):
    q = a // b
    r2 = 2 * (a - q * b)
    return q + ((r2 > b) | ((r2 == b) & ((q & 1) == 1)))


def _taps(img):
    """the nine reflect-101 neighbours of every pixel, [3][3] of int64 (H, W, C): tap (i, j) = pixel (y + i - 1, x + j - 1)"""
    H, W = img.shape[:2]
    I = img.astype(np.int64)
    ys = [A.reflect101(np.arange(H) + d, H) for d in (-1, 0, 1)]
    xs = [A.reflect101(np.arange(W) + d, W) for d in (-1, 0, 1)]
    return [[I[ys[i]][:, xs[j]] for j in range(3)] for i in range(3)]


def gaussian_blur3(img):
    t = _taps(img)
    acc = sum(int(GAUSS_W[3 * i + j]) * t[i][j] for i in range(3) for j in range(3))
    return ((acc + 8) >> 4).astype(np.uint8)


def motion_blur3(img, w9):
    w = [1 if int(v) else 0 for v in w9]
    s = sum(w)
    if s == 0:
        return img
    t = _taps(img)
    acc = sum(w[3 * i + j] * t[i][j] for i in range(3) for j in range(3))
    return _div_rne(acc, s).astype(np.uint8)


def motion_kernel(p0, p1):
    """the 0/1 taps of the line between two distinct points (x, y) of the 3 x 3 grid: both end points, and between end points two
    apart the middle point, a half rounded up"""
    (x0, y0), (x1, y1) = p0, p1
    assert (x0, y0) != (x1, y1) and all(0 <= v <= 2 for v in (x0, y0, x1, y1))
    k = np.zeros(9, dtype=np.uint8)
    k[3 * y0 + x0] = k[3 * y1 + x1] = 1
    if max(abs(x1 - x0), abs(y1 - y0)) == 2:
        k[3 * ((y0 + y1 + 1) // 2) + (x0 + x1 + 1) // 2] = 1
    return k


# ------------------------------------------------------------------------------------------------ CLAHE (8 x 8 tiles)
def _tile_geometry(H, W):
    Hp, Wp = -(-H // 8) * 8, -(-W // 8) * 8
    return Hp, Wp, Hp // 8, Wp // 8


def clahe_luts(plane, clip):
    """uint8 (H, W), H, W >= 8 -> the 64 tables, uint8 (8, 8, 256)"""
    H, W = plane.shape
    Hp, Wp, th, tw = _tile_geometry(H, W)
    pad = plane[A.reflect101(np.arange(Hp), H)][:, A.reflect101(np.arange(Wp), W)]
    scale = np.float32(255.0) / np.float32(th * tw)
    clip = max(int(clip), 1)
    luts = np.zeros((8, 8, 256), dtype=np.uint8)
    for ty in range(8):
        for tx in range(8):
            hist = np.bincount(pad[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].ravel(), minlength=256).astype(np.int64)
            excess = int(np.maximum(hist - clip, 0).sum())
            hist = np.minimum(hist, clip)
            batch = excess // 256
            resid = excess - 256 * batch
            hist += batch
            if resid:
                step = max(256 // resid, 1)
                hist[np.arange(0, 256, step)[:resid]] += 1
            v = np.cumsum(hist).astype(np.float32) * scale
            luts[ty, tx] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return luts


def clahe_apply(plane, luts):
    H, W = plane.shape
    _, _, th, tw = _tile_geometry(H, W)
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


def clahe_plane(plane, clip):
    return clahe_apply(plane, clahe_luts(plane, clip))


# ------------------------------------------------------------------------------------------------ lightness: the project's own rule
# sRGB -> linear (LIN, 14 fraction bits) -> D65 XYZ over the white point (Q12 rows that sum to 4096, so a grey stays X = Y = Z) ->
# f() (F, 15 fraction bits) -> L8; the way back keeps f(X) - f(Y) and f(Y) - f(Z), replaces f(Y), inverts f (FINV, indexed by f in
# 13 fraction bits up to 2.0) and the matrix, and goes linear -> sRGB through GAM.
FWD = np.array([[1777, 1541, 778], [871, 2929, 296], [73, 448, 3575]], dtype=np.int64)
INV = np.array([[12615, -6296, -2223], [-3773, 7684, 185], [217, -836, 4715]], dtype=np.int64)


def _round_ratio(num, den):
    """round(num / den), halves up, Python integers, den > 0"""
    return (2 * num + den) // (2 * den)


def _build_tables():
    lin = []
    for v in range(256):
        if v <= 10:                                               # v / 255 <= 0.04045
            lin.append(_round_ratio(16384 * v * 100, 255 * 1292))
            continue
        n, d = 1000 * v + 14025, 269025                            # ((v / 255 + 0.055) / 1.055) ** 2.4 = (n / d) ** (12 / 5)
        q = int(round(16384.0 * (n / d) ** 2.4))
        rhs = 32 * 16384 ** 5 * n ** 12
        while (2 * q - 1) ** 5 * d ** 12 > rhs:
            q -= 1
        while (2 * q + 1) ** 5 * d ** 12 <= rhs:
            q += 1
        lin.append(q)
    f = []
    for i in range(16385):
        if i * 1000000 <= 8856 * 16384:                           # t <= 0.008856: 7.787 t + 16 / 116
            f.append(_round_ratio(7787 * 2 * i * 29 + 131072 * 1000, 29000))
            continue
        q = int(round(32768.0 * (i / 16384.0) ** (1.0 / 3.0)))
        while (2 * q - 1) ** 3 > i << 34:
            q -= 1
        while (2 * q + 1) ** 3 <= i << 34:
            q += 1
        f.append(q)
    finv = []
    for j in range(16385):                                         # f = j / 8192
        if j * 1000000 > 206893 * 8192:
            finv.append((j ** 3 + (1 << 24)) >> 25)
        else:
            finv.append(max(0, _round_ratio((29 * j - 32768) * 2000, 29 * 7787)))
    gam = []
    for i in range(16385):
        if i * 10000000 <= 31308 * 16384:                         # t <= 0.0031308: 12.92 t
            gam.append(_round_ratio(255 * 1292 * i, 100 * 16384))
            continue
        q = int(round(269.025 * (i / 16384.0) ** (1.0 / 2.4) - 14.025))
        lhs = i ** 5 * 269025 ** 12
        while (1000 * q + 13525) ** 12 * 16384 ** 5 > lhs:
            q -= 1
        while (1000 * q + 14525) ** 12 * 16384 ** 5 <= lhs:
            q += 1
        gam.append(min(max(q, 0), 255))
    return (np.array(lin, dtype=np.int64), np.array(f, dtype=np.int64), np.array(finv, dtype=np.int64), np.array(gam, dtype=np.int64))


_TABLES = None


def lab_tables():
    """(LIN[256], F[16385], FINV[16385], GAM[16385]) as int64 arrays"""
    global _TABLES
    if _TABLES is None:
        _TABLES = _build_tables()
    return _TABLES


def _xyz_f(rgb):
    LIN, F, _, _ = lab_tables()
    lin = LIN[rgb.astype(np.int64)]
    xyz = (lin @ FWD.T + 2048) >> 12
    return F[xyz]


def rgb_to_l8(rgb):
    """uint8 (..., 3) -> L8 = round(L * 255 / 100) as int64"""
    fy = _xyz_f(rgb)[..., 1]
    return np.clip((2 * (116 * fy - 524288) * 255 + 3276800) // (2 * 3276800), 0, 255)


def l8_replace(rgb, l8):
    """the colour of rgb with its lightness replaced by l8 (int, 0..255) -> uint8 (..., 3)"""
    _, _, FINV, GAM = lab_tables()
    f = _xyz_f(rgb)
    fy2 = (2 * 32768 * (100 * np.asarray(l8, dtype=np.int64) + 4080) + 29580) // (2 * 29580)
    f2 = np.stack([fy2 + (f[..., 0] - f[..., 1]), fy2, fy2 - (f[..., 1] - f[..., 2])], axis=-1)
    t = FINV[(np.clip(f2, 0, 65535) + 2) >> 2]
    lin = np.clip((t @ INV.T + 2048) >> 12, 0, 16384)
    return GAM[lin].astype(np.uint8)


def clahe_image(img, clip):
    """uint8 (H, W, C): C = 1 on the plane, C = 3 on the lightness plane; anything else, or H or W < 8, is left as it is"""
    H, W, C = img.shape
    if C not in (1, 3) or H < 8 or W < 8:
        return img
    if C == 1:
        return clahe_plane(img[..., 0], clip)[..., None]
    return l8_replace(img, clahe_plane(rgb_to_l8(img).astype(np.uint8), clip).astype(np.int64))


# ------------------------------------------------------------------------------------------------ noise
_U64 = np.uint64


def hash64(seed, counter):
    """the splitmix64 finaliser of seed + (counter + 1) * 0x9E3779B97F4A7C15, uint64 arithmetic"""
    with np.errstate(over="ignore"):
        z = _U64(int(seed) & 0xFFFFFFFFFFFFFFFF) + (np.asarray(counter, dtype=np.uint64) + _U64(1)) * _U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
        return z ^ (z >> _U64(31))


_QN = None


def normal_table():
    """QN[0..1024] = round(4096 * Phi^-1(i / 1024)), the two ends at Phi^-1(1 / 4096) = -+3.4871: where the tails stop"""
    global _QN
    if _QN is None:
        from scipy.special import ndtri
        p = np.arange(1025, dtype=np.float64) / 1024.0
        p[0], p[1024] = 1.0 / 4096.0, 1.0 - 1.0 / 4096.0
        q = np.rint(ndtri(p) * 4096.0).astype(np.int64)
        q[512] = 0
        q[513:] = -q[:512][::-1]
        _QN = q
    return _QN


def normal_q14(seed, counter):
    """a standard-normal draw with 14 fraction bits: bits 40..63 of the hash pick a cell of the quantile table (10 bits) and a
    position in it (14 bits)"""
    QN = normal_table()
    r = (hash64(seed, counter) >> _U64(40)).astype(np.int64)
    k, fr = r >> 14, r & 16383
    return (QN[k] * (16384 - fr) + QN[k + 1] * fr) >> 12


def noise_offsets(seed, sigma_q8, H, W, C):
    """int64 (H, W, C): floor(g) of the noise of every byte; counter = (y * W + x) * 4 + c"""
    s = min(max(int(sigma_q8), 0), SIGMA_MAX)
    pix = np.arange(H * W, dtype=np.uint64).reshape(H, W, 1) * _U64(4) + np.arange(C, dtype=np.uint64)
    return (normal_q14(seed, pix) * s) >> 22


def add_noise(img, seed, sigma_q8):
    if min(max(int(sigma_q8), 0), SIGMA_MAX) == 0:
        return img
    H, W, C = img.shape
    return np.clip(img.astype(np.int64) + noise_offsets(seed, sigma_q8, H, W, C), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the three stages of one descriptor
def ext_stages(img, e):
    """the staged uint8 image (H, W, C) of the basic stages, one EXT_DTYPE record -> tone -> noise -> blur"""
    tone, blur = int(e["tone"]), int(e["blur"])
    a = img
    if tone == TONE_CLAHE:
        a = clahe_image(a, max(int(e["clahe_clip"]), 1))
    elif tone == TONE_TABLE:
        a = np.asarray(e["lut2"], dtype=np.uint8)[a]
    a = add_noise(a, int(e["seed"]), int(e["noise_sigma"]))
    if blur == BLUR_MOTION:
        a = motion_blur3(a, e["blur_w"])
    elif blur == BLUR_GAUSS:
        a = gaussian_blur3(a)
    return a


def augment_ext_desc(img, mask, d, e):
    """basic descriptor d (augment_ref.augment_desc), then the ext descriptor e (None = none) -> (image, mask or None)"""
    out, m = A.augment_desc(img, mask, d)
    return (out if e is None else ext_stages(out, e)), m


# ------------------------------------------------------------------------------------------------ float64 model of the lightness step
def float_l8_shift(rgb, shift):
    """CIE Lab in float64 (OpenCV's D65 matrix and constants): L quantised to L8 = round(L * 255 / 100), shifted and clipped, a and b
    kept, back to sRGB, clipped -> float64 (..., 3) in grey levels (not rounded)"""
    M = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
    c = rgb.astype(np.float64) / 255.0
    lin = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    xyz = lin @ (M / M.sum(1, keepdims=True)).T
    f = np.where(xyz > 0.008856, np.cbrt(xyz), 7.787 * xyz + 16.0 / 116.0)
    l8 = np.clip(np.rint((116.0 * f[..., 1] - 16.0) * 2.55) + shift, 0, 255)
    fy = (l8 / 2.55 + 16.0) / 116.0
    f2 = np.stack([fy + (f[..., 0] - f[..., 1]), fy, fy - (f[..., 1] - f[..., 2])], -1)
    t = np.where(f2 > 0.206893, f2 ** 3, np.maximum((f2 - 16.0 / 116.0) / 7.787, 0.0))
    lin2 = np.clip(t @ np.linalg.inv(M / M.sum(1, keepdims=True)).T, 0.0, 1.0)
    return 255.0 * np.where(lin2 <= 0.0031308, 12.92 * lin2, 1.055 * lin2 ** (1 / 2.4) - 0.055)
