"""numpy restatement of the augmentation rule that csrc/augment_u8.hip implements (include/uwm.h): flips -> rot90 ->
affine warp (OpenCV 4.x's 8-bit warpAffine fixed point: 10 coordinate bits, 5 interpolation bits, BORDER_REFLECT_101; written from
knowledge of the source and NOT run against cv2) -> per-value table -> HueSaturationValue (OpenCV's integer RGB -> HSV, the project's
own integer way back) -> Normalize's input.  Integer-only except the float64 coordinate setup.  A helper of tests/test_augment.py and
tests/test_augment_gpu.py, not itself a test."""
import numpy as np

IDENTITY_MINV = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
IDENTITY_LUT = np.arange(256, dtype=np.uint8)


def _rne(v):
    return np.rint(v).astype(np.int64)                       # round half to even


def fixed_coords(minv, H, W, r):
    """(X, Y) int64 [H][W]: 10-bit fixed-point source coordinates + rounding offset r; every product and sum rounded on its own"""
    m = [np.float64(v) for v in minv]
    x = np.arange(W, dtype=np.float64); y = np.arange(H, dtype=np.float64)
    adelta = _rne(m[0] * x * 1024.0); bdelta = _rne(m[3] * x * 1024.0)
    X0 = _rne((m[1] * y + m[2]) * 1024.0) + r; Y0 = _rne((m[4] * y + m[5]) * 1024.0) + r
    return X0[:, None] + adelta[None, :], Y0[:, None] + bdelta[None, :]


def reflect101(c, n):
    """BORDER_REFLECT_101 of any integer coordinate: period 2(n-1); n = 1 -> 0"""
    c = np.asarray(c, dtype=np.int64)
    if n == 1:
        return np.zeros_like(c)
    p = 2 * (n - 1)
    m = np.mod(c, p)                                          # non-negative
    return np.where(m < n, m, p - m)


def flip_rot(a, flags):
    """HorizontalFlip, VerticalFlip, then RandomRotate90(k) (counter-clockwise): uwm_preprocess_u8's flags"""
    if flags & 1:
        a = a[:, ::-1]
    if flags & 2:
        a = a[::-1]
    return np.rot90(a, (flags >> 2) & 3)


def warp_linear(img, minv):
    """uint8 (H, W, C) -> the same shape"""
    H, W = img.shape[:2]
    X, Y = fixed_coords(minv, H, W, 16)
    X >>= 5; Y >>= 5
    sx, fx, sy, fy = X >> 5, X & 31, Y >> 5, Y & 31
    x0, x1, y0, y1 = reflect101(sx, W), reflect101(sx + 1, W), reflect101(sy, H), reflect101(sy + 1, H)
    I = img.astype(np.int64)
    fx = fx[..., None]; fy = fy[..., None]
    acc = (32 - fx) * (32 - fy) * I[y0, x0] + fx * (32 - fy) * I[y0, x1] + (32 - fx) * fy * I[y1, x0] + fx * fy * I[y1, x1]
    return ((acc + 512) >> 10).astype(np.uint8)


def warp_nearest(m, minv):
    """uint8 (H, W) -> the same shape"""
    H, W = m.shape
    X, Y = fixed_coords(minv, H, W, 512)
    return m[reflect101(Y >> 10, H), reflect101(X >> 10, W)]


def _div_table(num, den_mul):
    i = np.arange(1, 256, dtype=np.float64)
    return np.concatenate([[0], _rne(num / (den_mul * i))])


SDIV = _div_table(255 << 12, 1.0)
HDIV = _div_table(180 << 12, 6.0)


def rgb_to_hsv(rgb):
    """uint8 (..., 3) -> int64 h (0..179), s, v: OpenCV's 8-bit rule"""
    I = rgb.astype(np.int64)
    r, g, b = I[..., 0], I[..., 1], I[..., 2]
    v = np.maximum(r, np.maximum(g, b)); d = v - np.minimum(r, np.minimum(g, b))
    s = (d * SDIV[v] + 2048) >> 12
    h0 = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))
    h = (h0 * HDIV[d] + 2048) >> 12
    return np.where(h < 0, h + 180, h), s, v


def hsv_to_rgb(h, s, v):
    """the project's own integer rule"""
    sec, f = h // 30, h % 30
    p = (v * (255 - s) + 127) // 255
    q = (v * (7650 - s * f) + 3825) // 7650
    t = (v * (7650 - s * (30 - f)) + 3825) // 7650
    r = np.choose(sec, [v, q, p, p, t, v]); g = np.choose(sec, [t, v, v, q, p, p]); b = np.choose(sec, [p, p, t, v, v, q])
    return np.stack([r, g, b], axis=-1).astype(np.uint8)


def hsv_shift(rgb, hue, sat, val):
    if hue == 0 and sat == 0 and val == 0:
        return rgb
    h, s, v = rgb_to_hsv(rgb)
    return hsv_to_rgb(np.mod(h + int(hue), 180), np.clip(s + int(sat), 0, 255), np.clip(v + int(val), 0, 255))


def augment_image(img, flags=0, minv=IDENTITY_MINV, lut=IDENTITY_LUT, hsv=(0, 0, 0)):
    """uint8 (H, W, C) -> the augmented uint8 image (what Normalize then takes)"""
    a = warp_linear(np.ascontiguousarray(flip_rot(img, flags)), minv)
    a = np.asarray(lut, dtype=np.uint8)[a]
    return hsv_shift(a, *hsv) if a.shape[2] == 3 else a


def augment_mask(m, flags=0, minv=IDENTITY_MINV, threshold=127):
    """uint8 (H, W) -> uint8 {0,1}"""
    return (warp_nearest(np.ascontiguousarray(flip_rot(m, flags)), minv) > threshold).astype(np.uint8)


def augment_desc(img, mask, d):
    """one record of data.AUG_DESC_DTYPE -> (image, mask or None)"""
    hsv = (int(d["hue"]), int(d["sat"]), int(d["val"]))
    out = augment_image(img, int(d["flags"]), tuple(d["minv"]), d["lut"], hsv)
    return out, (None if mask is None else augment_mask(mask, int(d["flags"]), tuple(d["minv"])))


# ------------------------------------------------------------------------------------------------ float models (sanity of the rule)
def float_warp(img, minv):
    """float64 bilinear warp with reflect-101: what the fixed-point rule approximates"""
    H, W = img.shape[:2]
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    sx = minv[0] * x + minv[1] * y + minv[2]; sy = minv[3] * x + minv[4] * y + minv[5]
    x0 = np.floor(sx).astype(np.int64); y0 = np.floor(sy).astype(np.int64)
    wx = (sx - x0)[..., None]; wy = (sy - y0)[..., None]
    I = img.astype(np.float64)
    xa, xb, ya, yb = reflect101(x0, W), reflect101(x0 + 1, W), reflect101(y0, H), reflect101(y0 + 1, H)
    return (I[ya, xa] * (1 - wx) + I[ya, xb] * wx) * (1 - wy) + (I[yb, xa] * (1 - wx) + I[yb, xb] * wx) * wy


def brute_reflect(c, n):
    """reflect-101 by walking, one reflection at a time"""
    if n == 1:
        return 0
    while c < 0 or c >= n:
        c = -c if c < 0 else 2 * (n - 1) - c
    return c
