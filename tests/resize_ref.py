"""numpy restatement of the resize rule that csrc/resize_u8.hip implements (include/uwm.h): OpenCV 4.x's plain C++
path for 8-bit INTER_LINEAR (HResizeLinear / VResizeLinear, fixed point with 11 coefficient bits) and resizeNN, written from the
source and NOT run against cv2.  A helper of tests/test_resize.py and tests/test_resize_gpu.py, not itself a test."""
import numpy as np


def taps(dst, src):
    """one axis, INTER_LINEAR: (s, s1, a0, a1)"""
    scale = 1.0 / (float(dst) / float(src))              # doubles, in this order
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64); f = f - s.astype(np.float32)
    lo = s < 0;        f[lo] = 0; s[lo] = 0
    hi = s >= src - 1; f[hi] = 0; s[hi] = src - 1
    a1 = np.rint(f * np.float32(2048)).astype(np.int64)                     # round half to even
    a0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    return s, np.minimum(s + 1, src - 1), a0, a1


def resize_u8_linear(img, H, W):
    if img.shape[:2] == (H, W):
        return img.copy()
    sx, sx1, a0, a1 = taps(W, img.shape[1]); sy, sy1, b0, b1 = taps(H, img.shape[0])
    I = img.astype(np.int64)
    hor = I[:, sx] * a0[None, :, None] + I[:, sx1] * a1[None, :, None]
    S0, S1 = hor[sy], hor[sy1]
    return ((((b0[:, None, None] * (S0 >> 4)) >> 16) + ((b1[:, None, None] * (S1 >> 4)) >> 16) + 2) >> 2).astype(np.uint8)


def nearest_index(dst, src):
    return np.minimum(np.floor(np.arange(dst) * (1.0 / (float(dst) / src))).astype(np.int64), src - 1)


def resize_u8_nearest(img, H, W):
    iy = nearest_index(H, img.shape[0])
    ix = nearest_index(W, img.shape[1])
    return img[iy][:, ix]


def float_bilinear(img, H, W):
    """float64 bilinear with align_corners = False (edge-clamped): what the fixed-point rule approximates"""
    h, w = img.shape[:2]
    fy = np.maximum((np.arange(H) + 0.5) * (h / H) - 0.5, 0.0); fx = np.maximum((np.arange(W) + 0.5) * (w / W) - 0.5, 0.0)
    y0 = np.minimum(np.floor(fy).astype(np.int64), h - 1); x0 = np.minimum(np.floor(fx).astype(np.int64), w - 1)
    y1 = np.minimum(y0 + 1, h - 1); x1 = np.minimum(x0 + 1, w - 1)
    wy = (fy - y0)[:, None, None]; wx = (fx - x0)[None, :, None]
    I = img.astype(np.float64)
    top = I[y0][:, x0] * (1 - wx) + I[y0][:, x1] * wx
    bot = I[y1][:, x0] * (1 - wx) + I[y1][:, x1] * wx
    return top * (1 - wy) + bot * wy


# the ragged batch of the tests: upscale, downscale, identity (at 64 x 64), exact 2x (at 64 x 64), one-pixel sides and the widths
# 186 / 68, where the order of operations of the nearest scale shows
SHAPES = [(37, 53), (150, 201), (128, 128), (64, 64), (1, 7), (97, 33), (480, 640), (50, 186), (9, 68)]
DESTS = [(64, 64), (64, 96)]


def images(C, shapes=SHAPES, seed=0):
    rng = np.random.default_rng(seed + 17 * C)
    return [rng.integers(0, 256, size=(h, w, C), dtype=np.uint8) for h, w in shapes]
