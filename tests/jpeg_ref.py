"""numpy restatement of uwm_jpeg_u8 (include/uwm.h): what a baseline 4:2:0 JPEG encode + decode does to the pixels of a uint8 RGB
image, H and W multiples of 16 — libjpeg's default path without the (lossless) entropy coding: fixed-point colour conversion, 2 x 2
chroma down-sampling, the "islow" integer DCT, integer quantisation, the integer inverse DCT, "fancy" triangle up-sampling and the
fixed-point colour conversion back.  test_jpeg.py holds it to Pillow (libjpeg-turbo), bit for bit; test_jpeg_gpu.py holds the kernels
to it.  Everything is computed in int64, and every product, sum and shift operand of the two DCTs is asserted to stay inside int32
(the kernels use 32-bit registers); STATS["max_abs"] is the largest such operand seen so far."""
from __future__ import annotations

import numpy as np

# Annex K of the JPEG standard, natural (row-major) order
LUMINANCE = np.array([16, 11, 10, 16, 24, 40, 51, 61,
                      12, 12, 14, 19, 26, 58, 60, 55,
                      14, 13, 16, 24, 40, 57, 69, 56,
                      14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77,
                      24, 35, 55, 64, 81, 104, 113, 92,
                      49, 64, 78, 87, 103, 121, 120, 101,
                      72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64)
CHROMINANCE = np.array([17, 18, 24, 47, 99, 99, 99, 99,
                        18, 21, 26, 66, 99, 99, 99, 99,
                        24, 26, 56, 99, 99, 99, 99, 99,
                        47, 66, 99, 99, 99, 99, 99, 99,
                        99, 99, 99, 99, 99, 99, 99, 99,
                        99, 99, 99, 99, 99, 99, 99, 99,
                        99, 99, 99, 99, 99, 99, 99, 99,
                        99, 99, 99, 99, 99, 99, 99, 99], dtype=np.int64)
STATS = {"max_abs": 0}
_INT32 = (1 << 31) - 1


def _c(x):
    """an operand of the DCTs: must fit int32"""
    m = int(np.abs(x).max()) if x.size else 0
    STATS["max_abs"] = max(STATS["max_abs"], m)
    assert m <= _INT32, f"DCT operand {m} leaves int32"
    return x


def _descale(x, n):
    """D(x, n) = (x + (1 << (n-1))) >> n, arithmetic shift; the sum is an operand too"""
    return _c(_c(x) + (1 << (n - 1))) >> n


def quant_tables(q: int):
    """-> (luminance, chrominance) int64[64], natural order, of quality q = 1..100 (jpeg_quality_scaling + force_baseline)"""
    q = int(q)
    if not 1 <= q <= 100:
        raise ValueError(f"quality {q} outside 1..100")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((t * s + 50) // 100, 1, 255) for t in (LUMINANCE, CHROMINANCE))


def rgb_to_ycc(img):
    r, g, b = (img[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def downsample(c):
    """h2v2: (sum of the four + bias) >> 2, bias 1 in even output columns, 2 in odd ones"""
    s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
    bias = 1 + (np.arange(s.shape[1], dtype=np.int64) & 1)
    return (s + bias[None, :]) >> 2


def _fdct_1d(d, first):
    """jfdctint's 1-D pass along the last axis (8 values); first = the row pass"""
    d = [_c(d[..., i]) for i in range(8)]
    t0, t7 = _c(d[0] + d[7]), _c(d[0] - d[7])
    t1, t6 = _c(d[1] + d[6]), _c(d[1] - d[6])
    t2, t5 = _c(d[2] + d[5]), _c(d[2] - d[5])
    t3, t4 = _c(d[3] + d[4]), _c(d[3] - d[4])
    t10, t13 = _c(t0 + t3), _c(t0 - t3)
    t11, t12 = _c(t1 + t2), _c(t1 - t2)
    n = 11 if first else 15
    o = [None] * 8
    if first:
        o[0], o[4] = _c(_c(t10 + t11) << 2), _c(_c(t10 - t11) << 2)
    else:
        o[0], o[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = _c(_c(t12 + t13) * 4433)
    o[2] = _descale(z1 + _c(t13 * 6270), n)
    o[6] = _descale(z1 - _c(t12 * 15137), n)
    z1, z2, z3, z4 = _c(t4 + t7), _c(t5 + t6), _c(t4 + t6), _c(t5 + t7)
    z5 = _c(_c(z3 + z4) * 9633)
    t4, t5, t6, t7 = _c(t4 * 2446), _c(t5 * 16819), _c(t6 * 25172), _c(t7 * 12299)
    z1, z2, z3, z4 = _c(z1 * -7373), _c(z2 * -20995), _c(z3 * -16069), _c(z4 * -3196)
    z3, z4 = _c(z3 + z5), _c(z4 + z5)
    o[7] = _descale(_c(t4 + z1) + z3, n)
    o[5] = _descale(_c(t5 + z2) + z4, n)
    o[3] = _descale(_c(t6 + z2) + z3, n)
    o[1] = _descale(_c(t7 + z1) + z4, n)
    return np.stack(o, -1)


def fdct(blocks):
    """[..., 8, 8] samples minus 128 -> 8 times their DCT: rows first, then columns"""
    rows = _fdct_1d(blocks, True)
    return np.swapaxes(_fdct_1d(np.swapaxes(rows, -1, -2), False), -1, -2)


def quantise(coef, table):
    """-> the dequantised coefficients [..., 8, 8]: coefficient = sign(c) * ((|c| + (qv >> 1)) / qv), qv = Q << 3, times Q"""
    qm = table.reshape(8, 8)
    qv = qm << 3
    a = (np.abs(coef) + (qv >> 1)) // qv
    return np.where(coef < 0, -a, a) * qm


def _idct_1d(d, first):
    """jidctint's 1-D pass along the last axis; first = the column pass (D(., 11)), else the row pass (D(., 18))"""
    d = [_c(d[..., i]) for i in range(8)]
    z2, z3 = d[2], d[6]
    z1 = _c(_c(z2 + z3) * 4433)
    t2 = _c(z1 - _c(z3 * 15137))
    t3 = _c(z1 + _c(z2 * 6270))
    t0, t1 = _c(_c(d[0] + d[4]) << 13), _c(_c(d[0] - d[4]) << 13)
    t10, t13 = _c(t0 + t3), _c(t0 - t3)
    t11, t12 = _c(t1 + t2), _c(t1 - t2)
    t0, t1, t2, t3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = _c(t0 + t3), _c(t1 + t2), _c(t0 + t2), _c(t1 + t3)
    z5 = _c(_c(z3 + z4) * 9633)
    t0, t1, t2, t3 = _c(t0 * 2446), _c(t1 * 16819), _c(t2 * 25172), _c(t3 * 12299)
    z1, z2, z3, z4 = _c(z1 * -7373), _c(z2 * -20995), _c(z3 * -16069), _c(z4 * -3196)
    z3, z4 = _c(z3 + z5), _c(z4 + z5)
    t0, t1 = _c(t0 + _c(z1 + z3)), _c(t1 + _c(z2 + z4))
    t2, t3 = _c(t2 + _c(z2 + z3)), _c(t3 + _c(z1 + z4))
    n = 11 if first else 18
    o = [_descale(t10 + t3, n), _descale(t11 + t2, n), _descale(t12 + t1, n), _descale(t13 + t0, n),
         _descale(t13 - t0, n), _descale(t12 - t1, n), _descale(t11 - t2, n), _descale(t10 - t3, n)]
    return np.stack(o, -1)


def idct(coef):
    """dequantised coefficients [..., 8, 8] -> samples 0..255: columns first, then rows, + 128, clamp"""
    cols = np.swapaxes(_idct_1d(np.swapaxes(coef, -1, -2), True), -1, -2)
    return np.clip(_idct_1d(cols, False) + 128, 0, 255)


def _blocks(p):
    h, w = p.shape
    return p.reshape(h // 8, 8, w // 8, 8).swapaxes(1, 2)


def _unblocks(b):
    nh, nw = b.shape[:2]
    return b.swapaxes(1, 2).reshape(nh * 8, nw * 8)


def plane_roundtrip(p, table):
    """one component plane (sizes multiples of 8) through fDCT -> quantise -> dequantise -> IDCT"""
    return _unblocks(idct(quantise(fdct(_blocks(p) - 128), table)))


def upsample(c):
    """h2v2 'fancy' (triangle) up-sampling of a chroma plane [h][w] -> [2h][2w]"""
    h, w = c.shape
    rows = np.arange(h)
    out = np.empty((2 * h, 2 * w), dtype=np.int64)
    for v in (0, 1):
        near = np.clip(rows + (1 if v else -1), 0, h - 1)
        s = 3 * c + c[near]
        left = s[:, np.clip(np.arange(w) - 1, 0, w - 1)]
        right = s[:, np.clip(np.arange(w) + 1, 0, w - 1)]
        out[v::2, 0::2] = (3 * s + left + 8) >> 4
        out[v::2, 1::2] = (3 * s + right + 7) >> 4
    return out


def ycc_to_rgb(y, cb, cr):
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def roundtrip(img, q: int):
    """uint8 (H, W, 3) RGB, H % 16 == W % 16 == 0 -> the image after a baseline 4:2:0 JPEG round trip at quality q (0 = unchanged)"""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.shape[0] % 16 or img.shape[1] % 16 or img.shape[0] < 16 \
            or img.shape[1] < 16:
        raise ValueError("roundtrip needs a uint8 (H, W, 3) image with H and W multiples of 16")
    if int(q) == 0:
        return img.copy()
    lum, chrom = quant_tables(q)
    y, cb, cr = rgb_to_ycc(img)
    y = plane_roundtrip(y, lum)
    cb = upsample(plane_roundtrip(downsample(cb), chrom))
    cr = upsample(plane_roundtrip(downsample(cr), chrom))
    return ycc_to_rgb(y, cb, cr)


def roundtrip_batch(images, quality):
    """uint8 (N, H, W, 3) and N qualities -> uint8 (N, H, W, 3)"""
    return np.stack([roundtrip(im, int(q)) for im, q in zip(np.asarray(images), quality)])


def normalise(u8, mean, std):
    """uwm_preprocess_u8's expression on uint8 (N, H, W, C): fma(float32(v), 1 / (255 std), -mean / std) as fp32 NCHW"""
    mean, std = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    mul = (np.float32(1.0) / (np.float32(255.0) * std)).astype(np.float32)
    add = (-mean / std).astype(np.float32)
    v = u8.astype(np.float64) * mul.astype(np.float64) + add.astype(np.float64)      # exact in float64, one rounding = the fma
    return np.ascontiguousarray(v.astype(np.float32).transpose(0, 3, 1, 2))


def sample_images(h, w, seed=0):
    """the image kinds of the tests: name -> uint8 (h, w, 3)"""
    g = np.random.default_rng(seed + 1000 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    out = {"noise": g.integers(0, 256, (h, w, 3), dtype=np.uint8),
           "noise01": (g.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8),
           "stripes": np.stack([(xx & 1) * 255, (yy & 1) * 255, ((xx + yy) & 1) * 255], -1).astype(np.uint8),
           "checker8": np.stack([(((xx >> 3) + (yy >> 3)) & 1) * 255, (((xx >> 3) + (yy >> 3) + 1) & 1) * 255,
                                 ((yy >> 3) & 1) * 255], -1).astype(np.uint8),
           "ramps": np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy) * 255 // (h + w - 2)], -1).astype(np.uint8)}
    return out
