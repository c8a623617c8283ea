"""numpy restatement of uwm_jpeg_ragged_u8 (include/uwm.h): what a baseline 4:2:0 JPEG encode + decode does to a uint8 RGB image of
ANY size — jpeg_ref.py's arithmetic (imported, with its int32 operand assertions) plus libjpeg's edge rule:
  Y       the last column and row replicated out to multiples of 8;
  Cb, Cr  columns (and an odd last row) replicated at full resolution, in front of the down-sampling; rows replicated behind it;
  back    the triangle filter on the cropped ceil(H/2) x ceil(W/2) plane — or, where that plane is at most 2 wide, plain replication.
test_jpeg_any.py holds it to Pillow (libjpeg-turbo) bit for bit; test_jpeg_any_gpu.py holds the kernels to it."""
from __future__ import annotations

import numpy as np

import jpeg_ref as J


def c8(x: int) -> int:
    return (int(x) + 7) // 8 * 8


def _pad_edge(p, rows, cols):
    """p [h][w] -> [rows][cols], the last row and column replicated"""
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def downsample_any(c, hc, wc):
    """a full-resolution chroma plane [H][W] -> the padded down-sampled plane [c8(hc)][c8(wc)]"""
    full = _pad_edge(c, 2 * hc, 2 * c8(wc))              # columns, and an odd last row, at full resolution
    return _pad_edge(J.downsample(full), c8(hc), c8(wc))      # rows behind the down-sampling


def upsample_any(c, H, W):
    """the cropped chroma plane [hc][wc] -> [H][W]"""
    if c.shape[1] > 2:
        return J.upsample(c)[:H, :W]
    return np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)[:H, :W]


def roundtrip_any(img, q: int):
    """uint8 (H, W, 3) RGB, H and W >= 1 -> the image after a baseline 4:2:0 JPEG round trip at quality q (0 = unchanged)"""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("roundtrip_any needs a uint8 (H, W, 3) image with H and W >= 1")
    if int(q) == 0:
        return img.copy()
    H, W = img.shape[:2]
    hc, wc = (H + 1) // 2, (W + 1) // 2
    lum, chrom = J.quant_tables(q)
    y, cb, cr = J.rgb_to_ycc(img)
    y = J.plane_roundtrip(_pad_edge(y, c8(H), c8(W)), lum)[:H, :W]
    cb = upsample_any(J.plane_roundtrip(downsample_any(cb, hc, wc), chrom)[:hc, :wc], H, W)
    cr = upsample_any(J.plane_roundtrip(downsample_any(cr, hc, wc), chrom)[:hc, :wc], H, W)
    return J.ycc_to_rgb(y, cb, cr)


def roundtrip_ragged(images, qualities):
    """a list of uint8 (h_i, w_i, 3) images and one quality each -> the list of round-tripped images"""
    if len(images) != len(qualities):
        raise ValueError("one quality per image")
    return [roundtrip_any(im, int(q)) for im, q in zip(images, qualities)]
