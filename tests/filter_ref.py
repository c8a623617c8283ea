"""numpy restatement of the dataset filter's rule (csrc/filter_u8.hip; include/uwm.h): per image of a ragged batch,
sigmoid of the logits -> bilinear resize of the PROBABILITIES to the image's own size -> > threshold -> [open, close with the 3 x 3
cross] -> the foreground count.  fp32 arithmetic in the kernel's order; the morphology is tests/maskpost_ref.py's.  A helper of
tests/test_filter.py and tests/test_filter_gpu.py, not itself a test.

What fp32 cannot pin down: the device's expf and numpy's may differ in the last bits, and the device compiler contracts a * b + c
into one fused multiply-add where it likes.  The coordinate `(Y + 0.5) * scale - 0.5` is such a pattern and IS fused on the device,
so `axis` models it fused (`fused=False` gives the other reading).  The products of the interpolation are left unfused here.  Tests
that compare masks bit for bit therefore first assert `margin(...)`: the distance of the closest fp64 value to the threshold, under
both readings of the coordinate, which must exceed what those last bits can move."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maskpost_ref as M  # noqa: E402

F = np.float32
CROSS = M.ellipse(3, 3)                   # cv2.getStructuringElement(MORPH_ELLIPSE, (3, 3)) = the cross


def sigmoid32(x):
    """1.f / (1.f + expf(-x)): the project's sigmoid (csrc/loss.hip)"""
    return F(1) / (F(1) + np.exp(-np.asarray(x, F), dtype=F))


def axis(dst, src, fused=True):
    """one axis of resize_logit (csrc/uwm_kernels.h): (i0, i1, weight of i1) for dst samples of src, fp32"""
    scale = F(src) / F(dst)
    c = np.arange(dst, dtype=F) + F(0.5)
    if fused:                                                                # fma(c, scale, -0.5): one rounding (the product is exact in fp64)
        f = (c.astype(np.float64) * np.float64(scale) - 0.5).astype(F)
    else:
        f = c * scale - F(0.5)
    f = np.maximum(f, F(0))
    i0 = np.minimum(f.astype(np.int64), src - 1)
    i1 = np.minimum(i0 + 1, src - 1)
    return i0, i1, f - i0.astype(F)


def _interp(p, H, W, dtype, fused=True):
    h, w = p.shape
    y0, y1, wy = axis(H, h, fused); x0, x1, wx = axis(W, w, fused)
    one = dtype(1)
    wy = wy.astype(dtype)[:, None]; wx = wx.astype(dtype)[None, :]
    p = p.astype(dtype)
    top = (one - wx) * p[y0][:, x0] + wx * p[y0][:, x1]                      # horizontal inside vertical
    bot = (one - wx) * p[y1][:, x0] + wx * p[y1][:, x1]
    return (one - wy) * top + wy * bot


def prob_resize(logits, H, W):
    """fp32 (h, w) logits -> fp32 (H, W): sigmoid at the taps first, then resize_logit's interpolation of the probabilities"""
    return _interp(sigmoid32(logits), H, W, F)


def logit_resize_sigmoid(logits, H, W):
    """the OTHER order, uwm_resize_threshold(apply_sigmoid = 1): interpolate the logits, then the sigmoid"""
    return sigmoid32(_interp(np.asarray(logits, F), H, W, F))


def prob_resize64(logits, H, W, fused=True):
    """the same value in fp64 from the fp32 weights: for the margin only"""
    x = np.asarray(logits, F).astype(np.float64)
    return _interp(1.0 / (1.0 + np.exp(-x)), H, W, np.float64, fused)


def margin(logits, H, W, threshold):
    """the least |fp64 value - threshold| over the H x W pixels, under both readings of the coordinate"""
    t = float(F(threshold))
    return min(float(np.abs(prob_resize64(logits, H, W, fu) - t).min()) for fu in (True, False))


def post_process(m):
    """bool (H, W) -> close(open(m, E(3,3)), E(3,3)), one iteration each (watermark_filter.py's _post_process_mask)"""
    return M.closing(M.opening(m, CROSS), CROSS)


def mask_from_prob(v, threshold, post):
    m = v > F(threshold)
    return post_process(m) if post else m


def filter_mask(logits, H, W, threshold, post):
    """steps 1 to 4 -> uint8 {0, 255} (H, W)"""
    return mask_from_prob(prob_resize(logits, H, W), threshold, post).astype(np.uint8) * 255


def filter_count(logits, H, W, threshold, post):
    """step 5 -> [foreground pixels, H * W]"""
    return [int(np.count_nonzero(filter_mask(logits, H, W, threshold, post))), H * W]
