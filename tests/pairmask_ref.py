"""numpy restatement of the pair-mask rule that csrc/pair_mask_u8.hip implements (include/uwm.h): the reference's
WatermarkDataset._generate_mask with use_blurred_mask = False — cv2.absdiff, cvtColor(RGB2GRAY) by OpenCV 4.x's 8-bit rule (15
coefficient bits), cv2.threshold, MORPH_OPEN with the 3 x 3 ellipse (a cross), GaussianBlur((3,3), 0.5) and a threshold at 127 — written
from the sources and NOT run against cv2.  The device kernel omits the closing blur + threshold because it is the identity on {0,255}
images; this restatement carries it (in float), so the tests show that identity instead of assuming it.  A helper of
tests/test_pairmask.py and tests/test_pairmask_gpu.py, not itself a test."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maskpost_ref as M  # noqa: E402
import resize_ref as R  # noqa: E402

CROSS = M.ellipse(3, 3)                  # cv2.getStructuringElement(MORPH_ELLIPSE, (3, 3))


def diff_gray(wm, clean):
    """cv2.absdiff then cvtColor(RGB2GRAY): (R*9798 + G*19235 + B*3735 + 16384) >> 15 on uint8 RGB (h, w, 3) -> int (h, w)"""
    d = np.abs(wm.astype(np.int64) - clean.astype(np.int64))
    return (d[..., 0] * 9798 + d[..., 1] * 19235 + d[..., 2] * 3735 + 16384) >> 15


def gaussian_kernel_3(sigma=0.5):
    """cv2.getGaussianKernel(3, 0.5): exp(-x^2 / (2 sigma^2)) at x = -1, 0, 1, normalised"""
    k = np.exp(-np.arange(-1, 2, dtype=np.float64) ** 2 / (2.0 * sigma * sigma))
    return k / k.sum()


def blur_threshold(mask_u8):
    """GaussianBlur((3,3), 0.5) with cv2's default BORDER_REFLECT_101 (an axis of one pixel reflects onto itself), rounded to uint8,
    then > 127 -> 255 / 0"""
    k = gaussian_kernel_3()
    m = mask_u8.astype(np.float64)
    p = np.pad(m, ((1, 1), (0, 0)), mode="reflect" if m.shape[0] > 1 else "edge")
    p = np.pad(p, ((0, 0), (1, 1)), mode="reflect" if m.shape[1] > 1 else "edge")
    H, W = m.shape
    out = np.zeros((H, W))
    for i in range(3):
        for j in range(3):
            out += k[i] * k[j] * p[i:i + H, j:j + W]
    return np.where(np.rint(out) > 127, 255, 0).astype(np.uint8)


def pair_mask(wm, clean, threshold, open=True, blur=True):
    """-> uint8 (h, w) in {0, 255} at the watermarked image's size.  open=False stops behind the threshold (steps 2-4 of the rule);
    blur=False leaves out the closing blur + threshold (what the device computes)."""
    if clean.shape != wm.shape:
        clean = R.resize_u8_linear(clean, wm.shape[0], wm.shape[1])          # cv2.resize(clean, (w, h)): INTER_LINEAR
    m = diff_gray(wm, clean) > int(threshold)
    if not open:
        return np.where(m, 255, 0).astype(np.uint8)
    m = M.opening(m, CROSS, 1)
    u8 = np.where(m, 255, 0).astype(np.uint8)
    return blur_threshold(u8) if blur else u8


def pair_from_plane(plane, threshold, seed=0):
    """a watermarked / clean pair whose thresholded difference is exactly `plane` (bool (h, w)): gray differences of threshold + 1
    where it is set and of exactly `threshold` elsewhere (equal R, G, B differences d give g = d: the coefficients sum to 2^15)"""
    rng = np.random.default_rng(seed)
    T = int(threshold)
    assert 0 <= T < 255
    h, w = plane.shape
    clean = rng.integers(0, 256 - (T + 1), size=(h, w, 3), dtype=np.int64)
    d = np.where(plane, T + 1, T)[..., None]
    sign = rng.integers(0, 2, size=(h, w, 1)) * 2 - 1                      # the difference in either direction
    lo = np.where(sign > 0, clean, clean + d)                              # wm = clean + d, or clean' = clean + d and wm = clean
    wm = np.where(sign > 0, clean + d, clean)
    return wm.astype(np.uint8), lo.astype(np.uint8)


# ------------------------------------------------------------------ hand-computed cases: (name, plane before the opening, plane after)
def _plane(h, w, pts):
    m = np.zeros((h, w), bool)
    for y, x in pts:
        m[y, x] = True
    return m


def _block(h, w, y0, x0, bh, bw):
    m = np.zeros((h, w), bool)
    m[y0:y0 + bh, x0:x0 + bw] = True
    return m


PLUS = [(1, 2), (2, 1), (2, 2), (2, 3), (3, 2)]                            # centre (2, 2)


def hand_cases():
    """Opening with the cross keeps exactly the union of the crosses that fit inside the foreground; a cross centred on a border pixel
    fits when its in-image arms do (the erosion ignores pixels outside the image)."""
    c = []
    c.append(("lone pixel vanishes", _plane(5, 5, [(2, 2)]), _plane(5, 5, [])))
    c.append(("2x2 block vanishes", _block(6, 6, 2, 2, 2, 2), _plane(6, 6, [])))
    c.append(("3x3 block becomes a cross", _block(7, 7, 2, 2, 3, 3), _plane(7, 7, [(2, 3), (3, 2), (3, 3), (3, 4), (4, 3)])))
    c.append(("plus survives", _plane(5, 5, PLUS), _plane(5, 5, PLUS)))
    # foreground touching each border: a 2-thick strip along the border survives whole where its crosses fit
    top = _block(6, 7, 0, 0, 2, 7)                                         # rows 0-1, all columns: centres on row 0 fit -> rows 0-1 stay
    c.append(("strip on the top border", top, top.copy()))
    bottom = _block(6, 7, 4, 0, 2, 7)
    c.append(("strip on the bottom border", bottom, bottom.copy()))
    left = _block(7, 6, 0, 0, 7, 2)
    c.append(("strip on the left border", left, left.copy()))
    right = _block(7, 6, 0, 4, 7, 2)
    c.append(("strip on the right border", right, right.copy()))
    # a 2x2 block in a corner: the corner pixel's cross has only two in-image arms, both set -> it fits, and dilating it
    # gives the corner and its two neighbours; the diagonal pixel goes
    c.append(("2x2 block in the top-left corner", _block(5, 5, 0, 0, 2, 2), _plane(5, 5, [(0, 0), (0, 1), (1, 0)])))
    c.append(("2x2 block in the bottom-right corner", _block(5, 5, 3, 3, 2, 2), _plane(5, 5, [(4, 4), (4, 3), (3, 4)])))
    # a lone pixel in a corner has no set in-image neighbour: it vanishes
    c.append(("lone corner pixel vanishes", _plane(4, 4, [(0, 0)]), _plane(4, 4, [])))
    # one-pixel images: the cross has no in-image arm, so the pixel is its own opening
    c.append(("1x1 foreground stays", _plane(1, 1, [(0, 0)]), _plane(1, 1, [(0, 0)])))
    # a 1 x 7 row: every vertical arm is outside; a run of 3 keeps all three (its centre fits), and so does a run of 2 at the
    # border (the end pixel's missing arm is ignored)
    c.append(("1x7 row", _plane(1, 7, [(0, 0), (0, 1), (0, 3), (0, 4), (0, 5)]),
              _plane(1, 7, [(0, 0), (0, 1), (0, 3), (0, 4), (0, 5)])))
    return c


# the RGB difference where the 15-bit integer rule and a rounded float 0.299 / 0.587 / 0.114 disagree:
# 2*19235 + 152*3735 + 16384 = 622574 = 18 * 32768 + 32750 -> 18, while 0.587*2 + 0.114*152 = 18.502 -> 19
GRAY_DISAGREE = ((0, 2, 152), 18, 19)
