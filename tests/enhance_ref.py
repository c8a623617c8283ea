"""Restatement of the reference's enhance_mask (src/scripts/enhance_masks.py:16-67) in numpy: what uwm_enhance_masks_ragged is held to.
OpenCV is not available to this project, so every OpenCV rule here is written out from its documented behaviour, not run.

  enhance_literal   steps 1 to 6 as the script performs them: grey close E(7,7), grey dilate E(2e+1, 2e+1), float32, Gaussian blur,
                    s times open / close E(5,5) ON FLOATS, threshold at 127, bilateralFilter(9, 75, 75), threshold at 127
  enhance_reduced   the chain the device runs: ... blur, threshold, s times a BINARY open / close E(5,5); no bilateral step

The blur is the library's own arithmetic (include/uwm.h), given its float32 taps: row pass then column pass, each
acc = t[c]*x[0]; acc += t[c+i] * (x[-i] + x[+i]) for i = 1 .. r in order, every operation rounded to float32 (numpy rounds each
array operation), border BORDER_REFLECT_101.  tests/test_enhance.py holds literal == reduced byte for byte on every case."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

# (expand_pixels, blur_kernel, smooth_iterations): the parameter sets of the issue; the last one runs on the small images only
PARAMS = ((10, 15, 2), (15, 21, 2), (0, 0, 0), (1, 3, 1), (2, 4, 1), (3, 7, 0), (4, 9, 1), (31, 63, 8))
TILE = 64                                     # the kernels' tile side (csrc/mask_enhance.hip: kT)
SMALL = 60                                    # images of at most this many pixels are "the small images"
STAGES = ("close", "dilate", "blur", "threshold", "smooth")


def ellipse_dx(size: int):
    """half-widths of the rows of cv2.getStructuringElement(MORPH_ELLIPSE, (size, size)), size odd: row i spans [r - dx, r + dx]"""
    assert size >= 1 and size % 2 == 1
    r = size // 2
    inv_r2 = 1.0 / (float(r) * r) if r else 0.0
    return [int(np.rint(r * np.sqrt((r * r - (i - r) * (i - r)) * inv_r2))) for i in range(size)]


def ellipse(size: int) -> np.ndarray:
    r = size // 2
    k = np.zeros((size, size), np.uint8)
    for i, dx in enumerate(ellipse_dx(size)):
        k[i, r - dx:r + dx + 1] = 1
    return k


def morph(a: np.ndarray, size: int, is_max: bool) -> np.ndarray:
    """grey dilation (max) / erosion (min) with E(size, size), anchor at the centre, pixels outside the image ignored; any dtype
    (min and max select, so the detour through float64 is exact for uint8 and float32)"""
    r = size // 2
    H, W = a.shape
    fill = -np.inf if is_max else np.inf
    p = np.pad(a.astype(np.float64), r, constant_values=fill)
    out = np.full((H, W), fill)
    for i, dx in enumerate(ellipse_dx(size)):
        win = sliding_window_view(p[i:i + H], 2 * dx + 1, axis=1)
        span = win.max(-1) if is_max else win.min(-1)
        seg = span[:, r - dx:r - dx + W]
        out = np.maximum(out, seg) if is_max else np.minimum(out, seg)
    return out.astype(a.dtype)


def dilate(a, size): return morph(a, size, True)
def erode(a, size): return morph(a, size, False)
def close_(a, size): return erode(dilate(a, size), size)
def open_(a, size): return dilate(erode(a, size), size)


def reflect101(p: int, n: int) -> int:
    """cv2.borderInterpolate(p, n, BORDER_REFLECT_101)"""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * (n - 1) - p
    return p


def _blur_pass(x: np.ndarray, taps: np.ndarray, axis: int) -> np.ndarray:
    c = len(taps) // 2
    n = x.shape[axis]
    acc = taps[c] * x
    for i in range(1, c + 1):
        lo = np.take(x, [reflect101(j - i, n) for j in range(n)], axis=axis)
        hi = np.take(x, [reflect101(j + i, n) for j in range(n)], axis=axis)
        acc = acc + taps[c + i] * (lo + hi)
        assert acc.dtype == np.float32
    return acc


def blur(f: np.ndarray, taps: np.ndarray) -> np.ndarray:
    """row pass (stored as float32), then column pass, in the arithmetic fixed in include/uwm.h"""
    taps = np.asarray(taps)
    assert f.dtype == np.float32 and taps.dtype == np.float32 and len(taps) % 2 == 1
    return _blur_pass(_blur_pass(f, taps, 1), taps, 0)


def gauss_taps_formula(k: int) -> np.ndarray:
    """cv2.getGaussianKernel(k, 0, CV_32F) for k >= 9, in double (before the rounding to float32)"""
    sigma = ((k - 1) * 0.5 - 1) * 0.3 + 0.8
    x = np.arange(k, dtype=np.float64) - (k - 1) * 0.5
    t = np.exp(-0.5 * x * x / (sigma * sigma))
    return t / t.sum()


def bilateral_9_75_75(u: np.ndarray) -> np.ndarray:
    """cv2.bilateralFilter(u, 9, 75, 75) on a uint8 image: radius 4, the 49 taps with i*i + j*j <= 16, float32 weights
    space[i,j] * colour[|v - v0|], BORDER_REFLECT_101, the quotient rounded half to even"""
    assert u.dtype == np.uint8
    radius, sigma = 4, 75.0
    coeff = -0.5 / (sigma * sigma)
    colour = np.exp(np.arange(256, dtype=np.float64) ** 2 * coeff).astype(np.float32)
    H, W = u.shape
    rows = [reflect101(y, H) for y in range(-radius, H + radius)]
    cols = [reflect101(x, W) for x in range(-radius, W + radius)]
    p = u[np.ix_(rows, cols)].astype(np.int32)
    v0 = u.astype(np.int32)
    total = np.zeros((H, W), np.float32)
    wsum = np.zeros((H, W), np.float32)
    taps = 0
    for i in range(-radius, radius + 1):
        for j in range(-radius, radius + 1):
            if i * i + j * j > radius * radius:
                continue
            taps += 1
            space = np.float32(np.exp((i * i + j * j) * coeff))
            v = p[radius + i:radius + i + H, radius + j:radius + j + W]
            w = space * colour[np.abs(v - v0)]
            total = total + v.astype(np.float32) * w
            wsum = wsum + w
    assert taps == 49 and total.dtype == np.float32
    return np.rint(total / wsum).astype(np.uint8)


def _binary(f) -> np.ndarray:
    return np.where(f > 127, 255, 0).astype(np.uint8)


def enhance_literal(m: np.ndarray, taps, expand_pixels: int, smooth_iterations: int) -> np.ndarray:
    """steps 1 to 6 of the script; taps: the float32 Gaussian taps, or None for blur_kernel = 0"""
    assert m.dtype == np.uint8 and m.ndim == 2
    m = close_(m, 7)
    m = dilate(m, 2 * expand_pixels + 1)
    f = m.astype(np.float32)
    if taps is not None:
        f = blur(f, taps)
    for _ in range(smooth_iterations):
        f = open_(f, 5)
        f = close_(f, 5)
    u = _binary(f)
    u = bilateral_9_75_75(u)
    return _binary(u)


def enhance_reduced(m: np.ndarray, taps, expand_pixels: int, smooth_iterations: int, skip=None) -> np.ndarray:
    """the reduced chain: close 7, dilate, blur, threshold, binary smoothing.  skip: one of STAGES to leave out (for the test that
    every stage matters on the cases); without the threshold the smoothing runs on the floats and the result is their rounding"""
    assert m.dtype == np.uint8 and m.ndim == 2 and skip in (None,) + STAGES
    if skip != "close":
        m = close_(m, 7)
    if skip != "dilate":
        m = dilate(m, 2 * expand_pixels + 1)
    f = m.astype(np.float32)
    if taps is not None and skip != "blur":
        f = blur(f, taps)
    u = f if skip == "threshold" else _binary(f)
    if skip != "smooth":
        for _ in range(smooth_iterations):
            u = open_(u, 5)
            u = close_(u, 5)
    return np.rint(u).clip(0, 255).astype(np.uint8) if skip == "threshold" else u


def _disc(img, cy, cx, r, value):
    y, x = np.ogrid[:img.shape[0], :img.shape[1]]
    img[(y - cy) ** 2 + (x - cx) ** 2 <= r * r] = value


def images():
    """the batch of the GPU test: blobs with holes, one-pixel lines, grey values around 127 / 128, all zero, all 255, sparse noise.
    The content of the larger images stays clear of one corner, so that the enlarged masks of the two big parameter sets do not
    fill them."""
    g = np.random.default_rng(20)
    out = []
    out.append(np.full((1, 1), 255, np.uint8))                                        # 1 x 1
    out.append(np.array([[0, 0, 255, 255, 0, 128, 127, 0, 0]], np.uint8))             # 1 x 9
    out.append(np.zeros((7, 1), np.uint8))                                            # 7 x 1: all zero
    out.append(((g.random((3, 5)) < 0.5) * 255).astype(np.uint8))                     # 3 x 5: smaller than every radius
    a = np.zeros((33, 65), np.uint8)                                                  # one-pixel lines and lone pixels, left part
    a[5, 2:16] = 255; a[2:20, 8] = 255; a[12, 3] = 255; a[22, 12] = 200; a[25, 4:9] = 128
    for d in range(8):
        a[24 + d, 10 + d] = 255
    out.append(a)
    a = np.zeros((64, 64), np.uint8)                                                  # a blob with holes, a ring, a gap
    _disc(a, 30, 30, 11, 255); _disc(a, 28, 27, 1, 0); _disc(a, 33, 34, 3, 0); a[30, 19:24] = 0
    a[20:24, 44:46] = 255; a[20:24, 49:51] = 255
    out.append(a)
    a = np.zeros((96, 200), np.uint8)                                                 # blobs, grey plateaus, sparse noise
    _disc(a, 40, 50, 14, 255); _disc(a, 40, 50, 2, 0); _disc(a, 45, 58, 4, 90)
    a[20:50, 100:130] = 128; a[25:45, 105:125] = 127; a[60:75, 95:125] = 127
    a[56:59, 20:60] = 255; a[30:34, 140:150] = 129; a[40, 150] = 255
    noise = g.random((40, 60)) < 0.02
    a[50:90, 5:65][noise] = 255
    a[10:14, 10:14] = np.array([[126, 127, 128, 129]] * 4, np.uint8)
    out.append(a)
    a = np.zeros((TILE + 1, TILE + 1), np.uint8)                                      # one pixel past the tile in each direction
    _disc(a, 24, 26, 9, 255); _disc(a, 24, 26, 2, 100); a[18:31, 40] = 255; a[10, 5:12] = 130
    a[3, 3] = 255; a[36, 12:20] = 255; a[38, 12:20] = 255
    out.append(a)
    out.append(np.zeros((12, 17), np.uint8))                                          # all zero
    out.append(np.full((9, 13), 255, np.uint8))                                       # all 255
    a = ((g.random((40, 56)) < 0.02) * 255).astype(np.uint8)                          # sparse noise
    a[:, 36:] = 0
    out.append(a)
    return out


def batch_for(params):
    """the images a parameter set runs on: all of them, or for (31, 63, 8) the small ones"""
    ims = images()
    return [im for im in ims if im.size <= SMALL] if params == PARAMS[-1] else ims
