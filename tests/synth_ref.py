"""numpy restatement of the logo-watermark synthesis rule that csrc/synth_u8.hip implements (include/uwm.h): the logo
branch of the reference's src/scripts/gen_data.py, stage by stage, on an RGBA patch:

  1 resize      Image.resize(LANCZOS) on RGBA: premultiply, horizontal then vertical pass to uint8, unpremultiply
  2 rotate      Image.rotate(angle, expand=True), NEAREST, fill 0 (Pillow's affine_fixed)
  3 stretch     stage 1 again; then optionally shear = cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT 0), restated from knowledge with
                the fixed point of tests/augment_ref.py (10 coordinate bits, 5 interpolation bits) and NOT run against cv2
  4 blur        ImageFilter.GaussianBlur: three horizontal and three vertical extended box blurs on all four channels
  5 defects     rectangles of alpha 0
  6 enhance     ImageEnhance.Brightness, Contrast, Color = Image.blend(degenerate, image, f) over RGB
  7 opacity     a = (uint8)(a * alpha) as a 256-entry table
  8 paste       Image.paste(patch, (x, y), patch) into the RGB image, and of the alpha plane into the L mask

Stages 1, 2, 4, 6, 7 and 8 are compared with Pillow bit for bit in tests/test_synth.py.  A job is one record of data.SYNTH_JOB_DTYPE
(= uwm_synth_job); the host draws every number and computes every size, so everything here is a pure function of its inputs.
math.sin, not np.sin: the tables are libm's.  A helper of tests/test_synth.py and tests/test_synth_gpu.py, not itself a test."""
import math

import numpy as np

PRECISION_BITS = 22


def muldiv255(x, y):
    t = x.astype(np.int64) * y + 128
    return ((t >> 8) + t) >> 8


# ------------------------------------------------------------------------------------------------ stage 1: LANCZOS resize
def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def lanczos(x):
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


def lanczos_ksize(insz, outsz):
    fs = max(insz / outsz, 1.0)
    return int(math.ceil(3.0 * fs)) * 2 + 1


def lanczos_table(insz, outsz):
    """-> int32 [outsz][2 + ksize]: per output index xmin, xmax (the tap count) and the 22-bit coefficients, zero past xmax"""
    scale = insz / outsz
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    tab = np.zeros((outsz, 2 + ksize), np.int32)
    for xx in range(outsz):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), insz) - xmin
        w = [lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        tab[xx, 0] = xmin; tab[xx, 1] = xmax
        for x, v in enumerate(w):
            tab[xx, 2 + x] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
    return tab


def resample_rows(a, outsz):
    """one pass along axis 1 of int64 [rows][insz][4] -> [rows][outsz][4], clipped to uint8 range"""
    tab = lanczos_table(a.shape[1], outsz)
    out = np.empty((a.shape[0], outsz, a.shape[2]), np.int64)
    for xx in range(outsz):
        xmin, xmax = int(tab[xx, 0]), int(tab[xx, 1])
        k = tab[xx, 2:2 + xmax].astype(np.int64)
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(a[:, xmin:xmin + xmax], k, axes=([1], [0]))
        out[:, xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def premultiply(p):
    q = p.astype(np.int64)
    q[..., :3] = muldiv255(q[..., :3], q[..., 3:4])
    return q


def unpremultiply(q):
    a = q[..., 3:4]
    safe = np.where(a == 0, 1, a)
    c = np.where((a == 0) | (a == 255), q[..., :3], np.minimum(255, (255 * q[..., :3]) // safe))
    return np.concatenate([c, a], axis=-1).astype(np.uint8)


def resize_rgba(p, w, h):
    """uint8 (H, W, 4) -> (h, w, 4): Image.resize((w, h), LANCZOS) of an RGBA image"""
    H, W = p.shape[:2]
    if (w, h) == (W, H):
        return p.copy()
    q = premultiply(p)
    if w != W:
        q = resample_rows(q, w)
    if h != H:
        q = resample_rows(q.transpose(1, 0, 2), h).transpose(1, 0, 2)
    return unpremultiply(q)


# ------------------------------------------------------------------------------------------------ stage 2: rotate(expand=True), NEAREST
def rotate_setup(w, h, angle):
    """Image.rotate's host arithmetic -> (matrix of 6 floats, expanded width, expanded height); angle % 360 == 0 is the identity and
    must not come here"""
    angle = angle % 360.0
    cx, cy = w / 2.0, h / 2.0
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]

    def tr(x, y, m):
        return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]

    m[2], m[5] = tr(-cx, -cy, m)
    m[2] += cx; m[5] += cy
    xs, ys = [], []
    for x, y in ((0, 0), (w, 0), (w, h), (0, h)):
        tx, ty = tr(x, y, m)
        xs.append(tx); ys.append(ty)
    nw = math.ceil(max(xs)) - math.floor(min(xs))
    nh = math.ceil(max(ys)) - math.floor(min(ys))
    m[2], m[5] = tr(-(nw - w) / 2.0, -(nh - h) / 2.0, m)
    return m, int(nw), int(nh)


def _fix16(v):
    return int(math.floor(v * 65536.0 + 0.5))


def rotate_nearest(p, m, nw, nh):
    """Pillow's affine_fixed: 16 fractional bits, outside the source gives 0"""
    H, W = p.shape[:2]
    a0, a1, a3, a4 = _fix16(m[0]), _fix16(m[1]), _fix16(m[3]), _fix16(m[4])
    a2 = _fix16(m[2] + m[0] * 0.5 + m[1] * 0.5)
    a5 = _fix16(m[5] + m[3] * 0.5 + m[4] * 0.5)
    x = np.arange(nw, dtype=np.int64)[None, :]; y = np.arange(nh, dtype=np.int64)[:, None]
    xin = (a2 + a1 * y + a0 * x) >> 16
    yin = (a5 + a4 * y + a3 * x) >> 16
    ok = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    out = p[np.clip(yin, 0, H - 1), np.clip(xin, 0, W - 1)]
    out[~ok] = 0
    return out


# ------------------------------------------------------------------------------------------------ stage 3b: shear (NOT run against cv2)
def shear_inverse(sx, sy):
    """cv2.warpAffine's inversion of M = [[1, sx, 0], [sy, 1, 0]] (float32 entries) in float64 -> the six entries of the inverse map"""
    M = [float(np.float32(1.0)), float(np.float32(sx)), 0.0, float(np.float32(sy)), float(np.float32(1.0)), 0.0]
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[4] * D, M[0] * D
    M[0] = A11; M[1] *= -D; M[3] *= -D; M[4] = A22
    b1 = -M[0] * M[2] - M[1] * M[5]
    b2 = -M[3] * M[2] - M[4] * M[5]
    return [M[0], M[1], b1, M[3], M[4], b2]


def _rne(v):
    return np.rint(v).astype(np.int64)


def shear(p, minv):
    """bilinear warp with the fixed point of tests/augment_ref.py; taps outside the patch read 0"""
    H, W = p.shape[:2]
    m = [np.float64(v) for v in minv]
    x = np.arange(W, dtype=np.float64); y = np.arange(H, dtype=np.float64)
    adelta = _rne(m[0] * x * 1024.0); bdelta = _rne(m[3] * x * 1024.0)
    X0 = _rne((m[1] * y + m[2]) * 1024.0) + 16; Y0 = _rne((m[4] * y + m[5]) * 1024.0) + 16
    X = (X0[:, None] + adelta[None, :]) >> 5; Y = (Y0[:, None] + bdelta[None, :]) >> 5
    sx, fx, sy, fy = X >> 5, (X & 31)[..., None], Y >> 5, (Y & 31)[..., None]
    I = p.astype(np.int64)

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        return np.where(ok[..., None], I[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], 0)

    acc = (32 - fx) * (32 - fy) * tap(sy, sx) + fx * (32 - fy) * tap(sy, sx + 1) + (32 - fx) * fy * tap(sy + 1, sx) + fx * fy * tap(sy + 1, sx + 1)
    return ((acc + 512) >> 10).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ stage 4: GaussianBlur
def blur_params(radius):
    """Pillow's _gaussian_blur_radius (3 passes) and the weights of ImagingHorizontalBoxBlur, in C's mixed float / double arithmetic
    -> (R, ww, fw)"""
    f32 = np.float32
    r = f32(radius)
    sigma2 = f32(f32(r * r) / f32(3))
    L = f32(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = f32(math.floor((float(L) - 1.0) / 2.0))
    a = f32(f32(f32(2) * l + f32(1)) * f32(f32(l * f32(l + f32(1))) - f32(f32(3) * sigma2)))
    a = f32(a / f32(f32(6) * f32(sigma2 - f32(f32(l + f32(1)) * f32(l + f32(1))))))
    fr = f32(l + a)
    R = int(fr)
    ww = int(f32(f32(1 << 24) / f32(f32(fr * f32(2)) + f32(1))))
    fw = (((1 << 24) - (2 * R + 1) * ww) & 0xFFFFFFFF) // 2
    return R, ww, fw


def box_blur_rows(a, R, ww, fw):
    """one extended box blur along axis 1 of int64 [rows][n][4], edges replicated"""
    n = a.shape[1]
    idx = np.arange(n)
    acc = np.zeros_like(a)
    for i in range(-R, R + 1):
        acc += a[:, np.clip(idx + i, 0, n - 1)]
    far = a[:, np.clip(idx - R - 1, 0, n - 1)] + a[:, np.clip(idx + R + 1, 0, n - 1)]
    return (ww * acc + fw * far + (1 << 23)) >> 24


def gaussian_blur(p, R, ww, fw):
    a = p.astype(np.int64)
    for _ in range(3):
        a = box_blur_rows(a, R, ww, fw)
    a = a.transpose(1, 0, 2)
    for _ in range(3):
        a = box_blur_rows(a, R, ww, fw)
    return a.transpose(1, 0, 2).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ stages 5-7
def erase(p, rects):
    p = p.copy()
    for x, y, w, h in rects:
        p[y:y + h, x:x + w, 3] = 0
    return p


def luma(p):
    I = p.astype(np.int64)
    return (19595 * I[..., 0] + 38470 * I[..., 1] + 7471 * I[..., 2] + 0x8000) >> 16


def blend(d, p, f):
    """Image.blend(degenerate, image, f) per channel value, in float32"""
    f = np.float32(f)
    d = np.asarray(d).astype(np.float32); p = np.asarray(p).astype(np.float32)
    t = d + f * (p - d)                                   # float32 products and sums, each rounded on its own
    if 0.0 <= f <= 1.0:
        return t.astype(np.int64).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int64))).astype(np.uint8)


def contrast_mean(p):
    """int(mean(L) + 0.5) over all pixels of the patch"""
    L = luma(p)
    return int(int(L.sum()) / L.size + 0.5)


def brightness(p, f):
    out = p.copy(); out[..., :3] = blend(np.zeros_like(p[..., :3]), p[..., :3], f); return out


def contrast(p, f):
    out = p.copy(); out[..., :3] = blend(np.full_like(p[..., :3], contrast_mean(p)), p[..., :3], f); return out


def color(p, f):
    out = p.copy(); out[..., :3] = blend(np.repeat(luma(p)[..., None], 3, axis=-1), p[..., :3], f); return out


def enhance(p, b, c, s):
    return color(contrast(brightness(p, b), c), s)


def opacity_lut(alpha):
    return (np.arange(256, dtype=np.uint8) * float(alpha)).astype(np.uint8)


def opacity(p, lut):
    out = p.copy(); out[..., 3] = np.asarray(lut, np.uint8)[p[..., 3]]; return out


# ------------------------------------------------------------------------------------------------ stage 8: paste
def paste(image, mask, patch, x, y):
    """in place: image uint8 (H, W, 3), mask uint8 (H, W) or None; the patch is clipped to the image"""
    H, W = image.shape[:2]
    h, w = patch.shape[:2]
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, W), min(y + h, H)
    if x1 <= x0 or y1 <= y0:
        return
    src = patch[y0 - y:y1 - y, x0 - x:x1 - x].astype(np.int64)
    a = src[..., 3:4]
    dst = image[y0:y1, x0:x1].astype(np.int64)
    t = src[..., :3] * a + dst * (255 - a) + 128
    image[y0:y1, x0:x1] = (((t >> 8) + t) >> 8).astype(np.uint8)
    if mask is not None:
        m = mask[y0:y1, x0:x1].astype(np.int64)
        t = a[..., 0] * a[..., 0] + m * (255 - a[..., 0]) + 128
        mask[y0:y1, x0:x1] = (((t >> 8) + t) >> 8).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the chain
def job_patch(logo, j):
    """stages 1-7 of one job record on its logo (uint8 (h, w, 4)) -> the RGBA patch that stage 8 pastes"""
    p = resize_rgba(logo, int(j["w1"]), int(j["h1"]))
    if j["rotate"]:
        p = rotate_nearest(p, [float(v) for v in j["rot"]], int(j["w2"]), int(j["h2"]))
    if j["stretch"]:
        p = resize_rgba(p, int(j["w3"]), int(j["h3"]))
        if j["shear"]:
            p = shear(p, [float(v) for v in j["shear_minv"]])
    if j["blur"]:
        p = gaussian_blur(p, int(j["blur_r"]), int(j["blur_ww"]), int(j["blur_fw"]))
    p = erase(p, [tuple(int(v) for v in j["defects"][i]) for i in range(int(j["ndefects"]))])
    if j["enhance"]:
        p = enhance(p, j["brightness"], j["contrast"], j["color"])
    return opacity(p, j["opacity"])


def synth_image(image, logos, jobs, skip=()):
    """one image and its K job records (applied in slot order) -> (synthesized image, pasted alpha mask); slots in `skip` are left out"""
    out = image.copy(); mask = np.zeros(image.shape[:2], np.uint8)
    for k, j in enumerate(jobs):
        if not j["enabled"] or k in skip:
            continue
        paste(out, mask, job_patch(logos[int(j["logo"])], j), int(j["x"]), int(j["y"]))
    return out, mask
