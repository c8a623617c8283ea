"""Logo-watermarked samples on the device (uwm_synth_u8, csrc/synth_u8.hip): the job record, the host arithmetic and
draws of the reference's gen_data.py, and the device call."""
import ctypes as C
import math

import numpy as np
import torch

from .. import _lib as L
from .._device import device_u8, ptr, upload_records, workspace
from .augment import IDENTITY_MINV
from .ragged import DESC_DTYPE, descs_tensor, mask_descs_for

SYNTH_JOB_DTYPE = np.dtype([("enabled", "<i4"), ("logo", "<i4"), ("w1", "<i4"), ("h1", "<i4"), ("rotate", "<i4"), ("w2", "<i4"), ("h2", "<i4"),
                            ("stretch", "<i4"), ("w3", "<i4"), ("h3", "<i4"), ("shear", "<i4"), ("blur", "<i4"), ("blur_r", "<i4"),
                            ("blur_ww", "<u4"), ("blur_fw", "<u4"), ("ndefects", "<i4"), ("defects", "<i4", (3, 4)), ("enhance", "<i4"),
                            ("brightness", "<f4"), ("contrast", "<f4"), ("color", "<f4"), ("x", "<i4"), ("y", "<i4"),
                            ("rot", "<f8", (6,)), ("shear_minv", "<f8", (6,)), ("opacity", "u1", (256,))])      # = uwm_synth_job, 488 bytes
assert SYNTH_JOB_DTYPE.itemsize == 488
SYNTH_SLOTS = 3                           # K: the reference pastes one to three logos
SYNTH_MAX_SLOTS = 8                       # what the kernels serve
SYNTH_MAX_SIDE = 32767


def empty_synth_jobs(*shape) -> np.ndarray:
    """job records with every stage off, every slot empty and the identity opacity table"""
    j = np.zeros(shape, SYNTH_JOB_DTYPE)
    j["opacity"] = np.arange(256, dtype=np.uint8)
    j["rot"] = IDENTITY_MINV; j["shear_minv"] = IDENTITY_MINV
    return j


def synth_rotate_setup(w, h, angle):
    """Image.rotate(angle, expand=True)'s host arithmetic -> (matrix of 6 floats, expanded width, expanded height)"""
    angle = angle % 360.0
    cx, cy = w / 2.0, h / 2.0
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]

    def tr(x, y):
        return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]

    m[2], m[5] = tr(-cx, -cy)
    m[2] += cx; m[5] += cy
    xs, ys = zip(*(tr(x, y) for x, y in ((0, 0), (w, 0), (w, h), (0, h))))
    nw = math.ceil(max(xs)) - math.floor(min(xs)); nh = math.ceil(max(ys)) - math.floor(min(ys))
    m[2], m[5] = tr(-(nw - w) / 2.0, -(nh - h) / 2.0)
    return m, int(nw), int(nh)


def synth_shear_inverse(sx, sy):
    """cv2.warpAffine's float64 inverse of M = [[1, sx, 0], [sy, 1, 0]] held as float32 (restated, not run against cv2)"""
    M = [1.0, float(np.float32(sx)), 0.0, float(np.float32(sy)), 1.0, 0.0]
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[4] * D, M[0] * D
    M[0] = A11; M[1] *= -D; M[3] *= -D; M[4] = A22
    return [M[0], M[1], -M[0] * M[2] - M[1] * M[5], M[3], M[4], -M[3] * M[2] - M[4] * M[5]]


def synth_blur_params(radius):
    """Pillow's _gaussian_blur_radius (3 passes) and ImagingHorizontalBoxBlur's weights, in C's float / double mix -> (R, ww, fw)"""
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
    return R, ww, (((1 << 24) - (2 * R + 1) * ww) & 0xFFFFFFFF) // 2


def synth_opacity_lut(alpha):
    return (np.arange(256, dtype=np.uint8) * float(alpha)).astype(np.uint8)


def _overlap_area(r1, r2):
    x1, y1, x2, y2 = max(r1[0], r2[0]), max(r1[1], r2[1]), min(r1[2], r2[2]), min(r1[3], r2[3])
    return (x2 - x1) * (y2 - y1) if x2 > x1 and y2 > y1 else 0


def _fitted_size(rng, lw, lh, W, H, low, high):
    """resize_watermark's draw: the logo's width a uniform share low..high of the image's, its height at most the share `high`"""
    w = int(W * rng.uniform(low, high))
    h = int(lh * w / lw)
    if h > H * high:
        h = int(H * high)
        w = int(lw * h / lh)
    return w, h


def _sample_effects(rng, jobs, k, lw, lh, W, H, enhance_transparent):
    """apply_watermark_effects' draws, in its order, into job record k -> the processed patch's (w, h), or None when a size reaches 0
    (Pillow's resize raises there and the reference goes on to the next logo; no further number is drawn)"""
    w, h = _fitted_size(rng, lw, lh, W, H, 0.03, 0.35)
    if w < 1 or h < 1:
        return None
    jobs["w1"][k], jobs["h1"][k] = w, h
    if rng.random() < 0.8:
        angle = rng.uniform(0, 360)
        if angle % 360.0 != 0.0:
            m, w, h = synth_rotate_setup(w, h, angle)
            jobs["rotate"][k], jobs["rot"][k], jobs["w2"][k], jobs["h2"][k] = 1, m, w, h
    if rng.random() < 0.75:
        hs, vs = rng.uniform(0.6, 1.6), rng.uniform(0.6, 1.6)
        w, h = int(w * hs), int(h * vs)
        if w < 1 or h < 1:
            return None
        jobs["stretch"][k], jobs["w3"][k], jobs["h3"][k] = 1, w, h
        if rng.random() < 0.6:
            sx, sy = rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4)
            jobs["shear"][k], jobs["shear_minv"][k] = 1, synth_shear_inverse(sx, sy)
    if rng.random() < 0.4:
        jobs["blur"][k] = 1
        jobs["blur_r"][k], jobs["blur_ww"][k], jobs["blur_fw"][k] = synth_blur_params(rng.uniform(0.5, 2.5))
    if rng.random() < 0.3:
        n = rng.randint(1, 3)
        for d in range(n):
            dw, dh = rng.randint(int(w * 0.05), int(w * 0.2)), rng.randint(int(h * 0.05), int(h * 0.2))
            jobs["defects"][k, d] = (rng.randint(0, max(0, w - dw)), rng.randint(0, max(0, h - dh)), dw, dh)
        jobs["ndefects"][k] = n
    alpha = rng.uniform(0.08, 0.45) if enhance_transparent else rng.uniform(0.25, 0.85)
    jobs["enhance"][k] = 1
    jobs["brightness"][k], jobs["contrast"][k], jobs["color"][k] = rng.uniform(0.4, 1.8), rng.uniform(0.5, 1.6), rng.uniform(0.5, 1.5)
    jobs["opacity"][k] = synth_opacity_lut(alpha)
    return w, h


def _plain_job(rng, jobs, k, lw, lh, W, H):
    """resize_watermark(original, size, 0.02, 0.12): job record k becomes stage 1 only -> (w, h) or None"""
    jobs[k] = empty_synth_jobs(1)[0]
    jobs["logo"][k] = k
    w, h = _fitted_size(rng, lw, lh, W, H, 0.02, 0.12)
    if w < 1 or h < 1:
        return None
    jobs["w1"][k], jobs["h1"][k] = w, h
    return w, h


def sample_synth_jobs(rng, image_size, logo_sizes, enhance_transparent=True, slots=SYNTH_SLOTS):
    """The host side of generate_multiple_watermarks_image for ONE image: `rng` a seeded random.Random (the script's own generator
    type, so uniform / randint / random mean what they mean there), image_size = (W, H), logo_sizes = [(w, h), ...] the chosen logos
    in paste order (at most `slots`).  Draws every effect parameter in the script's order, derives every size, runs the placement
    loop (20 attempts; accepted when the overlap with every placed rectangle is under 30 % of the patch, or when it is the first; an
    oversized patch falls back to the plain resize_watermark(.., 0.02, 0.12); a first logo that never fitted is placed anyway) and
    returns `slots` records of SYNTH_JOB_DTYPE whose `logo` is the index into logo_sizes.  A logo whose size reaches 0 is dropped
    (enabled = 0), as the reference's `except: continue` does."""
    W, H = int(image_size[0]), int(image_size[1])
    if len(logo_sizes) > slots:
        raise ValueError(f"sample_synth_jobs: {len(logo_sizes)} logos for {slots} slots")
    jobs = empty_synth_jobs(slots)
    placed = []
    for k, (lw, lh) in enumerate(logo_sizes):
        jobs["logo"][k] = k
        size = _sample_effects(rng, jobs, k, int(lw), int(lh), W, H, enhance_transparent)
        if size is None:
            continue
        done = False
        max_x = max_y = 0
        for _ in range(20):
            max_x, max_y = W - size[0], H - size[1]
            if max_x <= 0 or max_y <= 0:
                size = _plain_job(rng, jobs, k, int(lw), int(lh), W, H)
                if size is None:
                    break
                max_x, max_y = W - size[0], H - size[1]
            if max_x <= 0 or max_y <= 0:
                break
            x, y = rng.randint(0, max_x), rng.randint(0, max_y)
            region = (x, y, x + size[0], y + size[1])
            ratio = max([_overlap_area(region, r) / (size[0] * size[1]) for r in placed], default=0)
            if ratio < 0.3 or not placed:
                jobs["x"][k], jobs["y"][k], jobs["enabled"][k] = x, y, 1
                placed.append(region)
                done = True
                break
        if size is None:
            continue
        if not done and not placed:
            jobs["x"][k], jobs["y"][k], jobs["enabled"][k] = rng.randint(0, max(0, max_x)), rng.randint(0, max(0, max_y)), 1
    return jobs


def sample_synth_choice(rng, num_logos, transparent_ratio=0.6, multi_watermark_ratio=0.4, max_watermarks=3, transparent=None):
    """gen_data.py main()'s choices for one sample, logo branch only -> (enhance_transparent, [indices of the logos to paste]).  One
    departure: main() also makes the first count*ratio samples transparent whatever the draw; that quota needs the run's state, so
    here the draw alone decides.  transparent: that draw's result when the caller has made it already (main() makes it in front of
    the watermark-type draw, data.sample_synth_kind); it is then not made again."""
    if transparent is None:
        transparent = rng.random() < transparent_ratio
    single = rng.randrange(num_logos)
    if rng.random() < multi_watermark_ratio and num_logos > 1 and max_watermarks >= 2:
        chosen = rng.sample(range(num_logos), min(rng.randint(2, max_watermarks), num_logos))
        limit = max_watermarks
    else:
        chosen, limit = [single], 1
    n = rng.randint(1, limit)                                  # generate_multiple_watermarks_image's own count
    if len(chosen) == 1:
        picked = chosen * n
    else:
        picked = rng.sample(chosen, min(n, len(chosen)))
        while len(picked) < n:
            picked.append(rng.choice(chosen))
    return transparent, picked


def synth_job_needs(jobs, logo_descs):
    """-> (max_patch_pixels, max_taps) that uwm_synth_u8 needs to run every enabled job: the largest logo, intermediate or final patch
    and the largest coefficient table (out * (ksize + 2)), both at least 1"""
    need = [1, 1]

    def table(n_in, n_out):
        return n_out * (int(math.ceil(3.0 * max(n_in / n_out, 1.0))) * 2 + 1 + 2)

    for j in np.asarray(jobs).reshape(-1):
        if not j["enabled"] or not 0 <= int(j["logo"]) < len(logo_descs):
            continue
        w, h = int(logo_descs[int(j["logo"])]["w"]), int(logo_descs[int(j["logo"])]["h"])
        sizes = [(int(j["w1"]), int(j["h1"])), (int(j["w2"]), int(j["h2"])) if j["rotate"] else None,
                 (int(j["w3"]), int(j["h3"])) if j["stretch"] else None]
        if w < 1 or h < 1 or any(s is not None and min(s) < 1 for s in sizes):
            continue                                             # the device skips it
        need[0] = max(need[0], w * h)
        for step, s in enumerate(sizes):
            if s is None:
                continue
            if step != 1:                                        # a resize: the horizontal pass first
                if s[0] != w:
                    need[1] = max(need[1], table(w, s[0])); need[0] = max(need[0], s[0] * h)
                if s[1] != h:
                    need[1] = max(need[1], table(h, s[1]))
            need[0] = max(need[0], s[0] * s[1])
            w, h = s
    return need[0], need[1]


def device_synth(packed_images, image_descs, packed_logos, logo_descs, jobs, with_mask=False, inplace=False):
    """Paste the logos of `jobs` onto a ragged batch on the HIP device (uwm_synth_u8; the rule is in include/uwm.h).
    packed_images / image_descs: flat uint8 RGB images (pack_images); packed_logos / logo_descs: flat uint8 RGBA logos; jobs: an
    (N, K) array of SYNTH_JOB_DTYPE (sample_synth_jobs), K <= 8, whose `logo` indexes logo_descs.  -> (the synthesized batch — a copy
    unless inplace — in the layout of image_descs, the pasted alpha planes in the layout of mask_descs_for(image_descs) or None).
    The workspace is sized for this batch's jobs, allocated once per device and grown when needed.  No CPU fallback."""
    idesc, ldesc = np.ascontiguousarray(image_descs), np.ascontiguousarray(logo_descs)
    if idesc.dtype != DESC_DTYPE or ldesc.dtype != DESC_DTYPE or idesc.ndim != 1 or ldesc.ndim != 1 or len(idesc) == 0 or len(ldesc) == 0:
        raise ValueError("device_synth: image_descs and logo_descs must be non-empty 1-D data.DESC_DTYPE arrays")
    j = np.ascontiguousarray(jobs)
    if j.dtype != SYNTH_JOB_DTYPE or j.ndim != 2 or j.shape[0] != len(idesc) or not 1 <= j.shape[1] <= SYNTH_MAX_SLOTS:
        raise ValueError(f"device_synth: jobs must be an (N, K) array of data.SYNTH_JOB_DTYPE with N = {len(idesc)} images and K in 1..{SYNTH_MAX_SLOTS}")
    on = j["enabled"] != 0
    if ((j["logo"][on] < 0) | (j["logo"][on] >= len(ldesc))).any():
        raise ValueError(f"device_synth: an enabled job names a logo outside 0..{len(ldesc) - 1}")
    if (ldesc["offset"] % 4).any():
        raise ValueError("device_synth: every logo must start at a multiple of 4 bytes (pack_images does that)")
    if (j["ndefects"][on] < 0).any() or (j["ndefects"][on] > 3).any():
        raise ValueError("device_synth: ndefects must be 0..3")
    for name, t in (("packed_images", packed_images), ("packed_logos", packed_logos)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 1:
            raise RuntimeError(f"device_synth: {name} must be a flat uint8 tensor (no CPU fallback)")
    img = device_u8(packed_images, 1, "device_synth needs a HIP device (no CPU fallback)", upload=True)
    if int((idesc["offset"] + idesc["h"].astype(np.int64) * idesc["w"] * 3).max()) > img.numel():
        raise ValueError("device_synth: an image descriptor leaves packed_images")
    if int((ldesc["offset"] + ldesc["h"].astype(np.int64) * ldesc["w"] * 4).max()) > packed_logos.numel():
        raise ValueError("device_synth: a logo descriptor leaves packed_logos")
    out = img.contiguous() if inplace or img is not packed_images else img.clone()
    logos = packed_logos.to(out.device, non_blocking=True).contiguous()
    n, k = j.shape
    P, T = synth_job_needs(j, ldesc)
    md = mask_descs_for(idesc)
    mask = torch.empty(max(1, int((md["h"].astype(np.int64) * md["w"]).sum())), dtype=torch.uint8, device=out.device) if with_mask else None
    dd = descs_tensor(np.concatenate([idesc, md, ldesc]), out.device)
    jd = upload_records(j, out.device)
    step = DESC_DTYPE.itemsize
    with L.on_device(out):
        ws = workspace("synth", out.device, L.lib().uwm_synth_workspace_bytes(n, k, P, T), ValueError)
        L.check(L.lib().uwm_synth_u8(ptr(out), out.numel(), ptr(dd), ptr(mask), mask.numel() if with_mask else 0,
                                     C.c_void_p(dd.data_ptr() + n * step), ptr(logos), logos.numel(),
                                     C.c_void_p(dd.data_ptr() + 2 * n * step), len(ldesc), ptr(jd), n, k, P, T,
                                     ptr(ws), ws.numel(), C.c_void_p(L.stream_ptr(out.device))), ValueError)
    return out, mask
