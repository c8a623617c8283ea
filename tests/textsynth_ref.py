"""numpy restatement of the text-watermark synthesis rule that csrc/synth_text_u8.hip implements (include/uwm.h): the
text branch of the reference's src/scripts/gen_data.py on the coverage plane of one text, stage by stage:

  A colour    what ImageDraw.text(fill=ink) leaves on a transparent RGBA canvas: (ink, c) where the coverage c != 0, else 0
  B rotate    Image.rotate(angle, expand=True, fillcolor=(0, 0, 0, 0)), NEAREST          (synth_ref stage 2)
  C scale     Image.resize(LANCZOS) on RGBA                                              (synth_ref stage 1)
  D blur      ImageFilter.GaussianBlur                                                   (synth_ref stage 4)
  E enhance   ImageEnhance.Brightness, then Contrast, each optional; no Color            (synth_ref stage 6)
  F opacity   a = (uint8)(a * alpha) as a table                                          (synth_ref stage 7)
  G fit       zero to three more LANCZOS resizes
  H paste     Image.paste into the image; the mask by mask_mode: 0 pastes the alpha plane over the mask, 1 halves the mask and takes
              the maximum with the alpha planes pasted from 0 (generate_mixed_watermark)

tests/test_textsynth.py compares every stage and the whole chain with Pillow bit for bit.  A job is one record of
data.TEXT_JOB_DTYPE (= uwm_text_job).  A helper of tests/test_textsynth.py and tests/test_textsynth_gpu.py, not itself a test."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_ref as S  # noqa: E402


def colour(plane, ink):
    """uint8 (h, w) coverage -> uint8 (h, w, 4)"""
    out = np.zeros(plane.shape + (4,), np.uint8)
    out[..., :3] = np.where((plane != 0)[..., None], np.asarray(ink, np.uint8), 0)
    out[..., 3] = plane
    return out


def job_patch(plane, j):
    """stages A-G of one job record on its coverage plane -> the RGBA patch that stage H pastes"""
    p = colour(plane, [int(v) for v in j["ink"]])
    if j["rotate"]:
        p = S.rotate_nearest(p, [float(v) for v in j["rot"]], int(j["w2"]), int(j["h2"]))
    if j["scale"]:
        p = S.resize_rgba(p, int(j["w3"]), int(j["h3"]))
    if j["blur"]:
        p = S.gaussian_blur(p, int(j["blur_r"]), int(j["blur_ww"]), int(j["blur_fw"]))
    if j["brighten"]:
        p = S.brightness(p, j["brightness"])
    if j["recontrast"]:
        p = S.contrast(p, j["contrast"])
    p = S.opacity(p, j["opacity"])
    for w, h in j["fit"][:int(j["nfit"])]:
        p = S.resize_rgba(p, int(w), int(h))
    return p


def halve(mask):
    """Image.blend(0, mask, 0.5) of the RGB conversions, converted back to L"""
    return mask >> 1


def synth_text_image(image, mask, planes, jobs, mask_mode=0, skip=()):
    """one image, its mask plane (or None) and its K job records (applied in slot order) -> (synthesized image, mask); slots in
    `skip` are left out.  An image without a job that runs comes back as it is, its mask too"""
    out = image.copy()
    m = None if mask is None else mask.copy()
    live = [j for k, j in enumerate(jobs) if j["enabled"] and k not in skip]
    if not live:
        return out, m
    text = None if m is None else (m if mask_mode == 0 else np.zeros_like(m))
    for j in live:
        S.paste(out, text, job_patch(planes[int(j["glyph"])], j), int(j["x"]), int(j["y"]))
    if m is not None and mask_mode == 1:
        m = np.maximum(halve(m), text)
    return out, m
