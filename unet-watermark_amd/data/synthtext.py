"""Text-watermarked samples on the device (uwm_synth_text_u8, csrc/synth_text_u8.hip): the texts, the fonts and the
coverage plane a worker rasterises, the job record, the draws and sizes of the text branch of the reference's gen_data.py
(generate_text_content, apply_text_effects, generate_text_watermark), and the device call."""
import ctypes as C
import math
import os

import numpy as np
import torch

from .. import _lib as L
from .._device import device_u8, ptr, upload_records, workspace
from .augment import IDENTITY_MINV
from .ragged import DESC_DTYPE, descs_tensor, mask_descs_for
from .synth import SYNTH_MAX_SLOTS, synth_blur_params, synth_opacity_lut, synth_rotate_setup

TEXT_JOB_DTYPE = np.dtype([("enabled", "<i4"), ("glyph", "<i4"), ("ink", "<i4", (3,)), ("rotate", "<i4"), ("w2", "<i4"), ("h2", "<i4"),
                           ("scale", "<i4"), ("w3", "<i4"), ("h3", "<i4"), ("blur", "<i4"), ("blur_r", "<i4"), ("blur_ww", "<u4"),
                           ("blur_fw", "<u4"), ("brighten", "<i4"), ("recontrast", "<i4"), ("brightness", "<f4"), ("contrast", "<f4"),
                           ("nfit", "<i4"), ("fit", "<i4", (3, 2)), ("x", "<i4"), ("y", "<i4"), ("rot", "<f8", (6,)),
                           ("opacity", "u1", (256,))])      # = uwm_text_job, 416 bytes
assert TEXT_JOB_DTYPE.itemsize == 416
TEXT_MARGIN = 20                          # generate_text_watermark's margin around the text's bounding box
TEXT_INKS = ((255, 255, 255), (0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255), (0, 255, 255), (128, 128, 128))
FONT_EXTENSIONS = (".ttf", ".otf", ".ttc")
SYNTH_KINDS = ("logo", "text", "mixed")
# this project's own wording, in the kinds of the script's table: upper-case words, short phrases, URLs, CJK words and phrases, years
# and symbols, codes, mixed scripts.  --texts-file replaces it
DEFAULT_TEXTS = (
    ("STOCK", "PROOF", "ARCHIVE", "UNLICENSED", "SPECIMEN", "REVIEW", "PRIVATE", "MOCKUP"),
    ("Proof Copy", "Licensed Image", "Do Not Copy", "Stock Photo", "For Approval", "Low Resolution", "All Rights Reserved"),
    ("www.photo-archive.net", "images.studio.org", "stockpix.io", "gallery.press.com"),
    ("图库", "样张", "存档", "审阅", "授权", "私有"),
    ("图库样张", "未经授权", "请勿复制", "保留所有权利", "低分辨率预览"),
    ("2025", "©2025", "© 2019-2025", "®", "™", "№ 47", "Rev. 3", "v0.9"),
    ("#0042", "REF-7731", "ID 90210", "LOT:A17"),
    ("Proof 样张", "Stock 图库", "© 2025 图库", "ARCHIVE 存档", "授权 LICENSED"),
)


# ------------------------------------------------------------------------------------------------ texts and fonts
def load_texts(path=None):
    """-> a tuple of categories, each a tuple of texts: DEFAULT_TEXTS, or the lines of `path` (one text per line, surrounding white
    space dropped; blank lines separate categories)"""
    if path is None:
        return DEFAULT_TEXTS
    cats, cur = [], []
    with open(path, encoding="utf-8") as f:
        for line in f:
            line = line.strip()
            if line:
                cur.append(line)
            elif cur:
                cats.append(tuple(cur)); cur = []
    if cur:
        cats.append(tuple(cur))
    if not cats:
        raise ValueError(f"texts file {path} holds no text")
    return tuple(cats)


def require_freetype(what="text watermarks"):
    from PIL import features
    if not features.check("freetype2"):
        raise ValueError(f"{what} need a Pillow built with freetype (features.check('freetype2') is false here): scalable fonts cannot be "
                         "rasterised, so --text-watermark-ratio and --mixed-watermark-ratio must stay 0")


def has_cjk(text):
    return any("一" <= ch <= "鿿" for ch in text)


class FontSet:
    """The fonts a text may be drawn with: the ttf / otf / ttc files of `fonts_dir` in sorted order, or Pillow's embedded scalable font.
    Every font is opened with the BASIC layout engine, so a machine with raqm and one without render the same.  select(text) is the
    reference's select_compatible_font restated: a font is accepted when the text, drawn in black at size 24 at (10, 30) on a white
    200 x 100 canvas, leaves a mark and the variance of the grey image exceeds 50; the first accepted font wins, the first font
    otherwise.  For a text with CJK characters the fonts that accept a CJK sample are asked first (the reference asks its list of CJK
    fonts first).  Departure: the reference's list is macOS paths, and elsewhere it ends in load_default() at one small fixed size;
    here the drawn font_size is always honoured."""
    CJK_SAMPLE = "水印样本"

    def __init__(self, fonts_dir=None):
        require_freetype()
        if fonts_dir is None:
            self.paths = [None]
        else:
            if not os.path.isdir(fonts_dir):
                raise ValueError(f"fonts directory not found: {fonts_dir}")
            self.paths = [os.path.join(fonts_dir, f) for f in sorted(os.listdir(fonts_dir)) if f.lower().endswith(FONT_EXTENSIONS)]
            if not self.paths:
                raise ValueError(f"no {' / '.join(FONT_EXTENSIONS)} file in {fonts_dir}")
        self._fonts, self._accepts = {}, {}

    def font(self, index, size):
        from PIL import ImageFont
        key = (int(index), int(size))
        f = self._fonts.get(key)
        if f is None:
            path = self.paths[key[0]]
            f = ImageFont.load_default(key[1]) if path is None else ImageFont.truetype(path, key[1], layout_engine=ImageFont.Layout.BASIC)
            if len(self._fonts) >= 256:
                self._fonts.pop(next(iter(self._fonts)))
            self._fonts[key] = f
        return f

    def accepts(self, index, text):
        key = (int(index), text)
        ok = self._accepts.get(key)
        if ok is None:
            from PIL import Image, ImageDraw
            try:
                img = Image.new("RGB", (200, 100), "white")
                ImageDraw.Draw(img).text((10, 30), text, fill="black", font=self.font(index, 24))
                a = np.asarray(img)
                ok = bool((a < 255).any()) and float(np.var(np.mean(a, axis=2))) > 50
            except Exception:                                  # the reference's probe swallows a font that cannot draw the text
                ok = False
            self._accepts[key] = ok
        return ok

    def select(self, text):
        """-> the index of the font `text` is drawn with"""
        order = list(range(len(self.paths)))
        if has_cjk(text):
            order.sort(key=lambda i: not self.accepts(i, self.CJK_SAMPLE))      # stable: CJK-capable fonts first, each group in order
        for i in order:
            if self.accepts(i, text):
                return i
        return 0


def render_text_plane(text, font) -> np.ndarray:
    """The coverage plane of `text`: uint8 (ch, cw), the canvas of generate_text_watermark — the text's textbbox size plus a margin of
    20 on every side, the text drawn at (20, 20).  What ImageDraw.text(fill=ink) leaves on a transparent RGBA canvas of that size is
    (ink, coverage) where coverage != 0 and (0, 0, 0, 0) elsewhere (stage A of uwm_synth_text_u8; tests/test_textsynth.py holds it to
    Pillow); coverage is font.getmask2(text, 'L') at the draw position plus its offset, clipped — which is what drawing with fill 255
    on a zeroed 'L' canvas gives.  An empty text gives an all-zero 40 x 40 plane."""
    from PIL import Image, ImageDraw
    box = ImageDraw.Draw(Image.new("RGBA", (1, 1))).textbbox((0, 0), text, font=font)
    cw, ch = int(box[2] - box[0]) + 2 * TEXT_MARGIN, int(box[3] - box[1]) + 2 * TEXT_MARGIN
    canvas = Image.new("L", (cw, ch), 0)
    if text:
        ImageDraw.Draw(canvas).text((TEXT_MARGIN, TEXT_MARGIN), text, fill=255, font=font)
    return np.asarray(canvas, dtype=np.uint8).copy()


# ------------------------------------------------------------------------------------------------ the draws
def empty_text_jobs(*shape) -> np.ndarray:
    """job records with every stage off, every slot empty and the identity opacity table"""
    j = np.zeros(shape, TEXT_JOB_DTYPE)
    j["opacity"] = np.arange(256, dtype=np.uint8)
    j["rot"] = IDENTITY_MINV
    return j


def sample_synth_kind(rng, text_ratio, mixed_ratio) -> str:
    """main()'s watermark-type choice: one draw and the script's two comparisons -> 'logo' | 'text' | 'mixed'.  With both ratios 0 no
    number is drawn, so every logo sample stays what it is.  Departure (as sample_synth_choice's for transparency): the script also
    stops a type at count * ratio samples; that quota needs the run's state, so here the draw alone decides."""
    if text_ratio == 0 and mixed_ratio == 0:
        return "logo"
    r = rng.random()
    if r < text_ratio:
        return "text"
    if r < text_ratio + mixed_ratio:
        return "mixed"
    return "logo"


def sample_text(rng, texts=DEFAULT_TEXTS) -> str:
    """generate_text_content: a category, then a text of it"""
    return rng.choice(rng.choice(texts))


def sample_font_size(rng, image_size) -> int:
    m = min(int(image_size[0]), int(image_size[1]))
    return rng.randint(max(20, int(m * 0.03)), max(60, int(m * 0.15)))


def sample_text_job(rng, image_size, plane_size, enhance_transparent=True, glyph=0):
    """generate_text_watermark from its colour draw on, for ONE text whose coverage plane is plane_size = (cw, ch) on an image of
    image_size = (W, H): `rng` a seeded random.Random.  Draws, in the script's order: the ink (one of nine); rotation (p 0.7, -45..45
    degrees, expand); scale (p 0.6, 0.8..1.4 per axis); blur (p 0.3, radius 0.5..1.5); opacity (0.1..0.5 transparent, 0.3..0.8
    otherwise); brightness (p 0.5, 0.6..1.4); contrast (p 0.5, 0.7..1.3); then derives the fit sizes (wider than 0.8 W; taller than
    0.8 H; no room left: min(W / w, H / h) * 0.8), every size with the script's int() truncations, and draws the position.
    -> one record of TEXT_JOB_DTYPE, or None when a size reaches 0 (Pillow's resize raises there and the script skips the sample).
    The draws in front of this one are sample_text (category, text) and sample_font_size."""
    W, H = int(image_size[0]), int(image_size[1])
    w, h = int(plane_size[0]), int(plane_size[1])
    j = empty_text_jobs(1)[0]
    j["glyph"] = glyph
    j["ink"] = rng.choice(TEXT_INKS)
    if rng.random() < 0.7:
        angle = rng.uniform(-45, 45)
        if angle % 360.0 != 0.0:
            m, w, h = synth_rotate_setup(w, h, angle)
            j["rotate"], j["rot"], j["w2"], j["h2"] = 1, m, w, h
    if rng.random() < 0.6:
        sx, sy = rng.uniform(0.8, 1.4), rng.uniform(0.8, 1.4)
        w, h = int(w * sx), int(h * sy)
        if w < 1 or h < 1:
            return None
        j["scale"], j["w3"], j["h3"] = 1, w, h
    if rng.random() < 0.3:
        j["blur"] = 1
        j["blur_r"], j["blur_ww"], j["blur_fw"] = synth_blur_params(rng.uniform(0.5, 1.5))
    alpha = rng.uniform(0.1, 0.5) if enhance_transparent else rng.uniform(0.3, 0.8)
    if rng.random() < 0.5:
        j["brighten"], j["brightness"] = 1, rng.uniform(0.6, 1.4)
    if rng.random() < 0.5:
        j["recontrast"], j["contrast"] = 1, rng.uniform(0.7, 1.3)
    j["opacity"] = synth_opacity_lut(alpha)
    fits = []
    if w > W * 0.8:
        s = (W * 0.8) / w
        w, h = int(w * s), int(h * s); fits.append((w, h))
    if min(w, h) >= 1 and h > H * 0.8:
        s = (H * 0.8) / h
        w, h = int(w * s), int(h * s); fits.append((w, h))
    if min(w, h) >= 1 and (W - w <= 0 or H - h <= 0):
        s = min(W / w, H / h) * 0.8
        w, h = int(w * s), int(h * s); fits.append((w, h))
    if w < 1 or h < 1:
        return None
    j["nfit"] = len(fits)
    for f, size in enumerate(fits):
        j["fit"][f] = size
    j["x"], j["y"] = rng.randint(0, max(0, W - w)), rng.randint(0, max(0, H - h))
    j["enabled"] = 1
    return j


def sample_text_item(rng, image_size, texts, fonts, enhance_transparent=True):
    """every draw of one text watermark in the script's order, and the host rasterisation between them
    -> (coverage plane, one record of TEXT_JOB_DTYPE with glyph 0; enabled 0 when the job was dropped)"""
    text = sample_text(rng, texts)
    size = sample_font_size(rng, image_size)
    plane = render_text_plane(text, fonts.font(fonts.select(text), size))
    job = sample_text_job(rng, image_size, (plane.shape[1], plane.shape[0]), enhance_transparent)
    return plane, (job if job is not None else empty_text_jobs(1)[0])


def text_job_final_size(job, plane_size):
    """-> (w, h) of the patch stage H pastes"""
    w, h = int(plane_size[0]), int(plane_size[1])
    if job["rotate"]:
        w, h = int(job["w2"]), int(job["h2"])
    if job["scale"]:
        w, h = int(job["w3"]), int(job["h3"])
    if job["nfit"]:
        w, h = (int(v) for v in job["fit"][int(job["nfit"]) - 1])
    return w, h


def text_job_needs(jobs, plane_descs):
    """-> (max_patch_pixels, max_taps) that uwm_synth_text_u8 needs to run every enabled job: the largest plane, intermediate or final
    patch and the largest coefficient table (out * (ksize + 2)), both at least 1"""
    need = [1, 1]

    def table(n_in, n_out):
        return n_out * (int(math.ceil(3.0 * max(n_in / n_out, 1.0))) * 2 + 1 + 2)

    for j in np.asarray(jobs).reshape(-1):
        if not j["enabled"] or not 0 <= int(j["glyph"]) < len(plane_descs) or not 0 <= int(j["nfit"]) <= 3:
            continue
        w, h = int(plane_descs[int(j["glyph"])]["w"]), int(plane_descs[int(j["glyph"])]["h"])
        steps = [("rot", int(j["w2"]), int(j["h2"]))] if j["rotate"] else []
        steps += [("resize", int(j["w3"]), int(j["h3"]))] if j["scale"] else []
        steps += [("resize", int(s[0]), int(s[1])) for s in j["fit"][:int(j["nfit"])]]
        if w < 1 or h < 1 or any(min(s[1], s[2]) < 1 for s in steps):
            continue                                             # the device skips it
        need[0] = max(need[0], w * h)
        for what, tw, th in steps:
            if what == "resize":                                 # the horizontal pass first
                if tw != w:
                    need[1] = max(need[1], table(w, tw)); need[0] = max(need[0], tw * h)
                if th != h:
                    need[1] = max(need[1], table(h, th))
            need[0] = max(need[0], tw * th)
            w, h = tw, th
    return need[0], need[1]


# ------------------------------------------------------------------------------------------------ the device call
def device_synth_text(packed_images, image_descs, packed_planes, plane_descs, jobs, masks=None, mask_mode=0, inplace=False):
    """Paste the texts of `jobs` onto a ragged batch on the HIP device (uwm_synth_text_u8; the rule is in include/uwm.h).
    packed_images / image_descs: flat uint8 RGB images (pack_images); packed_planes / plane_descs: flat uint8 one-channel coverage
    planes (render_text_plane, packed with pack_images); jobs: an (N, K) array of TEXT_JOB_DTYPE (sample_text_job), K <= 8, whose
    `glyph` indexes plane_descs.  masks: None, or a flat uint8 tensor of mask planes in the layout of mask_descs_for(image_descs), or
    True for zeroed planes; mask_mode 0 pastes the text alpha over the planes, 1 applies the mixed rule (halve, then the maximum with
    the text alpha).  An image without a text that runs is left as it is, its mask plane too.  -> (the batch, the mask planes or
    None), copies unless inplace.  The workspace is sized for this batch's jobs.  No CPU fallback."""
    idesc, pdesc = np.ascontiguousarray(image_descs), np.ascontiguousarray(plane_descs)
    if idesc.dtype != DESC_DTYPE or pdesc.dtype != DESC_DTYPE or idesc.ndim != 1 or pdesc.ndim != 1 or len(idesc) == 0 or len(pdesc) == 0:
        raise ValueError("device_synth_text: image_descs and plane_descs must be non-empty 1-D data.DESC_DTYPE arrays")
    j = np.ascontiguousarray(jobs)
    if j.dtype != TEXT_JOB_DTYPE or j.ndim != 2 or j.shape[0] != len(idesc) or not 1 <= j.shape[1] <= SYNTH_MAX_SLOTS:
        raise ValueError(f"device_synth_text: jobs must be an (N, K) array of data.TEXT_JOB_DTYPE with N = {len(idesc)} images and K in 1..{SYNTH_MAX_SLOTS}")
    if mask_mode not in (0, 1):
        raise ValueError(f"device_synth_text: mask_mode must be 0 (paste) or 1 (mixed) (got {mask_mode!r})")
    on = j["enabled"] != 0
    if ((j["glyph"][on] < 0) | (j["glyph"][on] >= len(pdesc))).any():
        raise ValueError(f"device_synth_text: an enabled job names a plane outside 0..{len(pdesc) - 1}")
    if (pdesc["offset"] % 4).any():
        raise ValueError("device_synth_text: every plane must start at a multiple of 4 bytes (pack_images does that)")
    if (j["nfit"][on] < 0).any() or (j["nfit"][on] > 3).any():
        raise ValueError("device_synth_text: nfit must be 0..3")
    for name, t in (("packed_images", packed_images), ("packed_planes", packed_planes)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 1:
            raise RuntimeError(f"device_synth_text: {name} must be a flat uint8 tensor (no CPU fallback)")
    md = mask_descs_for(idesc)
    mbytes = max(1, int((md["h"].astype(np.int64) * md["w"]).sum()))
    if masks is not None and masks is not True and (not isinstance(masks, torch.Tensor) or masks.dtype != torch.uint8 or masks.dim() != 1 or
                                                    masks.numel() < mbytes):
        raise RuntimeError(f"device_synth_text: masks must be None, True or a flat uint8 tensor of at least {mbytes} bytes")
    img = device_u8(packed_images, 1, "device_synth_text needs a HIP device (no CPU fallback)", upload=True)
    if int((idesc["offset"] + idesc["h"].astype(np.int64) * idesc["w"] * 3).max()) > img.numel():
        raise ValueError("device_synth_text: an image descriptor leaves packed_images")
    if int((pdesc["offset"] + pdesc["h"].astype(np.int64) * pdesc["w"]).max()) > packed_planes.numel():
        raise ValueError("device_synth_text: a plane descriptor leaves packed_planes")
    out = img.contiguous() if inplace or img is not packed_images else img.clone()
    planes = packed_planes.to(out.device, non_blocking=True).contiguous()
    if masks is True:
        mask = torch.zeros(mbytes, dtype=torch.uint8, device=out.device)
    elif masks is not None:
        m = masks.to(out.device, non_blocking=True).contiguous()
        mask = m if inplace or m is not masks else m.clone()
    else:
        mask = None
    n, k = j.shape
    P, T = text_job_needs(j, pdesc)
    dd = descs_tensor(np.concatenate([idesc, md, pdesc]), out.device)
    jd = upload_records(j, out.device)
    step = DESC_DTYPE.itemsize
    with L.on_device(out):
        ws = workspace("synth_text", out.device, L.lib().uwm_synth_text_workspace_bytes(n, k, P, T), ValueError)
        L.check(L.lib().uwm_synth_text_u8(ptr(out), out.numel(), ptr(dd), ptr(mask), mask.numel() if mask is not None else 0,
                                          C.c_void_p(dd.data_ptr() + n * step), int(mask_mode), ptr(planes), planes.numel(),
                                          C.c_void_p(dd.data_ptr() + 2 * n * step), len(pdesc), ptr(jd), n, k, P, T,
                                          ptr(ws), ws.numel(), C.c_void_p(L.stream_ptr(out.device))), ValueError)
    return out, mask
