"""The datasets: tensors with the contract of the reference's dataset (/root/reference/src/utils/dataset.py:113-122,332-333,389-395)
— image fp32 NCHW normalised with the ImageNet mean/std, mask int64 {0,1} (H,W) — from a synthetic generator or a plain PIL folder
reader, and the raw ones that only decode files and leave resize, masks from pairs, logo synthesis, augmentation and Normalize to
the device (DeviceInputPipeline)."""
import os

import numpy as np
import torch
from torch.utils.data import Dataset

from ..constants import IMAGENET_MEAN, IMAGENET_STD
from .jpegragged import check_jpeg_quality
from .synth import SYNTH_SLOTS, sample_synth_choice, sample_synth_jobs
from .synthtext import FontSet, empty_text_jobs, load_texts, sample_synth_kind, sample_text_item

FOLDER_IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg")                             # FolderDataset / RawFolderDataset
PAIR_IMAGE_EXTENSIONS = (".jpg", ".jpeg", ".png", ".bmp", ".tiff", ".tif")      # the reference's _collect_image_files
LOGO_SUBDIRS = ("combined", "independent", "car_logo")        # gen_data.py's load_watermarks
LOGO_EXTENSIONS = (".png", ".jpg", ".jpeg")


def list_files(directory, extensions):
    """the paths of the files of `directory` whose names end in one of `extensions` (any letter case), sorted"""
    return [os.path.join(directory, f) for f in sorted(os.listdir(directory)) if f.lower().endswith(extensions)]


def read_u8(path, mode) -> np.ndarray:
    """the image file decoded to `mode` ('RGB', 'RGBA', 'L') as a uint8 array"""
    from PIL import Image
    return np.asarray(Image.open(path).convert(mode), dtype=np.uint8)


def mask_path(root, image_path):
    """<root>/masks/<the image's stem>.png"""
    return os.path.join(root, "masks", os.path.splitext(os.path.basename(image_path))[0] + ".png")


def normalized(img):
    """(3, H, W) fp32 in 0..1 -> Normalize with the ImageNet mean / std"""
    mean = torch.tensor(IMAGENET_MEAN).view(3, 1, 1); std = torch.tensor(IMAGENET_STD).view(3, 1, 1)
    return (img - mean) / std


class SyntheticWatermarkDataset(Dataset):
    """Smooth random backgrounds with a semi-transparent rectangular 'watermark'; mask = its footprint."""

    def __init__(self, length=256, img_size=512, seed=42):
        self.length, self.size, self.seed = int(length), int(img_size), int(seed)

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed * 100003 + i)
        s = self.size
        base = torch.rand(3, s // 16, s // 16, generator=g)
        img = torch.nn.functional.interpolate(base[None], size=(s, s), mode="bilinear", align_corners=False)[0]
        rh = int(torch.randint(s // 8, s // 2, (), generator=g)); rw = int(torch.randint(s // 8, s // 2, (), generator=g))
        y0 = int(torch.randint(0, s - rh, (), generator=g)); x0 = int(torch.randint(0, s - rw, (), generator=g))
        alpha = 0.3 + 0.4 * float(torch.rand((), generator=g))
        img[:, y0:y0 + rh, x0:x0 + rw] = (1 - alpha) * img[:, y0:y0 + rh, x0:x0 + rw] + alpha
        mask = torch.zeros(s, s, dtype=torch.int64)
        mask[y0:y0 + rh, x0:x0 + rw] = 1
        return normalized(img), mask


class FolderDataset(Dataset):
    """<root>/watermarked/*.{png,jpg} + <root>/masks/<same stem>.png (the reference's layout, dataset.py:60-84)."""

    def __init__(self, root, img_size=512):
        from PIL import Image  # noqa: F401
        self.root, self.size = root, int(img_size)
        self.files = [os.path.basename(p) for p in list_files(os.path.join(root, "watermarked"), FOLDER_IMAGE_EXTENSIONS)]

    def __len__(self):
        return len(self.files)

    def __getitem__(self, i):
        from PIL import Image
        path = os.path.join(self.root, "watermarked", self.files[i])
        img = Image.open(path).convert("RGB").resize((self.size, self.size), Image.BILINEAR)
        m = Image.open(mask_path(self.root, path)).convert("L").resize((self.size, self.size), Image.NEAREST)
        x = torch.from_numpy(np.asarray(img, dtype=np.float32) / 255.0).permute(2, 0, 1)
        return normalized(x), torch.from_numpy((np.asarray(m) > 127).astype(np.int64))


class RawFolderDataset(Dataset):
    """FolderDataset's files, decoded and nothing else: (image uint8 (h, w, 3) RGB, mask uint8 (h, w)) numpy arrays at the file's
    own size.  Resize, augmentation and Normalize happen on the device (DeviceInputPipeline)."""

    def __init__(self, root):
        from PIL import Image  # noqa: F401
        self.root = root
        self.files = [os.path.basename(p) for p in list_files(os.path.join(root, "watermarked"), FOLDER_IMAGE_EXTENSIONS)]

    def __len__(self):
        return len(self.files)

    def __getitem__(self, i):
        path = os.path.join(self.root, "watermarked", self.files[i])
        return read_u8(path, "RGB"), read_u8(mask_path(self.root, path), "L")


class RawPairDataset(Dataset):
    """The reference's dataset contract, decoded and nothing else: roots = [DATA.ROOT_DIR] + DATA.ADDITIONAL_ROOT_DIRS, each with
    watermarked/, clean/ and masks/.  The file list is every image file of every watermarked/ directory, sorted by path
    (dataset.py:57-69).  An image's mask is <stem>.png in the FIRST masks/ directory (in root order) that has a readable one; failing
    that, its clean counterpart is the file of the SAME NAME in the first clean/ directory that has a readable one
    (dataset.py:158-195).  Items are (image uint8 (h, w, 3) RGB, mask uint8 (h, w) or None, clean uint8 (h', w', 3) or None); the
    clean image is only read when there is no mask.  DeviceInputPipeline derives the missing masks on the device with
    `mask_threshold` (DATA.GENERATE_MASK_THRESHOLD); an image with neither gets a zero mask."""

    def __init__(self, roots, mask_threshold):
        from PIL import Image  # noqa: F401
        self.roots = [roots] if isinstance(roots, (str, os.PathLike)) else list(roots)
        if not self.roots:
            raise ValueError("RawPairDataset: no root directory")
        self.mask_threshold = int(mask_threshold)
        if not 0 <= self.mask_threshold <= 255:
            raise ValueError(f"RawPairDataset: mask_threshold must be 0..255 (got {mask_threshold})")
        dirs = [os.path.join(root, "watermarked") for root in self.roots]
        self.files = sorted(p for d in dirs if os.path.isdir(d) for p in list_files(d, PAIR_IMAGE_EXTENSIONS))
        self.mask_dirs = [os.path.join(r, "masks") for r in self.roots]
        self.clean_dirs = [os.path.join(r, "clean") for r in self.roots]

    def __len__(self):
        return len(self.files)

    def mask_paths(self, i):
        """the existing mask files of image i, in lookup order"""
        name = os.path.splitext(os.path.basename(self.files[i]))[0] + ".png"
        return [p for p in (os.path.join(d, name) for d in self.mask_dirs) if os.path.exists(p)]

    def clean_paths(self, i):
        name = os.path.basename(self.files[i])
        return [p for p in (os.path.join(d, name) for d in self.clean_dirs) if os.path.exists(p)]

    def missing_masks(self):
        """indices of the images without a mask file"""
        return [i for i in range(len(self.files)) if not self.mask_paths(i)]

    @staticmethod
    def _read(paths, mode):
        for p in paths:
            try:
                return read_u8(p, mode)
            except (OSError, ValueError):          # unreadable: the reference goes on to the next directory
                continue
        return None

    def __getitem__(self, i):
        img = read_u8(self.files[i], "RGB")
        m = self._read(self.mask_paths(i), "L")
        clean = self._read(self.clean_paths(i), "RGB") if m is None else None
        return img, m, clean


class DeviceU8Dataset(Dataset):
    """A dataset of (normalised fp32 image, {0,1} mask) pairs (SyntheticWatermarkDataset) converted ONCE to uint8 tensors on the
    device: images (n, S, S, C), masks (n, S, S) in {0, 255}.  Items are indices; DeviceInputPipeline gathers them on the device."""

    def __init__(self, base, device, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        xs, ms = zip(*(base[i] for i in range(len(base))))
        x = torch.stack(xs).to(device)
        c = x.shape[1]
        mean_t = torch.tensor(mean[:c], device=device).view(1, c, 1, 1); std_t = torch.tensor(std[:c], device=device).view(1, c, 1, 1)
        self.images = ((x * std_t + mean_t) * 255.0).round_().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        self.masks = (torch.stack(ms).to(device) > 0).to(torch.uint8) * 255

    def __len__(self):
        return self.images.shape[0]

    def __getitem__(self, i):
        return int(i)


def list_logos(logos_dir):
    """gen_data.py's load_watermarks: the image files of combined/, independent/ and car_logo/; a flat directory of logos also works"""
    files = []
    for sub in LOGO_SUBDIRS:
        d = os.path.join(logos_dir, sub)
        if os.path.isdir(d):
            files += list_files(d, LOGO_EXTENSIONS)
    if not files and os.path.isdir(logos_dir):
        files = list_files(logos_dir, LOGO_EXTENSIONS)
    return files


class RawSynthDataset(Dataset):
    """Clean photographs + a directory of logos -> the items the device turns into training pairs: (clean uint8 (h, w, 3) RGB,
    [logo uint8 (h', w', 4) RGBA, ...], jobs [SYNTH_SLOTS] of SYNTH_JOB_DTYPE).  Workers only decode and draw numbers
    (sample_synth_choice, sample_synth_jobs); DeviceInputPipeline pastes the logos with uwm_synth_u8 and derives the masks.  The
    draws of item i are a function of (seed, epoch, i): set_epoch(e) before an epoch's loader is made gives that epoch new samples,
    and a dataset that is never told the epoch (a validation split) reproduces its samples every time.  Decoded logos are kept in a
    per-process LRU of `cache` entries.

    text_watermark_ratio / mixed_watermark_ratio (the reference's defaults are 0.3 / 0.2; 0 / 0 here, so that a dataset made without
    them yields what it always has): the shares of samples that carry a text, or one or two logos and a text (sample_synth_kind).
    With either above 0 an item is (clean, logos, jobs, planes, text_jobs): planes a list of at most one uint8 (ch, cw) coverage
    plane that the worker rasterised (render_text_plane; fonts of fonts_dir or Pillow's embedded one, texts of texts_file or
    DEFAULT_TEXTS), text_jobs [1] of TEXT_JOB_DTYPE; a text sample has no logo job, a logo sample no text job.  With both 0 nothing
    more is drawn and items are the three-tuples above.

    jpeg_quality (the reference saves at 95; 0 here = no round trip, so that a dataset made without it yields what it always has): the
    items stay what they are; DeviceInputPipeline sends every synthesized image through uwm_jpeg_ragged_u8 at this quality behind the
    last stage — in front of the masks from pairs, as the reference's dataset sees its files — and a mixed sample once more between its
    logos and its text (the temporary file the script writes there)."""

    def __init__(self, clean_dir, logos_dir, seed=42, transparent_ratio=0.6, multi_watermark_ratio=0.4, max_watermarks=3,
                 mask_threshold=None, mask_source="pair", cache=64, text_watermark_ratio=0.0, mixed_watermark_ratio=0.0, fonts_dir=None,
                 texts_file=None, jpeg_quality=0):
        from PIL import Image  # noqa: F401
        self.jpeg_quality = check_jpeg_quality(jpeg_quality, "RawSynthDataset: jpeg_quality")
        self.text_ratio, self.mixed_ratio = check_synth_ratios(text_watermark_ratio, mixed_watermark_ratio)
        if not os.path.isdir(clean_dir):
            raise ValueError(f"RawSynthDataset: clean directory not found: {clean_dir}")
        self.files = list_files(clean_dir, LOGO_EXTENSIONS)
        self.logos = list_logos(logos_dir) if logos_dir is not None else []
        if not self.files or (not self.logos and self.text_ratio < 1):
            raise ValueError(f"RawSynthDataset: {len(self.files)} clean images in {clean_dir}, {len(self.logos)} logos in {logos_dir}: need both")
        if not 1 <= int(max_watermarks) <= SYNTH_SLOTS:
            raise ValueError(f"RawSynthDataset: max_watermarks must be 1..{SYNTH_SLOTS} (got {max_watermarks})")
        if mask_source not in ("pair", "alpha"):
            raise ValueError(f"RawSynthDataset: mask_source must be 'pair' or 'alpha' (got {mask_source!r})")
        self.seed, self.epoch = int(seed), 0
        self.transparent_ratio, self.multi_watermark_ratio = float(transparent_ratio), float(multi_watermark_ratio)
        self.max_watermarks, self.mask_threshold, self.mask_source = int(max_watermarks), mask_threshold, mask_source
        self.cache = int(cache)
        self._lru = {}
        self.with_text = self.text_ratio > 0 or self.mixed_ratio > 0
        if self.with_text:                                   # refused here, before any device work, where freetype is missing
            self.fonts, self.texts = FontSet(fonts_dir), load_texts(texts_file)

    def __len__(self):
        return len(self.files)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def _logo(self, i):
        a = self._lru.pop(i, None)
        if a is None:
            a = read_u8(self.logos[i], "RGBA")
            if len(self._lru) >= self.cache:
                self._lru.pop(next(iter(self._lru)))
        self._lru[i] = a                                     # most recently used last
        return a

    def draw(self, i, image_size):
        """-> (enhance_transparent, logo indices, decoded logos, jobs) of item i at this epoch"""
        return self.draw_sample(i, image_size)[:4]

    def draw_sample(self, i, image_size):
        """-> (enhance_transparent, logo indices, decoded logos, jobs, kind, planes, text_jobs) of item i at this epoch, in main()'s
        order: transparency, the watermark type, then the type's own draws (mixed: the logos with max_watermarks 2, then the text)"""
        import random
        rng = random.Random(f"uwm-synth:{self.seed}:{self.epoch}:{int(i)}")
        transparent = rng.random() < self.transparent_ratio
        kind = sample_synth_kind(rng, self.text_ratio, self.mixed_ratio)
        picked = []
        if kind != "text":
            picked = sample_synth_choice(rng, len(self.logos), self.transparent_ratio, self.multi_watermark_ratio,
                                         self.max_watermarks if kind == "logo" else min(2, self.max_watermarks), transparent=transparent)[1]
        logos = [self._logo(k) for k in picked]
        jobs = sample_synth_jobs(rng, image_size, [(a.shape[1], a.shape[0]) for a in logos], transparent)
        planes, text_jobs = [], empty_text_jobs(1)
        if kind != "logo":
            plane, text_jobs[0] = sample_text_item(rng, image_size, self.texts, self.fonts, transparent)
            planes = [plane]
        return transparent, picked, logos, jobs, kind, planes, text_jobs

    def __getitem__(self, i):
        clean = read_u8(self.files[i], "RGB")
        _, _, logos, jobs, _, planes, text_jobs = self.draw_sample(i, (clean.shape[1], clean.shape[0]))
        return (clean, logos, jobs, planes, text_jobs) if self.with_text else (clean, logos, jobs)


def check_synth_ratios(text_ratio, mixed_ratio):
    """-> the two ratios as floats; ValueError unless each is in [0, 1] and their sum at most 1"""
    t, m = float(text_ratio), float(mixed_ratio)
    if not (0.0 <= t <= 1.0 and 0.0 <= m <= 1.0) or t + m > 1.0:
        raise ValueError(f"text_watermark_ratio and mixed_watermark_ratio must each be in [0, 1] and sum to at most 1 (got {text_ratio}, {mixed_ratio})")
    return t, m


def list_collate(batch):
    """keeps the items as they are: raw images differ in size, so there is nothing to stack"""
    return list(batch)
