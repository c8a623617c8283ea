"""Sort a folder by predicted watermark area — counterpart of the reference's src/scripts/watermark_filter.py (WatermarkFilter):
every image's mask is predicted, and images whose mask covers less than `watermark_threshold` of the image are moved away or
deleted.  The reference runs one image at a time and brings every probability map to the host; here a batch goes through ONE
captured library call (WatermarkPredictor.watermark_counts -> uwm_filter_images_u8) that returns two integers per image.

The mask rule is watermark_filter.py's own and differs from predict's: sigmoid, THEN cv2-style bilinear resize of the probabilities
to the image's size, > PREDICT.THRESHOLD, and under PREDICT.POST_PROCESS an open and a close with the 3 x 3 ellipse.

Two deliberate departures from the reference:
  * an image that cannot be read (or whose count comes back as {0, 0}) is counted under `errors` and STAYS where it is; the reference
    catches the exception, reports (False, 0.0), and then moves or deletes the file as "no watermark";
  * files are deleted only with delete=True (`--delete`); the reference deletes whenever no target directory is given.  With neither
    a directory nor delete, a run only reports."""
from __future__ import annotations

import os
import shutil
from pathlib import Path
from typing import Optional

import numpy as np

IMAGE_EXTENSIONS = (".jpg", ".jpeg", ".png", ".bmp", ".tiff", ".tif")      # the reference's list; both letter cases are looked for


def list_images(input_dir) -> list:
    """the reference's file list: *<ext> and *<EXT> for every extension, in its order (a file is listed once)"""
    files, seen = [], set()
    for ext in IMAGE_EXTENSIONS:
        for pattern in (f"*{ext}", f"*{ext.upper()}"):
            for p in sorted(Path(input_dir).glob(pattern)):
                if p not in seen:
                    seen.add(p)
                    files.append(p)
    return files


def load_rgb(path) -> np.ndarray:
    """decode to uint8 (h, w, 3) RGB, as `main.py predict` does"""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def watermark_ratio(watermark_pixels: int, total_pixels: int) -> float:
    """the reference's arithmetic, in Python numbers: np.sum(mask > 0) / (h * w)"""
    if total_pixels <= 0:
        raise ValueError("the image was not counted")
    return int(watermark_pixels) / int(total_pixels)


def batch_ratios(paths, counts_fn, batch_size: int) -> list:
    """per path: its watermark ratio, or the exception that kept the image from being counted (left to the caller to report).
    counts_fn(images, full) -> (n, 2) integers {watermark pixels, h * w} for a list of decoded images; `full` says that the batch
    has batch_size images (those replay one captured graph; only the last, short batch runs without it)."""
    out = []
    for b in range(0, len(paths), batch_size):
        res, images = [], []
        for p in paths[b:b + batch_size]:
            try:
                images.append(load_rgb(p)); res.append(None)
            except Exception as e:      # noqa: BLE001  (an undecodable file is reported, not fatal)
                res.append(e)
        if images:
            counts = iter(counts_fn(images, len(images) == batch_size))
            for k, r in enumerate(res):
                if r is None:
                    c = next(counts)
                    try:
                        res[k] = watermark_ratio(c[0], c[1])
                    except ValueError as e:
                        res[k] = e
        out.extend(res)
    return out


def filter_folder(input_dir, ratios_fn, watermark_threshold: float, no_watermark_dir=None, dry_run: bool = False, delete: bool = False,
                  log=print) -> dict:
    """The reference's filter_images on ratios_fn(paths) -> per path a ratio or an exception.  -> {'total', 'with_watermark',
    'without_watermark', 'moved', 'errors'} ('moved' also counts deleted files, as there).  ratio >= watermark_threshold keeps the
    file; the others go to no_watermark_dir, or are deleted with delete=True; with neither, and in a dry run, nothing is touched.
    An image without a ratio counts under 'errors' and stays."""
    if no_watermark_dir and delete:
        raise ValueError("filter_images: give no_watermark_dir or delete=True, not both")
    log = log or (lambda *a: None)
    files = list_images(input_dir)
    stats = {"total": len(files), "with_watermark": 0, "without_watermark": 0, "moved": 0, "errors": 0}
    if not files:
        log(f"no image files in {input_dir}")
        return stats
    if no_watermark_dir and not dry_run:
        os.makedirs(no_watermark_dir, exist_ok=True)
    action = "move" if no_watermark_dir else "delete" if delete else None
    for path, ratio in zip(files, ratios_fn(files)):
        if isinstance(ratio, Exception):
            stats["errors"] += 1
            log(f"error: {path.name}: {ratio} (left in place)")
            continue
        if ratio >= watermark_threshold:
            stats["with_watermark"] += 1
            log(f"keep: {path.name} (watermark ratio: {ratio:.6f})")
            continue
        stats["without_watermark"] += 1
        try:
            if action is None:
                log(f"no watermark: {path.name} (watermark ratio: {ratio:.6f})")
            elif dry_run:
                log(f"[dry run] would {action}: {path.name} (watermark ratio: {ratio:.6f})")
            elif action == "move":
                target = os.path.join(no_watermark_dir, path.name)
                shutil.move(str(path), target)
                stats["moved"] += 1
                log(f"move: {path.name} -> {target} (watermark ratio: {ratio:.6f})")
            else:
                os.remove(str(path))
                stats["moved"] += 1
                log(f"delete: {path.name} (watermark ratio: {ratio:.6f})")
        except OSError as e:
            stats["errors"] += 1
            log(f"error: {path.name}: {e}")
    return stats


class WatermarkFilter:
    def __init__(self, model_path: Optional[str], config_path: Optional[str] = None, device: str = "auto", watermark_threshold: float = 0.001,
                 batch_size: Optional[int] = None, config=None, model=None, log=print):
        """model_path / config_path / device / watermark_threshold: the reference's arguments ('auto' = the HIP device; there is no
        CPU path).  batch_size: images per library call (default PREDICT.BATCH_SIZE).  config / model: a ready config node / model
        instead of files.  log: where the per-file lines go (None: nowhere)."""
        from .predict import WatermarkPredictor
        if device in ("auto", None):
            device = "cuda"
        self.predictor = WatermarkPredictor(model_path, config_path if config_path and os.path.exists(config_path) else None, config,
                                            device=device, model=model)
        self.cfg = self.predictor.cfg
        self.watermark_threshold = float(watermark_threshold)
        self.batch_size = max(1, int(batch_size or self.cfg.PREDICT.BATCH_SIZE))
        self.log = log

    # ---- one image, as the reference's methods
    def predict_mask(self, image_path) -> np.ndarray:
        """-> the uint8 {0,255} mask at the image's own size"""
        _, masks = self.predictor.watermark_counts([load_rgb(image_path)], return_masks=True, use_graph=False)
        return masks[0].cpu().numpy()

    def has_watermark(self, image_path):
        """-> (has_watermark, watermark_ratio): ratio = watermark pixels / (h * w), has_watermark = ratio >= watermark_threshold.  An
        unreadable image raises (the reference returns (False, 0.0), which its caller then treats as "no watermark")."""
        counts = self.predictor.watermark_counts([load_rgb(image_path)], use_graph=False)
        ratio = watermark_ratio(int(counts[0][0]), int(counts[0][1]))
        return ratio >= self.watermark_threshold, ratio

    def ratios(self, paths) -> list:
        """batch_ratios through watermark_counts: full batches replay one captured graph"""
        return batch_ratios(paths, lambda images, full: self.predictor.watermark_counts(images, use_graph=full), self.batch_size)

    def filter_images(self, input_dir, no_watermark_dir=None, dry_run: bool = False, delete: bool = False) -> dict:
        """filter_folder with this model's ratios and watermark_threshold"""
        return filter_folder(input_dir, self.ratios, self.watermark_threshold, no_watermark_dir, dry_run, delete, self.log)
