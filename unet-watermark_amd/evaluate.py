"""Score the masks a checkpoint predicts for a labelled folder, every image at its own size — `main.py evaluate`.  The folder is the
reference's dataset contract (watermarked/ + masks/, paired by file stem); the numbers are the reference's five metrics
(src/utils/metrics.py::get_metrics: IoU, F1, accuracy, recall, precision over tp / fp / fn / tn) and Boundary IoU (Cheng et al., CVPR
2021), which moves when a mask's rim is wrong where region IoU barely does.  A batch is predicted and counted on the device
(WatermarkPredictor.score_images -> uwm_score_masks_ragged): 64 bytes per image come back, no mask does.  The
reference has no such command: its validation metrics are computed at IMG_SIZE on resized masks, before any post-processing."""
from __future__ import annotations

import json
import os
import random
from typing import Optional

import numpy as np

from .filter import IMAGE_EXTENSIONS, load_rgb
from .scoring import (COUNT_FIELDS, MAX_RADIUS, SURFACE_FIELDS, boundary_radius, metrics_from_counts, summarize, summarize_surface,
                      surface_from_record)


def list_pairs(input_dir, masks_dir):
    """-> (sorted [(stem, image path, mask path)], sorted [(stem, image path)] of images without a mask): the files of the two folders
    matched by stem over jpg, jpeg, png, bmp, tiff and tif in either letter case, as extract.list_pairs matches; of several files
    with one stem the first in sorted order counts"""
    def by_stem(d):
        out = {}
        for f in sorted(os.listdir(d)):
            if f.lower().endswith(IMAGE_EXTENSIONS):
                out.setdefault(os.path.splitext(f)[0], os.path.join(d, f))
        return out
    im, mk = by_stem(input_dir), by_stem(masks_dir)
    return [(s, im[s], mk[s]) for s in sorted(im) if s in mk], [(s, im[s]) for s in sorted(im) if s not in mk]


def sample_pairs(pairs, limit=None, seed=0):
    """--limit: a seeded sample (random.Random(seed).sample over the sorted pairs), kept in sorted order"""
    if limit and int(limit) < len(pairs):
        return sorted(random.Random(f"uwm-evaluate:{int(seed)}").sample(pairs, int(limit)))
    return list(pairs)


def load_mask(path) -> np.ndarray:
    """decode to uint8 (h, w) grey; a colour file is converted by Pillow's 'L' rule, as enhance-masks converts"""
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im if im.mode == "L" else im.convert("L"), dtype=np.uint8)


def check_settings(mask_type=None, text_enhance=False, tile=False, tile_overlap=64, boundary_ratio=0.02, boundary_pixels=None,
                   batch_size=16, limit=None, tta=None):
    """the refusals of `evaluate`, before anything is created"""
    from .tta import view_mask
    view_mask(tta)
    if mask_type not in (None, "watermark", "text", "mixed"):
        raise ValueError(f"mask_type must be 'watermark', 'text' or 'mixed', got {mask_type!r}")
    if tile and text_enhance:
        raise ValueError("--tile cannot be combined with --text-enhance: enhancing the images before they are cut into tiles is not "
                         "built; run one or the other")
    if boundary_pixels is not None and boundary_ratio is not None:
        raise ValueError("give --boundary-ratio or --boundary-pixels, not both")
    if boundary_ratio is not None and not float(boundary_ratio) >= 0:
        raise ValueError(f"--boundary-ratio must not be negative, got {boundary_ratio!r}")
    if boundary_pixels is not None and not 0 <= int(boundary_pixels) <= MAX_RADIUS:
        raise ValueError(f"--boundary-pixels must be in 0..{MAX_RADIUS}, got {boundary_pixels!r}")
    if int(tile_overlap) < 0:
        raise ValueError(f"--tile-overlap must not be negative, got {tile_overlap!r}")
    if int(batch_size) < 1:
        raise ValueError(f"--batch-size must be at least 1, got {batch_size!r}")
    if limit is not None and int(limit) < 1:
        raise ValueError(f"--limit must be at least 1, got {limit!r}")


class Evaluator:
    def __init__(self, input_dir, masks_dir, model_path: Optional[str] = None, config_path: Optional[str] = None, mask_type: Optional[str] = None,
                 text_enhance: bool = False, tile: bool = False, tile_overlap: int = 64, boundary_ratio: Optional[float] = None,
                 boundary_pixels: Optional[int] = None, batch_size: int = 16, limit: Optional[int] = None, seed: int = 0, config=None,
                 model=None, scorer=None, log=print, tta: Optional[str] = None, surface: bool = False, surface_scorer=None):
        """input_dir / masks_dir: the images and their ground-truth masks, paired by stem.  model_path / config_path (or config /
        model: a ready config node / model) make the WatermarkPredictor that scores a batch; scorer(images, truths, radii) -> (n, 8)
        counts replaces it (tests).  mask_type / text_enhance / tile / tile_overlap: how the masks are predicted, as `predict
        --resize device` takes them.  boundary_ratio (default 0.02 of the diagonal) or boundary_pixels: Boundary IoU's distance.
        tta: the test-time-augmentation view set ('none' | 'hflip' | 'flips' | 'd4'), as `predict --tta`; recorded in the settings.
        surface: also measure the surface distances of every pair (Hausdorff, HD95, ASSD, covering radius): the result
        gains 'surface' and the settings 'surface_distance'.  surface_scorer(images, truths) -> ((n, 10) records, (n, 2) sums) is the
        test hook of that part, beside `scorer`."""
        if boundary_ratio is None and boundary_pixels is None:
            boundary_ratio = 0.02
        check_settings(mask_type, text_enhance, tile, tile_overlap, boundary_ratio, boundary_pixels, batch_size, limit, tta)
        self.input_dir, self.masks_dir = str(input_dir), str(masks_dir)
        self.settings = dict(input=self.input_dir, masks=self.masks_dir, model=model_path, config=config_path, mask_type=mask_type,
                             text_enhance=bool(text_enhance), tile=bool(tile), tile_overlap=int(tile_overlap),
                             boundary_ratio=None if boundary_ratio is None else float(boundary_ratio),
                             boundary_pixels=None if boundary_pixels is None else int(boundary_pixels), batch_size=int(batch_size),
                             limit=None if limit is None else int(limit), seed=int(seed), tta="none" if tta is None else tta)
        self.log = log or (lambda *a: None)
        self._scorer = scorer
        self._surface_scorer = surface_scorer
        self.surface = bool(surface)
        if self.surface:
            self.settings["surface_distance"] = True
        if scorer is None:
            import torch
            from .predict import WatermarkPredictor
            if not torch.cuda.is_available():
                raise RuntimeError("evaluate runs only on a HIP device (no CPU fallback)")
            self.predictor = WatermarkPredictor(model_path, config_path, config, device="cuda", model=model)
            self.settings["img_size"] = int(self.predictor.cfg.DATA.IMG_SIZE)
            self.settings["threshold"] = float(self.predictor.threshold)

    def radius(self, h: int, w: int) -> int:
        s = self.settings
        return s["boundary_pixels"] if s["boundary_pixels"] is not None else min(boundary_radius(h, w, s["boundary_ratio"]), MAX_RADIUS)

    def _score(self, images, truths, radii):
        """-> the (n, 8) counts and, with surface, the (n, 10) records and (n, 2) sums (else None, None)"""
        n = len(images)
        if self._scorer is not None:
            counts = np.asarray(self._scorer(images, truths, radii), dtype=np.int64).reshape(n, 8)
            if not self.surface:
                return counts, None, None
            if self._surface_scorer is None:
                raise RuntimeError("evaluate: a scorer hook with surface=True needs a surface_scorer hook")
            records, sums = self._surface_scorer(images, truths)
            return counts, np.asarray(records, dtype=np.int64).reshape(n, 10), np.asarray(sums, dtype=np.float64).reshape(n, 2)
        s = self.settings
        got = self.predictor.score_images(images, truths, s["mask_type"], s["text_enhance"], s["tile"], s["tile_overlap"],
                                          s["boundary_ratio"] if s["boundary_pixels"] is None else 0.02, s["boundary_pixels"], tta=s["tta"],
                                          **(dict(surface=True) if self.surface else {}))
        return (got[0], got[1][0], got[1][1]) if self.surface else (got, None, None)

    def run(self, per_image: bool = False) -> dict:
        """-> {'settings', 'images', 'errors', 'error_details' (per error {path, reason}), 'micro', 'imagewise'[, 'surface'][, 'per_image']}
        ('surface': scoring.summarize_surface over the counted pairs, with the surface option; each per-image record then gains
        'surface': the ten record fields, the two sums and the values of scoring.surface_from_record): every pair of the
        folders is decoded on the host, batched, predicted and counted; an unreadable file, an image without a mask and a mask whose
        size differs from its image's count under 'errors' and stop nothing."""
        s = self.settings
        pairs, orphans = list_pairs(self.input_dir, self.masks_dir)
        errors = [dict(path=p, reason="no mask with this stem") for _, p in orphans]
        rows, records, srows, ssums = [], [], [], []
        todo = sample_pairs(pairs, s["limit"], s["seed"])
        for b in range(0, len(todo), s["batch_size"]):
            paths, images, truths = [], [], []
            for _, ipath, mpath in todo[b:b + s["batch_size"]]:
                try:
                    im, t = load_rgb(ipath), load_mask(mpath)
                except Exception as e:      # noqa: BLE001  (an undecodable file is reported, not fatal)
                    errors.append(dict(path=ipath, reason=f"unreadable ({e.__class__.__name__}: {e})"))
                    continue
                if t.shape != im.shape[:2]:
                    errors.append(dict(path=ipath, reason=f"mask is {t.shape[1]} x {t.shape[0]}, image is {im.shape[1]} x {im.shape[0]}"))
                    continue
                paths.append(ipath); images.append(im); truths.append(t)
            if not images:
                continue
            radii = [self.radius(*im.shape[:2]) for im in images]
            counts, srec, ssum = self._score(images, truths, radii)
            for k, (p, im, d, row) in enumerate(zip(paths, images, radii, counts)):
                if int(row[7]) != 0:
                    errors.append(dict(path=p, reason="not counted by the device (status %d)" % int(row[7])))
                    continue
                if self.surface and int(srec[k][9]) != 0:
                    errors.append(dict(path=p, reason="surface distances not measured by the device (status %d)" % int(srec[k][9])))
                    continue
                rows.append([int(v) for v in row])
                if per_image:
                    records.append(dict(path=p, size=[int(im.shape[1]), int(im.shape[0])], radius=int(d),
                                        counts=dict(zip(COUNT_FIELDS, rows[-1])), metrics=metrics_from_counts(rows[-1])))
                if self.surface:
                    srows.append([int(v) for v in srec[k]]); ssums.append([float(v) for v in ssum[k]])
                    if per_image:
                        records[-1]["surface"] = dict(record=dict(zip(SURFACE_FIELDS, srows[-1])), sums=ssums[-1],
                                                      **surface_from_record(srows[-1], ssums[-1]))
        for e in errors:
            self.log(f"error: {e['path']}: {e['reason']}")
        out = dict(settings=s, images=len(rows), errors=len(errors), error_details=errors)
        out.update(summarize(np.asarray(rows, dtype=np.int64).reshape(-1, 8)))
        if self.surface:
            out["surface"] = summarize_surface(np.asarray(srows, dtype=np.int64).reshape(-1, 10), np.asarray(ssums, dtype=np.float64).reshape(-1, 2))
        if per_image:
            out["per_image"] = records
        return out


def format_summary(result) -> str:
    lines = [f"images: {result['images']}  errors: {result['errors']}"]
    for name in ("micro", "imagewise"):
        lines.append(f"{name:>9}: " + "  ".join(f"{k} {v:.4f}" for k, v in result[name].items()))
    if "surface" in result:
        sf = result["surface"]
        num = lambda v: "n/a" if v is None else f"{v:.3f}"      # noqa: E731
        lines.append(f"{'surface':>9}: " + "  ".join(f"{k} {num(v)}" for k, v in sf["imagewise"].items())
                     + f"  worst hd {num(sf['worst']['hd'])}  worst cover_radius {num(sf['worst']['cover_radius'])}"
                     + f"  (pixels; {sf['images']} defined, {sf['undefined']} undefined)")
    return "\n".join(lines)


def write_json(result, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=2)
