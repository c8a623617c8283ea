"""Remove the watermarks of a folder — `main.py repair`, the reference's front end (src/predict.py: step 1 predicts a mask, steps 2-4
hand image and mask to IOPaint's LaMa).  LaMa's weights do not ship, so the fill here is the weight-free membrane interpolant of
inpaint.py: it removes a logo from sky, wall, paper or skin and it smears texture; nothing here claims LaMa's quality.
The masks are predicted on the device and filled where they are (WatermarkPredictor.remove_watermarks: nothing crosses to the host
between prediction and fill), or, with a mask folder, read from files paired with the images by stem as `evaluate` pairs them.  Every
result is written as <stem>.png, so the files hold exactly the computed bytes."""
from __future__ import annotations

import os
from typing import Optional

import numpy as np

from .evaluate import list_pairs, load_mask, sample_pairs
from .filter import IMAGE_EXTENSIONS, load_rgb

COUNT_FIELDS = ("repaired", "nothing_to_fill", "no_known_pixel", "errors")
_STATUS_FIELD = {0: "repaired", 1: "nothing_to_fill", 2: "no_known_pixel"}


def check_settings(model=None, masks=None, mask_type="watermark", text_enhance=False, tile=False, tile_overlap=64, tta=None, cycles=None,
                   batch_size=16, limit=None):
    """the refusals of `repair`, before anything is created"""
    from .inpaint import check_cycles
    from .tta import view_mask
    if (model is None) == (masks is None):
        raise ValueError("give --model (predict the masks) or --masks (a folder of masks), one of the two")
    view_mask(tta)
    if mask_type not in ("watermark", "text", "mixed"):
        raise ValueError(f"mask_type must be 'watermark', 'text' or 'mixed', got {mask_type!r}")
    if tile and text_enhance:
        raise ValueError("--tile cannot be combined with --text-enhance: enhancing the images before they are cut into tiles is not "
                         "built; run one or the other")
    if masks is not None and (text_enhance or tile or (tta or "none") != "none"):
        raise ValueError("--text-enhance, --tile and --tta shape the prediction: they need --model, not --masks")
    if cycles is not None:
        check_cycles(cycles)
    if int(tile_overlap) < 0:
        raise ValueError(f"--tile-overlap must not be negative, got {tile_overlap!r}")
    if int(batch_size) < 1:
        raise ValueError(f"--batch-size must be at least 1, got {batch_size!r}")
    if limit is not None and int(limit) < 1:
        raise ValueError(f"--limit must be at least 1, got {limit!r}")


def _device_fill(images, masks, cycles):
    from .inpaint import inpaint_ragged
    res, stats = inpaint_ragged(images, masks, cycles, return_stats=True)
    return [r.cpu().numpy() for r in res], stats


def repair_folder(input_dir, output_dir, predictor=None, masks_dir=None, mask_type="watermark", text_enhance=False, tile=False,
                  tile_overlap=64, tta=None, cycles: Optional[int] = None, save_masks: Optional[str] = None, limit=None, seed=0,
                  batch_size=16, fill=None, log=print) -> dict:
    """-> {'repaired', 'nothing_to_fill', 'no_known_pixel', 'errors', 'error_details' (per error {path, reason})}.  predictor: a
    WatermarkPredictor whose remove_watermarks predicts and fills on the device; masks_dir: instead, the masks are files (a byte != 0
    after Pillow's 'L' conversion is a hole pixel) and `fill(images, masks, cycles) -> (arrays, stats)` fills them (default: the device
    call inpaint_ragged).  An unreadable file, an image without a mask and a mask of another size count under 'errors' and stop
    nothing; an image without a hole pixel, or without a known one, is written as it is and counted on its own."""
    from PIL import Image
    from .inpaint import DEFAULT_CYCLES, check_cycles
    cycles = check_cycles(DEFAULT_CYCLES if cycles is None else cycles)
    if (predictor is None) == (masks_dir is None):
        raise ValueError("repair_folder: a predictor or a mask folder, one of the two")
    errors = []
    if masks_dir is not None:
        pairs, orphans = list_pairs(input_dir, masks_dir)
        errors += [dict(path=p, reason="no mask with this stem") for _, p in orphans]
    else:
        seen = {}
        for f in sorted(os.listdir(input_dir)):
            if f.lower().endswith(IMAGE_EXTENSIONS):
                seen.setdefault(os.path.splitext(f)[0], os.path.join(input_dir, f))
        pairs = [(s, p, None) for s, p in sorted(seen.items())]
    todo = sample_pairs(pairs, limit, seed)
    os.makedirs(output_dir, exist_ok=True)
    if save_masks:
        os.makedirs(save_masks, exist_ok=True)
    counts = dict.fromkeys(COUNT_FIELDS, 0)
    fill = fill or _device_fill
    for b in range(0, len(todo), int(batch_size)):
        stems, paths, images, masks = [], [], [], []
        for stem, ipath, mpath in todo[b:b + int(batch_size)]:
            try:
                im = load_rgb(ipath)
                m = load_mask(mpath) if mpath is not None else None
            except Exception as e:      # noqa: BLE001  (an undecodable file is reported, not fatal)
                errors.append(dict(path=ipath, reason=f"unreadable ({e.__class__.__name__}: {e})"))
                continue
            if m is not None and m.shape != im.shape[:2]:
                errors.append(dict(path=ipath, reason=f"mask is {m.shape[1]} x {m.shape[0]}, image is {im.shape[1]} x {im.shape[0]}"))
                continue
            stems.append(stem); paths.append(ipath); images.append(im); masks.append(m)
        if not images:
            continue
        if predictor is not None:
            res, dmasks, stats = predictor.remove_watermarks(images, mask_type=mask_type, text_enhance=text_enhance, tile=tile,
                                                             overlap=tile_overlap, tta=tta, cycles=cycles, return_masks=True, return_stats=True)
            res = [r.cpu().numpy() for r in res]
            masks = [m.cpu().numpy() for m in dmasks] if save_masks else masks
        else:
            res, stats = fill(images, masks, cycles)
        for stem, p, r, m, st in zip(stems, paths, res, masks, stats):
            if int(st[1]) not in _STATUS_FIELD:
                errors.append(dict(path=p, reason="not filled by the device (status %d)" % int(st[1])))
                continue
            Image.fromarray(np.ascontiguousarray(r)).save(os.path.join(output_dir, stem + ".png"))
            if save_masks:
                Image.fromarray(((np.asarray(m) != 0) * np.uint8(255)).astype(np.uint8)).save(os.path.join(save_masks, stem + ".png"))
            counts[_STATUS_FIELD[int(st[1])]] += 1
    for e in errors:
        log(f"error: {e['path']}: {e['reason']}")
    counts["errors"] = len(errors)
    return dict(counts, error_details=errors)


def format_counts(result) -> str:
    return (f"repaired {result['repaired']}, nothing to fill {result['nothing_to_fill']}, no known pixel {result['no_known_pixel']}, "
            f"errors {result['errors']}")
