"""Pick the best checkpoint — counterpart of the reference's src/scripts/model_selector.py (ModelSelector), the step its training
cycle begins with (auto_train.py:117-141): a seeded sample of images goes through every `.pth` under a directory, each mask is
reduced to a few numbers, and the checkpoint with the highest detection rate wins.  The reference predicts one image at a time
and labels every mask on the host (cv2.connectedComponentsWithStats); here a batch goes through ONE captured library call
(WatermarkPredictor.mask_stats: forward, resize, threshold, _optimize_mask, component statistics) that returns 64 bytes per image.

The host logic below (sampling, metrics, statistics, summary, JSON) knows nothing of the device: it takes a
stats_fn(paths) -> (N, 8) rows of postprocess.STATS_FIELDS, or None per image that could not be predicted.

Deliberate departures from the reference:
  * masks are written only with save_masks (`--save-masks`); the reference writes one PNG per image and model;
  * an image that cannot be read is a failed prediction of every model, not fatal;
  * a model is keyed by its path relative to the model directory: for files directly in it that is the reference's basename; the
    reference lets same-named files of different sub-directories overwrite each other's entry;
  * no worker processes: one process, one device."""
from __future__ import annotations

import json
import os
import random
from datetime import datetime
from pathlib import Path
from typing import Optional

import numpy as np

IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".tiff")      # model_selector.py:238
RESULTS_FILE = "model_evaluation_results.json"
DETECTION_RATIO = 0.001                                            # a ratio above this (strictly) counts as a detection


def list_images(input_dir) -> list:
    """the reference's list: the files of the directory (not its sub-directories) with one of its extensions in either letter
    case, sorted; a single image file is a list of one"""
    input_dir = str(input_dir)
    if os.path.isdir(input_dir):
        return sorted(os.path.join(input_dir, f) for f in os.listdir(input_dir) if f.lower().endswith(IMAGE_EXTENSIONS))
    if os.path.isfile(input_dir) and input_dir.lower().endswith(IMAGE_EXTENSIONS):
        return [input_dir]
    return []


def list_models(model_dir) -> list:
    """every `.pth` under the directory, recursively, sorted by path; a single `.pth` file is a list of one"""
    model_dir = str(model_dir)
    if os.path.isdir(model_dir):
        return sorted(os.path.join(root, f) for root, _, files in os.walk(model_dir) for f in files if f.endswith(".pth"))
    if os.path.isfile(model_dir) and model_dir.endswith(".pth"):
        return [model_dir]
    return []


def model_key(model_path, model_dir) -> str:
    """the path relative to the model directory (the basename for a file directly in it, and for a single-file model_dir)"""
    if os.path.isdir(str(model_dir)):
        return os.path.relpath(str(model_path), str(model_dir))
    return os.path.basename(str(model_path))


def sample_images(image_paths, num_samples: int, seed: int = 42) -> list:
    """the reference's draw: random.seed(seed) (its main()), then the whole list when it is not longer than num_samples, else
    random.sample(list, num_samples)"""
    random.seed(seed)
    image_paths = list(image_paths)
    if len(image_paths) <= num_samples:
        return image_paths
    return random.sample(image_paths, num_samples)


def metrics_from_stats(row) -> dict:
    """calculate_watermark_metrics (model_selector.py:171-197) from one stats row.  The optimised mask is a union of whole
    components, so the kept components (entries 4, 5) are what connectedComponentsWithStats finds in it."""
    row = [int(v) for v in row]
    if len(row) != 8:
        raise ValueError("a stats row has 8 entries")
    if row[7] != 0 or row[6] <= 0:
        raise ValueError("the image was not processed (it does not fit the call's capacities)")
    total, pixels, area = row[6], row[2], row[5]
    return {"watermark_ratio": float(pixels / total), "watermark_pixels": pixels, "total_pixels": total, "num_components": row[4],
            "max_component_area": area, "max_component_ratio": float(area / total) if row[4] > 0 else 0.0}


def model_statistics(predictions) -> dict:
    """model_selector.py:123-147: population std, detection_rate = share of successful predictions with ratio > 0.001"""
    ok = [p for p in predictions if p["success"]]
    stats = {"total_predictions": len(predictions), "successful_predictions": len(ok), "failed_predictions": len(predictions) - len(ok)}
    if ok:
        r = [p["metrics"]["watermark_ratio"] for p in ok]
        stats.update(avg_watermark_ratio=float(np.mean(r)), std_watermark_ratio=float(np.std(r)), min_watermark_ratio=float(np.min(r)),
                     max_watermark_ratio=float(np.max(r)), detection_rate=float(np.mean([1 if v > DETECTION_RATIO else 0 for v in r])))
    else:
        stats.update(avg_watermark_ratio=0.0, std_watermark_ratio=0.0, min_watermark_ratio=0.0, max_watermark_ratio=0.0, detection_rate=0.0)
    return stats


def evaluate_model(model_path, name, images, stats_fn) -> dict:
    """one model's entry.  stats_fn(paths) -> per path a stats row, None, or an exception (why that image has no prediction)"""
    preds = []
    for path, row in zip(images, stats_fn(images)):
        entry = {"image_name": os.path.basename(path), "image_path": path, "mask_path": None, "metrics": None, "success": False, "error": None}
        try:
            if row is None or isinstance(row, Exception):
                raise row if isinstance(row, Exception) else ValueError("no prediction")
            entry.update(metrics=metrics_from_stats(row), success=True)
        except Exception as e:      # noqa: BLE001  (a failed prediction is recorded, as in the reference)
            entry["error"] = str(e)
        preds.append(entry)
    return {"model_path": model_path, "model_name": name, "model_info": None, "predictions": preds, "statistics": model_statistics(preds)}


def load_error_entry(model_path, name, error) -> dict:
    return {"model_path": model_path, "model_name": name, "model_info": None, "predictions": [], "statistics": None, "load_error": str(error)}


def summarize(models: dict, total_models: int) -> dict:
    """model_selector.py:369-401: max() over the models in their (sorted) order, so the first of equals wins"""
    good = [n for n, r in models.items() if "load_error" not in r and r["statistics"] is not None]
    out = {"total_models": total_models, "successful_models": len(good), "failed_models": total_models - len(good),
           "best_detection_model": None, "highest_ratio_model": None}
    if good:
        best = max(good, key=lambda n: models[n]["statistics"]["detection_rate"])
        high = max(good, key=lambda n: models[n]["statistics"]["avg_watermark_ratio"])
        out["best_detection_model"] = {"name": best, "detection_rate": models[best]["statistics"]["detection_rate"]}
        out["highest_ratio_model"] = {"name": high, "avg_ratio": models[high]["statistics"]["avg_watermark_ratio"]}
    return out


def run_selection(input_dir, model_dir, output_dir, make_stats_fn, num_samples: int = 100, seed: int = 42, log=print) -> dict:
    """The reference's run_evaluation.  make_stats_fn(model_path, name) -> stats_fn for that checkpoint; an exception it raises is
    that model's load_error and the run goes on.  Writes <output_dir>/model_evaluation_results.json and returns its content."""
    log = log or (lambda *a: None)
    os.makedirs(output_dir, exist_ok=True)
    images = sample_images(list_images(input_dir), num_samples, seed)
    model_paths = list_models(model_dir)
    res = {"timestamp": datetime.now().isoformat(), "input_dir": str(input_dir), "model_dir": str(model_dir), "num_samples": len(images),
           "selected_images": [os.path.basename(p) for p in images], "models": {}, "summary": {}}
    for path in model_paths:
        name = model_key(path, model_dir)
        try:
            stats_fn = make_stats_fn(path, name)
        except Exception as e:      # noqa: BLE001  (a checkpoint that does not load is reported, not fatal)
            res["models"][name] = load_error_entry(path, name, e)
            log(f"{name}: load failed - {e}")
            continue
        res["models"][name] = evaluate_model(path, name, images, stats_fn)
    res["summary"] = summarize(res["models"], len(model_paths))
    with open(os.path.join(output_dir, RESULTS_FILE), "w", encoding="utf-8") as f:
        json.dump(res, f, indent=2, ensure_ascii=False)
    print_summary(res, log)
    return res


def print_summary(res: dict, log=print):
    s = res["summary"]
    log("=" * 60)
    log(f"models: {s['total_models']}  evaluated: {s['successful_models']}  failed to load: {s['failed_models']}  images: {res['num_samples']}")
    if s["best_detection_model"]:
        log(f"best detection model: {s['best_detection_model']['name']} (detection rate {s['best_detection_model']['detection_rate']:.2%})")
        log(f"highest ratio model: {s['highest_ratio_model']['name']} (average ratio {s['highest_ratio_model']['avg_ratio']:.6f})")
    log("-" * 60)
    for name, r in res["models"].items():
        if "load_error" in r:
            log(f"{name}: load failed - {r['load_error']}")
            continue
        st = r["statistics"]
        log(f"{name}: predicted {st['successful_predictions']}/{st['total_predictions']}  detection rate {st['detection_rate']:.2%}  "
            f"average ratio {st['avg_watermark_ratio']:.6f}  range {st['min_watermark_ratio']:.6f} - {st['max_watermark_ratio']:.6f}")
    log("=" * 60)


def batch_stats(paths, stats_batch_fn, batch_size: int, load=None) -> list:
    """per path: its stats row, or the exception that kept the image from being decoded.  stats_batch_fn(images, full, paths) ->
    (n, 8) for a list of decoded images; `full` says that the batch has batch_size images (those replay one captured graph)."""
    if load is None:
        from .filter import load_rgb as load
    out = []
    for b in range(0, len(paths), batch_size):
        res, images, kept = [], [], []
        for p in paths[b:b + batch_size]:
            try:
                images.append(load(p)); res.append(None); kept.append(p)
            except Exception as e:      # noqa: BLE001  (an undecodable file is a failed prediction, not fatal)
                res.append(e)
        if images:
            rows = iter(stats_batch_fn(images, len(images) == batch_size, kept))
            res = [next(rows) if r is None else r for r in res]
        out.extend(res)
    return out


class ModelSelector:
    def __init__(self, input_dir, model_dir, output_dir, num_samples: int = 100, config=None, mask_type: str = "watermark",
                 batch_size: Optional[int] = None, seed: int = 42, save_masks: bool = False, log=print):
        """input_dir / model_dir / output_dir / num_samples / seed: the reference's arguments (model_dir may be one `.pth`).  config: a
        ready config node (default: the defaults).  mask_type: the _optimize_mask type every mask goes through ('watermark', as
        predict_mask's default).  batch_size: images per captured call (default PREDICT.BATCH_SIZE).  save_masks: also write
        <stem>_<model>_mask.png per image and model, as the reference always does."""
        from .config import get_cfg_defaults
        from .postprocess import mask_type_code
        mask_type_code(mask_type)
        self.input_dir, self.model_dir, self.output_dir = str(input_dir), str(model_dir), str(output_dir)
        self.num_samples, self.seed, self.mask_type, self.save_masks, self.log = int(num_samples), int(seed), mask_type, bool(save_masks), log
        self.cfg = config if config is not None else get_cfg_defaults()
        self.batch_size = max(1, int(batch_size or self.cfg.PREDICT.BATCH_SIZE))

    def _stats_fn(self, model_path, name):
        from .predict import WatermarkPredictor
        pred = WatermarkPredictor(model_path, None, self.cfg.clone() if hasattr(self.cfg, "clone") else self.cfg)
        tag = name.replace(os.sep, "_")
        tag = tag[:-len(".pth")] if tag.endswith(".pth") else tag

        def batch(images, full, paths):
            if not self.save_masks:
                return pred.mask_stats(images, self.mask_type, use_graph=full)
            from PIL import Image
            rows, masks = pred.mask_stats(images, self.mask_type, return_masks=True, use_graph=full)
            for p, m in zip(paths, masks):
                Image.fromarray(m.cpu().numpy()).save(os.path.join(self.output_dir, f"{Path(p).stem}_{tag}_mask.png"))
            return rows
        return lambda paths: batch_stats(paths, batch, self.batch_size)

    def run_evaluation(self) -> dict:
        return run_selection(self.input_dir, self.model_dir, self.output_dir, self._stats_fn, self.num_samples, self.seed, self.log)
