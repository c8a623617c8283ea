"""Checkpoint selection, the part that needs no device: sampling, the metrics of a stats row, per-model statistics, the summary and its
tie rule, model discovery, the JSON file, all with an injected stats function, and the `main.py select` command line."""
import json
import os
import random

import numpy as np
import pytest

KEYS = {"timestamp", "input_dir", "model_dir", "num_samples", "selected_images", "models", "summary"}
MODEL_KEYS = {"model_path", "model_name", "model_info", "predictions", "statistics"}
PRED_KEYS = {"image_name", "image_path", "mask_path", "metrics", "success", "error"}
METRIC_KEYS = {"watermark_ratio", "watermark_pixels", "total_pixels", "num_components", "max_component_area", "max_component_ratio"}
STAT_KEYS = {"total_predictions", "successful_predictions", "failed_predictions", "avg_watermark_ratio", "std_watermark_ratio",
             "min_watermark_ratio", "max_watermark_ratio", "detection_rate"}


@pytest.fixture(scope="module")
def S():
    import __graft_entry__ as g
    g.build()
    from unet_watermark_amd import select
    return select


def _touch(path, data=b"x"):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)


def _row(pixels, total, kept=1, kept_area=None, status=0):
    return [kept + 2, 999, pixels, 0, kept, pixels if kept_area is None else kept_area, total, status]


def test_sampling_is_random_seed_and_random_sample(S):
    paths = [f"img_{i:03d}.png" for i in range(50)]
    random.seed(7); want = random.sample(paths, 10)
    assert S.sample_images(paths, 10, 7) == want
    assert S.sample_images(paths, 10, 7) == want and S.sample_images(paths, 10, 8) != want
    assert S.sample_images(paths, 50, 7) == paths and S.sample_images(paths, 80, 7) == paths      # short list: all of it, in order
    random.seed(42); want = random.sample(paths, 49)
    assert S.sample_images(paths, 49) == want                                                    # the default seed is the script's 42


def test_lists_follow_the_reference(S, tmp_path):
    for name in ("b.PNG", "a.jpg", "c.jpeg", "d.bmp", "e.tiff", "f.tif", "g.txt", "sub/h.png"):
        _touch(str(tmp_path / "in" / name))
    assert [os.path.basename(p) for p in S.list_images(tmp_path / "in")] == ["a.jpg", "b.PNG", "c.jpeg", "d.bmp", "e.tiff"]
    assert S.list_images(tmp_path / "in" / "a.jpg") == [str(tmp_path / "in" / "a.jpg")] and S.list_images(tmp_path / "in" / "g.txt") == []
    for name in ("z.pth", "run1/a.pth", "run1/deep/b.pth", "run2/a.pth", "notes.txt", "c.PTH"):
        _touch(str(tmp_path / "m" / name))
    models = S.list_models(tmp_path / "m")
    assert [S.model_key(p, tmp_path / "m") for p in models] == [os.path.join("run1", "a.pth"), os.path.join("run1", "deep", "b.pth"),
                                                                os.path.join("run2", "a.pth"), "z.pth"]
    one = str(tmp_path / "m" / "run1" / "a.pth")
    assert S.list_models(one) == [one] and S.model_key(one, one) == "a.pth"
    assert S.list_models(tmp_path / "m" / "notes.txt") == [] and S.list_models(tmp_path / "nowhere") == []


def test_metrics_from_a_stats_row(S):
    m = S.metrics_from_stats([7, 900, 1200, 33, 2, 800, 4800, 0])
    assert set(m) == METRIC_KEYS
    assert m == {"watermark_ratio": 0.25, "watermark_pixels": 1200, "total_pixels": 4800, "num_components": 2, "max_component_area": 800,
                 "max_component_ratio": 800 / 4800}
    z = S.metrics_from_stats(np.array([3, 40, 0, 5, 0, 0, 100, 0]))                                # components found, none kept
    assert z["num_components"] == 0 and z["max_component_area"] == 0 and z["max_component_ratio"] == 0.0 and z["watermark_ratio"] == 0.0
    assert type(z["watermark_pixels"]) is int and type(z["watermark_ratio"]) is float
    for bad in ([0, 0, 0, 0, 0, 0, 0, 1], [1, 1, 1, 0, 1, 1, 0, 0], [1, 2, 3]):
        with pytest.raises(ValueError):
            S.metrics_from_stats(bad)


def test_statistics_are_the_references(S):
    ratios = [0.0, 0.001, 0.0011, 0.5]                                                            # exactly 0.001 is NOT a detection
    assert 1 / 1000 == 0.001                                                                     # (the ratio the row below gives)
    rows = [_row(0, 1000, kept=0), _row(1, 1000), _row(11, 10000), _row(500, 1000)]
    preds = S.evaluate_model("m.pth", "m.pth", [f"{i}.png" for i in range(4)], lambda paths: rows)["predictions"]
    assert [p["metrics"]["watermark_ratio"] for p in preds] == ratios
    st = S.model_statistics(preds)
    assert set(st) == STAT_KEYS
    assert st["detection_rate"] == 0.5 and st["avg_watermark_ratio"] == float(np.mean(ratios))
    assert st["std_watermark_ratio"] == float(np.std(ratios)) and st["std_watermark_ratio"] != float(np.std(ratios, ddof=1))
    assert (st["min_watermark_ratio"], st["max_watermark_ratio"]) == (0.0, 0.5)
    assert (st["total_predictions"], st["successful_predictions"], st["failed_predictions"]) == (4, 4, 0)


def test_failed_predictions_and_a_run_where_every_one_fails(S):
    rows = [_row(10, 100), None, OSError("cannot identify image file"), _row(0, 0, status=1)]
    r = S.evaluate_model("m.pth", "m.pth", ["a.png", "b.png", "c.png", "d.png"], lambda paths: rows)
    assert set(r) == MODEL_KEYS and all(set(p) == PRED_KEYS for p in r["predictions"])
    assert [p["success"] for p in r["predictions"]] == [True, False, False, False]
    assert "cannot identify" in r["predictions"][2]["error"] and r["predictions"][0]["error"] is None
    assert r["predictions"][1]["metrics"] is None and r["predictions"][3]["error"]
    st = r["statistics"]
    assert (st["total_predictions"], st["successful_predictions"], st["failed_predictions"]) == (4, 1, 3)
    assert st["detection_rate"] == 1.0 and st["avg_watermark_ratio"] == 0.1 and st["std_watermark_ratio"] == 0.0
    none = S.evaluate_model("m.pth", "m.pth", ["a.png", "b.png"], lambda paths: [None, None])["statistics"]
    assert none == {"total_predictions": 2, "successful_predictions": 0, "failed_predictions": 2, "avg_watermark_ratio": 0.0,
                    "std_watermark_ratio": 0.0, "min_watermark_ratio": 0.0, "max_watermark_ratio": 0.0, "detection_rate": 0.0}


def test_folder_run_ties_load_errors_and_the_json(S, tmp_path):
    for i in range(6):
        _touch(str(tmp_path / "in" / f"p{i}.png"))
    for name in ("a.pth", "b.pth", "broken.pth", "sub/c.pth"):
        _touch(str(tmp_path / "m" / name))
    # a and b detect 2 of 4 (a tie: a wins, first in sorted order); c detects as many with a higher average ratio
    table = {"a.pth": [20, 20, 0, 0], "b.pth": [30, 0, 10, 0], os.path.join("sub", "c.pth"): [0, 0, 900, 900]}
    seen = {}

    def make(path, name):
        if name == "broken.pth":
            raise RuntimeError("invalid load key")
        assert os.path.isfile(path)

        def fn(paths):
            seen[name] = list(paths)
            return [_row(v, 1000, kept=int(v > 0)) for v in table[name]]
        return fn

    lines = []
    res = S.run_selection(tmp_path / "in", tmp_path / "m", tmp_path / "out", make, num_samples=4, seed=3, log=lines.append)
    with open(tmp_path / "out" / "model_evaluation_results.json", encoding="utf-8") as f:
        on_disk = json.load(f)
    assert on_disk == res and set(res) == KEYS
    random.seed(3); want = random.sample(S.list_images(tmp_path / "in"), 4)
    assert res["selected_images"] == [os.path.basename(p) for p in want] and res["num_samples"] == 4
    assert all(v == want for v in seen.values())                                                  # every model sees the same sample
    assert list(res["models"]) == ["a.pth", "b.pth", "broken.pth", os.path.join("sub", "c.pth")]
    broken = res["models"]["broken.pth"]
    assert broken["load_error"] == "invalid load key" and broken["statistics"] is None and broken["predictions"] == []
    assert res["summary"] == {"total_models": 4, "successful_models": 3, "failed_models": 1,
                              "best_detection_model": {"name": "a.pth", "detection_rate": 0.5},
                              "highest_ratio_model": {"name": os.path.join("sub", "c.pth"), "avg_ratio": 0.45}}
    assert any("a.pth" in ln and "best detection" in ln for ln in lines) and any("broken.pth: load failed" in ln for ln in lines)
    # what auto_train._find_best_model reads
    best = res["summary"]["best_detection_model"]["name"]
    assert res["models"][best]["model_path"] == str(tmp_path / "m" / "a.pth")
    # no model loads: the summary names none
    empty = S.run_selection(tmp_path / "in", tmp_path / "m" / "broken.pth", tmp_path / "out2", make, log=None)
    assert empty["summary"] == {"total_models": 1, "successful_models": 0, "failed_models": 1, "best_detection_model": None,
                                "highest_ratio_model": None}
    assert empty["num_samples"] == 6


def test_batches_and_unreadable_images(S):
    calls = []

    def load(p):
        if "bad" in p:
            raise OSError(f"cannot read {p}")
        return p.upper()

    def stats_batch(images, full, paths):
        calls.append((list(images), full, list(paths)))
        return [_row(len(im), 100) for im in images]

    paths = ["a", "bad1", "bb", "ccc", "bad2", "dddd", "e"]
    out = S.batch_stats(paths, stats_batch, 3, load)
    assert [r[2] if isinstance(r, list) else type(r) for r in out] == [1, OSError, 2, 3, OSError, 4, 1]
    assert calls == [(["A", "BB"], False, ["a", "bb"]), (["CCC", "DDDD"], False, ["ccc", "dddd"]), (["E"], False, ["e"])]
    calls.clear()
    S.batch_stats(["a", "b", "c", "d"], stats_batch, 2, load)
    assert [c[1] for c in calls] == [True, True]


def test_main_select_help_and_missing_paths(capsys, tmp_path):
    from unet_watermark_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["select", "--help"])
    assert e.value.code == 0
    text = " ".join(capsys.readouterr().out.split())
    for word in ("--input", "--model", "--output", "--num-samples", "--seed", "--config", "--encoder", "--mask-type", "--batch-size",
                 "--save-masks", "only with --save-masks", "not fatal", "relative to --model", "no worker processes"):
        assert word in text, word
    args = cli.build_parser().parse_args(["select", "--input", "d", "--model", "m", "--output", "o"])
    assert (args.num_samples, args.seed, args.mask_type, args.save_masks, args.batch_size) == (100, 42, "watermark", False, None)
    with pytest.raises(SystemExit) as e:
        cli.build_parser().parse_args(["select", "--input", "d", "--model", "m", "--output", "o", "--mask-type", "auto"])
    assert e.value.code == 2
    capsys.readouterr()
    os.makedirs(tmp_path / "in")
    with pytest.raises(SystemExit) as e:
        cli.main(["select", "--input", str(tmp_path / "nowhere"), "--model", str(tmp_path / "in"), "--output", str(tmp_path / "o")])
    assert "input path not found" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(["select", "--input", str(tmp_path / "in"), "--model", str(tmp_path / "m.pth"), "--output", str(tmp_path / "o")])
    assert "model path not found" in str(e.value)
    assert not os.path.exists(tmp_path / "o")


def test_the_class_is_exported():
    import unet_watermark_amd as U
    assert U.ModelSelector is U.select.ModelSelector and U.select.DETECTION_RATIO == 0.001
    assert U.select.IMAGE_EXTENSIONS == (".png", ".jpg", ".jpeg", ".bmp", ".tiff")
