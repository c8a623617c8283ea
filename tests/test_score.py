"""Mask scoring, the part that needs no device: the restatement (tests/score_ref.py) against the window definition, the radius rule,
the metric formulas on hand-computed rows, the Evaluator's pairing and error accounting against a stub scorer, the `evaluate` parser
and its refusals, the new symbols of libuwm.so and their argument checks, which fail before any launch."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_ref as SR  # noqa: E402

NEW_SYMBOLS = ("uwm_score_masks_workspace_bytes", "uwm_score_masks_ragged")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from unet_watermark_amd import _lib
    _lib.lib()
    return _lib


@pytest.mark.parametrize("d", [1, 2, 3, 7, 40])
def test_the_restatement_equals_the_window_definition(d):
    rng = np.random.default_rng(100 + d)
    for h, w in ((1, 1), (5, 3), (17, 63), (9, 65), (33, 40), (40, 200), (81, 83)):
        for density in (0.5, 0.97, 1.0):
            m = rng.random((h, w)) < density
            m[h // 3:, : 2 * w // 3] |= density > 0.9                     # a block that survives the larger radii
            assert np.array_equal(SR.erode(m, d), SR.erode_brute(m, d)), (h, w, d, density)
    p = ((rng.random((40, 200)) < 0.97) * 255).astype(np.uint8)
    g = ((rng.random((40, 200)) < 0.9) * 255).astype(np.uint8)
    assert SR.counts(p, g, d).tolist() == SR.counts(p, g, d, SR.erode_brute).tolist()


def test_counts_on_a_hand_computed_pair():
    p = np.zeros((7, 9), np.uint8); p[1:6, 1:8] = 255                     # 5 x 7 block: its erosion by 1 is the inner 3 x 5
    g = np.zeros((7, 9), np.uint8); g[0:7, 0:4] = 128                     # touches three borders: erosion by 1 is rows 1..5, columns 1..2
    # the two bands meet where p's top and bottom rows cross g's last column: (1, 3) and (5, 3)
    assert SR.counts(p, g, 1).tolist() == [15, 20, 13, 15, 2, 35 - 15, 28 - 10, 0]
    assert SR.counts(p, g, 0).tolist() == [15, 20, 13, 15, 0, 0, 0, 0]
    assert SR.counts(p, g, 4).tolist() == [15, 20, 13, 15, 15, 35, 28, 0]          # 2d + 1 above a side: B(M) = M
    g[3, 3] = 127                                                          # 127 is background
    assert SR.counts(p, g, 0).tolist()[:4] == [14, 21, 13, 15]


def test_boundary_radius_is_the_papers_rule():
    from unet_watermark_amd.scoring import boundary_radius
    assert [boundary_radius(720, 1280), boundary_radius(2160, 3840), boundary_radius(8, 8)] == [29, 88, 1]
    assert boundary_radius(1280, 720) == 29 and boundary_radius(1000, 1000, 0.01) == 14 and boundary_radius(100, 100, 0) == 1


def test_metrics_from_counts_and_summarize_on_hand_computed_rows():
    from unet_watermark_amd.scoring import COUNT_FIELDS, METRIC_FIELDS, metrics_from_counts, summarize
    assert COUNT_FIELDS == ("tp", "fp", "fn", "tn", "boundary_intersection", "boundary_pred", "boundary_truth", "status") and len(METRIC_FIELDS) == 6
    a = [6, 2, 4, 8, 3, 5, 7, 0]
    ma = metrics_from_counts(a)
    assert ma == {"iou": 6 / 12, "f1": 12 / 18, "accuracy": 14 / 20, "recall": 6 / 10, "precision": 6 / 8, "boundary_iou": 3 / 9}
    empty = [0, 0, 0, 25, 0, 0, 0, 0]                                      # an all-empty pair: 1.0 everywhere
    assert set(metrics_from_counts(empty).values()) == {1.0}
    missed = [0, 0, 5, 20, 0, 0, 4, 0]                                     # nothing predicted: only precision is 0 / 0
    mm = metrics_from_counts(missed)
    assert mm == {"iou": 0.0, "f1": 0.0, "accuracy": 20 / 25, "recall": 0.0, "precision": 1.0, "boundary_iou": 0.0}
    s = summarize(np.array([a, empty, missed]))
    assert s["micro"] == metrics_from_counts([6, 2, 9, 53, 3, 5, 11, 0])
    assert s["micro"]["iou"] == 6 / 17 and s["micro"]["boundary_iou"] == 3 / 13
    for k in METRIC_FIELDS:
        assert s["imagewise"][k] == pytest.approx((ma[k] + 1.0 + mm[k]) / 3, abs=1e-15)
    both_empty = summarize(np.array([empty, empty]))
    assert set(both_empty["micro"].values()) == {1.0} and set(both_empty["imagewise"].values()) == {1.0}
    assert summarize(np.array([a, [0, 0, 0, 0, 0, 0, 0, 1]]))["micro"] == ma           # a misfit row is left out
    assert set(summarize(np.zeros((0, 8)))["imagewise"].values()) == {1.0}


def _folder(tmp_path):
    """six images: a png pair, a jpg image with a bmp mask, a colour mask, a mask of another size, an image without a mask, an unreadable one"""
    from PIL import Image
    rng = np.random.default_rng(3)
    im, mk = tmp_path / "watermarked", tmp_path / "masks"
    os.makedirs(im); os.makedirs(mk)
    shapes = {"a": (20, 30), "b": (31, 17), "c": (8, 8), "d": (12, 12), "e": (9, 9), "f": (10, 10)}
    truths = {}
    for s, (h, w) in shapes.items():
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(im / (s + (".jpg" if s == "b" else ".png")))
        truths[s] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    Image.fromarray(truths["a"]).save(mk / "a.png")
    Image.fromarray(truths["b"]).save(mk / "b.bmp")
    rgb = rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(mk / "c.png")
    truths["c"] = np.asarray(Image.fromarray(rgb).convert("L"))
    Image.fromarray(truths["d"][:-2]).save(mk / "d.png")
    (mk / "f.png").write_bytes(b"not an image")
    Image.fromarray(truths["a"]).save(mk / "unpaired.png")
    return shapes, truths


def test_evaluator_pairs_accounts_errors_and_writes_the_keys(tmp_path):
    from unet_watermark_amd.evaluate import Evaluator, format_summary, list_pairs, write_json
    from unet_watermark_amd.scoring import METRIC_FIELDS, summarize
    shapes, truths = _folder(tmp_path)
    pairs, orphans = list_pairs(tmp_path / "watermarked", tmp_path / "masks")
    assert [p[0] for p in pairs] == ["a", "b", "c", "d", "f"] and [o[0] for o in orphans] == ["e"]
    assert pairs[1][1].endswith("b.jpg") and pairs[1][2].endswith("b.bmp")
    seen = []

    def scorer(images, truths_in, radii):
        seen.append(([im.shape for im in images], [t.copy() for t in truths_in], list(radii)))
        return [[int((t > 127).sum()), i, 2, t.size - int((t > 127).sum()) - i - 2, 1, 2, 3, 0] for i, t in enumerate(truths_in)]
    ev = Evaluator(tmp_path / "watermarked", tmp_path / "masks", batch_size=2, scorer=scorer, log=None)
    res = ev.run(per_image=True)
    assert set(res) == {"settings", "images", "errors", "error_details", "micro", "imagewise", "per_image"}
    assert res["images"] == 3 and res["errors"] == 3
    reasons = {os.path.basename(e["path"]): e["reason"] for e in res["error_details"]}
    assert set(reasons) == {"d.png", "e.png", "f.png"}
    assert "no mask" in reasons["e.png"] and "unreadable" in reasons["f.png"] and reasons["d.png"] == "mask is 12 x 10, image is 12 x 12"
    assert [s for s, _, _ in seen] == [[(20, 30, 3), (31, 17, 3)], [(8, 8, 3)]]            # batches of two; d and f never reach the scorer
    assert np.array_equal(seen[0][1][0], truths["a"]) and np.array_equal(seen[0][1][1], truths["b"]) and np.array_equal(seen[1][1][0], truths["c"])
    assert seen[0][2] == [1, 1] and seen[1][2] == [1]
    rows = np.array([list(r["counts"].values()) for r in res["per_image"]])
    assert res["micro"] == summarize(rows)["micro"] and res["imagewise"] == summarize(rows)["imagewise"]
    assert [r["size"] for r in res["per_image"]] == [[30, 20], [17, 31], [8, 8]] and set(res["per_image"][0]["metrics"]) == set(METRIC_FIELDS)
    write_json(res, tmp_path / "out" / "r.json")
    assert json.loads((tmp_path / "out" / "r.json").read_text()) == json.loads(json.dumps(res))
    assert "images: 3  errors: 3" in format_summary(res) and "boundary_iou" in format_summary(res)
    plain = Evaluator(tmp_path / "watermarked", tmp_path / "masks", boundary_pixels=5, limit=2, seed=1, scorer=scorer, log=None).run()
    assert "per_image" not in plain and plain["images"] + plain["errors"] == 2 + 1 and seen[-1][2][0] == 5
    assert plain["settings"]["boundary_pixels"] == 5 and plain["settings"]["boundary_ratio"] is None


def test_evaluate_parser_and_refusals(tmp_path):
    from unet_watermark_amd import cli
    from unet_watermark_amd.evaluate import Evaluator
    a = cli.build_parser().parse_args(["evaluate", "--data-dir", "D", "--model", "m.pth"])
    assert (a.input, a.masks, a.data_dir, a.mask_type, a.text_enhance, a.tile, a.tile_overlap) == (None, None, "D", None, False, False, 64)
    assert (a.boundary_ratio, a.boundary_pixels, a.batch_size, a.limit, a.seed, a.output, a.per_image) == (None, None, 16, None, 0, None, False)
    a = cli.build_parser().parse_args(["evaluate", "--input", "I", "--masks", "M", "--model", "m.pth", "--mask-type", "text", "--text-enhance",
                                       "--boundary-pixels", "3", "--limit", "7", "--seed", "2", "--output", "o.json", "--per-image", "--tile",
                                       "--tile-overlap", "16", "--batch-size", "4", "--config", "c.yaml"])
    assert (a.input, a.masks, a.mask_type, a.text_enhance, a.boundary_pixels, a.limit, a.seed, a.output, a.per_image, a.tile, a.tile_overlap,
            a.batch_size, a.config) == ("I", "M", "text", True, 3, 7, 2, "o.json", True, True, 16, 4, "c.yaml")
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["evaluate", "--data-dir", "D", "--model", "m", "--mask-type", "auto"])
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["evaluate", "--data-dir", "D"])                       # --model is required
    out = tmp_path / "never" / "o.json"
    base = ["evaluate", "--model", str(tmp_path / "m.pth"), "--output", str(out)]
    dirs = ["--input", str(tmp_path), "--masks", str(tmp_path)]
    for argv, word in ((dirs + ["--data-dir", str(tmp_path)], "not both"), ([], "or --data-dir"), (["--input", str(tmp_path)], "go together"),
                       (["--masks", str(tmp_path)], "go together"),
                       (dirs + ["--boundary-ratio", "0.02", "--boundary-pixels", "3"], "not both"),
                       (dirs + ["--tile", "--text-enhance"], "--text-enhance"),
                       (dirs + ["--boundary-ratio", "-0.1"], "negative"), (dirs + ["--boundary-pixels", "-1"], "0..32767"),
                       (dirs + ["--boundary-pixels", "40000"], "0..32767"), (dirs + ["--batch-size", "0"], "at least 1"),
                       (["--data-dir", str(tmp_path / "absent")], "not found"), (dirs, "model file not found")):
        with pytest.raises(SystemExit, match=word):
            cli.main(base + argv)
    assert not out.parent.exists()
    for kw in (dict(tile=True, text_enhance=True), dict(boundary_ratio=0.02, boundary_pixels=2), dict(boundary_ratio=-1.0), dict(boundary_pixels=-3),
               dict(mask_type="auto")):
        with pytest.raises(ValueError):
            Evaluator(tmp_path, tmp_path, scorer=lambda *a: [], **kw)
    assert "evaluate" in cli.build_parser().format_help()


def test_no_cpu_fallback(tmp_path):
    from unet_watermark_amd import cli
    from unet_watermark_amd.evaluate import Evaluator
    from unet_watermark_amd.predict import WatermarkPredictor
    from unet_watermark_amd.scoring import score_masks_ragged
    buf = torch.zeros(64, dtype=torch.uint8)
    d = np.zeros(1, [("offset", "<i8"), ("h", "<i4"), ("w", "<i4")]); d[0] = (0, 8, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        score_masks_ragged(buf, buf, d, [1])
    with pytest.raises(RuntimeError, match="HIP device"):
        WatermarkPredictor(device="cpu")
    p = object.__new__(WatermarkPredictor)
    p.device = torch.device("cpu")
    with pytest.raises(RuntimeError, match="HIP device"):
        p.score_images([np.zeros((8, 8, 3), np.uint8)], [np.zeros((8, 8), np.uint8)])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            Evaluator(tmp_path, tmp_path)
        (tmp_path / "m.pth").write_bytes(b"x")
        with pytest.raises(SystemExit, match="HIP device"):
            cli.main(["evaluate", "--input", str(tmp_path), "--masks", str(tmp_path), "--model", str(tmp_path / "m.pth")])


def test_the_new_symbols_are_exported_and_declared(L):
    lib = L.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "uwm.h")).read()
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES and getattr(lib, name) is not None
        assert name + "(" in header
    one = lib.uwm_score_masks_workspace_bytes(1, 64, 1)
    assert one > 0 and one % 256 == 0
    big = lib.uwm_score_masks_workspace_bytes(4, 1 << 20, 4096)                 # six planes of mask_bytes / 64 + rows words
    assert 6 * 8 * ((1 << 20) // 64 + 4096) <= big < 6 * 8 * ((1 << 20) // 64 + 4096) + (1 << 16)
    assert lib.uwm_score_masks_workspace_bytes(4, 1 << 20, 8192) > big
    for bad in ((0, 64, 1), (-1, 64, 1), (65536, 64, 1), (1, 0, 1), (1, 64, 0), (1, 64, -5), (1, 1 << 41, 1), (1, 64, 1 << 41)):
        assert lib.uwm_score_masks_workspace_bytes(*bad) == 0, bad
        assert "uwm_score_masks_workspace_bytes" in lib.uwm_last_error().decode()


def test_uwm_score_masks_ragged_checks_arguments_before_any_launch(L):
    """a null pointer, N / mask_bytes / max_pixels / rows below 1 or too large, a misaligned pointer, a workspace that is too small:
    every such call returns non-zero with a message naming the function, and none reaches a launch (the pointers are host memory)"""
    lib = L.lib()
    keep = (C.c_uint8 * 8192)()
    p = C.c_void_p(C.addressof(keep) + (-C.addressof(keep)) % 16)
    odd4, odd2 = C.c_void_p(p.value + 4), C.c_void_p(p.value + 2)
    need = lib.uwm_score_masks_workspace_bytes(1, 64, 8)
    base = dict(pred=p, truth=p, mask_bytes=64, descs=p, radius=p, N=1, max_pixels=64, rows=8, counts=p, ws=p, ws_bytes=need, st=None)

    def bad(word, **kw):
        rc = lib.uwm_score_masks_ragged(*[kw.get(k, v) for k, v in base.items()])
        assert rc != 0, kw
        msg = lib.uwm_last_error().decode()
        assert "uwm_score_masks_ragged" in msg and word in msg, msg

    for k in ("pred", "truth", "descs", "radius", "counts", "ws"):
        bad("null", **{k: None})
    for k in ("N", "mask_bytes", "max_pixels", "rows"):
        bad(">= 1", **{k: 0})
    bad(">= 1", N=-3); bad(">= 1", rows=-1); bad(">= 1", max_pixels=-7)
    bad("too large", N=65536)
    bad("too large", max_pixels=2 ** 31 - 1)
    bad("too large", rows=1 << 41)
    bad("too large", mask_bytes=1 << 41)
    for k in ("descs", "counts", "ws"):
        bad("aligned", **{k: odd4})
    bad("aligned", radius=odd2)
    bad("too small", ws_bytes=need - 1)
    bad("too small", rows=4096)
    bad("too small", mask_bytes=1 << 20)
