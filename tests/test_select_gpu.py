"""Ragged post-processing inside predict_images, mask_stats, and checkpoint selection on a folder, on the device with a seeded,
untrained Unet('resnet18') at IMG_SIZE 64.  Both sides of every comparison start from the same thresholded masks and everything
behind them is integer work, so every comparison is exact."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maskpost_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES_A = [(17, 23), (200, 333), (64, 64), (90, 61), (131, 140)]
SIZES_B = [(60, 100), (23, 17), (150, 300), (64, 65), (33, 200)]          # no more bytes, pixels per image or rows than SIZES_A
SIZES_BIG = [(40, 40), (500, 700), (64, 64), (10, 10), (20, 300)]
_STATE = {}


def _model(dev, seed):
    import unet_watermark_amd as U
    from oracle import unet_oracle as O
    m = U.Unet("resnet18").to(dev)
    m.load_state_dict(O.build("resnet18", seed=seed).state_dict())
    xs, _ = O.synthetic_batch(2, 64, 64, seed=5)
    m.train()
    with torch.no_grad():                                          # representative running statistics
        for k in range(3):
            m(xs.to(dev) * (1.0 + 0.1 * k))
    return m.eval()


def _cfg():
    from unet_watermark_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults(); cfg.MODEL.NAME = "Unet"; cfg.MODEL.ENCODER_NAME = "resnet18"; cfg.DATA.IMG_SIZE = 64
    return cfg


def _images(shapes, seed):
    """smooth random images with a bright rectangle each: their logits differ from image to image"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    out = []
    for i, (h, w) in enumerate(shapes):
        base = rng.integers(0, 256, size=(h // 6 + 2, w // 6 + 2, 3), dtype=np.uint8)
        a = np.asarray(Image.fromarray(base).resize((w, h), Image.BILINEAR)).copy()
        a[h // 4: h // 4 + h // (2 + i % 3), w // 5: w // 5 + w // 2] = 255 - 40 * (i % 4)
        out.append(a)
    return out


def _median_logit(model, images, dev):
    """the median logit on `images` as the threshold, so that the masks are neither empty nor full"""
    import unet_watermark_amd as U
    from unet_watermark_amd.constants import IMAGENET_MEAN, IMAGENET_STD
    packed, descs, _ = U.pack_images(images)
    _, lg = model.predict_u8(U.device_resize(packed, descs, 64, 3), IMAGENET_MEAN, IMAGENET_STD, 0.0, return_logits=True)
    return float(lg.median())


def _pred(cuda):
    """one predictor for the module (its graphs are part of what is tested)"""
    if "pred" not in _STATE:
        import __graft_entry__ as g
        g.build()
        from unet_watermark_amd.predict import WatermarkPredictor
        pred = WatermarkPredictor(model=_model(cuda, 3), config=_cfg(), device=cuda, precision="f32")
        pred.threshold = _median_logit(pred.model, _images(SIZES_A, 51), cuda)
        _STATE["pred"] = pred
    return _STATE["pred"]


def _parent_route(pred, images, mask_type):
    """what predict_images(mask_type=...) was before the ragged call: the raw masks, then optimize_mask image by image"""
    from unet_watermark_amd.postprocess import optimize_mask
    return [optimize_mask(m, mask_type) for m in pred.predict_images(images, mask_type=None, use_graph=False)]


def _stats_of(mask, raw, mask_type):
    """the stats row recomputed from a returned mask: entries 2, 4, 5, 6 from the mask's own components; entries 0, 1, 3 need the
    pre-selection plane, which the restatement derives from the raw mask"""
    _, areas = R.components(mask > 127)
    a = areas[areas > 0]
    plane = R._chain(raw > 127, mask_type)
    _, pa = R.components(plane)
    flat = pa.reshape(-1)
    ids = np.nonzero(flat)[0]
    big = int(ids[np.argmax(flat[ids])]) if len(ids) else -1
    return [len(ids), int(flat[big]) if len(ids) else 0, int((mask > 127).sum()), big, len(a), int(a.max()) if len(a) else 0, mask.size, 0]


@pytest.mark.parametrize("mask_type", R.MASK_TYPES)
def test_predict_images_returns_the_masks_it_returned_before(cuda, mask_type):
    pred = _pred(cuda)
    images = _images(SIZES_A, 51)
    want = _parent_route(pred, images, mask_type)
    raw = pred.predict_images(images, use_graph=False)
    assert all(0.05 < float((m > 0).float().mean()) < 0.95 for m in raw)
    assert any(not torch.equal(r, w) for r, w in zip(raw, want))                   # the post-processing changes something
    for use_graph in (False, True):
        got, stats = pred.predict_images(images, mask_type=mask_type, use_graph=use_graph, return_stats=True)
        assert stats.dtype == np.int64 and stats.shape == (5, 8) and (stats[:, 7] == 0).all()
        for im, g, w in zip(images, got, want):
            assert g.dtype == torch.uint8 and tuple(g.shape) == im.shape[:2] and torch.equal(g, w), (mask_type, use_graph, im.shape)
        assert stats[:, 2].tolist() == [int((w > 0).sum()) for w in want] and stats[:, 6].tolist() == [h * w for h, w in SIZES_A]
    with pytest.raises(ValueError):
        pred.predict_images(images, return_stats=True)


def test_one_graph_serves_batches_that_fit_and_a_larger_one_recaptures(cuda):
    pred = _pred(cuda)
    a, b, big = _images(SIZES_A, 51), _images(SIZES_B, 52), _images(SIZES_BIG, 53)
    assert sum(h * w for h, w in SIZES_B) <= sum(h * w for h, w in SIZES_A) and sum(h for h, _ in SIZES_B) <= sum(h for h, _ in SIZES_A)
    assert max(h * w for h, w in SIZES_B) <= max(h * w for h, w in SIZES_A)
    pred.predict_images(a)
    pred.predict_images(a, mask_type="watermark")
    graph, plain = pred._graphs["images_post"].graph, pred._graphs["images"].graph
    assert graph is not None and plain is not None
    for imgs in (b, a, b):
        got = pred.predict_images(imgs, mask_type="watermark")
        assert pred._graphs["images_post"].graph is graph                                               # replayed, not re-captured
        for g, w in zip(got, _parent_route(pred, imgs, "watermark")):
            assert torch.equal(g, w)
    assert pred._graphs["images"].graph is plain                                                   # (the graph without post-processing is left alone)
    got = pred.predict_images(big, mask_type="watermark")                          # 500 x 700 exceeds every capacity
    assert pred._graphs["images_post"].graph is not graph and pred._graphs["images_post"].graph is not None
    for g, w in zip(got, _parent_route(pred, big, "watermark")):
        assert torch.equal(g, w)
    graph = pred._graphs["images_post"].graph
    for g, w in zip(pred.predict_images(a, mask_type="watermark"), _parent_route(pred, a, "watermark")):      # fits the grown capacities
        assert torch.equal(g, w)
    assert pred._graphs["images_post"].graph is graph


@pytest.mark.parametrize("mask_type", R.MASK_TYPES)
def test_mask_stats_equal_statistics_of_the_returned_masks(cuda, mask_type):
    pred = _pred(cuda)
    images = _images(SIZES_B, 52)
    raw = [m.cpu().numpy() for m in pred.predict_images(images, use_graph=False)]
    stats, masks = pred.mask_stats(images, mask_type, return_masks=True)
    only = pred.mask_stats(images, mask_type)
    assert isinstance(only, np.ndarray) and only.dtype == np.int64 and only.shape == (5, 8) and np.array_equal(only, stats)
    assert np.array_equal(pred.mask_stats(images, mask_type, use_graph=False), stats)
    for m, w in zip(masks, _parent_route(pred, images, mask_type)):
        assert torch.equal(m, w)
    for row, m, r in zip(stats, masks, raw):
        assert row.tolist() == _stats_of(m.cpu().numpy(), r, mask_type), (mask_type, m.shape)
    with pytest.raises(ValueError):
        pred.mask_stats(images, "auto")


def test_mask_stats_none_type_describes_the_raw_masks(cuda):
    pred = _pred(cuda)
    images = _images(SIZES_B, 52)
    stats, masks = pred.mask_stats(images, "none", return_masks=True)
    for row, m, r in zip(stats, masks, pred.predict_images(images, use_graph=False)):
        assert torch.equal(m, r)
        _, areas = R.components(r.cpu().numpy() > 127)
        a = areas[areas > 0]
        assert [row[0], row[1], row[2], row[4], row[5], row[6], row[7]] == [len(a), int(a.max()), int(a.sum()), len(a), int(a.max()), m.numel(), 0]


def test_model_selector_on_a_folder(cuda, tmp_path):
    from PIL import Image
    from unet_watermark_amd.checkpoint import save_checkpoint
    from unet_watermark_amd.predict import WatermarkPredictor
    from unet_watermark_amd.select import DETECTION_RATIO, ModelSelector
    shapes = [(48, 64), (50, 70), (61, 45), (33, 47), (120, 90), (40, 40), (75, 110)]
    images = _images(shapes, 54)
    os.makedirs(tmp_path / "in")
    for i, a in enumerate(images):
        Image.fromarray(a).save(str(tmp_path / "in" / f"im{i}.png"))
    with open(tmp_path / "in" / "broken.png", "wb") as f:
        f.write(b"not an image")
    os.makedirs(tmp_path / "m" / "run2")
    cfg = _cfg()
    models = {"a.pth": _model(cuda, 3), os.path.join("run2", "b.pth"): _model(cuda, 4)}
    for name, m in models.items():
        save_checkpoint(str(tmp_path / "m" / name), m, epoch=1)
    with open(tmp_path / "m" / "corrupt.pth", "wb") as f:
        f.write(b"\x00\x01 this is no checkpoint")
    cfg.PREDICT.THRESHOLD = _median_logit(models["a.pth"], images, cuda)
    sel = ModelSelector(tmp_path / "in", tmp_path / "m", tmp_path / "out", num_samples=100, config=cfg, mask_type="mixed", batch_size=3,
                        log=None)
    res = sel.run_evaluation()
    with open(tmp_path / "out" / "model_evaluation_results.json", encoding="utf-8") as f:
        assert json.load(f) == res
    assert set(res) == {"timestamp", "input_dir", "model_dir", "num_samples", "selected_images", "models", "summary"}
    assert res["num_samples"] == 8 and res["selected_images"] == ["broken.png"] + [f"im{i}.png" for i in range(7)]
    assert list(res["models"]) == ["a.pth", "corrupt.pth", os.path.join("run2", "b.pth")]
    bad = res["models"]["corrupt.pth"]
    assert bad["load_error"] and bad["statistics"] is None and bad["predictions"] == []
    assert res["summary"]["total_models"] == 3 and res["summary"]["successful_models"] == 2 and res["summary"]["failed_models"] == 1
    assert os.listdir(tmp_path / "out") == ["model_evaluation_results.json"]      # no masks without save_masks
    rates = {}
    for name, m in models.items():
        entry = res["models"][name]
        assert set(entry) == {"model_path", "model_name", "model_info", "predictions", "statistics"}
        assert entry["model_path"] == str(tmp_path / "m" / name) and "load_error" not in entry
        preds = entry["predictions"]
        assert [p["image_name"] for p in preds] == res["selected_images"]
        assert not preds[0]["success"] and preds[0]["error"] and all(p["success"] for p in preds[1:])
        stats = WatermarkPredictor(model=m, config=cfg, device=cuda).mask_stats(images, "mixed", use_graph=False)
        ratios = [int(r[2]) / int(r[6]) for r in stats]
        for p, r, row in zip(preds[1:], ratios, stats):
            assert p["metrics"] == {"watermark_ratio": r, "watermark_pixels": int(row[2]), "total_pixels": int(row[6]),
                                    "num_components": int(row[4]), "max_component_area": int(row[5]),
                                    "max_component_ratio": int(row[5]) / int(row[6]) if row[4] else 0.0}
        st = entry["statistics"]
        assert (st["total_predictions"], st["successful_predictions"], st["failed_predictions"]) == (8, 7, 1)
        assert st["detection_rate"] == float(np.mean([1 if r > DETECTION_RATIO else 0 for r in ratios]))
        assert st["avg_watermark_ratio"] == float(np.mean(ratios)) and st["std_watermark_ratio"] == float(np.std(ratios))
        assert st["min_watermark_ratio"] == min(ratios) and st["max_watermark_ratio"] == max(ratios)
        rates[name] = st["detection_rate"]
    assert res["models"]["a.pth"]["statistics"]["max_watermark_ratio"] > 0      # (the threshold is a's median logit)
    first_max = [n for n in ("a.pth", os.path.join("run2", "b.pth")) if rates[n] == max(rates.values())][0]
    assert res["summary"]["best_detection_model"] == {"name": first_max, "detection_rate": rates[first_max]}
    # with save_masks: one PNG per readable image and loaded model, equal to the predictor's masks
    sel = ModelSelector(tmp_path / "in", tmp_path / "m" / "a.pth", tmp_path / "out2", config=cfg, mask_type="mixed", batch_size=4, save_masks=True,
                        log=None)
    res2 = sel.run_evaluation()
    assert list(res2["models"]) == ["a.pth"] and res2["models"]["a.pth"]["statistics"] == res["models"]["a.pth"]["statistics"]
    assert sorted(os.listdir(tmp_path / "out2")) == sorted(["model_evaluation_results.json"] + [f"im{i}_a_mask.png" for i in range(7)])
    want = WatermarkPredictor(model=models["a.pth"], config=cfg, device=cuda).predict_images(images, mask_type="mixed", use_graph=False)
    for i, w in enumerate(want):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out2" / f"im{i}_a_mask.png")), w.cpu().numpy())
