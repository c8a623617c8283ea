"""Mask post-processing on the device against the numpy restatement (tests/maskpost_ref.py) and the golden case list
(tests/golden/maskpost.npz).  Everything here is integer work: every comparison is byte equality, no case is skipped."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maskpost_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ELEMENTS = [("ellipse", (s, s)) for s in (2, 3, 4, 5, 6, 7, 9, 11)] + [("rect", (5, 1)), ("rect", (1, 5))]


@pytest.fixture(scope="module")
def U(cuda):
    import __graft_entry__ as g
    g.build()
    import unet_watermark_amd as U
    return U


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _seeded():
    """the seeded masks of the case list, one (N,H,W) bool batch per size (width 517: not a multiple of 64 or 4)"""
    return [np.stack([R.synth(h, w, 100 + 7 * i + s) for s in range(2)]) for i, (h, w) in enumerate(R.SEEDED_SIZES)]


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


@pytest.mark.parametrize("shape,ksize", ELEMENTS, ids=[f"{s}{k[0]}x{k[1]}" for s, k in ELEMENTS])
def test_morph_equals_restatement(U, cuda, shape, ksize):
    k = R.element(R.ELLIPSE if shape == "ellipse" else R.RECT, *ksize)
    assert np.array_equal(U.structuring_element(shape, ksize), k)
    for batch in _seeded():
        x = _dev(batch.astype(np.uint8) * 255, cuda)
        for op, ref in (("dilate", R.dilate), ("erode", R.erode)):
            for it in (1, 2, 3):
                got = U.morphology(x, op, shape, ksize, it).cpu().numpy()
                want = np.stack([ref(m, k, it) for m in batch]).astype(np.uint8) * 255
                assert np.array_equal(got, want), (op, it, batch.shape, int((got != want).sum()))


def test_morph_threshold_is_127_and_single_image_shape(U, cuda):
    g = np.random.default_rng(5)
    raw = g.integers(0, 256, (45, 131), dtype=np.uint8)
    raw[0, :4] = (127, 128, 0, 255)
    k = R.ellipse(3, 3)
    got = U.morphology(_dev(raw, cuda), "dilate", "ellipse", 3).cpu().numpy()
    assert got.shape == raw.shape and np.array_equal(got, R.dilate(raw > 127, k).astype(np.uint8) * 255)


def test_components_equal_restatement(U, cuda):
    batches = _seeded() + [np.ones((1, 96, 160), bool), np.zeros((1, 96, 160), bool), np.ones((1, 1, 1), bool), np.ones((1, 1, 130), bool)]
    yy, xx = np.mgrid[:300, :517]
    batches.append((((yy // 3 + xx // 5) % 2 == 0) & ((yy * 7 + xx * 3) % 11 != 0))[None])      # many small touching cells
    spiral = np.zeros((129, 257), bool)                                                         # one long winding component
    for r in range(0, 64, 2):
        spiral[r, r:257 - r] = True; spiral[128 - r, r:257 - r] = True
        spiral[r:129 - r, 256 - r] = True; spiral[r + 2:129 - r, r] = True
    batches.append(spiral[None])
    for batch in batches:
        labels, areas = U.connected_components(_dev(batch.astype(np.uint8) * 255, cuda))
        labels, areas = labels.cpu().numpy(), areas.cpu().numpy()
        assert labels.dtype == np.int32 and areas.dtype == np.int32
        for i, m in enumerate(batch):
            wl, wa = R.components(m)
            assert np.array_equal(labels[i], wl), (batch.shape, i)
            assert np.array_equal(areas[i], wa), (batch.shape, i)


@pytest.mark.parametrize("mask_type", R.MASK_TYPES)
def test_optimize_mask_equals_golden(U, cuda, golden, mask_type):
    """the whole case list, out of place and in place, summaries included; a batch equals its images one by one; a second
    call gives the same bytes"""
    assert len(golden) == 10 + 2 * len(R.SEEDED_SIZES)
    for name, x, exp in golden:
        want, want_summary = exp[mask_type]
        xd = _dev(x, cuda)
        got, summary = U.optimize_mask(xd, mask_type, return_summary=True)
        assert got.shape == x.shape and got.dtype == torch.uint8 and summary.dtype == torch.int64
        bad = int((got.cpu().numpy() != want).sum())
        print(f"{mask_type} {name}: {bad} differing bytes, summary {summary.cpu().tolist()}")
        assert bad == 0, (name, bad)
        assert np.array_equal(summary.cpu().numpy(), want_summary), (name, summary.cpu().tolist(), want_summary.tolist())
        assert torch.equal(xd.cpu(), torch.from_numpy(x))                       # the input is left alone
        again = U.optimize_mask(xd, mask_type)
        assert torch.equal(again, got), name
        inplace = xd.clone()
        r, s2 = U.optimize_mask(inplace, mask_type, return_summary=True, out=inplace)
        assert r is inplace and torch.equal(inplace, got) and torch.equal(s2, summary), name
        for i in range(x.shape[0]):
            one, s1 = U.optimize_mask(xd[i], mask_type, return_summary=True)
            assert one.shape == x.shape[1:] and torch.equal(one, got[i]) and torch.equal(s1, summary[i]), (name, i)


def test_optimize_mask_takes_any_byte_values(U, cuda):
    g = np.random.default_rng(9)
    base = R.synth(120, 333, 4)
    raw = np.where(base, g.integers(128, 256, base.shape), g.integers(0, 128, base.shape)).astype(np.uint8)
    for t in R.MASK_TYPES:
        want, ws = R.optimize_mask(raw, t)
        got, s = U.optimize_mask(_dev(raw, cuda), t, return_summary=True)
        assert np.array_equal(got.cpu().numpy(), want) and s.cpu().tolist() == ws


def _predictor(U, cuda, freeze=False):
    from unet_watermark_amd.predict import WatermarkPredictor
    torch.manual_seed(3)
    pred = WatermarkPredictor(model=U.Unet("resnet18"), device="cuda", freeze=freeze)
    pred.threshold = 0.0                      # a random-weight model: raw logits around zero give busy masks
    return pred


@pytest.mark.parametrize("mask_type", R.MASK_TYPES)
def test_predictor_graph_replay_equals_two_steps(U, cuda, mask_type):
    pred = _predictor(U, cuda, freeze=True)
    g = torch.Generator().manual_seed(1)
    imgs = [torch.randint(0, 256, (2, 64, 96, 3), dtype=torch.uint8, generator=g).to(cuda) for _ in range(3)]
    for out_size in (None, (75, 133)):
        raws = [pred.predict_mask_u8(im, out_size=out_size).clone() for im in imgs]        # the parent path: one capture, two replays
        for im, raw in zip(imgs, raws):
            assert torch.equal(raw, pred.model.predict_u8(im, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), 0.0, False, out_size))
        wants = [U.optimize_mask(raw, mask_type, return_summary=True) for raw in raws]
        for rep in range(2):                  # the first call captures, the others replay
            for im, raw, (want, want_s) in zip(imgs, raws, wants):
                got, s = pred.predict_mask_u8(im, out_size=out_size, mask_type=mask_type, return_summary=True)
                assert torch.equal(got, want) and torch.equal(s, want_s)
                assert torch.equal(pred.predict_mask_u8(im, out_size=out_size, mask_type=mask_type), want)
        assert np.array_equal(wants[0][0][0].cpu().numpy(), R.optimize_mask(raws[0][0].cpu().numpy(), mask_type)[0])
        assert raws[0].any() and not raws[0].all()
        assert torch.equal(pred.predict_mask_u8(imgs[1], out_size=out_size, mask_type=mask_type, use_graph=False), wants[1][0])
        assert torch.equal(pred.predict_mask_u8(imgs[2], out_size=out_size), raws[2])      # None: the masks as they were
    x = pred.preprocess(imgs[0])
    raw = pred.predict_mask(x).clone()
    assert torch.equal(raw, U.threshold_mask(pred.logits(x, use_graph=False), 0.0))
    for _ in range(2):
        assert torch.equal(pred.predict_mask(x, mask_type=mask_type), U.optimize_mask(raw, mask_type))
    assert torch.equal(pred.predict_mask(x, mask_type=mask_type, use_graph=False), U.optimize_mask(raw, mask_type))
    with pytest.raises(ValueError):
        pred.predict_mask_u8(imgs[0], mask_type="logo")
    with pytest.raises(ValueError):
        pred.predict_mask_u8(imgs[0], return_summary=True)


def test_cli_writes_optimised_masks(U, cuda, tmp_path):
    from PIL import Image
    from unet_watermark_amd import cli
    from unet_watermark_amd.checkpoint import save_checkpoint
    from unet_watermark_amd.config import get_cfg_defaults
    from unet_watermark_amd.model import create_model_from_config
    cfg = get_cfg_defaults()
    cfg.MODEL.ENCODER_NAME = "resnet18"
    torch.manual_seed(5)
    save_checkpoint(str(tmp_path / "m.pth"), create_model_from_config(cfg), 1)
    src = tmp_path / "in"
    src.mkdir()
    g = np.random.default_rng(2)
    for name, (h, w) in (("a.png", (70, 101)), ("b.png", (96, 64))):
        Image.fromarray(g.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(src / name)
    common = ["predict", "--input", str(src), "--model", str(tmp_path / "m.pth"), "--encoder", "resnet18", "--threshold", "0.0",
              "--batch-size", "2"]
    cli.main(common + ["--output", str(tmp_path / "raw")])
    for t in R.MASK_TYPES:
        cli.main(common + ["--output", str(tmp_path / t), "--mask-type", t])
        for name, (h, w) in (("a_mask.png", (70, 101)), ("b_mask.png", (96, 64))):
            raw = np.asarray(Image.open(tmp_path / "raw" / name))
            got = np.asarray(Image.open(tmp_path / t / name))
            assert raw.shape == (h, w) and got.shape == (h, w) and raw.any()
            assert np.array_equal(got, R.optimize_mask(raw, t)[0]), (t, name)


def test_graph_survives_a_larger_eager_call(U, cuda):
    """the post-processing workspace is one buffer per device that grows; a captured graph keeps the buffer it was captured with"""
    from unet_watermark_amd import _device as D, postprocess as PP
    pred = _predictor(U, cuda)
    D._WORKSPACE.pop(("mask", D.resolve(cuda)), None)      # (earlier tests have grown the buffer: start from none)
    g = torch.Generator().manual_seed(4)
    im = torch.randint(0, 256, (1, 64, 64, 3), dtype=torch.uint8, generator=g).to(cuda)
    first, s_first = pred.predict_mask_u8(im, mask_type="mixed", return_summary=True)
    first, s_first = first.clone(), s_first.clone()
    small = PP.workspace(cuda, 1, 64, 64)
    big = _dev(R.synth(900, 1100, 8).astype(np.uint8) * 255, cuda)
    want = R.optimize_mask(big.cpu().numpy(), "mixed")[0]
    assert np.array_equal(U.optimize_mask(big, "mixed").cpu().numpy(), want)
    assert PP.workspace(cuda, 1, 64, 64).numel() >= PP.workspace(cuda, 1, 900, 1100).numel() > small.numel()
    again, s_again = pred.predict_mask_u8(im, mask_type="mixed", return_summary=True)       # a replay, on the old buffer
    assert torch.equal(again, first) and torch.equal(s_again, s_first)
