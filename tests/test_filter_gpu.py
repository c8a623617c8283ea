"""The dataset filter on the device (csrc/filter_u8.hip) against the numpy restatement (tests/filter_ref.py), the device morphology it
must agree with, and the layers built on it: uwm_filter_images_u8, WatermarkPredictor.watermark_counts and its captured graph,
WatermarkFilter on a folder.  Masks are compared bit for bit and counts exactly, no pixel is exempted; where the restatement's fp32
and the device's may differ in the last bits (expf, fused multiply-adds), the test first asserts that its INPUTS keep every pixel
further from the threshold than those bits reach (MARGIN)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

TILE_H, TILE_W = 32, 120                    # the kernel's tile (csrc/uwm_kernels.h: kFilterTileH, kFilterTileW)
# one-pixel sides, 3 x 3, rows that are not 4-byte aligned, one pixel past the tile in each dimension, and an image of 3 x 3 tiles
SIZES = [(1, 1), (1, 7), (7, 1), (3, 3), (37, 29), (TILE_H + 1, TILE_W + 1), (2 * TILE_H + 6, 2 * TILE_W + 10)]
PLANE = 16                                  # the logit planes are 16 x 16
THRESHOLDS = (0.5, 0.4)
# no fp64 value of a test's inputs may lie this close to the threshold: about four times the ~5e-7 that a 2-ulp expf, a division and
# three fp32 interpolation steps can move a value <= 1.  A condition on the inputs, not a tolerance
MARGIN = 2e-6
SEED = 1                                    # normal(0, 3) logits whose closest pixel keeps MARGIN at both thresholds (asserted below)
FILL = 77


def _lib():
    from unet_watermark_amd import _lib as L
    return L, L.lib()


def _P(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _mask_layout(shapes, rng):
    """mask descriptors at ANY alignment with gaps of 1..7 bytes in front of, between and behind the masks -> (descs, total bytes)"""
    from unet_watermark_amd.data import DESC_DTYPE
    descs = np.zeros(len(shapes), DESC_DTYPE)
    off = int(rng.integers(1, 8))
    for i, (h, w) in enumerate(shapes):
        descs[i] = (off, h, w)
        off += h * w + int(rng.integers(1, 8))
    return descs, off


def _strided(planes, ld, rng):
    """(N, h, w) fp32 -> a device tensor [N][h][w][ld] with the plane in channel 0 and large noise in the others"""
    x = (rng.normal(0, 50, planes.shape + (ld,))).astype(np.float32)
    x[..., 0] = planes
    return torch.from_numpy(x)


def _run(dev, logits, ld, descs, thr, post, nbytes=None, with_mask=True, mask_bytes=None, guard=0):
    """uwm_prob_mask_count_ragged on host arrays -> (counts (N, 2), the mask buffer or None)"""
    from unet_watermark_amd.data import descs_tensor
    L, lib = _lib()
    n, h, w = logits.shape[:3]
    lg = logits.to(dev).contiguous()
    d_t = descs_tensor(descs, dev)
    mask = torch.full((nbytes + guard,), FILL, dtype=torch.uint8, device=dev) if with_mask else None
    counts = torch.full((n, 2), -1, dtype=torch.int64, device=dev)
    need = lib.uwm_filter_workspace_bytes(n)
    assert need == n * 64 * 8
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    mb = 0 if not with_mask else nbytes if mask_bytes is None else mask_bytes
    L.check(lib.uwm_prob_mask_count_ragged(_P(lg), ld, n, h, w, _P(d_t), float(thr), int(post), _P(mask), mb, _P(counts), _P(ws), ws.numel(),
                                           C.c_void_p(L.stream_ptr(dev))))
    torch.cuda.synchronize(dev)
    return counts.cpu().numpy(), (mask.cpu().numpy() if with_mask else None)


def _check(out, descs, wants, what):
    covered = np.zeros(out.size, bool)
    for i, (d, want) in enumerate(zip(descs, wants)):
        o, h, w = int(d["offset"]), int(d["h"]), int(d["w"])
        got = out[o: o + h * w].reshape(h, w)
        assert np.array_equal(got, want), (what, i, (h, w), np.argwhere(got != want)[:5].tolist())
        covered[o: o + h * w] = True
    assert (out[~covered] == FILL).all(), what               # nothing written before, between or behind the masks


_CASE = {}


def _case():
    """the seeded logit planes, one per image of SIZES, and the restatement's masks per (threshold, post_process), computed once"""
    if not _CASE:
        rng = np.random.default_rng(SEED)
        planes = rng.normal(0, 3, (len(SIZES), PLANE, PLANE)).astype(np.float32)
        _CASE.update(planes=planes,
                     margin={t: min(R.margin(p, h, w, t) for p, (h, w) in zip(planes, SIZES)) for t in THRESHOLDS},
                     want={(t, post): [R.filter_mask(p, h, w, t, post) for p, (h, w) in zip(planes, SIZES)]
                           for t in THRESHOLDS for post in (0, 1)})
    return _CASE


def _counts_of(masks):
    return [[int(np.count_nonzero(m)), m.size] for m in masks]


@pytest.mark.parametrize("ld", [1, 4])
def test_masks_and_counts_equal_the_restatement_on_a_ragged_batch(cuda, ld):
    c = _case()
    for t in THRESHOLDS:                                     # the margin precondition: a statement about the inputs, on the CPU
        assert c["margin"][t] > MARGIN, (t, c["margin"][t])
    frac = np.mean(np.concatenate([m.ravel() for m in c["want"][(0.5, 0)]]) > 0)
    assert 0.3 < frac < 0.7, frac
    big0, big1 = c["want"][(0.5, 0)][-1], c["want"][(0.5, 1)][-1]
    assert (big0 != big1).any() and big1.any() and not big1.all()      # the morphology changes some pixels and keeps some
    rng = np.random.default_rng(31)
    logits = _strided(c["planes"], ld, rng)
    for t in THRESHOLDS:
        for post in (0, 1):
            descs, nbytes = _mask_layout(SIZES, rng)
            counts, out = _run(cuda, logits, ld, descs, t, post, nbytes)
            _check(out, descs, c["want"][(t, post)], f"ld={ld} t={t} post={post}")
            assert counts.tolist() == _counts_of(c["want"][(t, post)]), (ld, t, post)


def test_without_a_mask_the_counts_are_the_same(cuda):
    c = _case()
    rng = np.random.default_rng(32)
    descs, _ = _mask_layout(SIZES, rng)
    logits = torch.from_numpy(c["planes"])
    for post in (0, 1):
        counts, out = _run(cuda, logits, 1, descs, 0.5, post, with_mask=False)
        assert out is None and counts.tolist() == _counts_of(c["want"][(0.5, post)])
    descs["offset"] = -5                                     # without a mask the offsets are not read
    counts, _ = _run(cuda, logits, 1, descs, 0.5, 1, with_mask=False)
    assert counts.tolist() == _counts_of(c["want"][(0.5, 1)])


def _noise_planes():
    """two busy planes of 3 x 3 tiles at the image's own size (the resize is the identity, sigmoid(+-5) is far from the threshold):
    pixel noise of density 0.5 and 0.7, where every pass of the morphology changes pixels on every tile boundary"""
    h, w = 2 * TILE_H + 6, 2 * TILE_W + 10
    rng = np.random.default_rng(33)
    return np.stack([np.where(rng.random((h, w)) < d, 5.0, -5.0) for d in (0.5, 0.7)]).astype(np.float32)


def test_busy_planes_across_tile_boundaries_and_the_device_morphology(cuda):
    """masks of noise planes equal the restatement's, and the post-processed masks equal postprocess.morphology chained on the
    thresholded ones (erode, dilate = open; dilate, erode = close; ellipse 3 x 3), bit for bit"""
    from unet_watermark_amd.postprocess import morphology
    planes = _noise_planes()
    n, h, w = planes.shape
    rng = np.random.default_rng(34)
    descs, nbytes = _mask_layout([(h, w)] * n, rng)
    res = {}
    for post in (0, 1):
        want = [R.filter_mask(p, h, w, 0.5, post) for p in planes]
        counts, out = _run(cuda, torch.from_numpy(planes), 1, descs, 0.5, post, nbytes)
        _check(out, descs, want, f"noise, post={post}")
        assert counts.tolist() == _counts_of(want)
        res[post] = [out[int(d["offset"]): int(d["offset"]) + h * w].reshape(h, w) for d in descs]
    assert all((a != b).any() for a, b in zip(res[0], res[1]))
    # the same chain on the ragged random batch of the first test, image by image
    c = _case()
    descs, nbytes = _mask_layout(SIZES, rng)
    logits = torch.from_numpy(c["planes"])
    _, raw = _run(cuda, logits, 1, descs, 0.4, 0, nbytes)
    _, post = _run(cuda, logits, 1, descs, 0.4, 1, nbytes)
    pairs = list(zip(res[0], res[1])) + [(raw[int(d["offset"]): int(d["offset"]) + int(d["h"]) * int(d["w"])].reshape(int(d["h"]), int(d["w"])),
                                          post[int(d["offset"]): int(d["offset"]) + int(d["h"]) * int(d["w"])].reshape(int(d["h"]), int(d["w"])))
                                         for d in descs]
    for m0, m1 in pairs:
        m = torch.from_numpy(np.ascontiguousarray(m0)).to(cuda)
        for op in ("erode", "dilate", "dilate", "erode"):
            m = morphology(m, op, "ellipse", 3)
        assert np.array_equal(m.cpu().numpy(), m1), m0.shape


def test_a_misfit_descriptor_costs_that_image_only(cuda):
    """a side of 0, a side above 2^30, a negative offset, a region that ends behind mask_bytes: counts {0, 0}, no byte written; the
    neighbours' masks, counts and the bytes around them as without the misfits"""
    shapes = [(20, 30), (16, 16), (9, 13), (12, 40), (TILE_H + 3, 50), (8, 8), (10, 10)]
    rng = np.random.default_rng(35)
    planes = rng.normal(0, 3, (len(shapes), PLANE, PLANE)).astype(np.float32)
    assert min(R.margin(p, h, w, 0.5) for p, (h, w) in zip(planes, shapes)) > MARGIN
    want = [R.filter_mask(p, h, w, 0.5, 1) for p, (h, w) in zip(planes, shapes)]
    descs, nbytes = _mask_layout(shapes, rng)
    good, _ = _run(cuda, torch.from_numpy(planes), 1, descs, 0.5, 1, nbytes)
    assert good.tolist() == _counts_of(want)
    bad = descs.copy()
    bad[1]["h"] = 0
    bad[2]["w"] = (1 << 30) + 1
    bad[3]["offset"] = -4
    bad[5]["h"] = -7
    guard = 64
    mask_bytes = int(descs[6]["offset"]) + 50                # image 6: its mask ends behind mask_bytes
    counts, out = _run(cuda, torch.from_numpy(planes), 1, bad, 0.5, 1, nbytes, mask_bytes=mask_bytes, guard=guard)
    keep = lambda i: np.full(shapes[i], FILL, np.uint8)      # noqa: E731
    _check(out[:nbytes], descs, [want[0], keep(1), keep(2), keep(3), want[4], keep(5), keep(6)], "misfits")
    assert (out[nbytes:] == FILL).all()
    assert counts.tolist() == [good[0].tolist(), [0, 0], [0, 0], [0, 0], good[4].tolist(), [0, 0], [0, 0]]
    # without a mask only the sides can misfit
    counts, _ = _run(cuda, torch.from_numpy(planes), 1, bad, 0.5, 1, with_mask=False)
    assert counts.tolist() == [good[0].tolist(), [0, 0], [0, 0], good[3].tolist(), good[4].tolist(), [0, 0], good[6].tolist()]


def test_the_order_of_sigmoid_and_resize_differs_from_resize_threshold(cuda):
    """logits -1 and +5 resized from 2 to 4 columns: pixel 1 (weight 0.25 on +5) is 0.45 probability first and 0.62 logit first; the
    existing uwm_resize_threshold(apply_sigmoid = 1) keeps its order"""
    from unet_watermark_amd.data import DESC_DTYPE
    from unet_watermark_amd.metrics import resize_threshold
    lg = np.array([[[-1.0, 5.0]]], np.float32)
    assert R.margin(lg[0], 1, 4, 0.5) > 0.04
    descs = np.zeros(1, DESC_DTYPE); descs[0] = (0, 1, 4)
    counts, out = _run(cuda, torch.from_numpy(lg), 1, descs, 0.5, 0, 4)
    assert out.tolist() == [0, 0, 255, 255] and counts.tolist() == [[2, 4]]
    old = resize_threshold(torch.from_numpy(lg).to(cuda), (1, 4), 0.5, apply_sigmoid=True).cpu().numpy()
    assert old.tolist() == [[[0, 255, 255, 255]]]
    assert np.array_equal(old[0] > 0, R.logit_resize_sigmoid(lg[0], 1, 4) > 0.5)


# ------------------------------------------------------------------------------------------------ the model call, the predictor, the folder
def _predictor(dev, frozen=False):
    import unet_watermark_amd as U
    from oracle import unet_oracle as O
    from unet_watermark_amd.config import get_cfg_defaults
    from unet_watermark_amd.predict import WatermarkPredictor
    m = U.Unet("resnet18").to(dev)
    m.load_state_dict(O.build("resnet18", seed=3).state_dict())
    xs, _ = O.synthetic_batch(2, 64, 64, seed=5)
    m.train()
    with torch.no_grad():                                          # representative running statistics
        for k in range(3):
            m(xs.to(dev) * (1.0 + 0.1 * k))
    m.eval()
    cfg = get_cfg_defaults(); cfg.MODEL.NAME = "Unet"; cfg.MODEL.ENCODER_NAME = "resnet18"; cfg.DATA.IMG_SIZE = 64
    return WatermarkPredictor(model=m, config=cfg, device=dev, precision="f32", freeze=frozen)


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


def _median_threshold(pred, images):
    """a probability threshold at the median of the model's probabilities on `images`, so that the masks are neither empty nor full"""
    from unet_watermark_amd.data import descs_tensor, pack_images
    packed, descs, mdescs = pack_images(images)
    dev = pred.device
    counts = torch.zeros((len(images), 2), dtype=torch.int64, device=dev)
    _, logits = pred.model.filter_images_u8(packed.to(dev), descs_tensor(descs, dev), descs_tensor(mdescs, dev), counts, len(images), (64, 64),
                                            (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), 0.5, True, None, return_logits=True)
    return 1.0 / (1.0 + math.exp(-float(logits.median())))


@pytest.mark.parametrize("frozen", [False, True])
def test_filter_images_u8_equals_the_count_kernel_on_its_logits(cuda, frozen):
    from unet_watermark_amd.data import descs_tensor, pack_images
    pred = _predictor(cuda, frozen)
    images = _images([(48, 64), (90, 61), (TILE_H + 8, TILE_W + 9)], 41)
    thr = _median_threshold(pred, images)
    packed, descs, mdescs = pack_images(images)
    nbytes = int(mdescs["offset"][-1]) + images[-1].shape[0] * images[-1].shape[1]
    for post in (True, False):
        mask = torch.full((nbytes,), FILL, dtype=torch.uint8, device=cuda)
        counts = torch.full((3, 2), -1, dtype=torch.int64, device=cuda)
        _, logits = pred.model.filter_images_u8(packed.to(cuda), descs_tensor(descs, cuda), descs_tensor(mdescs, cuda), counts, 3, (64, 64),
                                                (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), thr, post, mask, return_logits=True)
        assert bool(pred.model._frozen) == frozen
        assert logits.shape == (3, 1, 64, 64)
        want_counts, want = _run(cuda, logits.contiguous().view(3, 64, 64).cpu(), 1, mdescs, thr, post, nbytes)
        assert np.array_equal(mask.cpu().numpy(), want) and counts.cpu().numpy().tolist() == want_counts.tolist()
        c = counts.cpu().numpy()
        assert (c[:, 1] == [a.shape[0] * a.shape[1] for a in images]).all() and 0 < c[:, 0].sum() < c[:, 1].sum()
        # no mask: the same counts, nothing else written
        counts2 = torch.full((3, 2), -1, dtype=torch.int64, device=cuda)
        pred.model.filter_images_u8(packed.to(cuda), descs_tensor(descs, cuda), descs_tensor(mdescs, cuda), counts2, 3, (64, 64),
                                    (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), thr, post)
        assert torch.equal(counts2, counts)


def test_one_captured_graph_serves_batches_of_other_sizes(cuda):
    """watermark_counts: the graph captured on the first batch is replayed on a second batch of other sizes and gives that batch's
    eager results, masks included"""
    pred = _predictor(cuda)
    a = _images([(70, 130), (40, 50), (TILE_H + 1, TILE_W + 1)], 42)
    b = _images([(33, 31), (1, 1), (60, 100)], 43)
    pred.threshold = _median_threshold(pred, a)
    eager = {k: pred.watermark_counts(x, return_masks=True, use_graph=False) for k, x in (("a", a), ("b", b))}
    assert 0 < eager["a"][0][:, 0].sum() < eager["a"][0][:, 1].sum()
    got = pred.watermark_counts(a, return_masks=True)
    graph = pred._graphs["counts"].graph
    assert graph is not None
    for k, x in (("a", a), ("b", b), ("a", a)):
        counts, masks = pred.watermark_counts(x, return_masks=True)
        assert pred._graphs["counts"].graph is graph, k                      # replayed, not re-captured
        assert counts.dtype == np.int64 and counts.shape == (3, 2) and counts.tolist() == eager[k][0].tolist(), k
        for m, e, im in zip(masks, eager[k][1], x):
            assert m.shape == im.shape[:2] and torch.equal(m, e), k
    assert got[0].tolist() == eager["a"][0].tolist()
    # counts only: a graph of its own (no mask pointer in it), the same numbers; post_process=None reads the config
    assert pred.watermark_counts(b).tolist() == eager["b"][0].tolist()
    pred.cfg.PREDICT.POST_PROCESS = False
    off = pred.watermark_counts(b)
    assert off.tolist() == pred.watermark_counts(b, post_process=False, use_graph=False).tolist()


def test_watermark_filter_on_a_folder(cuda, tmp_path):
    from PIL import Image
    from unet_watermark_amd.filter import WatermarkFilter
    pred = _predictor(cuda)
    images = _images([(48, 64), (50, 70), (61, 45), (33, 47), (TILE_H + 8, TILE_W + 9), (40, 40)], 44)
    root, out = tmp_path / "in", tmp_path / "out"
    os.makedirs(root)
    for i, a in enumerate(images):
        Image.fromarray(a).save(str(root / f"im{i}.png"))
    pred.cfg.PREDICT.THRESHOLD = _median_threshold(pred, images)
    lines = []
    flt = WatermarkFilter(None, config=pred.cfg, model=pred.model, device=cuda, batch_size=4, log=lines.append)
    ratios = {}
    for i, a in enumerate(images):
        has, ratio = flt.has_watermark(str(root / f"im{i}.png"))
        m = flt.predict_mask(str(root / f"im{i}.png"))
        assert m.shape == a.shape[:2] and m.dtype == np.uint8 and set(np.unique(m).tolist()) <= {0, 255}
        assert ratio == int(np.count_nonzero(m)) / (a.shape[0] * a.shape[1]) and has == (ratio >= flt.watermark_threshold)
        ratios[f"im{i}.png"] = ratio
    order = sorted(ratios.values())
    k = int(np.argmax(np.diff(order)))                       # the threshold goes into the widest gap of the sorted ratios
    assert order[k + 1] - order[k] > 0.01, order
    flt.watermark_threshold = (order[k] + order[k + 1]) / 2
    low = sorted(n for n, r in ratios.items() if r < flt.watermark_threshold)
    stats = flt.filter_images(str(root), no_watermark_dir=str(out))
    assert stats == {"total": 6, "with_watermark": 6 - len(low), "without_watermark": len(low), "moved": len(low), "errors": 0}
    assert sorted(os.listdir(out)) == low and sorted(os.listdir(root)) == sorted(set(ratios) - set(low))
    assert sum(ln.startswith("move:") for ln in lines) == len(low) and sum(ln.startswith("keep:") for ln in lines) == 6 - len(low)
