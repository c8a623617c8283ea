"""uwm_score_masks_ragged on the device: a ragged batch of the smallest shapes that can go wrong, a row wider than one LDS stretch,
misfits, pred == truth, repeatability and aliasing, a replayed graph, WatermarkPredictor.score_images on the three predict paths and
`main.py evaluate` end to end.  Every count is an integer: every comparison is equality with the restatement (tests/score_ref.py)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0x5A                                   # what guard bands must keep
GUARD = 64
SHAPES = ((1, 1), (1, 70), (5, 3), (17, 63), (17, 64), (9, 65), (33, 127), (33, 128), (33, 129), (40, 200), (130, 257))
RADII = (0, 1, 2, 3, 7, 31, 32, 33, 40, 300)
KINDS = ("half", "dense", "denser", "set", "clear", "rectangle", "grey")


@pytest.fixture(scope="module")
def L(cuda):
    import __graft_entry__ as g
    g.build()
    from unet_watermark_amd import _lib
    _lib.lib()
    return _lib


def _mask(kind, h, w, rng):
    if kind in ("half", "dense", "denser"):
        return ((rng.random((h, w)) < {"half": 0.5, "dense": 0.9, "denser": 0.99}[kind]) * 255).astype(np.uint8)
    if kind == "set":
        return np.full((h, w), 255, np.uint8)
    if kind == "clear":
        return np.zeros((h, w), np.uint8)
    if kind == "rectangle":                   # filled, touching the top and the left border
        m = np.zeros((h, w), np.uint8)
        m[: max(1, 3 * h // 4), : max(1, 5 * w // 6)] = 255
        return m
    return rng.choice(np.array([126, 127, 128, 129], np.uint8), size=(h, w))      # grey values either side of the > 127 rule


def _descs(shapes, first=0):
    """the masks back to back from byte `first` on, so most regions start unaligned -> (descs, total bytes)"""
    from unet_watermark_amd.data import DESC_DTYPE
    d = np.zeros(len(shapes), DESC_DTYPE)
    off = first
    for i, (h, w) in enumerate(shapes):
        d[i] = (off, h, w)
        off += h * w
    return d, off


def _pack(masks, descs, nbytes):
    buf = np.full(nbytes + GUARD, FILL, np.uint8)
    for m, d in zip(masks, descs):
        o = int(d["offset"])
        buf[o:o + m.size] = m.reshape(-1)
    return buf


def _call(L, cuda, pred, truth, descs, radii, nbytes, max_pixels=None, rows=None, alias=False):
    """the ABI call on host buffers of nbytes + GUARD bytes, of which the call is told nbytes -> counts (N, 8); checks that neither
    input was written and that the guard entries behind the radii, the counts and the workspace are intact"""
    from unet_watermark_amd.data import descs_tensor
    lib = L.lib()
    n = len(descs)
    if max_pixels is None:
        max_pixels = int((descs["h"].astype(np.int64) * descs["w"]).max())
    if rows is None:
        rows = int(descs["h"].sum())
    p = torch.from_numpy(pred).to(cuda)
    t = p if alias else torch.from_numpy(truth).to(cuda)
    dd = descs_tensor(descs, cuda)
    rr = torch.full((n + 4,), -12345, dtype=torch.int32, device=cuda)
    rr[:n] = torch.tensor(list(radii), dtype=torch.int32)
    counts = torch.full((n + 1, 8), -77, dtype=torch.int64, device=cuda)
    need = lib.uwm_score_masks_workspace_bytes(n, nbytes, rows)
    assert need > 0
    ws = torch.empty(need + 256, dtype=torch.uint8, device=cuda)
    ws[need:] = FILL
    L.check(lib.uwm_score_masks_ragged(C.c_void_p(p.data_ptr()), C.c_void_p(t.data_ptr()), nbytes, C.c_void_p(dd.data_ptr()),
                                       C.c_void_p(rr.data_ptr()), n, max_pixels, rows, C.c_void_p(counts.data_ptr()), C.c_void_p(ws.data_ptr()),
                                       need, C.c_void_p(L.stream_ptr(cuda))))
    torch.cuda.synchronize(cuda)
    assert bool((ws[need:] == FILL).all()), "a write behind the workspace"
    assert bool((counts[n] == -77).all()), "a write behind the counts"
    assert bool((rr[n:] == -12345).all()), "the radii were written"
    assert np.array_equal(p.cpu().numpy(), pred), "pred was written"
    if not alias:
        assert np.array_equal(t.cpu().numpy(), truth), "truth was written"
    assert np.array_equal(dd.cpu().numpy(), descs_tensor(descs).numpy()), "the descriptors were written"
    return counts[:n].cpu().numpy()


_BATCH = {}


def _batch():
    """every shape at every radius, the mask kinds dealt round-robin: 110 pairs, with their reference counts (computed once)"""
    if not _BATCH:
        rng = np.random.default_rng(2021)
        shapes, radii, preds, truths = [], [], [], []
        for r, d in enumerate(RADII):
            for i, (h, w) in enumerate(SHAPES):
                shapes.append((h, w)); radii.append(d)
                preds.append(_mask(KINDS[(i + r) % len(KINDS)], h, w, rng))
                truths.append(_mask(KINDS[(i + 3 * r + 2) % len(KINDS)], h, w, rng))
        descs, nbytes = _descs(shapes, first=3)
        _BATCH.update(shapes=shapes, radii=radii, preds=preds, truths=truths, descs=descs, nbytes=nbytes,
                      want=SR.counts_batch(preds, truths, radii))
    return _BATCH


def test_one_ragged_batch_of_the_smallest_shapes_that_can_go_wrong(L, cuda):
    b = _batch()
    got = _call(L, cuda, _pack(b["preds"], b["descs"], b["nbytes"]), _pack(b["truths"], b["descs"], b["nbytes"]), b["descs"], b["radii"],
                b["nbytes"])
    for i, (s, d) in enumerate(zip(b["shapes"], b["radii"])):
        assert got[i].tolist() == b["want"][i].tolist(), (i, s, d)
    assert (got[:, :4].sum(axis=1) == [h * w for h, w in b["shapes"]]).all()
    assert any(2 * d + 1 > min(s) for s, d in zip(b["shapes"], b["radii"])) and (got[[d == 0 for d in b["radii"]], 4:7] == 0).all()
    assert (b["want"][:, 4] > 0).sum() > 40 and len({tuple(r) for r in b["want"][:, 4:7].tolist()}) > 60      # the boundary part is exercised


def test_a_row_wider_than_one_stretch_and_a_column_of_many_segments(L, cuda):
    """a 3 x 100000 pair (one wave's LDS stretch holds 1536 words less the halo: 1566 words need two) at a small and a large radius
    on both sides of the stretch border, and a 5000 x 3 pair whose columns take many segments; a run of set pixels crosses the border"""
    rng = np.random.default_rng(7)
    shapes = [(3, 100000), (131, 100000), (5000, 3)]
    radii = [1, 65, 1]
    preds = [_mask("denser", h, w, rng) for h, w in shapes]
    truths = [_mask("denser", h, w, rng) for h, w in shapes]
    for m in preds[:2]:
        m[:, 90000:99000] = 255
    preds[1][:, 40000:] = 255
    truths[1][:, 60000:] = 255
    preds[2][1000:3000] = 255
    descs, nbytes = _descs(shapes, first=1)
    got = _call(L, cuda, _pack(preds, descs, nbytes), _pack(truths, descs, nbytes), descs, radii, nbytes)
    want = SR.counts_batch(preds, truths, radii)
    assert got.tolist() == want.tolist()
    assert want[1][5] < (preds[1] > 127).sum() and want[1][4] > 0                  # E_65 is not empty there


def test_radii_of_several_words_on_either_side_of_the_one_word_per_lane_limit(L, cuda):
    """a row with its halo of ceil(d / 64) words on either side is served from registers up to 64 words and from LDS beyond: 60 + 2 * 2
    words is the last that fits, 61 + 2 * 2 the first that does not; 300 x 400 at d = 70 and 130 shifts by more than a word"""
    rng = np.random.default_rng(13)
    shapes = [(300, 400), (300, 400), (200, 3840), (210, 3900), (140, 4000)]
    radii = [70, 130, 88, 100, 64]
    preds, truths = [], []
    for h, w in shapes:
        p, t = _mask("denser", h, w, rng), _mask("rectangle", h, w, rng)
        p[2:, w // 10: w - 3] = 255
        t[5:, : w // 2] |= _mask("denser", h - 5, w // 2, rng)
        preds.append(p); truths.append(t)
    descs, nbytes = _descs(shapes, first=2)
    got = _call(L, cuda, _pack(preds, descs, nbytes), _pack(truths, descs, nbytes), descs, radii, nbytes)
    want = SR.counts_batch(preds, truths, radii)
    assert got.tolist() == want.tolist()
    assert all(0 < row[5] < (p > 127).sum() and row[4] > 0 for row, p in zip(want, preds))      # no erosion is empty or the identity


def test_misfits_get_status_one_and_cost_their_neighbours_nothing(L, cuda):
    from unet_watermark_amd.data import DESC_DTYPE
    rng = np.random.default_rng(11)
    good = [(17, 64), (33, 129), (9, 65), (40, 200)]
    masks = [(_mask("dense", h, w, rng), _mask("rectangle", h, w, rng)) for h, w in good]
    gd, nbytes = _descs(good, first=5)
    descs = np.zeros(9, DESC_DTYPE)
    radii = [2, 2, 3, 2, 1, 2, 40000, 7, -1]
    descs[0] = gd[0]
    descs[1] = (0, 0, 5)                          # a zero side
    descs[2] = gd[1]
    descs[3] = (0, 90, 100)                       # h * w above max_pixels (it would fit the buffer)
    descs[4] = gd[2]
    descs[5] = (nbytes - 3, 4, 5)                 # leaves the buffer
    descs[6] = (0, 5, 5)                          # d = 40000
    descs[7] = gd[3]
    descs[8] = (0, 5, 5)                          # d = -1
    where = {0: 0, 2: 1, 4: 2, 7: 3}
    pred = _pack([m[0] for m in masks], gd, nbytes)
    truth = _pack([m[1] for m in masks], gd, nbytes)
    rows = sum(h for h, _ in good)
    want = {i: SR.counts(*masks[k], radii[i]) for i, k in where.items()}
    got = _call(L, cuda, pred, truth, descs, radii, nbytes, max_pixels=8000, rows=rows)
    for i in range(9):
        assert got[i].tolist() == (want[i] if i in where else SR.MISFIT).tolist(), i
    short = _call(L, cuda, pred, truth, descs, radii, nbytes, max_pixels=8000, rows=rows - 1)      # a row capacity one short: the last one
    for i in range(9):
        assert short[i].tolist() == (want[i] if i in where and i != 7 else SR.MISFIT).tolist(), i


def test_pred_equal_to_truth_repeatability_and_aliasing(L, cuda):
    b = _batch()
    pred, truth = _pack(b["preds"], b["descs"], b["nbytes"]), _pack(b["truths"], b["descs"], b["nbytes"])
    one = _call(L, cuda, pred, truth, b["descs"], b["radii"], b["nbytes"])
    two = _call(L, cuda, pred, truth, b["descs"], b["radii"], b["nbytes"])
    assert np.array_equal(one, two) and np.array_equal(one, b["want"])
    same = _call(L, cuda, pred, pred.copy(), b["descs"], b["radii"], b["nbytes"])
    alias = _call(L, cuda, pred, None, b["descs"], b["radii"], b["nbytes"], alias=True)
    assert np.array_equal(same, alias)
    assert (same[:, 1] == 0).all() and (same[:, 2] == 0).all() and (same[:, 7] == 0).all()
    assert (same[:, 4] == same[:, 5]).all() and (same[:, 5] == same[:, 6]).all()
    assert np.array_equal(same, SR.counts_batch(b["preds"], b["preds"], b["radii"]))


def test_a_captured_call_replays_on_a_batch_of_other_sizes(L, cuda):
    """one torch.cuda.graph capture of the call alone at N = 4; bytes, descriptors and radii are then overwritten with a batch of
    different sizes and radii that fits the same capacities, and the replay equals the eager result and the restatement"""
    from unet_watermark_amd.data import descs_tensor
    lib = L.lib()
    rng = np.random.default_rng(5)
    n, nbytes, max_pixels, rows = 4, 24000, 8000, 400
    batches = []
    for shapes, radii, first in ((((17, 64), (33, 129), (40, 200), (9, 65)), (1, 3, 7, 0), 0), (((60, 90), (1, 70), (33, 128), (130, 57)), (2, 1, 40, 5), 7)):
        preds = [_mask(k, h, w, rng) for k, (h, w) in zip(("half", "rectangle", "dense", "grey"), shapes)]
        truths = [_mask(k, h, w, rng) for k, (h, w) in zip(("rectangle", "denser", "rectangle", "half"), shapes)]
        descs, used = _descs(shapes, first)
        assert used <= nbytes and sum(h for h, _ in shapes) <= rows
        batches.append((preds, truths, descs, radii))
    p = torch.zeros(nbytes, dtype=torch.uint8, device=cuda)
    t = torch.zeros(nbytes, dtype=torch.uint8, device=cuda)
    dd = torch.zeros(16 * n, dtype=torch.uint8, device=cuda)
    rr = torch.zeros(n, dtype=torch.int32, device=cuda)
    counts = torch.zeros((n, 8), dtype=torch.int64, device=cuda)
    need = lib.uwm_score_masks_workspace_bytes(n, nbytes, rows)
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)

    def load(batch):
        preds, truths, descs, radii = batch
        p.copy_(torch.from_numpy(_pack(preds, descs, nbytes)[:nbytes]))
        t.copy_(torch.from_numpy(_pack(truths, descs, nbytes)[:nbytes]))
        dd.copy_(descs_tensor(descs))
        rr.copy_(torch.tensor(radii, dtype=torch.int32))

    def call():
        L.check(lib.uwm_score_masks_ragged(C.c_void_p(p.data_ptr()), C.c_void_p(t.data_ptr()), nbytes, C.c_void_p(dd.data_ptr()),
                                           C.c_void_p(rr.data_ptr()), n, max_pixels, rows, C.c_void_p(counts.data_ptr()),
                                           C.c_void_p(ws.data_ptr()), need, C.c_void_p(L.stream_ptr(cuda))))
    load(batches[0])
    call()
    torch.cuda.synchronize(cuda)
    assert counts.cpu().numpy().tolist() == SR.counts_batch(*batches[0][:2], batches[0][3]).tolist()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    load(batches[1])
    call()
    torch.cuda.synchronize(cuda)
    eager = counts.cpu().numpy().copy()
    counts.fill_(-1)
    g.replay()
    torch.cuda.synchronize(cuda)
    assert np.array_equal(counts.cpu().numpy(), eager)
    assert eager.tolist() == SR.counts_batch(*batches[1][:2], batches[1][3]).tolist()


# ---------------------------------------------------------------- the predictor and the command
SIZES = ((50, 70), (64, 64), (97, 130), (150, 81))
_STATE = {}


def _model(dev):
    import unet_watermark_amd as U
    from oracle import unet_oracle as O
    m = U.Unet("resnet18").to(dev)
    m.load_state_dict(O.build("resnet18", seed=3).state_dict())
    xs, _ = O.synthetic_batch(2, 64, 64, seed=5)
    m.train()
    with torch.no_grad():                                          # representative running statistics
        for k in range(3):
            m(xs.to(dev) * (1.0 + 0.1 * k))
    return m.eval()


def _cfg():
    from unet_watermark_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults(); cfg.MODEL.NAME = "Unet"; cfg.MODEL.ENCODER_NAME = "resnet18"; cfg.DATA.IMG_SIZE = 64
    cfg.PREDICT.BATCH_SIZE = 4
    return cfg


def _images(shapes, seed):
    """smooth random images with a bright rectangle each, and random blob truths of the same sizes"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    images, truths = [], []
    for i, (h, w) in enumerate(shapes):
        base = rng.integers(0, 256, size=(h // 6 + 2, w // 6 + 2, 3), dtype=np.uint8)
        a = np.asarray(Image.fromarray(base).resize((w, h), Image.BILINEAR)).copy()
        a[h // 4: h // 4 + h // (2 + i % 3), w // 5: w // 5 + w // 2] = 255 - 40 * (i % 4)
        images.append(a)
        coarse = rng.integers(0, 256, size=(h // 9 + 2, w // 9 + 2), dtype=np.uint8)
        truths.append(np.asarray(Image.fromarray(coarse).resize((w, h), Image.BILINEAR)).copy())       # grey: binarised by the call
    return images, truths


def _median_logit(model, images):
    import unet_watermark_amd as U
    from unet_watermark_amd.constants import IMAGENET_MEAN, IMAGENET_STD
    packed, descs, _ = U.pack_images(images)
    _, lg = model.predict_u8(U.device_resize(packed, descs, 64, 3), IMAGENET_MEAN, IMAGENET_STD, 0.0, return_logits=True)
    return float(lg.median())


def _pred(cuda):
    if "pred" not in _STATE:
        import __graft_entry__ as g
        g.build()
        from unet_watermark_amd.predict import WatermarkPredictor
        pred = WatermarkPredictor(model=_model(cuda), config=_cfg(), device=cuda, precision="f32")
        pred.threshold = _median_logit(pred.model, _images(SIZES, 61)[0])
        _STATE["pred"] = pred
    return _STATE["pred"]


@pytest.mark.parametrize("case", ["plain", "watermark", "tiled"])
def test_score_images_counts_the_masks_the_predict_paths_return(cuda, case):
    from unet_watermark_amd.scoring import boundary_radius
    pred = _pred(cuda)
    images, truths = _images(SIZES, 61)
    if case == "tiled":
        predict = lambda: pred.predict_images_tiled(images, overlap=16)
        kw = dict(tile=True, overlap=16)
    else:
        mt = "watermark" if case == "watermark" else None
        predict = lambda: pred.predict_images(images, mask_type=mt)
        kw = dict(mask_type=mt)
    before = [m.cpu().numpy() for m in predict()]
    pixels = 4 if case == "plain" else None
    counts, masks = pred.score_images(images, truths, boundary_pixels=pixels, return_masks=True, **kw)
    only = pred.score_images(images, truths, boundary_pixels=pixels, **kw)
    after = [m.cpu().numpy() for m in predict()]
    radii = [pixels if pixels is not None else boundary_radius(h, w) for h, w in SIZES]
    assert radii == ([4] * 4 if pixels else [2, 2, 3, 3])
    assert counts.dtype == np.int64 and counts.shape == (4, 8) and np.array_equal(counts, only)
    for b, a, m in zip(before, after, masks):
        assert np.array_equal(b, a) and np.array_equal(b, m.cpu().numpy())
    assert counts.tolist() == SR.counts_batch(before, truths, radii).tolist()
    assert all(0 < (b > 127).mean() < 1 for b in before) or case == "watermark"
    with pytest.raises(ValueError, match="truth 2"):
        pred.score_images(images, truths[:2] + [truths[2][:-1]] + truths[3:], **kw)
    with pytest.raises(ValueError, match="tile"):
        pred.score_images(images, truths, tile=True, text_enhance=True)


def test_main_evaluate_end_to_end(cuda, tmp_path):
    from PIL import Image
    from unet_watermark_amd import cli
    from unet_watermark_amd.checkpoint import save_checkpoint
    from unet_watermark_amd.scoring import COUNT_FIELDS, METRIC_FIELDS, summarize
    pred = _pred(cuda)
    shapes = SIZES + ((40, 90),)
    images, truths = _images(shapes, 62)
    os.makedirs(tmp_path / "d" / "watermarked"); os.makedirs(tmp_path / "d" / "masks")
    for i, (a, t) in enumerate(zip(images, truths)):
        Image.fromarray(a).save(tmp_path / "d" / "watermarked" / f"im{i}.png")
        Image.fromarray(t[:-1] if i == 4 else t).save(tmp_path / "d" / "masks" / (f"im{i}.bmp" if i == 1 else f"im{i}.png"))      # one mask a row short
    save_checkpoint(str(tmp_path / "m.pth"), pred.model, epoch=1)
    (tmp_path / "c.yaml").write_text(f"MODEL:\n  NAME: Unet\n  ENCODER_NAME: resnet18\nDATA:\n  IMG_SIZE: 64\nPREDICT:\n  THRESHOLD: {pred.threshold!r}\n")
    out = tmp_path / "o" / "scores.json"
    res = cli.main(["evaluate", "--data-dir", str(tmp_path / "d"), "--model", str(tmp_path / "m.pth"), "--config", str(tmp_path / "c.yaml"),
                    "--mask-type", "mixed", "--batch-size", "3", "--output", str(out), "--per-image"])
    js = json.loads(out.read_text())
    assert set(js) >= {"settings", "images", "errors", "micro", "imagewise", "per_image"}
    assert js["images"] == 4 and js["errors"] == 1 and res["images"] == 4
    assert "im4" in js["error_details"][0]["path"] and "mask is" in js["error_details"][0]["reason"]
    assert js["settings"]["mask_type"] == "mixed" and js["settings"]["boundary_ratio"] == 0.02 and js["settings"]["img_size"] == 64
    rows = np.array([[r["counts"][k] for k in COUNT_FIELDS] for r in js["per_image"]], dtype=np.int64)
    assert js["micro"] == summarize(rows)["micro"] and js["imagewise"] == summarize(rows)["imagewise"]
    assert [r["size"] for r in js["per_image"]] == [[w, h] for h, w in SIZES] and [r["radius"] for r in js["per_image"]] == [2, 2, 3, 3]
    assert all(set(r["metrics"]) == set(METRIC_FIELDS) for r in js["per_image"])
    masks = [m.cpu().numpy() for m in pred.predict_images(images[:4], mask_type="mixed")]
    assert rows.tolist() == SR.counts_batch(masks, truths[:4], [2, 2, 3, 3]).tolist()
