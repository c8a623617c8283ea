"""Prediction at native resolution on the device (csrc/tile_u8.hip, uwm_predict_tiled_u8, WatermarkPredictor.predict_images_tiled)
against the numpy restatement (tests/tiled_ref.py).  The gather, the tile-logit store and the blended logit planes are float32 values
compared bit for bit, the masks byte for byte; no pixel is exempted.  Where the sigmoid is applied the device's expf and numpy's may
differ in the last bits, so that test first asserts that its threshold keeps every pixel further away than those bits reach (MARGIN:
a condition on the inputs, as in tests/test_filter_gpu.py).

Unet-resnet18 with seeded weights, tile 64 (the smallest the encoder's /32 allows), forward batch 8, overlap 16.  The image sizes hit
each edge of the rule: 64 x 64 one tile without padding; 100 x 70 two tiles per axis with a clamped last tile; 65 x 200 one pixel
past the tile; 40 x 30 and 3 x 150 reflection, also with a side shorter than the reflect radius; 64 x 129; and 70 x 161, where the
clamped last tile starts one pixel behind its neighbour and three tiles share pixels."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_ref as FR  # noqa: E402
import tiled_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

T, N, OVERLAP = 64, 8, 16
SIZES = [(64, 64), (100, 70), (65, 200), (40, 30), (3, 150), (64, 129), (70, 161)]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
MARGIN = 2e-6                               # see tests/test_filter_gpu.py: four times what a 2-ulp expf and a division can move a value <= 1
FILL = 77


def _lib():
    from unet_watermark_amd import _lib as L
    return L, L.lib()


def _P(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _images(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]


def _pack_with_gaps(imgs, seed=5):
    """the images at 4-byte-aligned offsets with random bytes between them; the buffer ends with the last image's last byte"""
    from unet_watermark_amd.data import DESC_DTYPE
    rng = np.random.default_rng(seed)
    descs = np.zeros(len(imgs), DESC_DTYPE)
    off = 4 * int(rng.integers(1, 8))
    for i, a in enumerate(imgs):
        descs[i] = (off, a.shape[0], a.shape[1])
        end = off + a.size
        off = (end + 3) // 4 * 4 + 4 * int(rng.integers(1, 8))
    buf = rng.integers(0, 256, size=end, dtype=np.uint8)
    for a, d in zip(imgs, descs):
        buf[d["offset"]: d["offset"] + a.size] = a.reshape(-1)
    return buf, descs


def _predictor(dev):
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
    cfg = get_cfg_defaults(); cfg.MODEL.NAME = "Unet"; cfg.MODEL.ENCODER_NAME = "resnet18"; cfg.DATA.IMG_SIZE = T
    cfg.PREDICT.BATCH_SIZE = N
    return WatermarkPredictor(model=m, config=cfg, device=dev, precision="f32")


_CASE = {}


def _case(dev):
    """computed once and left unchanged: the predictor, the images, their plan, the reference tiles (numpy crops through the device's
    uwm_op_preprocess_u8_nhwc4), the device's tile-logit store of one eager call, and the restatement's blend of that store"""
    if _CASE:
        return _CASE
    import unet_watermark_amd as U
    from unet_watermark_amd import tiling
    from unet_watermark_amd.data import descs_tensor
    L, lib = _lib()
    pred = _predictor(dev)
    imgs = _images(SIZES, 1)
    tiles, plans = tiling.plan_batch(SIZES, T, T, OVERLAP, N)
    K = len(tiles)
    assert K == 32 and int((tiles["image"] >= 0).sum()) == 1 + 4 + 8 + 1 + 3 + 3 + 8
    crops = np.zeros((K, T, T, 3), np.uint8)
    for k, t in enumerate(tiles):
        if t["image"] >= 0:
            crops[k] = R.crop(imgs[t["image"]], int(t["y0"]), int(t["x0"]), T, T)
    mc, sc = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    want = torch.full((K, T, T, 4), float("nan"), device=dev)
    crops_t = torch.from_numpy(crops).to(dev)
    L.check(lib.uwm_op_preprocess_u8_nhwc4(_P(crops_t), K * T * T, 3, mc, sc, _P(want), C.c_void_p(L.stream_ptr(dev))))
    want[torch.from_numpy(tiles["image"] < 0).to(dev)] = 0.0      # a padding tile is all zeros, not Normalize(0)
    # one eager call through the model: masks at threshold 0, the ragged logit plane and the store
    packed, descs, mdescs = U.pack_images(imgs)
    areas = descs["h"].astype(np.int64) * descs["w"]
    mask_bytes = int(areas.sum())
    dv = dict(packed=packed.to(dev), descs=descs_tensor(descs, dev), mdescs=descs_tensor(mdescs, dev),
              tiles=tiling.table_tensor(tiles, dev), plans=tiling.table_tensor(plans, dev))
    mask = torch.full((mask_bytes,), FILL, dtype=torch.uint8, device=dev)
    plane = torch.full((mask_bytes,), float("nan"), device=dev)
    pred.model.predict_tiled_u8(dv["packed"], dv["descs"], dv["mdescs"], mask, len(imgs), dv["tiles"], dv["plans"], K, N, (T, T), OVERLAP,
                                MEAN, STD, 0.0, False, plane)
    torch.cuda.synchronize(dev)
    store = pred.model._tile_store.clone()
    store_np = store.cpu().numpy()
    blended = []
    for i, (h, w) in enumerate(SIZES):
        f, cnt = int(plans[i]["first"]), int(plans[i]["ny"]) * int(plans[i]["nx"])
        blended.append(R.blend(store_np[f: f + cnt], h, w, T, T, OVERLAP))
    _CASE.update(pred=pred, imgs=imgs, tiles=tiles, plans=plans, K=K, crops=crops, want=want, dv=dv, descs=descs, mdescs=mdescs, areas=areas,
                 mask_bytes=mask_bytes, mask0=mask.clone(), plane=plane.clone(), store=store, blended=blended)
    return _CASE


def _split(buf, c):
    return [buf[int(o): int(o) + int(a)].reshape(int(h), int(w)) for o, a, h, w in zip(c["mdescs"]["offset"], c["areas"], c["descs"]["h"], c["descs"]["w"])]


def test_gather_equals_preprocess_of_the_numpy_crops(cuda):
    """the tiles of the plan, padding entries, an image index out of range, origins that are negative or beyond the image: one launch;
    the guard floats around the output stay as they were"""
    from unet_watermark_amd import tiling
    from unet_watermark_amd.data import descs_tensor
    L, lib = _lib()
    c = _case(cuda)
    buf, descs = _pack_with_gaps(c["imgs"])
    tiles = c["tiles"].copy()
    bad = np.zeros(8, tiling.TILE_DTYPE)
    bad[0] = (len(SIZES), 0, 0, 0); bad[1] = (1 << 30, 0, 0, 0); bad[2] = (-7, 0, 0, 0)      # image out of range
    bad[3] = (1, -1, 0, 1); bad[4] = (1, 0, -1, 1)                                          # a negative origin
    bad[5] = (1, 100, 0, 1); bad[6] = (1, 0, 70, 1); bad[7] = (4, 3, 0, 0)                  # an origin beyond the image
    table = np.concatenate([tiles, bad])
    K = len(table)
    guard = 64
    out = torch.full((K * T * T * 4 + 2 * guard,), float(FILL), device=cuda)
    mc, sc = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    buf_t, descs_t, table_t = torch.from_numpy(buf).to(cuda), descs_tensor(descs, cuda), tiling.table_tensor(table, cuda)
    L.check(lib.uwm_op_tile_norm_u8_nhwc4(_P(buf_t), buf_t.numel(), _P(descs_t), len(SIZES), _P(table_t), K, 3, T, T, mc, sc, C.c_void_p(out.data_ptr() + 4 * guard), C.c_void_p(L.stream_ptr(cuda))))
    torch.cuda.synchronize(cuda)
    got = out[guard: -guard].view(K, T, T, 4)
    assert torch.equal(got[:c["K"]].view(torch.int32), c["want"].view(torch.int32))
    assert float(got[:c["K"], ..., 3].abs().max()) == 0.0                    # the padding channel
    pad = torch.from_numpy(tiles["image"] < 0).to(cuda)
    assert int(pad.sum()) == 4 and float(got[:c["K"]][pad].abs().max()) == 0.0 and float(got[c["K"]:].abs().max()) == 0.0
    assert bool((out[:guard] == FILL).all()) and bool((out[-guard:] == FILL).all())
    # the reflection really happened: the 3 x 150 image's first tile repeats rows 0 1 2 1 0 ...
    k3 = int(c["plans"][4]["first"])
    assert torch.equal(got[k3, 3], got[k3, 1]) and torch.equal(got[k3, 4], got[k3, 0]) and not torch.equal(got[k3, 0], got[k3, 1])


def test_the_tile_logit_store_equals_plain_forwards_of_the_tiles(cuda):
    c = _case(cuda)
    pred = c["pred"]
    x = c["want"][..., :3].permute(0, 3, 1, 2).contiguous()
    for k0 in range(0, c["K"], N):
        lg = pred.logits(x[k0: k0 + N], use_graph=False)
        assert lg.shape == (N, 1, T, T)
        assert torch.equal(lg[:, 0].contiguous().view(torch.int32), c["store"][k0: k0 + N].view(torch.int32)), k0
    assert float(c["store"].std()) > 1e-3


@pytest.mark.parametrize("apply_sigmoid", [False, True])
def test_blended_planes_and_masks_equal_the_restatement(cuda, apply_sigmoid):
    c = _case(cuda)
    pred = c["pred"]
    planes = [p.cpu().numpy() for p in _split(c["plane"], c)]
    for i, (got, want) in enumerate(zip(planes, c["blended"])):              # the eager call of _case, threshold 0
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (SIZES[i], np.argwhere(got != want)[:5].tolist())
    for got, want in zip(_split(c["mask0"], c), c["blended"]):
        assert np.array_equal(got.cpu().numpy(), R.predict_mask(want, 0.0, False))
    # the 64 x 64 image is one tile without padding: its plane is the plain forward's logits of that tile
    x = c["want"][:N, ..., :3].permute(0, 3, 1, 2).contiguous()
    assert np.array_equal(planes[0].view(np.int32), pred.logits(x, use_graph=False)[0, 0].cpu().numpy().view(np.int32))
    # a threshold in the middle of the values, so that both classes are there
    allv = np.concatenate([b.reshape(-1) for b in c["blended"]])
    if apply_sigmoid:
        p64 = np.sort(1.0 / (1.0 + np.exp(-allv.astype(np.float64))))
        mid = p64[int(0.45 * p64.size): int(0.55 * p64.size)]
        j = int(np.argmax(np.diff(mid)))
        thr = float(np.float32(0.5 * (mid[j] + mid[j + 1])))                 # the widest gap between neighbouring values around the median
        assert np.abs(p64 - thr).min() > MARGIN                              # the precondition: no pixel within MARGIN of the threshold
    else:
        thr = float(np.median(allv))
    old = pred.threshold
    try:
        pred.threshold = thr
        for use_graph in (False, True):
            masks, lgs = pred.predict_images_tiled(c["imgs"], OVERLAP, apply_sigmoid, return_logits=True, use_graph=use_graph)
            assert len(masks) == len(SIZES)
            for i, (m, lg, want) in enumerate(zip(masks, lgs, c["blended"])):
                assert m.dtype == torch.uint8 and tuple(m.shape) == SIZES[i] and lg.dtype == torch.float32
                assert np.array_equal(lg.cpu().numpy().view(np.int32), want.view(np.int32)), (SIZES[i], use_graph)
                wm = R.predict_mask(want, thr, apply_sigmoid, FR.sigmoid32)
                assert np.array_equal(m.cpu().numpy(), wm), (SIZES[i], use_graph, int((m.cpu().numpy() != wm).sum()))
            assert 0.05 < float((torch.cat([m.reshape(-1) for m in masks]) > 0).float().mean()) < 0.95      # both classes are there
            plain = pred.predict_images_tiled(c["imgs"], OVERLAP, apply_sigmoid, use_graph=use_graph)
            assert all(torch.equal(a, b) for a, b in zip(plain, masks))      # without return_logits: the same masks
    finally:
        pred.threshold = old


def _graphs_of(pred, group):
    """key -> captured graph of the predictor's entries of one group ('tiled', 'tta')"""
    return {e.key: e.graph for e in pred._graphs.values() if e.group == group}


def test_a_captured_call_replays_on_another_batch_with_the_same_chunk_count(cuda):
    c = _case(cuda)
    pred = c["pred"]
    pred.threshold = float(np.median(np.concatenate([b.reshape(-1) for b in c["blended"]])))
    try:
        first = pred.predict_images_tiled(c["imgs"], OVERLAP)
        graphs = _graphs_of(pred, "tiled")
        key = [k for k in graphs if len(k) == 8 and k[:3] == (len(SIZES), c["K"] // N, N) and k[5] is False and k[7] is False and k[6] == pred.threshold]
        assert len(key) == 1
        other = _images([(w, h) for h, w in SIZES], 2)                       # other sizes, the same number of tiles and bytes
        eager = pred.predict_images_tiled(other, OVERLAP, use_graph=False)
        replay = pred.predict_images_tiled(other, OVERLAP)
        assert _graphs_of(pred, "tiled")[key[0]] is graphs[key[0]]                # replayed, not captured again
        for a, b, (h, w) in zip(eager, replay, SIZES):
            assert tuple(b.shape) == (w, h) and torch.equal(a, b)
        assert any(0.05 < float((m > 0).float().mean()) < 0.95 for m in replay)
        again = pred.predict_images_tiled(other, OVERLAP)
        assert all(torch.equal(a, b) for a, b in zip(replay, again))         # two runs are identical
        back = pred.predict_images_tiled(c["imgs"], OVERLAP)
        assert all(torch.equal(a, b) for a, b in zip(first, back))
    finally:
        pred.threshold = float(pred.cfg.PREDICT.THRESHOLD)


def test_a_misfit_image_gets_zeros_and_costs_only_itself(cuda):
    from unet_watermark_amd.data import descs_tensor
    c = _case(cuda)
    pred, dv = c["pred"], c["dv"]
    thr = float(np.median(np.concatenate([b.reshape(-1) for b in c["blended"]])))

    def run(descs_t, mask, plans_t=None):
        pred.model.predict_tiled_u8(dv["packed"], descs_t, dv["mdescs"], mask, len(SIZES), dv["tiles"], dv["plans"] if plans_t is None else plans_t,
                                    c["K"], N, (T, T), OVERLAP, MEAN, STD, thr, False, None)
        torch.cuda.synchronize(cuda)
        return mask
    good = _split(run(dv["descs"], torch.full((c["mask_bytes"],), FILL, dtype=torch.uint8, device=cuda)), c)
    assert 0.05 < float((torch.cat([m.reshape(-1) for m in good]) > 0).float().mean()) < 0.95      # both classes are there
    bad = c["descs"].copy()
    bad[2]["h"] = 1 << 20                                                    # the region leaves the buffer
    bad[5]["offset"] = -4
    got = _split(run(descs_tensor(bad, cuda), torch.full((c["mask_bytes"],), FILL, dtype=torch.uint8, device=cuda)), c)
    for i, (g, w) in enumerate(zip(got, good)):
        assert (not g.any()) if i in (2, 5) else torch.equal(g, w), i
    # a plan entry that disagrees with the formula, or does not fit K: zeros for that image
    from unet_watermark_amd import tiling
    plans = c["plans"].copy()
    plans[1]["nx"] = 3
    plans[6]["first"] = c["K"] - 2
    got = _split(run(dv["descs"], torch.full((c["mask_bytes"],), FILL, dtype=torch.uint8, device=cuda), tiling.table_tensor(plans, cuda)), c)
    for i, (g, w) in enumerate(zip(got, good)):
        assert (not g.any()) if i in (1, 6) else torch.equal(g, w), i
    # a mask buffer one byte short: the last image is skipped, nothing of it is written
    short = torch.full((c["mask_bytes"],), FILL, dtype=torch.uint8, device=cuda)
    run(dv["descs"], short[:-1])
    o = int(c["mdescs"]["offset"][-1])
    assert bool((short[o:] == FILL).all())
    for g, w in zip(_split(short, c)[:-1], good[:-1]):
        assert torch.equal(g, w)


def test_mask_type_runs_the_ragged_post_processing_on_the_blended_masks(cuda):
    import unet_watermark_amd as U
    c = _case(cuda)
    pred = c["pred"]
    pred.threshold = float(np.median(np.concatenate([b.reshape(-1) for b in c["blended"]])))
    try:
        raw = pred.predict_images_tiled(c["imgs"], OVERLAP)
        want = _split(U.optimize_masks_ragged(torch.cat([m.reshape(-1) for m in raw]), c["mdescs"], "watermark"), c)
        for use_graph in (False, True):
            got = pred.predict_images_tiled(c["imgs"], OVERLAP, mask_type="watermark", use_graph=use_graph)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), use_graph
        assert any(not torch.equal(a, b) for a, b in zip(raw, want))         # the post-processing did something
    finally:
        pred.threshold = float(pred.cfg.PREDICT.THRESHOLD)
    with pytest.raises(ValueError):
        pred.predict_images_tiled(c["imgs"], OVERLAP, mask_type="logo")
    with pytest.raises(ValueError):
        pred.predict_images_tiled(c["imgs"], T // 2 + 1)


def test_predict_images_is_unchanged_by_a_tiled_call(cuda):
    c = _case(cuda)
    pred = c["pred"]
    before = [m.clone() for m in pred.predict_images(c["imgs"])]
    graph = pred._graphs["images"].graph
    pred.predict_images_tiled(c["imgs"], OVERLAP)
    pred.predict_images_tiled(c["imgs"], OVERLAP, mask_type="text", use_graph=False)
    after = pred.predict_images(c["imgs"])
    assert pred._graphs["images"].graph is graph                                             # the default path's graph stays as captured
    assert all(torch.equal(a, b) for a, b in zip(before, after))
