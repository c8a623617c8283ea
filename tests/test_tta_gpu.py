"""Test-time augmentation on the device (csrc/tta.hip, uwm_predict_images_tta_u8, uwm_predict_tiled_tta_u8, the predictor's `tta`)
against the torch restatements of unet_watermark_amd/tta.py.  Float planes are compared bit for bit (as int32 views), masks byte for
byte; no pixel is exempted.  The one bounded comparison is the equivariance test, whose bound is derived there.

Unet-resnet18 with seeded weights in the exact-fp32 mode, IMG_SIZE 64, forward batch 4.  The references run the plain eval forward
(pred.logits, no graph) on the same slot chunks of apply_view'ed inputs and merge them with tta.merge_views."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiled_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

T, N, OVERLAP = 64, 4, 16
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FILL = 77
SIZES = [(64, 64), (100, 70), (3, 150), (40, 30)]
CODE_SETS = [1 << c for c in range(8)] + [0xFF]


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


def _bits(t):
    return t.contiguous().view(torch.int32)


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


def _resize_norm(imgs, dev, H=T, W=T):
    """the existing uwm_op_resize_norm_u8_nhwc4 on the packed images -> (n, H, W, 4)"""
    import unet_watermark_amd as U
    from unet_watermark_amd.data import descs_tensor
    L, lib = _lib()
    packed, descs, _ = U.pack_images(imgs)
    out = torch.full((len(imgs), H, W, 4), float("nan"), device=dev)
    mc, sc = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    packed_t, descs_t = packed.to(dev), descs_tensor(descs, dev)              # (both alive until the launch has run)
    L.check(lib.uwm_op_resize_norm_u8_nhwc4(_P(packed_t), packed.numel(), _P(descs_t), len(imgs), 3, H, W, mc, sc, _P(out),
                                            C.c_void_p(L.stream_ptr(dev))))
    torch.cuda.synchronize(dev)
    return out


def _viewed(base, mask, slots):
    """base (n, H, W, 4) planes -> the first `slots` slots (slots, H', W', 4) of the set: apply_view per slot, zeros for padding"""
    from unet_watermark_amd import tta
    codes = tta.view_codes(mask)
    k = len(codes)
    out = []
    for s in range(slots):
        i, c = s // k, codes[s % k]
        if i >= base.shape[0]:
            out.append(torch.zeros_like(out[0]))
        else:
            out.append(tta.apply_view(base[i].permute(2, 0, 1), c).permute(1, 2, 0).contiguous())
    return torch.stack(out)


def _ref_merged(pred, base, mask, batch=N):
    """the restatement of the model-level merge: base (n, T, T, 4) network inputs -> (merged (n, T, T), the mapped-back logit planes
    (n, k, T, T)): the slots, `batch` at a time and padded with zeros, through the plain eval forward, then tta.merge_views"""
    from unet_watermark_amd import tta
    n, codes = base.shape[0], tta.view_codes(mask)
    k = len(codes)
    table, chunks = tta.plan_slots(n, mask, batch)
    x = _viewed(base, mask, chunks * batch)[..., :3].permute(0, 3, 1, 2).contiguous()
    lg = torch.cat([pred.logits(x[s0: s0 + batch], use_graph=False)[:, 0] for s0 in range(0, chunks * batch, batch)])
    planes = lg[: n * k].view(n, k, T, T)
    back = torch.stack([torch.stack([tta.invert_view(planes[i, j], codes[j]) for j in range(k)]) for i in range(n)])
    return tta.merge_views(planes, mask), back


def _ragged_masks(planes, sizes, thr, dev, apply_sigmoid=False):
    """uwm_resize_threshold_ragged of (n, T, T) planes (ld = 1) -> the list of masks at `sizes`"""
    from unet_watermark_amd.data import DESC_DTYPE, descs_tensor
    L, lib = _lib()
    d = np.zeros(len(sizes), DESC_DTYPE)
    off = 0
    for i, (h, w) in enumerate(sizes):
        d[i] = (off, h, w)
        off += h * w
    mask = torch.full((off,), FILL, dtype=torch.uint8, device=dev)
    planes, d_t = planes.contiguous(), descs_tensor(d, dev)
    L.check(lib.uwm_resize_threshold_ragged(_P(planes), 1, len(sizes), T, T, _P(d_t), float(thr), int(apply_sigmoid), _P(mask), off,
                                            C.c_void_p(L.stream_ptr(dev))))
    torch.cuda.synchronize(dev)
    return [mask[int(o): int(o) + h * w].view(h, w) for o, (h, w) in zip(d["offset"], sizes)]


_CASE = {}


def _case(dev):
    """computed once and left unchanged: the predictor, three images of different sizes, their network inputs, and the restatement's
    merged planes for hflip and d4 (forward batch 4: 6 slots padded to 8, 24 slots)"""
    if _CASE:
        return _CASE
    pred = _predictor(dev)
    sizes = [(100, 70), (64, 64), (40, 131)]
    imgs = _images(sizes, 21)
    base = _resize_norm(imgs, dev)
    ref = {name: _ref_merged(pred, base, name) for name in ("hflip", "d4")}
    thr = float(ref["d4"][0].median())
    _CASE.update(pred=pred, sizes=sizes, imgs=imgs, base=base, ref=ref, thr=thr)
    return _CASE


# ------------------------------------------------------------------------------------------------ the kernels alone
@pytest.mark.parametrize("side", [5, 64])
def test_viewed_resize_norm_equals_apply_view_of_the_plain_call(cuda, side):
    """every single code and d4; slot ranges that start inside an image and run into the padding; guard floats around the output"""
    from unet_watermark_amd.data import descs_tensor
    L, lib = _lib()
    imgs = _images(SIZES, 1)
    buf, descs = _pack_with_gaps(imgs)
    n = len(imgs)
    buf_t, descs_t = torch.from_numpy(buf).to(cuda), descs_tensor(descs, cuda)
    mc, sc = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    base = torch.full((n, side, side, 4), float("nan"), device=cuda)
    st = C.c_void_p(L.stream_ptr(cuda))
    L.check(lib.uwm_op_resize_norm_u8_nhwc4(_P(buf_t), buf_t.numel(), _P(descs_t), n, 3, side, side, mc, sc, _P(base), st))
    assert _bits(base).ne(_bits(_resize_norm(imgs, cuda, side, side))).sum() == 0          # (gaps or not: the same planes)
    guard = 64
    for mask in CODE_SETS:
        k = bin(mask).count("1")
        total = n * k + 3                                                     # three padding slots behind the images
        want = _viewed(base, mask, total)
        for s0, ns in ((0, total), (k // 2 + 1, total - k // 2 - 1), (n * k - 1, 4)):
            stage_bytes = lib.uwm_view_stage_bytes(mask, ns, side, side)
            assert stage_bytes <= min(ns, (ns + k - 2) // k + 1) * side * side * 16
            stage = torch.empty(stage_bytes // 4, device=cuda)
            out = torch.full((ns * side * side * 4 + 2 * guard,), float(FILL), device=cuda)
            L.check(lib.uwm_op_resize_norm_view_u8_nhwc4(_P(buf_t), buf_t.numel(), _P(descs_t), n, 3, side, side, mc, sc, mask, s0, ns, _P(stage),
                                                         stage_bytes, C.c_void_p(out.data_ptr() + 4 * guard), st))
            torch.cuda.synchronize(cuda)
            got = out[guard: -guard].view(ns, side, side, 4)
            assert torch.equal(_bits(got), _bits(want[s0: s0 + ns])), (hex(mask), s0, ns)
            assert float(got[..., 3].abs().max()) == 0.0                      # the padding channel
            assert float(got[max(n * k - s0, 0):].abs().max()) == 0.0         # the padding slots
            assert bool((out[:guard] == FILL).all()) and bool((out[-guard:] == FILL).all())
    assert not torch.equal(_viewed(base, 0x02, 1), _viewed(base, 0x01, 1))    # a view moves pixels


def test_viewed_resize_norm_of_a_4_by_6_plane_takes_the_flips_and_refuses_a_quarter_turn(cuda):
    from unet_watermark_amd.data import descs_tensor
    L, lib = _lib()
    imgs = _images(SIZES, 1)
    buf, descs = _pack_with_gaps(imgs)
    n, H, W = len(imgs), 4, 6
    buf_t, descs_t = torch.from_numpy(buf).to(cuda), descs_tensor(descs, cuda)
    mc, sc = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    base = torch.full((n, H, W, 4), float("nan"), device=cuda)
    st = C.c_void_p(L.stream_ptr(cuda))
    L.check(lib.uwm_op_resize_norm_u8_nhwc4(_P(buf_t), buf_t.numel(), _P(descs_t), n, 3, H, W, mc, sc, _P(base), st))
    stage = torch.empty(lib.uwm_view_stage_bytes(0x55, 4 * n, H, W) // 4, device=cuda)      # (the bound of the longest range below)
    assert stage.numel() == 5 * H * W * 4
    for mask in (0x01, 0x04, 0x10, 0x40, 0x55):
        k = bin(mask).count("1")
        out = torch.full((n * k, H, W, 4), float(FILL), device=cuda)
        L.check(lib.uwm_op_resize_norm_view_u8_nhwc4(_P(buf_t), buf_t.numel(), _P(descs_t), n, 3, H, W, mc, sc, mask, 0, n * k, _P(stage), 4 * stage.numel(),
                                                     _P(out), st))
        torch.cuda.synchronize(cuda)
        assert torch.equal(_bits(out), _bits(_viewed(base, mask, n * k))), hex(mask)
    out = torch.full((n, H, W, 4), float(FILL), device=cuda)
    for mask in (0x02, 0x08, 0x20, 0x80, 0xFF):
        rc = lib.uwm_op_resize_norm_view_u8_nhwc4(_P(buf_t), buf_t.numel(), _P(descs_t), n, 3, H, W, mc, sc, mask, 0, n, _P(stage), 4 * stage.numel(), _P(out), st)
        assert rc != 0 and b"H == W" in lib.uwm_last_error(), hex(mask)
    torch.cuda.synchronize(cuda)
    assert bool((out == FILL).all())                                          # refused before any launch


def test_viewed_tile_gather_equals_apply_view_of_the_plain_call(cuda):
    from unet_watermark_amd import tiling
    from unet_watermark_amd.data import descs_tensor
    L, lib = _lib()
    sizes = [(100, 70), (3, 150)]
    imgs = _images(sizes, 2)
    buf, descs = _pack_with_gaps(imgs)
    tiles, _ = tiling.plan_batch(sizes, T, T, OVERLAP, 4)
    K = len(tiles)
    assert K == 8 and int((tiles["image"] >= 0).sum()) == 4 + 3               # one padding entry inside the table
    buf_t, descs_t, tiles_t = torch.from_numpy(buf).to(cuda), descs_tensor(descs, cuda), tiling.table_tensor(tiles, cuda)
    mc, sc = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    st = C.c_void_p(L.stream_ptr(cuda))
    base = torch.full((K, T, T, 4), float("nan"), device=cuda)
    L.check(lib.uwm_op_tile_norm_u8_nhwc4(_P(buf_t), buf_t.numel(), _P(descs_t), len(imgs), _P(tiles_t), K, 3, T, T, mc, sc, _P(base), st))
    torch.cuda.synchronize(cuda)
    assert float(base[7].abs().max()) == 0.0 and float(base[0].abs().max()) > 0.0
    guard = 64
    for mask in CODE_SETS:
        k = bin(mask).count("1")
        total = K * k + 2
        want = _viewed(base, mask, total)
        for s0, ns in ((0, total), (k // 2 + 1, 5), (K * k - 1, 3)):
            stage_bytes = lib.uwm_view_stage_bytes(mask, ns, T, T)
            stage = torch.empty(stage_bytes // 4, device=cuda)
            out = torch.full((ns * T * T * 4 + 2 * guard,), float(FILL), device=cuda)
            L.check(lib.uwm_op_tile_norm_view_u8_nhwc4(_P(buf_t), buf_t.numel(), _P(descs_t), len(imgs), _P(tiles_t), K, 3, T, T, mc, sc, mask, s0, ns,
                                                       _P(stage), stage_bytes, C.c_void_p(out.data_ptr() + 4 * guard), st))
            torch.cuda.synchronize(cuda)
            got = out[guard: -guard].view(ns, T, T, 4)
            assert torch.equal(_bits(got), _bits(want[s0: s0 + ns])), (hex(mask), s0, ns)
            assert float(got[..., 3].abs().max()) == 0.0 and not bool(got[max(K * k - s0, 0):].any())      # the padding channel, the padding slots
            assert bool((out[:guard] == FILL).all()) and bool((out[-guard:] == FILL).all())
    rc = lib.uwm_op_tile_norm_view_u8_nhwc4(_P(buf_t), buf_t.numel(), _P(descs_t), len(imgs), _P(tiles_t), K, 3, 64, 32, mc, sc, 0x02, 0, 4, _P(base),
                                            4 * base.numel(), _P(base), st)
    assert rc != 0 and b"H == W" in lib.uwm_last_error()


@pytest.mark.parametrize("mask", [0x01, 0x11, 0x55, 0xFF, 0x26])
def test_merge_alone_equals_the_host_restatement_whatever_the_chunking(cuda, mask):
    """synthetic planes from 1e-6 to 1e3 in magnitude, element stride 3, 37 x 37 (more than one workgroup, a ragged rim), three items
    and two padding slots: as one range and in chunks of 3 slots"""
    from unet_watermark_amd import tta
    L, lib = _lib()
    k, items, S, ld = bin(mask).count("1"), 3, 37, 3
    slots = items * k + 2
    rng = np.random.default_rng(100 + mask)
    mag = np.float32(10.0) ** rng.uniform(-6, 3, (slots, S, S)).astype(np.float32)
    planes = torch.from_numpy((mag * rng.choice([-1.0, 1.0], mag.shape)).astype(np.float32)).to(cuda)
    strided = torch.full((slots, S, S, ld), float("nan"), device=cuda)
    strided[..., 0] = planes
    want = tta.merge_views(planes[: items * k].view(items, k, S, S), mask)
    st = C.c_void_p(L.stream_ptr(cuda))
    guard = 16
    results = []
    for step in (slots, 3):
        buf = torch.full((items * S * S + 2 * guard,), float(FILL), device=cuda)
        store = C.c_void_p(buf.data_ptr() + 4 * guard)
        for s0 in range(0, slots, step):
            ns = min(step, slots - s0)
            L.check(lib.uwm_op_view_merge(_P(strided[s0:]), ld, S, S, mask, s0, ns, items, store, st))
        torch.cuda.synchronize(cuda)
        got = buf[guard: -guard].view(items, S, S)
        assert torch.equal(_bits(got), _bits(want)), (hex(mask), step, int(_bits(got).ne(_bits(want)).sum()))
        assert bool((buf[:guard] == FILL).all()) and bool((buf[-guard:] == FILL).all())
        results.append(got.clone())
    assert torch.equal(_bits(results[0]), _bits(results[1]))
    if mask == 0x01:
        assert torch.equal(_bits(results[0]), _bits(planes[:items]))          # k = 1, code 0: the input, bit for bit


# ------------------------------------------------------------------------------------------------ the model
def _graphs_of(pred, group):
    """key -> captured graph of the predictor's entries of one group ('tiled', 'tta')"""
    return {e.key: e.graph for e in pred._graphs.values() if e.group == group}


@pytest.mark.parametrize("name", ["hflip", "d4"])
def test_predict_images_merges_the_plain_forwards_of_the_viewed_inputs(cuda, name):
    c = _case(cuda)
    pred = c["pred"]
    want, _ = c["ref"][name]
    old = pred.threshold
    try:
        pred.threshold = c["thr"]
        want_masks = _ragged_masks(want, c["sizes"], c["thr"], cuda)
        assert 0.05 < float((torch.cat([m.reshape(-1) for m in want_masks]) > 0).float().mean()) < 0.95      # both classes are there
        for use_graph in (False, True):
            masks, merged = pred.predict_images(c["imgs"], tta=name, return_logits=True, use_graph=use_graph)
            assert merged.shape == (3, T, T) and torch.equal(_bits(merged), _bits(want)), (name, use_graph)
            for m, w, s in zip(masks, want_masks, c["sizes"]):
                assert m.dtype == torch.uint8 and tuple(m.shape) == s and torch.equal(m, w), (name, use_graph, s)
        # another batch of other sizes with the same counts replays the same graph
        graphs = _graphs_of(pred, "tta")
        other = _images([(33, 90), (80, 80), (64, 17)], 22)
        ref_other, _ = _ref_merged(pred, _resize_norm(other, cuda), name)
        masks, merged = pred.predict_images(other, tta=name, return_logits=True)
        assert _graphs_of(pred, "tta") == graphs                # replayed: the same keys, the same graph objects
        assert torch.equal(_bits(merged), _bits(ref_other))
        for m, w in zip(masks, _ragged_masks(ref_other, [(33, 90), (80, 80), (64, 17)], c["thr"], cuda)):
            assert torch.equal(m, w)
        assert not torch.equal(_bits(merged), _bits(want))
    finally:
        pred.threshold = old
    if name == "d4":
        plain = _ref_merged(pred, c["base"], "none")[0]
        assert not torch.equal(_bits(plain), _bits(want))                     # the views did something


def test_the_sigmoid_is_applied_to_the_mean_of_the_logits(cuda):
    c = _case(cuda)
    pred = c["pred"]
    want, _ = c["ref"]["hflip"]
    old = pred.threshold
    try:
        pred.threshold = float(torch.sigmoid(want.double()).median())
        got = pred.predict_images(c["imgs"], apply_sigmoid=True, tta="hflip", use_graph=False)
        for m, w in zip(got, _ragged_masks(want, c["sizes"], pred.threshold, cuda, True)):
            assert torch.equal(m, w)
    finally:
        pred.threshold = old


def test_the_merged_logits_do_not_depend_on_the_forward_batch(cuda):
    c = _case(cuda)
    pred = c["pred"]
    try:
        got = {}
        for batch in (2, 8):
            pred.cfg.PREDICT.BATCH_SIZE = batch
            for name in ("hflip", "d4"):
                got[(batch, name)] = pred.predict_images(c["imgs"], tta=name, return_logits=True, use_graph=False)[1]
    finally:
        pred.cfg.PREDICT.BATCH_SIZE = N
    for name in ("hflip", "d4"):
        assert torch.equal(_bits(got[(2, name)]), _bits(got[(8, name)])), name
        assert torch.equal(_bits(got[(2, name)]), _bits(c["ref"][name][0])), name


def test_d4_is_equivariant_and_hflip_is_not(cuda):
    """64 x 64 images, so the resize is the identity and the eight network inputs of view_g(img) are the eight of img in another order:
    the same eight planes are summed in another order and divided by 8.  Each order's sum is off the exact one by at most
    (k - 1) u sum|l_j| <= (k - 1) k u max|l_j|, the division by k brings that to (k - 1) u max|l_j| and adds u |v| <= u max|l_j|; two
    such results differ by at most 2 k u max_j |l_j| per pixel, u = 2^-24."""
    from unet_watermark_amd import tta
    c = _case(cuda)
    pred = c["pred"]
    img = _images([(64, 64)], 31)[0]
    t = torch.from_numpy(img).permute(2, 0, 1)
    turned = [tta.apply_view(t, g).permute(1, 2, 0).contiguous().numpy() for g in range(8)]
    _, back = _ref_merged(pred, _resize_norm([img], cuda), "d4")
    peak = back[0].abs().amax(0)                                              # max_j |l_j| per pixel, in img's frame
    _, merged = pred.predict_images(turned, tta="d4", return_logits=True, use_graph=False)
    assert float(merged[0].std()) > 1e-3
    for g in range(8):
        want, bound = tta.apply_view(merged[0], g), 2 * 8 * 2.0 ** -24 * tta.apply_view(peak, g)
        assert bool(((merged[g].double() - want.double()).abs() <= bound.double()).all()), g
    _, hf = pred.predict_images([turned[0], turned[1]], tta="hflip", return_logits=True, use_graph=False)
    diff = (hf[1].double() - tta.apply_view(hf[0], 1).double()).abs()
    assert bool((diff > 2 * 8 * 2.0 ** -24 * tta.apply_view(peak, 1).double()).any())      # the test can fail: hflip is not closed under a turn


# ------------------------------------------------------------------------------------------------ tiled
@pytest.mark.parametrize("name", ["flips", "d4"])
def test_tiled_store_blend_and_masks(cuda, name):
    from unet_watermark_amd import tiling
    L, lib = _lib()
    c = _case(cuda)
    pred = c["pred"]
    sizes = [(100, 70), (70, 161)]
    imgs = _images(sizes, 41)
    tiles, plans = tiling.plan_batch(sizes, T, T, OVERLAP, N)
    K = len(tiles)
    assert K == 12 and int((tiles["image"] >= 0).sum()) == 4 + 8
    crops = np.stack([R.crop(imgs[t["image"]], int(t["y0"]), int(t["x0"]), T, T) for t in tiles])
    crops = torch.from_numpy(np.ascontiguousarray(crops)).to(cuda)      # (a fancy-indexed crop is not C-ordered, and np.stack keeps its order)
    base = torch.full((K, T, T, 4), float("nan"), device=cuda)
    mc, sc = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    L.check(lib.uwm_op_preprocess_u8_nhwc4(_P(crops), K * T * T, 3, mc, sc, _P(base), C.c_void_p(L.stream_ptr(cuda))))
    want_store, _ = _ref_merged(pred, base, name)
    store_np = want_store.cpu().numpy()
    blended = []
    for i, (h, w) in enumerate(sizes):
        f, cnt = int(plans[i]["first"]), int(plans[i]["ny"]) * int(plans[i]["nx"])
        blended.append(R.blend(store_np[f: f + cnt], h, w, T, T, OVERLAP))
    old = pred.threshold
    try:
        pred.threshold = float(np.median(np.concatenate([b.reshape(-1) for b in blended])))
        for use_graph in (False, True):
            masks, lgs = pred.predict_images_tiled(imgs, OVERLAP, return_logits=True, use_graph=use_graph, tta=name)
            if not use_graph:
                assert torch.equal(_bits(pred.model._tile_store), _bits(want_store)), name
            for m, lg, want, s in zip(masks, lgs, blended, sizes):
                assert tuple(m.shape) == s and np.array_equal(lg.cpu().numpy().view(np.int32), want.view(np.int32)), (name, use_graph, s)
                assert np.array_equal(m.cpu().numpy(), R.predict_mask(want, pred.threshold, False)), (name, use_graph, s)
            assert 0.05 < float((torch.cat([m.reshape(-1) for m in masks]) > 0).float().mean()) < 0.95
        plain = pred.predict_images_tiled(imgs, OVERLAP, return_logits=True)[1]
        assert any(not torch.equal(_bits(a), _bits(b)) for a, b in zip(plain, lgs))      # the views did something
    finally:
        pred.threshold = old


# ------------------------------------------------------------------------------------------------ composition
def test_mask_type_and_scoring_compose_with_tta(cuda):
    import unet_watermark_amd as U
    from unet_watermark_amd.scoring import boundary_radius, score_masks_ragged
    c = _case(cuda)
    pred = c["pred"]
    old = pred.threshold
    try:
        pred.threshold = c["thr"]
        raw = pred.predict_images(c["imgs"], tta="d4")
        _, _, mdescs = U.pack_images(c["imgs"])
        flat = torch.cat([m.reshape(-1) for m in raw])
        post = U.optimize_masks_ragged(flat, mdescs, "watermark")
        want = [post[int(o): int(o) + h * w].view(h, w) for o, (h, w) in zip(mdescs["offset"], c["sizes"])]
        for use_graph in (False, True):
            got = pred.predict_images(c["imgs"], mask_type="watermark", tta="d4", use_graph=use_graph)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), use_graph
        assert any(not torch.equal(a, b) for a, b in zip(raw, want))          # the post-processing did something
        rng = np.random.default_rng(51)
        truths = [(rng.random(s) < 0.4).astype(np.uint8) * 255 for s in c["sizes"]]
        truth = torch.cat([torch.from_numpy(t).reshape(-1) for t in truths]).to(cuda)
        radii = [boundary_radius(h, w, 0.02) for h, w in c["sizes"]]
        want_counts = score_masks_ragged(flat, truth, mdescs, radii).cpu().numpy()
        got_counts = pred.score_images(c["imgs"], truths, tta="d4")
        assert np.array_equal(got_counts, want_counts) and int(want_counts[:, 0].sum()) > 0 and (want_counts[:, 7] == 0).all()
        tiled = pred.predict_images_tiled(c["imgs"], OVERLAP, tta="hflip")
        tiled_counts = score_masks_ragged(torch.cat([m.reshape(-1) for m in tiled]), truth, mdescs, radii).cpu().numpy()
        assert np.array_equal(pred.score_images(c["imgs"], truths, tile=True, overlap=OVERLAP, tta="hflip"), tiled_counts)
    finally:
        pred.threshold = old


def test_nothing_changes_without_the_flag(cuda):
    c = _case(cuda)
    pred = c["pred"]
    rng = np.random.default_rng(61)
    truths = [(rng.random(s) < 0.4).astype(np.uint8) * 255 for s in c["sizes"]]
    old = pred.threshold
    try:
        pred.threshold = c["thr"]

        def snapshot(**kw):
            a = [m.clone() for m in pred.predict_images(c["imgs"], **kw)]
            b, bl = pred.predict_images_tiled(c["imgs"], OVERLAP, return_logits=True, **kw)
            s = pred.score_images(c["imgs"], truths, **kw)
            return a, [m.clone() for m in b], [x.clone() for x in bl], s
        before = snapshot()
        graph, xkeys = pred._graphs["images"].graph, set(_graphs_of(pred, "tiled"))
        pred.predict_images(c["imgs"], tta="d4")
        pred.predict_images_tiled(c["imgs"], OVERLAP, tta="flips")
        pred.score_images(c["imgs"], truths, tta="hflip")
        for kw in ({}, dict(tta=None), dict(tta="none"), dict(tta=1)):
            after = snapshot(**kw)
            assert all(torch.equal(x, y) for x, y in zip(before[0], after[0])), kw
            assert all(torch.equal(x, y) for x, y in zip(before[1], after[1])), kw
            assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(before[2], after[2])), kw
            assert np.array_equal(before[3], after[3]), kw
        assert pred._graphs["images"].graph is graph and xkeys <= set(_graphs_of(pred, "tiled"))          # the default paths' graphs stay as captured
        # the plain call is what views = 0x01 computes through the new entry: the same masks
        eager = pred.predict_images(c["imgs"], use_graph=False)
        assert all(torch.equal(x, y) for x, y in zip(eager, before[0]))
        assert all(torch.equal(x, y) for x, y in zip(_ragged_masks(_ref_merged(pred, c["base"], "none", 3)[0], c["sizes"], c["thr"], cuda), before[0]))
    finally:
        pred.threshold = old
    with pytest.raises(ValueError):
        pred.predict_images(c["imgs"], tta="rot")
    with pytest.raises(ValueError):
        pred.predict_images(c["imgs"], return_logits=True)


def test_a_misfit_image_gets_zeros_and_costs_only_itself(cuda):
    import unet_watermark_amd as U
    from unet_watermark_amd import tiling
    from unet_watermark_amd.data import descs_tensor
    c = _case(cuda)
    pred = c["pred"]
    packed, descs, mdescs = U.pack_images(c["imgs"])
    areas = descs["h"].astype(np.int64) * descs["w"]
    mask_bytes = int(areas.sum())
    packed_t, mdescs_t = packed.to(cuda), descs_tensor(mdescs, cuda)

    def split(buf):
        return [buf[int(o): int(o) + int(a)] for o, a in zip(mdescs["offset"], areas)]

    def run(descs_np, mask):
        pred.model.predict_images_tta_u8(packed_t, descs_tensor(descs_np, cuda), mdescs_t, mask, 3, N, (T, T), 0xFF, MEAN, STD, c["thr"], False)
        torch.cuda.synchronize(cuda)
        return pred.model._merged_store.clone()
    good_mask = torch.full((mask_bytes,), FILL, dtype=torch.uint8, device=cuda)
    good = run(descs, good_mask)
    assert torch.equal(_bits(good), _bits(c["ref"]["d4"][0]))
    bad = descs.copy()
    bad[1]["h"] = 1 << 20                                                     # the region leaves the buffer: the network sees zeros
    bad_mask = torch.full((mask_bytes,), FILL, dtype=torch.uint8, device=cuda)
    got = run(bad, bad_mask)
    zero_in = c["base"].clone()
    zero_in[1] = 0.0
    want = _ref_merged(pred, zero_in, "d4")[0]
    assert torch.equal(_bits(got), _bits(want)) and not torch.equal(_bits(got[1]), _bits(good[1]))
    for i in (0, 2):
        assert torch.equal(_bits(got[i]), _bits(good[i])) and torch.equal(split(bad_mask)[i], split(good_mask)[i]), i
    # a mask buffer one byte short: the last image is skipped, nothing of it is written
    short = torch.full((mask_bytes,), FILL, dtype=torch.uint8, device=cuda)
    run(descs, short[:-1])
    assert bool((split(short)[2] == FILL).all()) and all(torch.equal(split(short)[i], split(good_mask)[i]) for i in (0, 1))
    # tiled: the image's mask is zeros, as without views
    tiles, plans = tiling.plan_batch(c["sizes"], T, T, OVERLAP, N)
    tiles_t, plans_t = tiling.table_tensor(tiles, cuda), tiling.table_tensor(plans, cuda)

    def run_tiled(descs_np):
        mask = torch.full((mask_bytes,), FILL, dtype=torch.uint8, device=cuda)
        pred.model.predict_tiled_tta_u8(packed_t, descs_tensor(descs_np, cuda), mdescs_t, mask, 3, tiles_t, plans_t, len(tiles), N, (T, T), OVERLAP, 0x11,
                                        MEAN, STD, c["thr"], False, None)
        torch.cuda.synchronize(cuda)
        return split(mask)
    tg, tb = run_tiled(descs), run_tiled(bad)
    assert not tb[1].any() and tg[1].any() and torch.equal(tb[0], tg[0]) and torch.equal(tb[2], tg[2])
