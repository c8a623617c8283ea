"""uwm_text_enhance_ragged on the device: one ragged batch (tests/textenh_ref.py: images) packed at odd offsets, every comparison
byte-exact against the literal restatement — the enhanced images, the dilated edge planes and the status words; twice with equal
bytes, one image per call, the same images in another order, and misfits beside good images.  Then end to end through
WatermarkPredictor.predict_images on a random-weight Unet("resnet18") at IMG_SIZE 64: text_enhance=True equals feeding the
restatement's images, eager and graph-replayed, and the default path keeps its graph and its bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import textenh_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu
DESC = np.dtype([("offset", "<i8"), ("h", "<i4"), ("w", "<i4")])
FILL = 0xA5


@pytest.fixture(scope="module")
def cases():
    """[(name, image, enhanced, edges, status)]: the restatement of every case, computed once and left unchanged"""
    out = []
    for name, im in T.images():
        enhanced, edges, status = T.text_enhance(im)
        for a in (im, enhanced, edges):
            a.setflags(write=False)
        out.append((name, im, enhanced, edges, status))
    return out


def pack_odd(arrays, per_pixel):
    """the arrays back to back with gaps, every one at an ODD offset -> (flat uint8 filled with FILL outside them, descs)"""
    descs = np.zeros(len(arrays), DESC)
    off = 1
    for i, a in enumerate(arrays):
        descs[i] = (off, a.shape[0], a.shape[1])
        off += a.shape[0] * a.shape[1] * per_pixel
        off += 2 if off % 2 else 3
    flat = np.full(off + 5, FILL, dtype=np.uint8)
    for a, d in zip(arrays, descs):
        flat[int(d["offset"]): int(d["offset"]) + a.size] = a.reshape(-1)
    return flat, descs


def run(cuda, images, descs=None, edesc=None, max_pixels=None, total_pixels=None):
    """one call -> (out bytes, edge bytes, status), host arrays; out and edges start as FILL"""
    from unet_watermark_amd import _lib as L
    from unet_watermark_amd.textenh import text_enhance_workspace
    flat, d0 = pack_odd(images, 3)
    eflat, e0 = pack_odd([im[:, :, 0] for im in images], 1)
    descs = d0 if descs is None else descs
    edesc = e0 if edesc is None else edesc
    n = len(images)
    areas = [im.shape[0] * im.shape[1] for im in images]
    max_pixels = max(areas) if max_pixels is None else max_pixels
    total_pixels = sum(areas) if total_pixels is None else total_pixels
    src = torch.from_numpy(flat).to(cuda)
    dst = torch.full_like(src, FILL)
    edges = torch.full((eflat.size,), FILL, dtype=torch.uint8, device=cuda)
    dd = torch.from_numpy(np.concatenate([descs, edesc]).view(np.uint8).copy()).to(cuda)
    ws = text_enhance_workspace(cuda, total_pixels, n)
    p = lambda t, o=0: C.c_void_p(t.data_ptr() + o)      # noqa: E731
    L.check(L.lib().uwm_text_enhance_ragged(p(src), p(dst), src.numel(), p(dd), n, 3, max_pixels, total_pixels, p(edges), edges.numel(),
                                            p(dd, 16 * n), p(ws), ws.numel(), C.c_void_p(L.stream_ptr(cuda))))
    torch.cuda.synchronize(cuda)
    assert torch.equal(src.cpu(), torch.from_numpy(flat))                  # the input is left alone
    return dst.cpu().numpy(), edges.cpu().numpy(), ws[:4 * n].view(torch.int32).cpu().numpy().copy(), d0, e0


def expected(cases_, order, d0, e0, sizes, untouched=()):
    """the bytes the call must leave: FILL everywhere but the images' regions.  sizes: (out bytes, edge bytes)"""
    out = np.full(sizes[0], FILL, dtype=np.uint8)
    edges = np.full(sizes[1], FILL, dtype=np.uint8)
    for k, i in enumerate(order):
        if k in untouched:
            continue
        _, _, enhanced, ed, _ = cases_[i]
        out[int(d0["offset"][k]): int(d0["offset"][k]) + enhanced.size] = enhanced.reshape(-1)
        edges[int(e0["offset"][k]): int(e0["offset"][k]) + ed.size] = ed.reshape(-1)
    return out, edges


def check(cases_, order, got_out, got_edges, status, d0, e0):
    want_out, want_edges = expected(cases_, order, d0, e0, (got_out.size, got_edges.size))
    for k, i in enumerate(order):                                         # per image first: a failure names its case
        name, im, enhanced, ed, st = cases_[i]
        o, e = int(d0["offset"][k]), int(e0["offset"][k])
        assert status[k] == st, name
        assert np.array_equal(got_edges[e: e + ed.size].reshape(ed.shape), ed), name
        assert np.array_equal(got_out[o: o + im.size].reshape(im.shape), enhanced), name
    assert np.array_equal(got_out, want_out) and np.array_equal(got_edges, want_edges)      # and nothing outside the images was written


def test_the_batch_equals_the_restatement_and_two_runs_give_equal_bytes(cuda, cases):
    order = list(range(len(cases)))
    images = [cases[i][1] for i in order]
    out1, edges1, status1, d0, e0 = run(cuda, images)
    assert all(int(d["offset"]) % 2 == 1 for d in d0) and all(int(d["offset"]) % 2 == 1 for d in e0)
    check(cases, order, out1, edges1, status1, d0, e0)
    out2, edges2, status2, _, _ = run(cuda, images)
    assert np.array_equal(out1, out2) and np.array_equal(edges1, edges2) and np.array_equal(status1, status2)
    by_name = {c[0]: k for k, c in enumerate(cases)}
    assert status1[by_name["small 12x40"]] == T.COPIED and (status1[:by_name["small 12x40"]] == T.DONE).all()
    # hysteresis crossed every tile of the strong spiral and left nothing of the weak one
    e = int(e0["offset"][by_name["spiral strong"]])
    assert (edges1[e: e + 96 * 200] == 255).sum() > 3000
    e = int(e0["offset"][by_name["spiral weak"]])
    assert not edges1[e: e + 96 * 200].any()


def test_one_image_per_call(cuda, cases):
    for i in range(len(cases)):
        out, edges, status, d0, e0 = run(cuda, [cases[i][1]])
        check(cases, [i], out, edges, status, d0, e0)


def test_the_same_images_in_another_order(cuda, cases):
    order = [8, 3, 9, 0, 7, 5, 2, 6, 1, 4]
    out, edges, status, d0, e0 = run(cuda, [cases[i][1] for i in order])
    check(cases, order, out, edges, status, d0, e0)


def test_misfits_are_reported_and_cost_the_others_nothing(cuda, cases):
    order = [0, 1, 3, 6]
    images = [cases[i][1] for i in order]
    flat, d0 = pack_odd(images, 3)
    _, e0 = pack_odd([im[:, :, 0] for im in images], 1)
    # image 1's region leaves the buffer; image 2 exceeds max_pixels (40 * 64 = 2560 > 2000)
    bad = d0.copy()
    bad["offset"][1] = flat.size - 10
    out, edges, status, _, _ = run(cuda, images, descs=bad, max_pixels=2000, total_pixels=16 * 16 + 40 * 48)
    assert status.tolist() == [T.DONE, T.MISFIT, T.MISFIT, T.DONE]
    want_out, want_edges = expected(cases, order, d0, e0, (out.size, edges.size), untouched=(1, 2))
    assert np.array_equal(out, want_out) and np.array_equal(edges, want_edges)
    # the planes of the workspace hold 16 * 16 + 17 * 23 pixels: the images from the third on do not fit; an edge descriptor of
    # another size is a misfit too
    ebad = e0.copy()
    ebad["w"][0] += 1
    out, edges, status, _, _ = run(cuda, images, edesc=ebad, total_pixels=16 * 16 + 17 * 23)
    assert status.tolist() == [T.MISFIT, T.DONE, T.MISFIT, T.MISFIT]
    want_out, want_edges = expected(cases, order, d0, e0, (out.size, edges.size), untouched=(0, 2, 3))
    assert np.array_equal(out, want_out) and np.array_equal(edges, want_edges)


def test_enhance_text_features_returns_the_restatement(cuda, cases):
    from unet_watermark_amd.textenh import enhance_text_features
    images = [c[1] for c in cases]
    got, edges, status = enhance_text_features(images, cuda, return_edges=True, return_status=True)
    assert status.tolist() == [c[4] for c in cases]
    for (name, im, enhanced, ed, _), g, e in zip(cases, got, edges):
        assert g.dtype == torch.uint8 and g.device.type == "cuda" and tuple(g.shape) == im.shape
        assert np.array_equal(g.cpu().numpy(), enhanced) and np.array_equal(e.cpu().numpy(), ed), name
    plain = enhance_text_features(images[:2], cuda)
    assert len(plain) == 2 and np.array_equal(plain[1].cpu().numpy(), cases[1][2])


# ------------------------------------------------------------------------------------------------ the predictor
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
    cfg = get_cfg_defaults(); cfg.MODEL.NAME = "Unet"; cfg.MODEL.ENCODER_NAME = "resnet18"; cfg.DATA.IMG_SIZE = 64
    return WatermarkPredictor(model=m, config=cfg, device=dev, precision="f32")


def test_predict_images_with_text_enhance_equals_predicting_the_enhanced_images(cuda, cases):
    import unet_watermark_amd as U
    from unet_watermark_amd.constants import IMAGENET_MEAN as MEAN, IMAGENET_STD as STD
    pred = _predictor(cuda)
    pick = ("33x130", "spiral strong", "40x64", "small 12x40", "borders")
    imgs = [c[1] for c in cases if c[0] in pick]
    ref_enhanced = [c[2] for c in cases if c[0] in pick]
    assert any(not np.array_equal(a, b) for a, b in zip(imgs, ref_enhanced))
    packed, descs, _ = U.pack_images(ref_enhanced)
    _, lg = pred.model.predict_u8(U.device_resize(packed, descs, 64, 3), MEAN[:3], STD[:3], 0.0, return_logits=True)
    pred.threshold = float(lg.median())
    for mask_type in ("text", None):
        before = [m.clone() for m in pred.predict_images(imgs, mask_type=mask_type)]                 # today's path, flag off
        want = [m.clone() for m in pred.predict_images(ref_enhanced, mask_type=mask_type)]
        if mask_type is None:
            assert all(0.02 < float((m > 0).float().mean()) < 0.98 for m in want)
        assert any(not torch.equal(a, b) for a, b in zip(before, want))                               # the enhancement matters to the masks
        default_graph = pred._graphs["images_post"].graph if mask_type else pred._graphs["images"].graph
        assert default_graph is not None
        for use_graph in (True, False, True):
            got = pred.predict_images(imgs, mask_type=mask_type, text_enhance=True, use_graph=use_graph)
            for a, g, w in zip(imgs, got, want):
                assert g.dtype == torch.uint8 and tuple(g.shape) == a.shape[:2] and torch.equal(g, w), (mask_type, use_graph, a.shape)
        # the default path: the same graph object as before, and today's bytes
        for use_graph in (True, False):
            again = pred.predict_images(imgs, mask_type=mask_type, use_graph=use_graph)
            assert all(torch.equal(a, b) for a, b in zip(again, before))
        assert (pred._graphs["images_post"].graph if mask_type else pred._graphs["images"].graph) is default_graph
        assert (pred._graphs["text_images_post"].graph if mask_type else pred._graphs["text_images"].graph) is not None
    stats = pred.mask_stats(imgs, "text", text_enhance=True)
    assert np.array_equal(stats, pred.mask_stats(ref_enhanced, "text"))


def test_a_graph_captured_on_an_index_less_device_pins_the_workspaces_it_replays_on(cuda):
    """WatermarkPredictor(device="cuda"): the captured calls took their workspaces under their buffers' device, cuda:0.  The entry's
    keep must hold those very tensors, so that a larger eager call, which replaces them in the store, leaves the graph replaying on
    memory it owns."""
    import unet_watermark_amd as U
    from unet_watermark_amd import _device as D
    from unet_watermark_amd.constants import IMAGENET_MEAN as MEAN, IMAGENET_STD as STD
    from unet_watermark_amd.postprocess import optimize_masks_ragged
    pred = _predictor("cuda")
    rng = np.random.default_rng(11)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((40, 56), (72, 48))]
    packed, descs, _ = U.pack_images(imgs)
    _, lg = pred.model.predict_u8(U.device_resize(packed, descs, 64, 3), MEAN[:3], STD[:3], 0.0, return_logits=True)
    pred.threshold = float(lg.median())
    for name in ("mask_ragged", "text_enhance"):                   # (earlier tests have grown the buffers: start from none)
        D._WORKSPACE.pop((name, cuda), None)
    kw = dict(mask_type="watermark", text_enhance=True, return_stats=True)
    eager, eager_stats = pred.predict_images(imgs, use_graph=False, **kw)
    first, first_stats = pred.predict_images(imgs, **kw)          # the capture
    pred.predict_images(imgs, **kw)                                # a replay
    entry = pred._graphs["text_images_post"]
    for name in ("mask_ragged", "text_enhance"):
        assert any(t is D._WORKSPACE[(name, cuda)] for t in entry.keep), name
    pinned = D._WORKSPACE[("mask_ragged", cuda)]
    big = np.zeros(1, DESC)
    big[0] = (0, 900, 1100)
    optimize_masks_ragged(torch.zeros(900 * 1100, dtype=torch.uint8, device=cuda), big)
    assert D._WORKSPACE[("mask_ragged", cuda)] is not pinned      # the store moved on to a larger buffer
    again, again_stats = pred.predict_images(imgs, **kw)          # a replay, on the pinned one
    assert pred._graphs["text_images_post"] is entry
    assert first_stats[:, 6].tolist() == [40 * 56, 72 * 48] and not first_stats[:, 7].any()      # every image was served
    assert np.array_equal(again_stats, first_stats) and np.array_equal(first_stats, eager_stats)
    for a, f, e in zip(again, first, eager):
        assert torch.equal(a, f) and torch.equal(f, e)
