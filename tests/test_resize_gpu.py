"""cv2-convention resize on the device (csrc/resize_u8.hip) against the numpy restatement (tests/resize_ref.py), and the ragged
predict path built on it.  All outputs are integers (or fp32 values compared bit for bit): every comparison is exact, no case is
exempted."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)
INTERPS = (("linear", 1, R.resize_u8_linear), ("nearest", 0, R.resize_u8_nearest))


def _lib():
    from unet_watermark_amd import _lib as L
    return L, L.lib()


def _P(t):
    return C.c_void_p(t.data_ptr())


def _pack_with_gaps(imgs, gap_seed=5, exact_end=False):
    """the images at 4-byte-aligned offsets with 4..28 random bytes between them (a kernel that reads a neighbour's bytes shows);
    exact_end: the buffer ends with the last image's last byte (its size need not be a multiple of 4)"""
    from unet_watermark_amd.data import DESC_DTYPE
    rng = np.random.default_rng(gap_seed)
    descs = np.zeros(len(imgs), DESC_DTYPE)
    off = 4 * int(rng.integers(1, 8))
    for i, a in enumerate(imgs):
        descs[i] = (off, a.shape[0], a.shape[1])
        end = off + a.size
        off = (end + 3) // 4 * 4 + 4 * int(rng.integers(1, 8))
    buf = rng.integers(0, 256, size=end if exact_end else off, dtype=np.uint8)
    for a, d in zip(imgs, descs):
        buf[d["offset"]: d["offset"] + a.size] = a.reshape(-1)
    return buf, descs


_REF = {}


def _reference(C_, dst, name, fn, imgs):
    key = (C_, dst, name)
    if key not in _REF:
        _REF[key] = np.stack([fn(a, *dst) for a in imgs])
    return _REF[key]


def _resize(lib, L, dev, buf_t, descs_t, n, C_, dst, code, nbytes=None):
    out = torch.full((n, dst[0], dst[1], C_), 77, dtype=torch.uint8, device=dev)
    L.check(lib.uwm_resize_u8(_P(buf_t), buf_t.numel() if nbytes is None else nbytes, _P(descs_t), n, C_, dst[0], dst[1], code, _P(out),
                              C.c_void_p(L.stream_ptr(dev))))
    return out


@pytest.mark.parametrize("dst", R.DESTS)
@pytest.mark.parametrize("C_", [3, 1, 4])
def test_resize_u8_equals_the_restatement_on_a_ragged_batch(cuda, C_, dst):
    """upscale, downscale, identity, exact 2x, one-pixel sides and the 186 / 68 widths in ONE launch, both interpolations"""
    from unet_watermark_amd.data import descs_tensor
    L, lib = _lib()
    imgs = R.images(C_)
    buf, descs = _pack_with_gaps(imgs)
    buf_t, descs_t = torch.from_numpy(buf).to(cuda), descs_tensor(descs, cuda)
    for name, code, fn in INTERPS:
        out = _resize(lib, L, cuda, buf_t, descs_t, len(imgs), C_, dst, code).cpu().numpy()
        want = _reference(C_, dst, name, fn, imgs)
        for i, a in enumerate(imgs):
            assert np.array_equal(out[i], want[i]), (name, C_, dst, a.shape[:2], int(np.abs(out[i].astype(int) - want[i]).max()))


@pytest.mark.parametrize("C_,shapes", [(1, [(3, 16383), (3, 16385), (2, 40000)]), (3, [(2, 5462), (3, 6000), (3, 5461)]),
                                       (4, [(2, 4096), (2, 4097), (5, 3)])])
def test_resize_u8_rows_at_and_beyond_the_staging_width(cuda, C_, shapes):
    """source rows of exactly the widest staged size (16384 bytes; 16383 with a row that starts off a dword boundary) and wider ones,
    which are gathered from global memory; the buffer ends with the last image's last byte"""
    from unet_watermark_amd.data import descs_tensor
    L, lib = _lib()
    imgs = R.images(C_, shapes, seed=3)
    buf, descs = _pack_with_gaps(imgs, exact_end=True)
    buf_t, descs_t = torch.from_numpy(buf).to(cuda), descs_tensor(descs, cuda)
    dst = (5, 96)
    for name, code, fn in INTERPS:
        out = _resize(lib, L, cuda, buf_t, descs_t, len(imgs), C_, dst, code).cpu().numpy()
        for i, a in enumerate(imgs):
            assert np.array_equal(out[i], fn(a, *dst)), (name, C_, a.shape[:2])


def test_a_descriptor_outside_the_buffer_costs_that_image_only(cuda):
    """h*w*C beyond src_bytes, a negative offset, a zero side: zeros for that image, the others untouched by it"""
    from unet_watermark_amd.data import descs_tensor
    L, lib = _lib()
    imgs = R.images(3, [(20, 30), (16, 16), (7, 9), (12, 40)], seed=9)
    buf, descs = _pack_with_gaps(imgs)
    bad = descs.copy()
    bad[0]["h"] = 1 << 20
    bad[1]["offset"] = -4
    bad[2]["w"] = 0
    buf_t = torch.from_numpy(buf).to(cuda)
    out = _resize(lib, L, cuda, buf_t, descs_tensor(bad, cuda), 4, 3, (24, 24), 1).cpu().numpy()
    assert not out[:3].any()
    assert np.array_equal(out[3], R.resize_u8_linear(imgs[3], 24, 24))
    short = int(descs[3]["offset"]) + imgs[3].size - 1            # src_bytes one byte short of the last image
    out = _resize(lib, L, cuda, buf_t, descs_tensor(descs, cuda), 4, 3, (24, 24), 1, nbytes=short).cpu().numpy()
    assert not out[3].any()
    for i in range(3):
        assert np.array_equal(out[i], R.resize_u8_linear(imgs[i], 24, 24))


@pytest.mark.parametrize("C_", [3, 1])
def test_fused_resize_normalize_equals_resize_then_preprocess(cuda, C_):
    from unet_watermark_amd.data import descs_tensor
    L, lib = _lib()
    imgs = R.images(C_)
    buf, descs = _pack_with_gaps(imgs)
    buf_t, descs_t = torch.from_numpy(buf).to(cuda), descs_tensor(descs, cuda)
    n, st = len(imgs), C.c_void_p(L.stream_ptr(cuda))
    mc, sc = (C.c_float * C_)(*MEAN[:C_]), (C.c_float * C_)(*STD[:C_])
    for dst in R.DESTS:
        u8 = _resize(lib, L, cuda, buf_t, descs_t, n, C_, dst, 1)
        want = torch.full((n, dst[0], dst[1], 4), float("nan"), device=cuda)
        L.check(lib.uwm_op_preprocess_u8_nhwc4(_P(u8), n * dst[0] * dst[1], C_, mc, sc, _P(want), st))
        out = torch.full((n, dst[0], dst[1], 4), float("nan"), device=cuda)
        L.check(lib.uwm_op_resize_norm_u8_nhwc4(_P(buf_t), buf_t.numel(), _P(descs_t), n, C_, dst[0], dst[1], mc, sc, _P(out), st))
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), (C_, dst)
        assert float(out[..., C_:].abs().max()) == 0.0 if C_ < 4 else True


@pytest.mark.parametrize("apply_sigmoid", [False, True])
@pytest.mark.parametrize("ld", [1, 4])
def test_resize_threshold_ragged_equals_the_uniform_call_per_image(cuda, apply_sigmoid, ld):
    from unet_watermark_amd.data import DESC_DTYPE, descs_tensor
    L, lib = _lib()
    sizes = [(150, 201), (64, 96), (33, 50)]
    n, h, w = 3, 64, 96
    lg = torch.randn(n, h, w, ld, generator=torch.Generator().manual_seed(4)).to(cuda)
    thr = 0.55 if apply_sigmoid else 0.2
    st = C.c_void_p(L.stream_ptr(cuda))
    descs = np.zeros(n, DESC_DTYPE)
    off = 3                                                        # (mask offsets need no alignment)
    for i, (H, W) in enumerate(sizes):
        descs[i] = (off, H, W)
        off += H * W + 5
    mask = torch.full((off,), 77, dtype=torch.uint8, device=cuda)
    L.check(lib.uwm_resize_threshold_ragged(_P(lg), ld, n, h, w, _P(descs_tensor(descs, cuda)), thr, int(apply_sigmoid), _P(mask),
                                            mask.numel(), st))
    covered = torch.zeros(off, dtype=torch.bool, device=cuda)
    for i, (H, W) in enumerate(sizes):
        want = torch.empty((1, H, W), dtype=torch.uint8, device=cuda)
        L.check(lib.uwm_resize_threshold(_P(lg[i]), ld, 1, h, w, H, W, thr, int(apply_sigmoid), _P(want), None, st))
        o = int(descs[i]["offset"])
        assert torch.equal(mask[o: o + H * W].view(1, H, W), want), (i, H, W)
        assert 0.1 < float((want > 0).float().mean()) < 0.9
        covered[o: o + H * W] = True
    assert bool((mask[~covered] == 77).all())                      # nothing written between the masks
    # a mask that does not fit mask_bytes is skipped, the others are written
    first = mask.clone()
    mask.fill_(77)
    L.check(lib.uwm_resize_threshold_ragged(_P(lg), ld, n, h, w, _P(descs_tensor(descs, cuda)), thr, int(apply_sigmoid), _P(mask),
                                            mask.numel() - 6, st))
    o = int(descs[2]["offset"])
    assert bool((mask[o:] == 77).all()) and torch.equal(mask[:o], first[:o])


def test_device_resize_takes_what_pack_images_makes(cuda):
    import unet_watermark_amd as U
    imgs = R.images(3)
    packed, descs, _ = U.pack_images(imgs)
    for interp, fn in (("linear", R.resize_u8_linear), ("nearest", R.resize_u8_nearest)):
        out = U.device_resize(packed, descs, (64, 96), 3, interp=interp)
        assert out.shape == (len(imgs), 64, 96, 3) and out.dtype == torch.uint8 and out.device.type == "cuda"
        assert np.array_equal(out.cpu().numpy(), _reference(3, (64, 96), interp, fn, imgs))
    assert np.array_equal(U.device_resize(packed, descs, 64, 3).cpu().numpy(), _reference(3, (64, 64), "linear", R.resize_u8_linear, imgs))


# ------------------------------------------------------------------------------------------------ the predictor
def _predictor(dev, frozen):
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


@pytest.mark.parametrize("frozen", [False, True])
def test_predict_images_equals_resize_then_predict_mask_u8_per_image(cuda, frozen):
    """masks of a ragged batch = device_resize -> predict_mask_u8(out_size = that image's size), with and without the text
    post-processing, eager and graph-replayed; a second batch of other sizes replays the SAME graph"""
    import unet_watermark_amd as U
    pred = _predictor(cuda, frozen)
    assert pred.model.frozen == frozen
    batches = [R.images(3, [(37, 53), (150, 201), (64, 64), (97, 33)], seed=1), R.images(3, [(50, 186), (9, 68), (128, 128), (33, 50)], seed=2)]

    def expected(imgs, mask_type):
        packed, descs, _ = U.pack_images(imgs)
        small = U.device_resize(packed, descs, 64, 3)
        return [pred.predict_mask_u8(small, out_size=a.shape[:2], use_graph=False, mask_type=mask_type)[i].clone() for i, a in enumerate(imgs)]

    packed, descs, _ = U.pack_images(batches[0])
    _, lg = pred.model.predict_u8(U.device_resize(packed, descs, 64, 3), MEAN[:3], STD[:3], 0.0, return_logits=True)
    pred.threshold = float(lg.median())
    graphs = []
    for imgs in batches:
        want = expected(imgs, None)
        assert all(0.05 < float((m > 0).float().mean()) < 0.95 for m in want)
        for use_graph in (False, True):
            got = pred.predict_images(imgs, use_graph=use_graph)
            assert len(got) == len(imgs)
            for a, g, m in zip(imgs, got, want):
                assert g.dtype == torch.uint8 and tuple(g.shape) == a.shape[:2] and torch.equal(g, m), a.shape
        graphs.append(pred._graphs["images"].graph)
        want = expected(imgs, "text")
        for g, m in zip(pred.predict_images(imgs, mask_type="text"), want):
            assert torch.equal(g, m)
        assert pred.model.frozen == frozen
    assert graphs[0] is not None and graphs[1] is graphs[0] and pred._graphs["images"].graph is graphs[0]
    # a batch that does not fit the staging buffers is still right (buffers grow, the graph is captured again)
    big = R.images(3, [(300, 400), (64, 64), (10, 10), (200, 50)], seed=4)
    for g, m in zip(pred.predict_images(big), expected(big, None)):
        assert torch.equal(g, m)
    assert pred._graphs["images"].graph is not graphs[0]
