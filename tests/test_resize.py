"""cv2-convention resize, the part that needs no device: self-checks of the numpy restatement (tests/resize_ref.py) that the device
kernels are compared with, the host side of data.pack_images, and the argument checks of the new entry points, which fail before
any launch.  Every comparison is exact except the `< 1` bound against float bilinear."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from unet_watermark_amd import _lib
    _lib.lib()
    return _lib


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("C_", [1, 3, 4])
def test_reference_is_the_identity_at_equal_size(C_):
    for img in R.images(C_):
        h, w = img.shape[:2]
        assert np.array_equal(R.resize_u8_linear(img, h, w), img)
        assert np.array_equal(R.resize_u8_nearest(img, h, w), img)
        # the general formula gives the identity too (the kernels have no special case): every tap is (s, 2048, 0)
        s, s1, a0, a1 = R.taps(w, w)
        assert np.array_equal(s, np.arange(w)) and (a0 == 2048).all() and (a1 == 0).all()


def test_reference_exact_2x_shrink_is_the_rounded_box_mean():
    """OpenCV's own shortcut for an exact 2x shrink: (s00 + s01 + s10 + s11 + 2) >> 2"""
    for img in R.images(3, [(128, 128), (64, 192), (2, 2), (480, 640)]):
        h, w = img.shape[:2]
        I = img.astype(np.int64)
        box = (I[0::2, 0::2] + I[0::2, 1::2] + I[1::2, 0::2] + I[1::2, 1::2] + 2) >> 2
        assert np.array_equal(R.resize_u8_linear(img, h // 2, w // 2), box.astype(np.uint8))


@pytest.mark.parametrize("dst", R.DESTS)
def test_reference_linear_stays_within_one_grey_level_of_float_bilinear(dst):
    worst = 0.0
    for C_ in (1, 3, 4):
        for img in R.images(C_):
            out = R.resize_u8_linear(img, *dst)
            assert out.dtype == np.uint8 and out.shape == (*dst, C_)
            worst = max(worst, float(np.abs(out.astype(np.float64) - R.float_bilinear(img, *dst)).max()))
    print(f"max |fixed-point - float bilinear| at {dst}: {worst:.3f}")
    assert worst < 1.0


def test_reference_nearest_pins_the_order_of_operations():
    """1.0 / (dst / src) is not src / dst in doubles: the index differs at 186 -> 64 (and 68 -> 96, 198 -> 32), so a kernel that
    divides the other way round is caught by the batch of the GPU test"""
    for src, dst in ((186, 64), (68, 96), (198, 32)):
        other = np.minimum(np.floor(np.arange(dst) * (float(src) / float(dst))).astype(np.int64), src - 1)
        assert not np.array_equal(R.nearest_index(dst, src), other), (src, dst)
    assert (50, 186) in R.SHAPES and (9, 68) in R.SHAPES and (64, 64) in R.DESTS and (64, 96) in R.DESTS
    img = R.images(1, [(5, 186)])[0]
    assert np.array_equal(R.resize_u8_nearest(img, 5, 64), img[:, R.nearest_index(64, 186)])


# ------------------------------------------------------------------------------------------------ pack_images (host)
def test_pack_images_offsets_descriptors_and_bytes(L):
    from unet_watermark_amd import data as D
    imgs = R.images(3)
    imgs[2] = torch.from_numpy(imgs[2])                       # tensors are taken too
    packed, descs, mdescs = D.pack_images(imgs)
    assert packed.dtype == torch.uint8 and packed.dim() == 1
    assert descs.dtype == D.DESC_DTYPE and D.DESC_DTYPE.itemsize == 16 and len(descs) == len(mdescs) == len(imgs)
    off = descs["offset"]
    assert (off % 4 == 0).all() and off[0] == 0 and (np.diff(off) > 0).all()
    flat = packed.numpy()
    moff = 0
    for im, d, m in zip(imgs, descs, mdescs):
        a = np.asarray(im)
        assert (d["h"], d["w"]) == a.shape[:2] == (m["h"], m["w"])
        assert np.array_equal(flat[d["offset"]: d["offset"] + a.size].reshape(a.shape), a)
        assert m["offset"] == moff
        moff += a.shape[0] * a.shape[1]
    last = np.asarray(imgs[-1])
    assert off[-1] + last.size <= packed.numel() < off[-1] + last.size + 4
    assert all(                                               # images do not overlap
        int(o1) >= int(o0) + np.asarray(im).size for im, o0, o1 in zip(imgs, off[:-1], off[1:]))
    t = D.descs_tensor(descs)
    assert t.dtype == torch.uint8 and t.numel() == 16 * len(imgs)
    assert np.array_equal(t.numpy().view(D.DESC_DTYPE), descs)


def test_pack_images_rejects_what_the_device_would_only_clamp(L):
    from unet_watermark_amd import data as D
    ok = np.zeros((4, 5, 3), np.uint8)
    with pytest.raises(ValueError, match=r"\(h, w, C\)"):
        D.pack_images([ok, np.zeros((4, 5), np.uint8)])
    with pytest.raises(ValueError, match="channels"):
        D.pack_images([ok, np.zeros((4, 5, 1), np.uint8)])
    with pytest.raises(TypeError, match="uint8"):
        D.pack_images([ok, np.zeros((4, 5, 3), np.float32)])
    with pytest.raises(ValueError, match=">= 1"):
        D.pack_images([ok, np.zeros((0, 5, 3), np.uint8)])
    with pytest.raises(ValueError, match=">= 1"):
        D.pack_images([np.zeros((4, 0, 3), np.uint8)])
    with pytest.raises(ValueError, match="no images"):
        D.pack_images([])


def test_python_layer_has_no_cpu_fallback(L):
    from unet_watermark_amd import data as D
    packed, descs, _ = D.pack_images([np.zeros((4, 5, 3), np.uint8)])
    with pytest.raises(ValueError, match="interp"):
        D.device_resize(packed, descs, 8, 3, interp="cubic")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            D.device_resize(packed, descs, 8, 3)


# ------------------------------------------------------------------------------------------------ argument checks, no device
def test_new_entry_points_check_arguments_before_any_launch(L):
    """a null pointer, C = 5, interp = 2, H = 0, a misaligned buffer, std = 0: every such call returns non-zero with a message and
    none reaches a launch (the pointers are host memory)"""
    lib = L.lib()
    buf = (C.c_uint8 * 4096)()
    p = C.c_void_p(C.addressof(buf) + (-C.addressof(buf)) % 16)
    odd = C.c_void_p(p.value + 2)
    mean = (C.c_float * 4)(0.5, 0.5, 0.5, 0.5); std = (C.c_float * 4)(0.25, 0.25, 0.25, 0.25); std0 = (C.c_float * 4)(0.25, 0.0, 0.25, 0.25)

    def bad(rc, word):
        assert rc != 0
        msg = lib.uwm_last_error().decode()
        assert word in msg, msg

    bad(lib.uwm_resize_u8(None, 64, p, 1, 3, 8, 8, 1, p, None), "null")
    bad(lib.uwm_resize_u8(p, 64, None, 1, 3, 8, 8, 1, p, None), "null")
    bad(lib.uwm_resize_u8(p, 64, p, 1, 3, 8, 8, 1, None, None), "null")
    bad(lib.uwm_resize_u8(p, 64, p, 1, 5, 8, 8, 1, p, None), "1..4")
    bad(lib.uwm_resize_u8(p, 64, p, 1, 0, 8, 8, 1, p, None), "1..4")
    bad(lib.uwm_resize_u8(p, 64, p, 1, 3, 8, 8, 2, p, None), "interp")
    bad(lib.uwm_resize_u8(p, 64, p, 1, 3, 8, 8, -1, p, None), "interp")
    bad(lib.uwm_resize_u8(p, 64, p, 1, 3, 0, 8, 1, p, None), ">= 1")
    bad(lib.uwm_resize_u8(p, 64, p, 1, 3, 8, 0, 1, p, None), ">= 1")
    bad(lib.uwm_resize_u8(p, 64, p, 0, 3, 8, 8, 1, p, None), ">= 1")
    bad(lib.uwm_resize_u8(p, 0, p, 1, 3, 8, 8, 1, p, None), ">= 1")
    bad(lib.uwm_resize_u8(odd, 64, p, 1, 3, 8, 8, 1, p, None), "aligned")
    bad(lib.uwm_resize_u8(p, 64, odd, 1, 3, 8, 8, 1, p, None), "aligned")

    bad(lib.uwm_op_resize_norm_u8_nhwc4(None, 64, p, 1, 3, 8, 8, mean, std, p, None), "null")
    bad(lib.uwm_op_resize_norm_u8_nhwc4(p, 64, None, 1, 3, 8, 8, mean, std, p, None), "null")
    bad(lib.uwm_op_resize_norm_u8_nhwc4(p, 64, p, 1, 3, 8, 8, None, std, p, None), "null")
    bad(lib.uwm_op_resize_norm_u8_nhwc4(p, 64, p, 1, 3, 8, 8, mean, None, p, None), "null")
    bad(lib.uwm_op_resize_norm_u8_nhwc4(p, 64, p, 1, 3, 8, 8, mean, std, None, None), "null")
    bad(lib.uwm_op_resize_norm_u8_nhwc4(p, 64, p, 1, 5, 8, 8, mean, std, p, None), "1..4")
    bad(lib.uwm_op_resize_norm_u8_nhwc4(p, 64, p, 1, 3, 0, 8, mean, std, p, None), ">= 1")
    bad(lib.uwm_op_resize_norm_u8_nhwc4(p, 64, p, 1, 3, 8, 8, mean, std, odd, None), "aligned")
    bad(lib.uwm_op_resize_norm_u8_nhwc4(p, 64, p, 1, 3, 8, 8, mean, std0, p, None), "positive")

    lg = C.c_void_p(p.value)
    bad(lib.uwm_resize_threshold_ragged(None, 1, 1, 8, 8, p, 0.5, 0, p, 64, None), "null")
    bad(lib.uwm_resize_threshold_ragged(lg, 1, 1, 8, 8, None, 0.5, 0, p, 64, None), "null")
    bad(lib.uwm_resize_threshold_ragged(lg, 1, 1, 8, 8, p, 0.5, 0, None, 64, None), "null")
    bad(lib.uwm_resize_threshold_ragged(lg, 1, 1, 0, 8, p, 0.5, 0, p, 64, None), ">= 1")
    bad(lib.uwm_resize_threshold_ragged(lg, 1, 0, 8, 8, p, 0.5, 0, p, 64, None), ">= 1")
    bad(lib.uwm_resize_threshold_ragged(lg, 0, 1, 8, 8, p, 0.5, 0, p, 64, None), ">= 1")
    bad(lib.uwm_resize_threshold_ragged(lg, 1, 1, 8, 8, p, 0.5, 0, p, 0, None), ">= 1")
    bad(lib.uwm_resize_threshold_ragged(lg, 1, 1, 8, 8, odd, 0.5, 0, p, 64, None), "aligned")

    # uwm_predict_images_u8 on a real (unbound) handle: null arguments first, then "call uwm_bind first" — never a launch
    desc = L.uwm_unet_desc(18, 3, 1, (C.c_int * 5)(256, 128, 64, 32, 16), 1e-5, 0.1, 0)
    h = C.c_void_p()
    assert lib.uwm_create(C.byref(desc), C.byref(h)) == 0
    try:
        args = lambda **kw: [kw.get(k, v) for k, v in dict(h=h, src=p, src_bytes=64, ind=p, mean=mean, std=std, thr=0.5, sig=0, outd=p,
                                                            mask=p, mask_bytes=64, logits=None, ws=p, ws_bytes=4096, N=1, H=64, W=64,
                                                            st=None).items()]
        for k in ("h", "src", "ind", "mean", "std", "outd", "mask", "ws"):
            bad(lib.uwm_predict_images_u8(*args(**{k: None})), "null")
        bad(lib.uwm_predict_images_u8(*args(H=0)), "Wrong input shape")
        bad(lib.uwm_predict_images_u8(*args(W=48)), "Wrong input shape")
        bad(lib.uwm_predict_images_u8(*args(N=0)), "batch size")
        bad(lib.uwm_predict_images_u8(*args()), "uwm_bind")
    finally:
        lib.uwm_destroy(h)


def test_cli_and_predictor_take_the_resize_switch(L):
    import inspect
    from unet_watermark_amd import cli
    from unet_watermark_amd.predict import WatermarkPredictor
    with pytest.raises(SystemExit):
        cli.main(["predict", "--input", "a", "--output", "b", "--model", "c", "--resize", "gpu"])
    sig = inspect.signature(WatermarkPredictor.predict_images).parameters
    assert sig["apply_sigmoid"].default is False and sig["mask_type"].default is None and sig["use_graph"].default is True
    base = ["predict", "--input", "a", "--output", "b", "--model", "c"]
    assert cli.build_parser().parse_args(base).resize == "host"                    # today's path stays the default
    assert cli.build_parser().parse_args(base + ["--resize", "device"]).resize == "device"
