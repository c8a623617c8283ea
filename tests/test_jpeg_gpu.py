"""ImageCompression on the device (csrc/jpeg_u8.hip) against the numpy restatement of its rule (tests/jpeg_ref.py, itself held to
Pillow in test_jpeg.py), the transparent_watermark recipe built on it, and `main.py train --augment config --jpeg device`.  Every
comparison is bit-equal: there is no tolerance and no case is exempted."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ext_ref as R  # noqa: E402
import augment_ref as A  # noqa: E402
import jpeg_ref as J  # noqa: E402

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# (H, W, qualities): the smallest shapes where each part can go wrong; the image kinds cycle through the batch
SHAPES = {
    "16x16": (16, 16, [1, 50, 60, 77, 100]),               # one MCU: every up-sampling edge at once
    "16x48": (16, 48, [2, 25, 60, 95, 100]),               # interior chroma neighbours along x only; 3 MCUs = a partial workgroup
    "48x16": (48, 16, [5, 49, 51, 77, 100]),               # interior chroma neighbours along y only
    "32x32": (32, 32, [1, 10, 60, 90, 100]),               # interior neighbours on both axes
    "64x96": (64, 96, [0, 1, 60, 77, 100]),                # pass-through, the 255 clamp, per-image tables, six workgroups per image
}
KINDS = ("noise", "noise01", "stripes", "checker8", "ramps")
_CASES = {}


def _D():
    from unet_watermark_amd import data
    return data


def _case(name, shift):
    """(images, qualities, expected images): image i is kind (i + shift) % 5.  Computed once."""
    key = (name, shift)
    if key not in _CASES:
        h, w, q = SHAPES[name]
        kinds = J.sample_images(h, w, seed=shift)
        img = np.stack([kinds[KINDS[(i + shift) % 5]] for i in range(len(q))])
        _CASES[key] = (img, np.asarray(q, dtype=np.int32), J.roundtrip_batch(img, q))
    return _CASES[key]


def _abi_call(cuda, img, q, want_f=True, want_u8=True):
    from unet_watermark_amd import _lib as L
    n, h, w, _ = img.shape
    x = torch.from_numpy(img).to(cuda); qd = torch.from_numpy(q).to(cuda)
    ws = torch.empty(int(L.lib().uwm_jpeg_workspace_bytes(n, h, w)), dtype=torch.uint8, device=cuda)
    out = torch.full((n, 3, h, w), float("nan"), device=cuda) if want_f else None
    u8 = torch.full((n, h, w, 3), 7, dtype=torch.uint8, device=cuda) if want_u8 else None
    ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)      # noqa: E731
    L.check(L.lib().uwm_jpeg_u8(ptr(x), ptr(qd), n, h, w, (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD), ptr(ws), ws.numel(), ptr(out),
                                ptr(u8), C.c_void_p(L.stream_ptr(cuda))))
    torch.cuda.synchronize()
    return out, u8


@pytest.mark.parametrize("name", list(SHAPES))
def test_uwm_jpeg_u8_equals_the_reference(cuda, name):
    D = _D()
    for shift in range(5):                                              # every image kind at every quality of the shape
        img, q, want = _case(name, shift)
        out, u8 = _abi_call(cuda, img, q)
        got = u8.cpu().numpy()
        diff = np.abs(got.astype(int) - want.astype(int))
        print(f"{name} shift {shift}: {int((diff != 0).sum())} bytes differ, largest {int(diff.max())}")
        assert np.array_equal(got, want), [(i, int(q[i]), int(diff[i].max())) for i in range(len(q)) if diff[i].any()]
        assert torch.equal(out.view(torch.int32), D.device_preprocess(u8, None, None, MEAN, STD).view(torch.int32))
        assert np.array_equal(out.cpu().numpy().view(np.int32), J.normalise(want, MEAN, STD).view(np.int32))
    # either output alone
    img, q, want = _case(name, 0)
    only_f, none = _abi_call(cuda, img, q, want_u8=False)
    assert none is None and torch.equal(only_f.view(torch.int32), out_bits(cuda, want))
    none, only_u8 = _abi_call(cuda, img, q, want_f=False)
    assert none is None and np.array_equal(only_u8.cpu().numpy(), want)


def out_bits(cuda, u8_np):
    return _D().device_preprocess(torch.from_numpy(u8_np).to(cuda), None, None, MEAN, STD).view(torch.int32)


def test_quality_zero_returns_the_input_bytes(cuda):
    D = _D()
    img = np.stack(list(J.sample_images(32, 48).values()))
    x = torch.from_numpy(img).to(cuda)
    out, u8 = D.device_jpeg(x, np.zeros(5, dtype=np.int32), MEAN, STD, return_u8=True)
    assert torch.equal(u8, x)
    assert torch.equal(out.view(torch.int32), D.device_preprocess(x, None, None, MEAN, STD).view(torch.int32))
    # and an image beside one that is compressed is untouched
    out, u8 = D.device_jpeg(x, [0, 30, 0, 100, 0], MEAN, STD, return_u8=True)
    assert np.array_equal(u8.cpu().numpy(), J.roundtrip_batch(img, [0, 30, 0, 100, 0]))
    assert torch.equal(u8[0::2], x[0::2]) and not torch.equal(u8[1], x[1])


def test_device_jpeg_refuses_on_the_device_too(cuda):
    D = _D()
    x = torch.zeros((2, 16, 16, 3), dtype=torch.uint8, device=cuda)
    with pytest.raises(ValueError, match="C must be 3"):
        D.device_jpeg(x[..., :1], [60, 0])
    with pytest.raises(ValueError, match="multiples of 16"):
        D.device_jpeg(torch.zeros((2, 24, 16, 3), dtype=torch.uint8, device=cuda), [60, 0])
    with pytest.raises(ValueError, match=r"1\.\.100"):
        D.device_jpeg(x, [60, 101])
    with pytest.raises(ValueError, match="int32"):
        D.device_jpeg(x, torch.zeros(2, dtype=torch.int64, device=cuda))
    assert D.device_jpeg(x, [60, 0]).shape == (2, 3, 16, 16)


def test_transparent_watermark_recipe_equals_the_numpy_chain(cuda):
    """DeviceInputPipeline('transparent_watermark').train_batch = augment_ref -> augment_ext_ref -> jpeg_ref -> Normalize"""
    D = _D()
    src = D.DeviceU8Dataset(D.SyntheticWatermarkDataset(8, 32, seed=3), cuda, MEAN, STD)
    pipe = D.DeviceInputPipeline(32, cuda, source=src, recipe="transparent_watermark", mean=MEAN, std=STD)
    x, m = pipe.train_batch(list(range(8)), torch.Generator().manual_seed(2))
    torch.cuda.synchronize()
    p, e, q = D.sample_transparent_recipe(8, 32, 32, torch.Generator().manual_seed(2))
    assert (q != 0).sum() >= 3 and (q == 0).any() and e["noise_sigma"].any() and e["blur"].any()      # the seed draws every late stage
    img, mask = src.images.cpu().numpy(), src.masks.cpu().numpy()
    want_u8, want_m = [], []
    for i in range(8):
        a, mm = A.augment_desc(img[i], mask[i], p[i])
        want_u8.append(J.roundtrip(R.ext_stages(a, e[i]), int(q[i])))
        want_m.append(mm)
    want_u8 = np.stack(want_u8)
    assert x.shape == (8, 3, 32, 32) and x.dtype == torch.float32 and m.dtype == torch.uint8
    assert np.array_equal(m.cpu().numpy(), np.stack(want_m))
    assert np.array_equal(x.cpu().numpy().view(np.int32), J.normalise(want_u8, MEAN, STD).view(np.int32))
    assert torch.equal(x.view(torch.int32), out_bits(cuda, want_u8))
    # the other recipes run as before: two values
    pipe2 = D.DeviceInputPipeline(32, cuda, source=src, recipe="enhanced", mean=MEAN, std=STD)
    assert len(pipe2.train_batch(list(range(8)), torch.Generator().manual_seed(2))) == 2


def test_one_captured_graph_serves_new_images_and_qualities(cuda):
    D = _D()
    a = _case("32x32", 0)
    b = _case("32x32", 3)
    b = (b[0][::-1].copy(), np.asarray([100, 0, 61, 33, 7], dtype=np.int32), None)
    x = torch.empty((5, 32, 32, 3), dtype=torch.uint8, device=cuda); qd = torch.empty(5, dtype=torch.int32, device=cuda)

    def load(c):
        x.copy_(torch.from_numpy(c[0])); qd.copy_(torch.from_numpy(c[1]))

    load(a)
    D.device_jpeg(x, qd, MEAN, STD)                                  # the first call allocates the workspace
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, u8 = D.device_jpeg(x, qd, MEAN, STD, return_u8=True)
    for c in (a, b, a):
        load(c)
        out.zero_(); u8.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got_f, got_u8 = out.clone(), u8.clone()
        eager_f, eager_u8 = D.device_jpeg(x, qd, MEAN, STD, return_u8=True)
        assert torch.equal(got_u8, eager_u8) and torch.equal(got_f.view(torch.int32), eager_f.view(torch.int32))
        assert np.array_equal(got_u8.cpu().numpy(), J.roundtrip_batch(c[0], c[1]))


def test_train_with_the_transparent_watermark_recipe(cuda, tmp_path, capsys):
    from unet_watermark_amd import cli
    args = ["train", "--synthetic", "16", "--epochs", "1", "--batch-size", "8", "--lr", "0.002", "--no-early-stopping", "--img-size", "64",
            "--encoder", "resnet18", "--model", "Unet", "--workers", "0", "--augment", "config",
            "--model-save-path", str(tmp_path / "t.pth"), "--checkpoint-dir", str(tmp_path / "ck")]
    hist = cli.main(args + ["--jpeg", "device"])
    said = capsys.readouterr().out
    assert "serving the 'transparent_watermark' recipe" in said and "ImageCompression" in said and "reflect" in said
    print("transparent_watermark:", hist[0]["train_loss"], hist[0]["val_loss"])
    assert len(hist) == 1 and np.isfinite(hist[0]["train_loss"]) and np.isfinite(hist[0]["val_loss"])
    with pytest.raises(ValueError, match="ImageCompression"):
        cli.main(args)
