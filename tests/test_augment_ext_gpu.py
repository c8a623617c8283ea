"""The enhanced recipe's stages on the device (csrc/augment_ext_u8.hip) against the numpy restatement of their rule
(tests/augment_ext_ref.py) behind the basic stages' (tests/augment_ref.py), and the training path built on them (`main.py train
--augment config --augmentation-type enhanced`).  Every comparison is bit-equal: there is no tolerance and no case is exempted."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ext_ref as R  # noqa: E402
import augment_ref as A  # noqa: E402
import test_augment_gpu as G  # noqa: E402   the batches, flag words and affine maps of the basic stages' test

pytestmark = pytest.mark.gpu

MEAN, STD = G.MEAN, G.STD
# (H, W, C, flag words): the smallest shapes where each part can go wrong
SHAPES = {
    "32x32x3": (32, 32, 3, list(range(16))),               # tiles 4 x 4, every flag word
    "20x36x3": (20, 36, 3, [0, 1, 2, 3, 1, 2, 3]),         # padded to 24 x 40, tiles 3 x 5
    "64x48x1": (64, 48, 1, [0, 3, 1, 2, 0, 1, 3]),         # grey CLAHE, tiles 8 x 6
    "8x8x3": (8, 8, 3, [0, 5, 10, 15, 6, 9, 3]),           # one-pixel tiles
    "5x300x4": (5, 300, 4, [3, 1, 0, 2, 1, 3, 2]),         # four channels, more than one 256-lane stride
    "1x7x1": (1, 7, 1, [0, 1, 2, 3, 1, 0, 2]),             # reflect-101 at n = 1
}
SINGLE = ("clahe", "gamma", "noise", "motion", "gauss")
MODES = SINGLE + ("all", "mixed")
_STAGED = {}


def _D():
    from unet_watermark_amd import data
    return data


def _motion_kernels():
    D = _D()
    pts = [(x, y) for y in range(3) for x in range(3)]
    seen = {}
    for a in pts:
        for b in pts:
            if a != b:
                seen.setdefault(bytes(D.motion_kernel(a, b)), D.motion_kernel(a, b))
    return list(seen.values())


def _clahe_ok(h, w, c):
    return c in (1, 3) and h >= 8 and w >= 8


def _staged(name):
    """(images, masks, basic descriptors, staged uint8 images of the basic stages, expected masks): computed once per shape"""
    if name not in _STAGED:
        h, w, c, flag_list = SHAPES[name]
        img, mask = G._batch(len(flag_list), h, w, c, seed=len(name) + h)
        p = G._descs(h, w, flag_list, c)
        want = [A.augment_desc(img[i], mask[i], p[i]) for i in range(len(flag_list))]
        _STAGED[name] = (img, mask, p, np.stack([a for a, _ in want]), np.stack([m for _, m in want]))
    return _STAGED[name]


def _ext(name, mode):
    """one ext descriptor per image, all different; image 0 draws nothing.  clahe_clip cycles 1, 3, tileArea; the motion kernels
    cycle through all of them; sigma covers the recipe's range and the clamp."""
    D = _D()
    h, w, c, flag_list = SHAPES[name]
    n = len(flag_list)
    e = D.identity_aug_ext_params(n)
    kernels = _motion_kernels()
    area = ((h + 7) // 8) * ((w + 7) // 8)
    for i in range(1, n):
        m = mode if mode != "mixed" else (SINGLE + ("all",))[(i - 1) % 6]
        if m == "clahe" and not _clahe_ok(h, w, c):
            m = "gamma"
        tone = m in ("clahe", "gamma", "all")
        if tone and (m == "clahe" or (m == "all" and _clahe_ok(h, w, c) and i % 2)):
            e["tone"][i] = D.TONE_CLAHE
            e["clahe_clip"][i] = (1, 3, area)[i % 3]
        elif tone:
            e["tone"][i] = D.TONE_TABLE
            e["lut2"][i] = D.gamma_lut((0.8, 1.2, 0.93)[i % 3])
        if m in ("noise", "all"):
            e["noise_sigma"][i] = (573, 1402, 16383, 1000)[i % 4]
            e["seed"][i] = (0x9E3779B97F4A7C15 * (i + 1) + len(name)) & 0xFFFFFFFFFFFFFFFF
        if m == "motion" or (m == "all" and i % 2 == 0):
            e["blur"][i] = D.BLUR_MOTION
            e["blur_w"][i] = kernels[(i * 7 + len(name)) % len(kernels)]
        elif m in ("gauss", "all"):
            e["blur"][i] = D.BLUR_GAUSS
    return e


def _compare(cuda, img, mask, p, e, staged, want_m, tag):
    D = _D()
    c = img.shape[3]
    want = np.stack([staged[i] if e is None else R.ext_stages(staged[i], e[i]) for i in range(len(p))])
    x, m = torch.from_numpy(img).to(cuda), torch.from_numpy(mask).to(cuda)
    out, mo, u8 = D.device_augment(x, m, p, MEAN, STD, return_u8=True, ext=e)
    got = u8.cpu().numpy()
    for i in range(len(p)):
        diff = int(np.abs(got[i].astype(int) - want[i]).max())
        changed = int((want[i] != staged[i]).sum())
        print(tag, "image", i, "tone", None if e is None else int(e["tone"][i]), "max |diff|", diff, "bytes the stages changed", changed)
        assert np.array_equal(got[i], want[i]), (tag, i, diff)
    assert np.array_equal(mo.cpu().numpy(), want_m)
    norm = D.device_preprocess(u8, None, None, MEAN, STD)
    assert out.shape == (len(p), c, img.shape[1], img.shape[2]) and torch.equal(out.view(torch.int32), norm.view(torch.int32))
    # masks are the basic path's; without masks / without the uint8 copy the same values
    basic = D.device_augment(x, m, p, MEAN, STD)
    assert torch.equal(mo, basic[1])
    only = D.device_augment(x, None, p, MEAN, STD, ext=e)
    assert isinstance(only, torch.Tensor) and torch.equal(only.view(torch.int32), out.view(torch.int32))
    return want


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_ext_stages_equal_the_restatement(cuda, name, mode):
    h, w, c, _ = SHAPES[name]
    if mode == "clahe" and not _clahe_ok(h, w, c):
        with pytest.raises(ValueError, match="CLAHE needs"):         # the host refuses; nothing is launched
            e = _D().identity_aug_ext_params(len(SHAPES[name][3])); e["tone"][1] = 1
            img, mask, p, _, _ = _staged(name)
            _D().device_augment(torch.from_numpy(img).to(cuda), None, p, MEAN, STD, ext=e)
        return
    img, mask, p, staged, want_m = _staged(name)
    e = _ext(name, mode)
    want = _compare(cuda, img, mask, p, e, staged, want_m, f"{name}/{mode}")
    assert np.array_equal(want[0], staged[0])                         # image 0 draws nothing
    # (a stage may leave an image as it is: the val = -255 descriptor makes a black image, which gamma keeps)
    assert sum(bool((want[i] != staged[i]).any()) for i in range(1, len(p))) >= (len(p) - 1) // 2, "the drawn stages change their images"


def test_every_motion_kernel_and_a_gaussian_on_one_row(cuda):
    D = _D()
    kernels = _motion_kernels()
    n = len(kernels)
    rng = np.random.default_rng(3)
    for h, w in ((9, 11), (1, 7)):
        img = rng.integers(0, 256, size=(n + 1, h, w, 3), dtype=np.uint8)
        mask = rng.integers(0, 256, size=(n + 1, h, w), dtype=np.uint8)
        p = D.identity_aug_params(n + 1)
        e = D.identity_aug_ext_params(n + 1)
        e["blur"][:n] = D.BLUR_MOTION
        e["blur_w"][:n] = np.stack(kernels)
        e["blur"][n] = D.BLUR_GAUSS
        e["noise_sigma"][::2] = 1402
        e["seed"] = np.arange(n + 1, dtype=np.uint64) * np.uint64(977) + np.uint64(5)
        _compare(cuda, img, mask, p, e, img, (mask > 127).astype(np.uint8), f"motion {h}x{w}")


def test_no_ext_and_identity_ext_equal_uwm_augment_u8(cuda):
    """ext = NULL through the ABI (no workspace), ext = None and identity descriptors through device_augment: uwm_augment_u8's bits"""
    D = _D()
    from unet_watermark_amd import _lib as L
    for name in ("32x32x3", "5x300x4"):
        img, mask, p, staged, want_m = _staged(name)
        n, h, w, c = img.shape
        x, m = torch.from_numpy(img).to(cuda), torch.from_numpy(mask).to(cuda)
        out, mo, u8 = D.device_augment(x, m, p, MEAN, STD, return_u8=True)
        assert np.array_equal(u8.cpu().numpy(), staged)
        for ext in (None, D.identity_aug_ext_params(n)):
            o2, m2, u2 = D.device_augment(x, m, p, MEAN, STD, return_u8=True, ext=ext)
            assert torch.equal(o2.view(torch.int32), out.view(torch.int32)) and torch.equal(m2, mo) and torch.equal(u2, u8)
        dd = torch.from_numpy(p.view(np.uint8).reshape(-1).copy()).to(cuda)
        o3, m3, u3 = torch.empty_like(out), torch.empty_like(mo), torch.empty_like(u8)
        mean_c = (C.c_float * c)(*MEAN[:c]); std_c = (C.c_float * c)(*STD[:c])
        ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
        L.check(L.lib().uwm_augment_ext_u8(ptr(x), ptr(m), ptr(dd), None, n, h, w, c, mean_c, std_c, 127, None, 0, ptr(o3), ptr(m3), ptr(u3),
                                           C.c_void_p(L.stream_ptr(cuda))))
        assert torch.equal(o3.view(torch.int32), out.view(torch.int32)) and torch.equal(m3, mo) and torch.equal(u3, u8)


def test_sampled_enhanced_parameters_run_through_the_kernels(cuda):
    """what `--augment config` feeds the kernels for the enhanced recipe: a sampled batch equals the restatement as well"""
    D = _D()
    img, mask = G._batch(24, 32, 32, 3, seed=22)
    p, e = D.sample_aug_recipe(24, 32, 32, torch.Generator().manual_seed(5), "enhanced")
    assert (e["tone"] == 1).any() and (e["tone"] == 2).any() and e["noise_sigma"].any() and e["blur"].any()
    want = [A.augment_desc(img[i], mask[i], p[i]) for i in range(24)]
    _compare(cuda, img, mask, p, e, np.stack([a for a, _ in want]), np.stack([m for _, m in want]), "sampled")


def test_one_captured_graph_serves_a_second_batch_of_descriptors(cuda):
    D = _D()
    from unet_watermark_amd import _lib as L
    name = "32x32x3"
    img, mask, p, staged, want_m = _staged(name)
    n, h, w, c = img.shape
    batches = [(img, mask, p, _ext(name, "mixed"), staged, want_m)]
    img2, mask2 = G._batch(n, h, w, c, seed=77)
    p2 = p[::-1].copy()
    want2 = [A.augment_desc(img2[i], mask2[i], p2[i]) for i in range(n)]
    batches.append((img2, mask2, p2, _ext(name, "all")[::-1].copy(), np.stack([a for a, _ in want2]), np.stack([m for _, m in want2])))
    x = torch.empty((n, h, w, c), dtype=torch.uint8, device=cuda); m = torch.empty((n, h, w), dtype=torch.uint8, device=cuda)
    dd = torch.empty(n * D.AUG_DESC_DTYPE.itemsize, dtype=torch.uint8, device=cuda)
    ed = torch.empty(n * D.AUG_EXT_DTYPE.itemsize, dtype=torch.uint8, device=cuda)
    ws = torch.empty(int(L.lib().uwm_augment_ext_workspace_bytes(n, h, w, c)), dtype=torch.uint8, device=cuda)
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=cuda); mo = torch.empty_like(m); u8 = torch.empty_like(x)
    mean_c = (C.c_float * c)(*MEAN[:c]); std_c = (C.c_float * c)(*STD[:c])
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

    def call():
        L.check(L.lib().uwm_augment_ext_u8(ptr(x), ptr(m), ptr(dd), ptr(ed), n, h, w, c, mean_c, std_c, 127, ptr(ws), ws.numel(), ptr(out),
                                           ptr(mo), ptr(u8), C.c_void_p(L.stream_ptr(cuda))))

    def load(b):
        x.copy_(torch.from_numpy(b[0])); m.copy_(torch.from_numpy(b[1]))
        dd.copy_(torch.from_numpy(b[2].view(np.uint8).reshape(-1).copy())); ed.copy_(torch.from_numpy(b[3].view(np.uint8).reshape(-1).copy()))

    load(batches[0])
    call()                                                           # the first call on a device uploads the tables: not capturable
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for b in batches:
        load(b)
        out.zero_(); mo.zero_(); u8.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want = np.stack([R.ext_stages(b[4][i], b[3][i]) for i in range(n)])
        assert np.array_equal(u8.cpu().numpy(), want) and np.array_equal(mo.cpu().numpy(), b[5])
        assert torch.equal(out.view(torch.int32), D.device_preprocess(u8, None, None, MEAN, STD).view(torch.int32))


# ------------------------------------------------------------------------------------- main.py train --augment config
def _train(root, tmp, tag, aug_type):
    from unet_watermark_amd import cli
    return cli.main(["train", "--data-dir", str(root), "--epochs", "1", "--batch-size", "2", "--lr", "0.002", "--no-early-stopping",
                     "--img-size", "64", "--encoder", "resnet18", "--model", "Unet", "--workers", "0", "--augment", "config",
                     "--augmentation-type", aug_type, "--model-save-path", str(tmp / f"{tag}.pth"), "--checkpoint-dir", str(tmp / f"ck_{tag}")])


def test_train_with_the_enhanced_recipe_on_a_folder_of_mixed_sizes(cuda, tmp_path, capsys):
    root = tmp_path / "data"
    G._write_folder(root)
    a = _train(root, tmp_path, "a", "enhanced")
    assert "serving the 'enhanced' recipe" in capsys.readouterr().out
    b = _train(root, tmp_path, "b", "enhanced")
    assert len(a) == 1 and np.isfinite(a[0]["train_loss"]) and np.isfinite(a[0]["val_loss"])
    print("enhanced:", a[0]["train_loss"], a[0]["val_loss"], "rerun:", b[0]["train_loss"], b[0]["val_loss"])
    assert a[0]["train_loss"] == b[0]["train_loss"] and a[0]["val_loss"] == b[0]["val_loss"]
    basic = _train(root, tmp_path, "c", "basic")
    assert "serving the 'basic' recipe" in capsys.readouterr().out
    print("basic through --augment config:", basic[0]["train_loss"])
    assert np.isfinite(basic[0]["train_loss"]) and basic[0]["train_loss"] != a[0]["train_loss"]
    from unet_watermark_amd import cli
    with pytest.raises(ValueError, match="ImageCompression"):
        _train(root, tmp_path, "d", "transparent_watermark")
    assert cli.build_parser().parse_args(["train", "--augment", "basic"]).augment == "basic"


# ------------------------------------------------------------------------------------- the wrappers' shared per-device workspaces
def test_workspaces_grow_and_are_reused_without_changing_a_result(cuda):
    """CLAHE on 2 x 16x16x3, on 3 x 32x48x3 (its workspace has to grow), a JPEG round trip on 2 x 16x16x3 and the first call again, one
    after the other through the public wrappers: the fourth result is the first, and every result is what the same call gives when
    no workspace exists yet.  The smallest shapes the kernels take: CLAHE needs H, W >= 8, JPEG multiples of 16."""
    D = _D()

    def clear():
        D._EXT_WORKSPACE.clear(); D._JPEG_WORKSPACE.clear()

    def clahe(n, h, w):
        img, mask = G._batch(n, h, w, 3, seed=n + h)
        x, m = torch.from_numpy(img).to(cuda), torch.from_numpy(mask).to(cuda)
        e = D.identity_aug_ext_params(n)
        e["tone"], e["clahe_clip"] = D.TONE_CLAHE, 2
        return lambda: D.device_augment(x, m, D.identity_aug_params(n), MEAN, STD, return_u8=True, ext=e)

    def jpeg(n, h, w):
        x = torch.from_numpy(G._batch(n, h, w, 3, seed=5)[0]).to(cuda)
        return lambda: D.device_jpeg(x, np.array([35, 90][:n], dtype=np.int32), MEAN, STD, return_u8=True)

    def run(call):
        res = call()
        torch.cuda.synchronize()
        return [t.cpu().numpy().view(np.uint8) for t in res]      # bytes, so fp32 results compare bit for bit

    first = clahe(2, 16, 16)
    calls = [first, clahe(3, 32, 48), jpeg(2, 16, 16), first]
    clear()
    got = [run(c) for c in calls]
    assert all(np.array_equal(a, b) for a, b in zip(got[3], got[0]))
    assert not np.array_equal(got[0][2], G._batch(2, 16, 16, 3, seed=18)[0])      # (CLAHE did change the images)
    for c, g in zip(calls, got):
        clear()
        fresh = run(c)
        assert len(fresh) == len(g) and all(np.array_equal(a, b) for a, b in zip(fresh, g))
