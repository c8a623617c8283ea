"""Masks from watermarked / clean pairs on the device (csrc/pair_mask_u8.hip) against the numpy restatement (tests/pairmask_ref.py,
which carries the reference's closing blur + threshold that the kernel omits), and the input pipeline, `main.py masks` and
`main.py train` built on it.  All outputs are integers: every comparison is exact, no case is exempted."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairmask_ref as P  # noqa: E402
import resize_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

TILE_H, TILE_W = 32, 120                    # the kernel's tile (csrc/uwm_kernels.h: kPairMaskTileH, kPairMaskTileW)
# one-pixel sides, 3 x 3, rows that are not 4-byte aligned, one pixel past the tile in each dimension, and an image of 3 x 3 tiles
SIZES = [(1, 1), (1, 7), (7, 1), (3, 3), (37, 29), (TILE_H + 1, TILE_W + 1), (2 * TILE_H + 6, 2 * TILE_W + 10)]
FILL = 77


def _lib():
    from unet_watermark_amd import _lib as L
    return L, L.lib()


def _P(t):
    return C.c_void_p(t.data_ptr())


def _pack(imgs, rng, align=4):
    """images back to back at `align`-byte-aligned offsets with random bytes before, between and behind them (a kernel that reads a
    neighbour's bytes, or writes them, shows) -> (buffer, descs)"""
    from unet_watermark_amd.data import DESC_DTYPE
    descs = np.zeros(len(imgs), DESC_DTYPE)
    off = align * int(rng.integers(1, 8))
    for i, a in enumerate(imgs):
        descs[i] = (off, a.shape[0], a.shape[1])
        off = (off + a.size + align - 1) // align * align + align * int(rng.integers(1, 8))
    buf = rng.integers(0, 256, size=off, dtype=np.uint8)
    for a, d in zip(imgs, descs):
        buf[d["offset"]: d["offset"] + a.size] = a.reshape(-1)
    return buf, descs


def _run(dev, wm, wd, cl, cd, md, mask, thr, open_, mask_bytes=None):
    from unet_watermark_amd.data import descs_tensor
    L, lib = _lib()
    wm_t, cl_t = torch.from_numpy(wm).to(dev), torch.from_numpy(cl).to(dev)
    wd_t, cd_t, md_t = descs_tensor(wd, dev), descs_tensor(cd, dev), descs_tensor(md, dev)      # (alive until the launch has run)
    L.check(lib.uwm_pair_mask_u8(_P(wm_t), wm_t.numel(), _P(wd_t), _P(cl_t), cl_t.numel(), _P(cd_t), len(wd), 3, int(thr), int(open_), _P(mask),
                                 mask.numel() if mask_bytes is None else mask_bytes, _P(md_t), C.c_void_p(L.stream_ptr(dev))))
    torch.cuda.synchronize(dev)
    return mask.cpu().numpy()


def _mask_layout(shapes, rng):
    """mask descriptors at ANY alignment with gaps -> (descs, total bytes)"""
    return _pack([np.zeros((h, w, 1), np.uint8) for h, w in shapes], rng, align=1)[1::-1]


def _check(out, md, wants, what):
    covered = np.zeros(out.size, bool)
    for i, (d, want) in enumerate(zip(md, wants)):
        o, h, w = int(d["offset"]), int(d["h"]), int(d["w"])
        got = out[o: o + h * w].reshape(h, w)
        assert np.array_equal(got, want), (what, i, (h, w), np.argwhere(got != want)[:5].tolist())
        covered[o: o + h * w] = True
    assert (out[~covered] == FILL).all(), what               # nothing written before, between or behind the masks


_PAIRS = {}


def _random_pairs():
    """seeded random pairs of SIZES, the threshold at the median of their gray differences, and the restatement's masks (computed once)"""
    if not _PAIRS:
        rng = np.random.default_rng(21)
        wms = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]
        cls = [np.clip(a.astype(int) + rng.integers(-40, 41, a.shape), 0, 255).astype(np.uint8) for a in wms]
        thr = int(np.median(np.concatenate([P.diff_gray(a, b).ravel() for a, b in zip(wms, cls)])))
        _PAIRS.update(wms=wms, cls=cls, thr=thr,
                      want={o: [P.pair_mask(a, b, thr, open=bool(o)) for a, b in zip(wms, cls)] for o in (0, 1)})
    return _PAIRS


@pytest.mark.parametrize("open_", [0, 1])
def test_pair_mask_equals_the_restatement_on_a_ragged_batch(cuda, open_):
    p = _random_pairs()
    frac = np.mean(np.concatenate([m.ravel() for m in p["want"][0]]) > 0)
    assert 0.4 < frac < 0.6, frac                            # about half of the pixels are over the threshold
    assert 0.02 < np.mean(p["want"][1][-1] > 0) < frac       # the opening removes some and keeps some
    rng = np.random.default_rng(22)
    wm, wd = _pack(p["wms"], rng); cl, cd = _pack(p["cls"], rng)
    md, nbytes = _mask_layout(SIZES, rng)
    out = _run(cuda, wm, wd, cl, cd, md, torch.full((nbytes.size,), FILL, dtype=torch.uint8, device=cuda), p["thr"], open_)
    _check(out, md, p["want"][open_], f"open={open_}")


def _composite():
    """hand-computed structures at the corners of a 3 x 3-tile image and across its tile boundaries (rows 32 | 64, columns 120 | 240)
    -> (plane before, plane after the opening)"""
    h, w = 2 * TILE_H + 6, 2 * TILE_W + 10
    before, after = np.zeros((h, w), bool), np.zeros((h, w), bool)

    def put(y, x, case):
        b, a = case
        before[y:y + b.shape[0], x:x + b.shape[1]] |= b
        after[y:y + a.shape[0], x:x + a.shape[1]] |= a

    block3 = (np.ones((3, 3), bool), np.array(P.CROSS, bool))
    plus = (np.array(P.CROSS, bool), np.array(P.CROSS, bool))
    block2 = (np.ones((2, 2), bool), np.zeros((2, 2), bool))
    lone = (np.ones((1, 1), bool), np.zeros((1, 1), bool))
    put(TILE_H - 1, TILE_W - 1, block3)                       # a 3 x 3 block on the crossing of two tile boundaries -> a cross
    put(2 * TILE_H - 2, TILE_W + 20, block3)                  # ... two rows above the second row boundary, one below
    put(TILE_H - 1, 9, plus)                                  # a plus across a row boundary survives
    put(9, 2 * TILE_W - 1, plus)                              # ... and across a column boundary
    put(TILE_H - 1, 60, block2)                               # a 2 x 2 block across a row boundary vanishes
    put(50, TILE_W - 1, block2)                               # ... and across a column boundary
    put(20, 20, lone); put(TILE_H, 2 * TILE_W, lone)          # lone pixels, one the first pixel of a tile
    # 2 x 2 blocks in the four corners: the corner pixel and its two neighbours stay (the erosion ignores pixels outside the image)
    for y, x, gone in ((0, 0, (1, 1)), (0, w - 2, (1, 0)), (h - 2, 0, (0, 1)), (h - 2, w - 2, (0, 0))):
        a = np.ones((2, 2), bool); a[gone] = False
        put(y, x, (np.ones((2, 2), bool), a))
    # a strip two pixels thick along the bottom border, across a column boundary: the crosses centred on the border row fit except at
    # the two ends, so everything stays but the two upper end pixels
    strip = np.ones((2, 30), bool)
    kept = strip.copy(); kept[0, 0] = kept[0, -1] = False
    put(h - 2, TILE_W - 15, (strip, kept))
    return before, after


def test_pair_mask_on_hand_computed_cases(cuda):
    """every plane of pairmask_ref.hand_cases as an image of its own (structures at image corners and borders), and the composite
    image with structures across tile boundaries; the expected planes are the hand-computed ones AND the restatement's"""
    cases = [(b, a) for _, b, a in P.hand_cases()] + [_composite()]
    thr = 15
    pairs = [P.pair_from_plane(b, thr, seed=i) for i, (b, _) in enumerate(cases)]
    want = [np.where(a, 255, 0).astype(np.uint8) for _, a in cases]
    for (wm_i, cl_i), wnt in zip(pairs, want):
        assert np.array_equal(P.pair_mask(wm_i, cl_i, thr), wnt)
    rng = np.random.default_rng(23)
    wm, wd = _pack([p[0] for p in pairs], rng); cl, cd = _pack([p[1] for p in pairs], rng)
    md, nbytes = _mask_layout([b.shape for b, _ in cases], rng)
    out = _run(cuda, wm, wd, cl, cd, md, torch.full((nbytes.size,), FILL, dtype=torch.uint8, device=cuda), thr, 1)
    _check(out, md, want, "hand cases")
    out = _run(cuda, wm, wd, cl, cd, md, torch.full((nbytes.size,), FILL, dtype=torch.uint8, device=cuda), thr, 0)
    _check(out, md, [np.where(b, 255, 0).astype(np.uint8) for b, _ in cases], "hand cases, open=0")
    # the threshold is strict and gray is the 15-bit integer rule: one launch of two one-row images
    (r, g, b), gray, _ = P.GRAY_DISAGREE
    wms = [np.array([[[40 + gray, 40 + gray, 40 + gray], [40 + gray + 1] * 3]], np.uint8), np.array([[[r, g, b]]], np.uint8)]
    cls = [np.full((1, 2, 3), 40, np.uint8), np.zeros((1, 1, 3), np.uint8)]
    wm, wd = _pack(wms, rng); cl, cd = _pack(cls, rng)
    md, nbytes = _mask_layout([(1, 2), (1, 1)], rng)
    out = _run(cuda, wm, wd, cl, cd, md, torch.full((nbytes.size,), FILL, dtype=torch.uint8, device=cuda), gray, 0)
    _check(out, md, [np.array([[0, 255]], np.uint8), np.array([[0]], np.uint8)], "g == T, g == T + 1, the disagreeing triple")


def test_skipped_and_misfit_images_and_the_bytes_around_the_masks(cuda):
    """clean_descs[i].h == 0 keeps the pre-filled mask; a pair of different sizes, and descriptors that leave their buffers, zero it; a
    mask that does not fit mask_bytes is not written; nothing is written behind mask_bytes"""
    shapes = [(20, 30), (16, 16), (9, 13), (12, 40), (TILE_H + 3, 50), (8, 8), (10, 10)]
    rng = np.random.default_rng(24)
    wms = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    cls = [np.clip(a.astype(int) + rng.integers(-40, 41, a.shape), 0, 255).astype(np.uint8) for a in wms]
    cls[2] = rng.integers(0, 256, (13, 9, 3), dtype=np.uint8)                  # image 2: the clean image has another size
    thr = 18
    wm, wd = _pack(wms, rng); cl, cd = _pack(cls, rng)
    md, nbytes = _mask_layout(shapes, rng)
    cd[1]["h"] = 0                                                             # image 1: skipped
    wd[3]["h"] = 1 << 24                                                       # image 3: the watermarked descriptor leaves its buffer
    cd[5]["offset"] = -4                                                       # image 5: a negative offset
    guard = 64
    mask_bytes = int(md[6]["offset"]) + 50                                     # image 6: its mask ends behind mask_bytes
    out = _run(cuda, wm, wd, cl, cd, md, torch.full((nbytes.size + guard,), FILL, dtype=torch.uint8, device=cuda), thr, 1, mask_bytes=mask_bytes)
    zero = lambda i: np.zeros(shapes[i], np.uint8)      # noqa: E731
    keep = lambda i: np.full(shapes[i], FILL, np.uint8)      # noqa: E731
    want = [P.pair_mask(wms[0], cls[0], thr), keep(1), zero(2), zero(3), P.pair_mask(wms[4], cls[4], thr), zero(5), keep(6)]
    assert want[0].any() and want[4].any()
    _check(out, md, want, "skipped and misfit images")
    assert (out[mask_bytes:] == FILL).all()


# ------------------------------------------------------------------------------------------------ one captured launch, any sizes
def test_one_captured_launch_serves_batches_of_other_sizes(cuda):
    from unet_watermark_amd.data import DESC_DTYPE, descs_tensor
    L, lib = _lib()
    rng = np.random.default_rng(25)
    batches = []
    for shapes in ([(40, 50), (7, 9), (TILE_H + 1, TILE_W + 1)], [(1, 1), (70, 130), (33, 31)]):
        wms = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
        cls = [np.clip(a.astype(int) + rng.integers(-40, 41, a.shape), 0, 255).astype(np.uint8) for a in wms]
        batches.append((shapes, _pack(wms, rng), _pack(cls, rng), _mask_layout(shapes, rng), [P.pair_mask(a, b, 20) for a, b in zip(wms, cls)]))
    size = lambda k: max(b[k][0].size for b in batches)      # noqa: E731
    wm_t = torch.zeros(size(1), dtype=torch.uint8, device=cuda); cl_t = torch.zeros(size(2), dtype=torch.uint8, device=cuda)
    mask = torch.zeros(max(b[3][1].size for b in batches), dtype=torch.uint8, device=cuda)
    descs = torch.zeros(3 * 3 * DESC_DTYPE.itemsize, dtype=torch.uint8, device=cuda)
    step = 3 * DESC_DTYPE.itemsize

    def call():
        L.check(lib.uwm_pair_mask_u8(_P(wm_t), wm_t.numel(), C.c_void_p(descs.data_ptr()), _P(cl_t), cl_t.numel(), C.c_void_p(descs.data_ptr() + step),
                                     3, 3, 20, 1, _P(mask), mask.numel(), C.c_void_p(descs.data_ptr() + 2 * step), C.c_void_p(L.stream_ptr(cuda))))

    def load(b):
        _, (wm, wd), (cl, cd), (md, _), _ = b
        wm_t[:wm.size].copy_(torch.from_numpy(wm)); cl_t[:cl.size].copy_(torch.from_numpy(cl))
        descs.copy_(descs_tensor(np.concatenate([wd, cd, md])))
        mask.fill_(FILL)

    load(batches[0])
    call()                                                   # eager, and the warm-up of the capture
    torch.cuda.synchronize()
    _check(mask.cpu().numpy(), batches[0][3][0], batches[0][4], "eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for k in (1, 0):
        load(batches[k])
        graph.replay()
        torch.cuda.synchronize()
        _check(mask.cpu().numpy(), batches[k][3][0], batches[k][4], f"replay on batch {k}")


# ------------------------------------------------------------------------------------------------ the input pipeline and the CLI
def _save(path, arr):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path)


def _scene(rng, h, w, i):
    """a smooth clean image and its watermarked version: a rectangle blended towards white, plus a few specks that the opening removes"""
    from PIL import Image
    base = rng.integers(0, 256, size=(h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8)
    clean = np.asarray(Image.fromarray(base).resize((w, h), Image.BILINEAR)).copy()
    wm = clean.copy()
    y0, x0 = h // 4 + i % 3, w // 5 + i % 4
    reg = wm[y0: y0 + h // 3, x0: x0 + w // 2].astype(int)
    wm[y0: y0 + h // 3, x0: x0 + w // 2] = (reg * 5 // 10 + 120).astype(np.uint8)
    for _ in range(6):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        wm[y, x] = 255 - wm[y, x]
    return wm, clean


def _mixed_dataset(root, rng):
    """six images: 0 a file mask (and a clean image that must not be used), 1 and 4 generated masks, 2 a clean image of another size,
    3 neither, 5 a file mask only -> per image (wm, the mask the reference would use)"""
    from PIL import Image
    thr, out = 15, []
    for i, (h, w) in enumerate([(48, 64), (50, 70), (61, 45), (33, 47), (TILE_H + 8, TILE_W + 9), (40, 40)]):
        wm, clean = _scene(rng, h, w, i)
        _save(f"{root}/watermarked/im{i}.png", wm)
        if i in (0, 5):
            m = np.where(rng.random((h, w)) < 0.3, 255, 0).astype(np.uint8)
            _save(f"{root}/masks/im{i}.png", m)
        if i == 2:
            clean = np.asarray(Image.fromarray(clean).resize((w // 2 + 3, h // 2 + 5), Image.BILINEAR)).copy()
        if i in (0, 1, 2, 4):
            _save(f"{root}/clean/im{i}.png", clean)
        out.append((wm, m if i in (0, 5) else P.pair_mask(wm, clean, thr) if i in (1, 2, 4) else np.zeros((h, w), np.uint8)))
    return thr, out


def test_pipeline_derives_the_missing_masks(cuda, tmp_path):
    """to_u8 on a dataset that mixes a file mask, generated masks, a clean image of another size and an image with neither = the
    restatement at the image's own size, then the nearest resize"""
    from unet_watermark_amd.data import DeviceInputPipeline, RawPairDataset
    root = str(tmp_path / "d")
    thr, want = _mixed_dataset(root, np.random.default_rng(26))
    assert all(want[i][1].any() and not want[i][1].all() for i in (1, 2, 4))
    ds = RawPairDataset([root], thr)
    assert ds.missing_masks() == [1, 2, 3, 4]
    pipe = DeviceInputPipeline(32, cuda, source=ds)
    for order in ([0, 1, 2, 3, 4, 5], [3, 2], [5, 0], [4]):                    # a batch without a clean image takes no pair launch
        x, m = pipe.to_u8([ds[i] for i in order])
        assert x.shape == (len(order), 32, 32, 3) and m.shape == (len(order), 32, 32) and m.dtype == torch.uint8
        for k, i in enumerate(order):
            assert np.array_equal(m[k].cpu().numpy(), R.resize_u8_nearest(want[i][1], 32, 32)), (order, i)
            assert np.array_equal(x[k].cpu().numpy(), R.resize_u8_linear(want[i][0], 32, 32)), (order, i)
    xv, mv = pipe.val_batch([ds[i] for i in (1, 2)])
    assert xv.shape == (2, 3, 32, 32) and set(mv.unique().tolist()) <= {0, 1}
    assert np.array_equal(mv[0].cpu().numpy() * 255, R.resize_u8_nearest(want[1][1], 32, 32))


def test_pair_dataset_with_every_mask_present_equals_the_folder_dataset(cuda, tmp_path):
    from unet_watermark_amd.data import DeviceInputPipeline, RawFolderDataset, RawPairDataset
    root = str(tmp_path / "d")
    rng = np.random.default_rng(27)
    for i, (h, w) in enumerate([(48, 64), (50, 70), (33, 47)]):
        wm, clean = _scene(rng, h, w, i)
        _save(f"{root}/watermarked/im{i}.png", wm); _save(f"{root}/clean/im{i}.png", clean)
        _save(f"{root}/masks/im{i}.png", np.where(rng.random((h, w)) < 0.4, 255, 0).astype(np.uint8))
    pair, folder = RawPairDataset([root], 15), RawFolderDataset(root)
    assert pair.missing_masks() == [] and [os.path.basename(p) for p in pair.files] == folder.files
    a = DeviceInputPipeline(32, cuda, source=pair).to_u8([pair[i] for i in range(3)])
    b = DeviceInputPipeline(32, cuda, source=folder).to_u8([folder[i] for i in range(3)])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and bool(a[1].any())


def test_main_masks_writes_the_restatements_pngs(cuda, tmp_path, capsys):
    from PIL import Image
    from unet_watermark_amd import cli
    root = str(tmp_path / "d")
    thr, want = _mixed_dataset(root, np.random.default_rng(28))
    before = {f: open(f"{root}/masks/{f}", "rb").read() for f in os.listdir(f"{root}/masks")}
    res = cli.main(["masks", "--data-dir", root, "--threshold", str(thr), "--batch-size", "2"])
    assert (res["written"], res["skipped"], res["no_clean"]) == (3, 2, 1)
    assert "wrote 3 masks" in capsys.readouterr().out
    assert sorted(os.listdir(f"{root}/masks")) == [f"im{i}.png" for i in (0, 1, 2, 4, 5)]
    for i in (1, 2, 4):
        got = np.asarray(Image.open(f"{root}/masks/im{i}.png"))
        assert got.dtype == np.uint8 and np.array_equal(got, want[i][1]), i
    for f, data in before.items():                                             # existing masks are left alone
        assert open(f"{root}/masks/{f}", "rb").read() == data
    res = cli.main(["masks", "--data-dir", root, "--threshold", str(thr)])     # a second run has nothing to write
    assert (res["written"], res["skipped"], res["no_clean"]) == (0, 5, 1)


def test_train_on_a_pair_dataset_without_masks(cuda, tmp_path, capsys):
    from unet_watermark_amd import cli
    root = str(tmp_path / "d")
    rng = np.random.default_rng(29)
    for i, (h, w) in enumerate([(64, 64), (50, 70), (90, 61), (64, 96), (33, 47), (128, 128), (71, 71), (40, 100)]):
        wm, clean = _scene(rng, h, w, i)
        _save(f"{root}/watermarked/im{i}.png", wm); _save(f"{root}/clean/im{i}.png", clean)
    hist = cli.main(["train", "--data-dir", root, "--synthetic", "0", "--augment", "basic", "--epochs", "1", "--batch-size", "2", "--lr", "0.002",
                     "--no-early-stopping", "--img-size", "64", "--encoder", "resnet18", "--model", "Unet", "--workers", "0",
                     "--model-save-path", str(tmp_path / "m.pth"), "--checkpoint-dir", str(tmp_path / "ck")])
    assert "8 of 8 images have no mask file" in capsys.readouterr().out
    assert len(hist) == 1 and np.isfinite(hist[0]["train_loss"]) and np.isfinite(hist[0]["val_loss"])
    assert not os.path.exists(f"{root}/masks")                                 # training writes nothing
