"""Masks from watermarked / clean pairs, the part that needs no device: self-checks of the numpy restatement (tests/pairmask_ref.py)
that the device kernel is compared with, RawPairDataset's file lookup, the argument checks of uwm_pair_mask_u8, which fail before any
launch, and the refusal of --use-blurred-mask on a pair dataset.  Every comparison is exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maskpost_ref as M  # noqa: E402
import pairmask_ref as P  # noqa: E402


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from unet_watermark_amd import _lib
    _lib.lib()
    return _lib


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("name,before,after", P.hand_cases(), ids=[c[0] for c in P.hand_cases()])
def test_restatement_on_hand_computed_planes(name, before, after):
    """the opening of each plane, worked out by hand in pairmask_ref.hand_cases, through the whole rule (pair -> difference -> gray ->
    threshold -> opening -> blur + threshold), at two thresholds"""
    for T in (15, 0):
        wm, clean = P.pair_from_plane(before, T, seed=3)
        assert np.array_equal(P.pair_mask(wm, clean, T, open=False) > 0, before), name      # the pair encodes the plane
        assert np.array_equal(P.pair_mask(wm, clean, T) > 0, after), name
        assert np.array_equal(P.pair_mask(wm, clean, T, blur=False) > 0, after), name


def test_the_element_is_a_cross():
    assert P.CROSS.tolist() == [[0, 1, 0], [1, 1, 1], [0, 1, 0]]


def test_threshold_is_strict():
    """g == T gives 0 and g == T + 1 gives 255 (cv2.THRESH_BINARY: src > thresh)"""
    clean = np.full((1, 2, 3), 40, np.uint8)
    wm = clean.copy()
    wm[0, 0] += 15; wm[0, 1] += 16                                   # equal channel differences d give g = d
    assert P.diff_gray(wm, clean).tolist() == [[15, 16]]
    assert P.pair_mask(wm, clean, 15, open=False).tolist() == [[0, 255]]
    assert P.pair_mask(clean, wm, 15, open=False).tolist() == [[0, 255]]      # absdiff: either direction
    assert P.pair_mask(wm, clean, 16, open=False).tolist() == [[0, 0]]
    assert P.pair_mask(wm, clean, 14, open=False).tolist() == [[255, 255]]


def test_gray_is_the_15_bit_integer_rule_not_rounded_float():
    (r, g, b), want, float_says = P.GRAY_DISAGREE
    wm = np.array([[[r, g, b]]], np.uint8); clean = np.zeros((1, 1, 3), np.uint8)
    assert (r * 9798 + g * 19235 + b * 3735 + 16384) >> 15 == want == int(P.diff_gray(wm, clean)[0, 0])
    assert int(np.rint(0.299 * r + 0.587 * g + 0.114 * b)) == float_says != want
    assert P.pair_mask(wm, clean, want, open=False)[0, 0] == 0           # the float value would pass this threshold
    assert 9798 + 19235 + 3735 == 1 << 15
    white = np.full((1, 1, 3), 255, np.uint8)
    assert int(P.diff_gray(white, clean)[0, 0]) == 255


def test_blur_and_threshold_is_the_identity_on_binary_images():
    """step 6 of the rule on 200 seeded random {0,255} images of mixed sizes and densities"""
    k = P.gaussian_kernel_3()
    assert abs(k.sum() - 1) < 1e-15 and round(255 * k[1] ** 2) == 158 and round(255 * (1 - k[1] ** 2)) == 97      # a lone 255 / a 0 among eight 255s
    rng = np.random.default_rng(11)
    for i in range(200):
        h, w = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        m = np.where(rng.random((h, w)) < rng.random(), 255, 0).astype(np.uint8)
        assert np.array_equal(P.blur_threshold(m), m), (i, h, w)


def test_a_clean_image_of_another_size_is_resized_first():
    import resize_ref as R
    rng = np.random.default_rng(5)
    wm = rng.integers(0, 256, (20, 31, 3), dtype=np.uint8); clean = rng.integers(0, 256, (13, 17, 3), dtype=np.uint8)
    assert np.array_equal(P.pair_mask(wm, clean, 30), P.pair_mask(wm, R.resize_u8_linear(clean, 20, 31), 30))
    assert np.array_equal(P.pair_mask(wm, clean, 30, blur=False) > 0, M.opening(P.diff_gray(wm, R.resize_u8_linear(clean, 20, 31)) > 30, P.CROSS))


# ------------------------------------------------------------------------------------------------ RawPairDataset
def _png(path, arr):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path)


def _img(v, h=6, w=5):
    return np.full((h, w, 3), v, np.uint8)


def test_raw_pair_dataset_lists_every_root_and_looks_masks_up_before_clean_images(tmp_path, L):
    from unet_watermark_amd.data import RawPairDataset
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _png(f"{a}/watermarked/x1.png", _img(10)); _png(f"{a}/watermarked/x2.png", _img(20)); _png(f"{a}/watermarked/x4.png", _img(40))
    _png(f"{b}/watermarked/x0.png", _img(5)); _png(f"{b}/watermarked/x3.bmp", _img(30))
    with open(f"{a}/watermarked/notes.txt", "w") as f:
        f.write("not an image")
    _png(f"{b}/masks/x1.png", np.full((6, 5), 255, np.uint8))            # x1 (root a): its mask lives in root b
    _png(f"{a}/masks/x0.png", np.full((6, 5), 7, np.uint8))              # x0 (root b): masks in both roots, the first root wins
    _png(f"{b}/masks/x0.png", np.full((6, 5), 9, np.uint8))
    _png(f"{a}/clean/x1.png", _img(11))                                  # never read: x1 has a mask
    _png(f"{b}/clean/x2.png", _img(22, 3, 4))                            # x2: no mask, clean image (of another size) in root b
    _png(f"{a}/clean/x3.bmp", _img(33)); _png(f"{b}/clean/x3.bmp", _img(34))      # x3: clean by the SAME file name, the first root wins
    _png(f"{a}/clean/x4.jpg", _img(44))                                  # x4: another extension is another name -> neither
    ds = RawPairDataset([a, b], 15)
    assert ds.files == sorted([f"{a}/watermarked/x1.png", f"{a}/watermarked/x2.png", f"{a}/watermarked/x4.png", f"{b}/watermarked/x0.png",
                               f"{b}/watermarked/x3.bmp"])                # sorted by path: root a's files first
    assert [os.path.basename(p) for p in ds.files] == ["x1.png", "x2.png", "x4.png", "x0.png", "x3.bmp"]
    assert ds.missing_masks() == [1, 2, 4] and ds.mask_threshold == 15 and len(ds) == 5
    img, m, c = ds[0]
    assert img.shape == (6, 5, 3) and img[0, 0, 0] == 10 and m.shape == (6, 5) and m[0, 0] == 255 and c is None
    img, m, c = ds[1]
    assert img[0, 0, 0] == 20 and m is None and c.shape == (3, 4, 3) and c[0, 0, 0] == 22
    img, m, c = ds[2]
    assert img[0, 0, 0] == 40 and m is None and c is None
    img, m, c = ds[3]
    assert img[0, 0, 0] == 5 and m[0, 0] == 7 and c is None
    img, m, c = ds[4]
    assert img[0, 0, 0] == 30 and m is None and c[0, 0, 0] == 33
    with open(f"{a}/masks/x0.png", "wb") as f:                            # an unreadable mask file: the next directory is tried
        f.write(b"broken")
    assert ds[3][1][0, 0] == 9
    one = RawPairDataset(b, 10)                                           # a single root as a string
    assert [os.path.basename(p) for p in one.files] == ["x0.png", "x3.bmp"] and one.missing_masks() == [1]
    with pytest.raises(ValueError, match="0..255"):
        RawPairDataset([a], 256)


def test_cli_picks_the_pair_dataset_only_where_the_data_needs_it(tmp_path, L):
    from unet_watermark_amd import cli
    from unet_watermark_amd.config import get_cfg_defaults
    from unet_watermark_amd.data import RawFolderDataset, RawPairDataset
    root, extra = str(tmp_path / "d"), str(tmp_path / "e")
    for i in range(3):
        _png(f"{root}/watermarked/i{i}.png", _img(10 * i)); _png(f"{root}/masks/i{i}.png", np.zeros((6, 5), np.uint8))
    _png(f"{extra}/watermarked/j.png", _img(1))
    cfg = get_cfg_defaults(); cfg.DATA.ROOT_DIR = root; cfg.DATA.GENERATE_MASK_THRESHOLD = 12
    assert cli._pair_dataset(cfg) is None                                 # every mask is a file: the folder dataset, as before
    tr, _ = cli._datasets(cfg, 0, "cuda")
    assert isinstance(tr.dataset, RawFolderDataset)
    cfg.DATA.ADDITIONAL_ROOT_DIRS = [extra]
    tr, _ = cli._datasets(cfg, 0, "cuda")
    assert isinstance(tr.dataset, RawPairDataset) and len(tr.dataset) == 4 and tr.dataset.mask_threshold == 12
    cfg.DATA.ADDITIONAL_ROOT_DIRS = []
    os.remove(f"{root}/masks/i1.png")
    tr, _ = cli._datasets(cfg, 0, "cuda")
    assert isinstance(tr.dataset, RawPairDataset) and tr.dataset.missing_masks() == [1]
    from unet_watermark_amd.data import FolderDataset
    assert isinstance(cli._datasets(cfg, 0, None)[0].dataset, FolderDataset)      # the host path is left alone


def test_use_blurred_mask_is_refused_on_a_pair_dataset(tmp_path, L):
    from unet_watermark_amd import cli
    root = str(tmp_path / "d")
    _png(f"{root}/watermarked/a.png", _img(10)); _png(f"{root}/clean/a.png", _img(12))
    for augment in ("basic", "none"):
        with pytest.raises(ValueError, match="use-blurred-mask.*not served"):
            cli.main(["train", "--data-dir", root, "--use-blurred-mask", "--augment", augment])
    assert cli.build_parser().parse_args(["masks", "--data-dir", root, "--threshold", "9"]).threshold == 9


def test_python_layer_refuses_on_the_host(L):
    import torch
    from unet_watermark_amd import data as D
    packed, descs, mdescs = D.pack_images([np.zeros((4, 5, 3), np.uint8)])
    assert D.mask_descs_for(descs).tolist() == mdescs.tolist()
    two = D.pack_images([np.zeros((4, 5, 3), np.uint8), np.zeros((3, 3, 3), np.uint8)])
    assert D.mask_descs_for(two[1]).tolist() == two[2].tolist() == [(0, 4, 5), (20, 3, 3)]
    with pytest.raises(ValueError, match="0..255"):
        D.device_pair_mask(packed, descs, packed, descs, 256)
    with pytest.raises(ValueError, match="one length"):
        D.device_pair_mask(packed, descs, packed, descs[:0], 15)
    with pytest.raises(ValueError, match="come together"):
        D.device_pair_mask(packed, descs, packed, descs, 15, mask=torch.zeros(20, dtype=torch.uint8))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            D.device_pair_mask(packed, descs, packed, descs, 15)
    assert D.stage_clean([None, None], two[1], "cpu") == (None, None)


# ------------------------------------------------------------------------------------------------ argument checks, no device
def test_uwm_pair_mask_u8_checks_arguments_before_any_launch(L):
    """a null pointer, C != 3, a threshold outside 0..255, N <= 0, an empty buffer, a misaligned buffer or descriptor array: every such
    call returns non-zero with a message and none reaches a launch (the pointers are host memory)"""
    lib = L.lib()
    buf = (C.c_uint8 * 4096)()
    p = C.c_void_p(C.addressof(buf) + (-C.addressof(buf)) % 16)
    odd = C.c_void_p(p.value + 2); odd4 = C.c_void_p(p.value + 4)
    base = dict(wm=p, wm_bytes=64, wmd=p, clean=p, clean_bytes=64, cd=p, N=1, C=3, thr=15, open=1, mask=p, mask_bytes=64, md=p, st=None)

    def bad(word, **kw):
        rc = lib.uwm_pair_mask_u8(*[kw.get(k, v) for k, v in base.items()])
        assert rc != 0, kw
        msg = lib.uwm_last_error().decode()
        assert "uwm_pair_mask_u8" in msg and word in msg, msg

    for k in ("wm", "wmd", "clean", "cd", "mask", "md"):
        bad("null", **{k: None})
    for c in (1, 4, 0):
        bad("C must be 3", C=c)
    for t in (-1, 256):
        bad("0..255", thr=t)
    for n in (0, -3):
        bad(">= 1", N=n)
    for k in ("wm_bytes", "clean_bytes", "mask_bytes"):
        bad(">= 1", **{k: 0})
    bad("too large", N=1 << 26)
    bad("aligned", wm=odd); bad("aligned", clean=odd)
    for k in ("wmd", "cd", "md"):
        bad("aligned", **{k: odd4})
