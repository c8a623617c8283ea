"""The dataset filter, the part that needs no device: self-checks of the numpy restatement (tests/filter_ref.py) that the device kernel
is compared with, the new symbols of libuwm.so and their argument checks, which fail before any launch, the folder logic of
filter.py with an injected count function, and the `main.py filter` command line.  Every comparison is exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from unet_watermark_amd import _lib
    _lib.lib()
    return _lib


def _plane(rows):
    return np.array([[ch == "#" for ch in r] for r in rows])


def _logits(plane):
    """confident logits of a bool plane: at equal size the resize is the identity and sigmoid(+-5) is far from any threshold used"""
    return np.where(plane, 5.0, -5.0).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_the_order_of_sigmoid_and_resize_shows():
    """logits -1 and +5, weight 0.25 on the second (output pixel 1 of 4 from 2 taps): sigmoid(0.5) = 0.62 logit first,
    0.75 * 0.269 + 0.25 * 0.993 = 0.45 probability first"""
    lg = np.array([[-1.0, 5.0]], np.float32)
    i0, i1, wx = R.axis(4, 2)
    assert (int(i0[1]), int(i1[1]), float(wx[1])) == (0, 1, 0.25)
    assert abs(float(R.logit_resize_sigmoid(lg, 1, 4)[0, 1]) - 0.6225) < 1e-4
    assert abs(float(R.prob_resize(lg, 1, 4)[0, 1]) - 0.4500) < 1e-4
    assert (R.logit_resize_sigmoid(lg, 1, 4) > 0.5).tolist() == [[False, True, True, True]]
    assert (R.filter_mask(lg, 1, 4, 0.5, False) > 0).tolist() == [[False, False, True, True]]
    assert R.filter_count(lg, 1, 4, 0.5, False) == [2, 4]


def test_the_element_is_a_cross():
    assert R.CROSS.tolist() == [[0, 1, 0], [1, 1, 1], [0, 1, 0]]


HOLE = (["........." ,
         ".........",
         "..#####..",
         "..#####..",
         "..##.##..",
         "..#####..",
         "..#####..",
         ".........",
         "........."],
        # the open leaves the four crosses around (3,3), (3,5), (5,3), (5,5): a one-pixel hole at (4,4) between four set neighbours
        ["........." ,
         ".........",
         "...#.#...",
         "..#####..",
         "...#.#...",
         "..#####..",
         "...#.#...",
         ".........",
         "........."],
        # ... which the close fills
        ["........." ,
         ".........",
         "...#.#...",
         "..#####..",
         "...###...",
         "..#####..",
         "...#.#...",
         ".........",
         "........."])
# a 2 x 2 block in a corner, a lone pixel, a strip two pixels thick along the bottom border: the erosion ignores pixels outside the
# image, so the corner pixel and the border row's inner pixels survive it; the dilation reads 0 outside
BORDER = (["##......",
           "##......",
           ".....#..",
           "........",
           "..#####.",
           "..#####."],
          ["##......",
           "#.......",
           "........",
           "........",
           "...###..",
           "..#####."])


def test_restatement_on_hand_computed_planes():
    before, opened, closed = (_plane(p) for p in HOLE)
    assert np.array_equal(R.M.opening(before, R.CROSS), opened)
    assert np.array_equal(R.post_process(before), closed)
    assert not opened[4, 4] and closed[4, 4] and opened[3, 4] and opened[5, 4] and opened[4, 3] and opened[4, 5]
    assert np.array_equal(R.filter_mask(_logits(before), 9, 9, 0.5, True) > 0, closed)
    assert R.filter_count(_logits(before), 9, 9, 0.5, True) == [int(closed.sum()), 81]
    before, after = (_plane(p) for p in BORDER)
    assert before[2, 5] and not after[2, 5]                                  # the isolated pixel goes with the open
    assert np.array_equal(R.filter_mask(_logits(before), 6, 8, 0.5, True) > 0, after)
    assert R.filter_count(_logits(before), 6, 8, 0.5, True) == [11, 48]
    # post_process = 0 leaves the thresholded plane
    assert np.array_equal(R.filter_mask(_logits(before), 6, 8, 0.5, False) > 0, before)
    assert R.filter_count(_logits(before), 6, 8, 0.5, False) == [int(before.sum()), 48]


def test_a_one_pixel_image():
    """from a 1 x 1 plane every tap is the one logit; from a 4 x 4 plane the pixel is the mean of the four centre taps; the erosions
    ignore all four neighbours, which lie outside"""
    for post in (False, True):
        assert R.filter_mask(np.array([[3.0]], np.float32), 1, 1, 0.5, post).tolist() == [[255]]
        assert R.filter_count(np.array([[-3.0]], np.float32), 1, 1, 0.5, post) == [0, 1]
    lg = np.full((4, 4), -4.0, np.float32); lg[1:3, 1:3] = 4.0              # fy = fx = 1.5: the mean of the four centre taps
    assert R.filter_count(lg, 1, 1, 0.5, True) == [1, 1]
    assert R.filter_count(-lg, 1, 1, 0.5, True) == [0, 1]


def test_threshold_is_strict_and_the_sigmoid_is_the_projects():
    assert float(R.sigmoid32(0.0)) == 0.5
    z = np.zeros((2, 2), np.float32)
    assert R.filter_count(z, 2, 2, 0.5, False) == [0, 4]                     # v == threshold: background
    assert R.filter_count(z, 2, 2, 0.4999, False) == [4, 4]


def test_margin_is_the_distance_to_the_threshold():
    lg = np.array([[-1.0, 5.0]], np.float32)
    want = min(abs(v - 0.5) for v in (0.2689414, 0.45003283, 0.81221575, 0.9933072))
    assert abs(R.margin(lg, 1, 4, 0.5) - want) < 1e-6
    assert R.margin(np.zeros((2, 2), np.float32), 3, 3, 0.5) == 0.0


# ------------------------------------------------------------------------------------------------ symbols and argument checks, no device
def test_the_new_symbols_are_exported_and_declared(L):
    lib = L.lib()
    for name in ("uwm_filter_workspace_bytes", "uwm_prob_mask_count_ragged", "uwm_filter_images_u8"):
        assert name in L.SIGNATURES and getattr(lib, name) is not None
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "uwm.h")).read()
    for name in ("uwm_filter_workspace_bytes", "uwm_prob_mask_count_ragged", "uwm_filter_images_u8"):
        assert name + "(" in header
    assert lib.uwm_filter_workspace_bytes(1) == 64 * 8 and lib.uwm_filter_workspace_bytes(5) == 5 * 64 * 8
    for n in (0, -2, 1 << 26):
        assert lib.uwm_filter_workspace_bytes(n) == 0
        assert "uwm_filter_workspace_bytes" in lib.uwm_last_error().decode()


def _host_block():
    buf = (C.c_uint8 * 8192)()
    p = C.c_void_p(C.addressof(buf) + (-C.addressof(buf)) % 16)
    return buf, p, C.c_void_p(p.value + 2), C.c_void_p(p.value + 4)


def test_uwm_prob_mask_count_ragged_checks_arguments_before_any_launch(L):
    """a null pointer, N / h / w / ld below 1, a threshold that is not finite, a misaligned pointer, a workspace that is too small:
    every such call returns non-zero with a message and none reaches a launch (the pointers are host memory)"""
    lib = L.lib()
    keep, p, odd, odd4 = _host_block()
    base = dict(logits=p, ld=1, N=1, h=16, w=16, descs=p, thr=0.5, post=1, mask=p, mask_bytes=64, counts=p, ws=p, ws_bytes=512, st=None)

    def bad(word, **kw):
        rc = lib.uwm_prob_mask_count_ragged(*[kw.get(k, v) for k, v in base.items()])
        assert rc != 0, kw
        msg = lib.uwm_last_error().decode()
        assert "uwm_prob_mask_count_ragged" in msg and word in msg, msg

    for k in ("logits", "descs", "counts", "ws"):
        bad("null", **{k: None})
    for k in ("h", "w", "ld"):
        bad(">= 1", **{k: 0})
    for n in (0, -3):
        bad(">= 1", N=n)
    bad("too large", N=1 << 26)
    for t in (float("nan"), float("inf"), -float("inf")):
        bad("finite", thr=t)
    bad(">= 1", mask_bytes=0)
    bad("aligned", logits=odd)
    for k in ("descs", "counts", "ws"):
        bad("aligned", **{k: odd4})
    bad("too small", ws_bytes=511)
    bad("too small", N=2, ws_bytes=512)


def test_uwm_filter_images_u8_checks_arguments_before_any_launch(L):
    lib = L.lib()
    keep, p, odd, odd4 = _host_block()
    desc = L.uwm_unet_desc(encoder=18, in_channels=3, classes=1, decoder_channels=(C.c_int * 5)(256, 128, 64, 32, 16), bn_eps=1e-5,
                           bn_momentum=0.1, arch=0)
    h = C.c_void_p()
    L.check(lib.uwm_create(C.byref(desc), C.byref(h)))
    try:
        f3 = (C.c_float * 3)(0.5, 0.5, 0.5)
        base = dict(h=h, src=p, src_bytes=64, ind=p, mean=f3, std=f3, thr=0.5, post=1, outd=p, mask=None, mask_bytes=0, counts=p, logits=None,
                    ws=p, ws_bytes=1 << 40, fws=p, fws_bytes=512, N=1, H=64, W=64, st=None)

        def bad(word, **kw):
            rc = lib.uwm_filter_images_u8(*[kw.get(k, v) for k, v in base.items()])
            assert rc != 0, kw
            msg = lib.uwm_last_error().decode()
            assert "uwm_filter_images_u8" in msg and word in msg, msg

        for k in ("h", "src", "ind", "mean", "std", "outd", "counts", "ws", "fws"):
            bad("null", **{k: None})
        bad(">= 1", N=0)
        for t in (float("nan"), float("inf")):
            bad("finite", thr=t)
        bad(">= 1", mask=p, mask_bytes=0)
        for k in ("outd", "counts", "fws"):
            bad("aligned", **{k: odd4})
        bad("too small", fws_bytes=8)
        bad("uwm_bind")                                                      # every argument is fine, but nothing is bound: still no launch
    finally:
        lib.uwm_destroy(h)


# ------------------------------------------------------------------------------------------------ the folder logic, counts injected
def _png(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(path, format="PNG")


def _white_counts(calls):
    """the injected count function: an image's white pixels are its "watermark"; records (batch length, full) per call"""
    def fn(images, full):
        calls.append((len(images), full))
        return np.array([[int((im[..., 0] == 255).sum()), im.shape[0] * im.shape[1]] for im in images], np.int64)
    return fn


def _folder(root):
    """ten 10 x 10 images with 0, 1, 2, 5 ... white pixels under every extension of the list in mixed case, one undecodable file, one
    file that is no image -> {name: white pixels}"""
    os.makedirs(root)
    names = {"a.png": 0, "b.PNG": 1, "c.jpg": 2, "d.JPEG": 5, "e.bmp": 10, "f.TIF": 0, "g.tiff": 3, "h.JPG": 1, "i.jpeg": 40, "j.BMP": 2}
    for name, white in names.items():
        a = np.zeros((10, 10, 3), np.uint8)
        a.reshape(-1, 3)[:white] = 255
        _png(os.path.join(root, name), a)                                    # (PNG bytes under every name: the decoder goes by content)
    with open(os.path.join(root, "broken.png"), "wb") as f:
        f.write(b"this is not a png")
    with open(os.path.join(root, "notes.txt"), "w") as f:
        f.write("not an image")
    return names


def _run(root, thr, bs=4, **kw):
    from unet_watermark_amd import filter as F
    calls, lines = [], []
    stats = F.filter_folder(root, lambda paths: F.batch_ratios(paths, _white_counts(calls), bs), thr, log=lines.append, **kw)
    return stats, calls, lines


def test_filter_folder_moves_deletes_or_only_reports(tmp_path):
    from unet_watermark_amd import filter as F
    root = str(tmp_path / "in")
    names = _folder(root)
    listed = [p.name for p in F.list_images(root)]
    assert sorted(listed) == sorted(list(names) + ["broken.png"]) and len(set(listed)) == len(listed)      # both letter cases, once each
    thr = 0.02                                                               # 2 of 100 pixels: ratio == threshold keeps the file
    low = sorted(n for n, wh in names.items() if wh / 100 < thr)
    assert low == ["a.png", "b.PNG", "f.TIF", "h.JPG"] and names["c.jpg"] / 100 == thr
    want = {"total": 11, "with_watermark": 6, "without_watermark": 4, "moved": 0, "errors": 1}
    before = sorted(os.listdir(root))

    # a dry run touches nothing, with a directory or with delete
    for kw in (dict(no_watermark_dir=str(tmp_path / "out"), dry_run=True), dict(delete=True, dry_run=True)):
        stats, calls, lines = _run(root, thr, **kw)
        assert stats == want and sorted(os.listdir(root)) == before and not (tmp_path / "out").exists()
        assert sum("[dry run]" in ln for ln in lines) == 4
        # eleven paths in batches of four; the undecodable one (sixth in the list's order) rides in none
        assert calls == [(4, True), (3, False), (3, False)]
    # neither a directory nor delete: a report only
    stats, _, lines = _run(root, thr)
    assert stats == want and sorted(os.listdir(root)) == before
    assert sum(ln.startswith("no watermark:") for ln in lines) == 4 and sum(ln.startswith("keep:") for ln in lines) == 6
    assert sum(ln.startswith("error: broken.png") for ln in lines) == 1
    # a directory and delete together are refused
    with pytest.raises(ValueError, match="not both"):
        F.filter_folder(root, lambda paths: [0.0] * len(paths), thr, no_watermark_dir=str(tmp_path / "out"), delete=True)
    # a target directory moves exactly the files below the threshold; the undecodable file stays and counts under errors
    out = str(tmp_path / "out")
    stats, _, lines = _run(root, thr, no_watermark_dir=out)
    assert stats == dict(want, moved=4)
    assert sorted(os.listdir(out)) == low
    assert sorted(os.listdir(root)) == sorted(set(before) - set(low)) and "broken.png" in os.listdir(root)
    assert sum(ln.startswith("move:") for ln in lines) == 4
    # delete=True deletes exactly the files below the (now higher) threshold
    thr2 = 0.05
    low2 = sorted(n for n, wh in names.items() if wh / 100 < thr2 and n not in low)
    assert low2 == ["c.jpg", "g.tiff", "j.BMP"] and names["d.JPEG"] / 100 == thr2
    stats, _, _ = _run(root, thr2, delete=True)
    assert stats == {"total": 7, "with_watermark": 3, "without_watermark": 3, "moved": 3, "errors": 1}
    assert sorted(os.listdir(root)) == sorted(set(before) - set(low) - set(low2))
    assert sorted(os.listdir(out)) == low                                    # (nothing else was moved)


def test_batches_and_images_that_are_not_counted(tmp_path):
    """full batches are flagged (they replay the captured graph), only the last one is short; an undecodable file rides in no batch; an
    image whose count comes back as {0, 0} is an error, not "no watermark\""""
    from unet_watermark_amd import filter as F
    root = str(tmp_path / "in")
    os.makedirs(root)
    for i in range(9):
        _png(os.path.join(root, f"im{i}.png"), np.full((4, 4, 3), 255 if i % 2 else 0, np.uint8))
    with open(os.path.join(root, "im4.png"), "wb") as f:
        f.write(b"\x89PNG broken")
    calls = []
    res = F.batch_ratios(F.list_images(root), _white_counts(calls), 4)
    assert calls == [(4, True), (3, False), (1, False)]                      # im4 is missing from the second batch of four paths
    assert [r if not isinstance(r, Exception) else "E" for r in res] == [0.0, 1.0, 0.0, 1.0, "E", 1.0, 0.0, 1.0, 0.0]
    zero = lambda images, full: np.zeros((len(images), 2), np.int64)      # noqa: E731
    stats = F.filter_folder(root, lambda paths: F.batch_ratios(paths, zero, 4), 0.5, delete=True, log=None)
    assert stats == {"total": 9, "with_watermark": 0, "without_watermark": 0, "moved": 0, "errors": 9} and len(os.listdir(root)) == 9
    assert F.filter_folder(str(tmp_path / "empty_missing"), lambda p: [], 0.5, log=None)["total"] == 0
    assert F.watermark_ratio(1, 3) == 1 / 3
    with pytest.raises(ValueError):
        F.watermark_ratio(0, 0)


# ------------------------------------------------------------------------------------------------ the command line
def test_main_filter_help_and_the_exclusive_actions(capsys):
    from unet_watermark_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["filter", "--help"])
    assert e.value.code == 0
    text = " ".join(capsys.readouterr().out.split())
    for word in ("--no-watermark-dir", "--delete", "--dry-run", "--batch-size", "stays where it is", "only with --delete", "only reports"):
        assert word in text, word
    args = cli.build_parser().parse_args(["filter", "--input", "d", "--model", "m.pth"])
    assert args.threshold == 0.0001 and not args.delete and args.no_watermark_dir is None and not args.dry_run
    with pytest.raises(SystemExit) as e:
        cli.build_parser().parse_args(["filter", "--input", "d", "--model", "m.pth", "--no-watermark-dir", "o", "--delete"])
    assert e.value.code == 2
    assert "not allowed with" in capsys.readouterr().err


def test_the_class_is_exported():
    import unet_watermark_amd as U
    assert U.WatermarkFilter is U.filter.WatermarkFilter
    assert U.filter.IMAGE_EXTENSIONS == (".jpg", ".jpeg", ".png", ".bmp", ".tiff", ".tif")
