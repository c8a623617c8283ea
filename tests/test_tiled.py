"""Prediction at native resolution, the part that needs no device: the tile plan (unet_watermark_amd/tiling.py) against its rule and
against the independent restatement (tests/tiled_ref.py), the restatement's blend on cases whose answer is known, the argument
checks of the new C entries (made before any launch), and the command line."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiled_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("uwm_op_tile_norm_u8_nhwc4", "uwm_tile_blend_threshold_ragged", "uwm_predict_tiled_workspace_bytes", "uwm_predict_tiled_u8")
# (len, T, overlap): shorter than / equal to / one past the tile, one stride past, between strides, overlap 0 and T / 2, odd sizes
AXES = [(1, 64, 16), (40, 64, 16), (64, 64, 16), (65, 64, 16), (112, 64, 16), (113, 64, 16), (129, 64, 16), (161, 64, 16), (200, 64, 16),
        (200, 64, 0), (200, 64, 32), (2160, 512, 64), (3840, 512, 64), (1000, 96, 7), (5, 1, 0), (33, 32, 16)]


@pytest.fixture(scope="module")
def tiling():
    from unet_watermark_amd import tiling as T
    return T


@pytest.mark.parametrize("length,T,overlap", AXES)
def test_an_axis_of_the_plan_keeps_its_rule(tiling, length, T, overlap):
    o = tiling.axis_origins(length, T, overlap)
    S = T - overlap
    assert o == R.axis_origins(length, T, overlap)
    assert len(o) == tiling.axis_count(length, T, overlap) == (1 if length <= T else -(-(length - T) // S) + 1)      # the formula
    assert all(0 <= v <= max(length - T, 0) for v in o)                       # every origin in [0, max(len - T, 0)]
    assert o == sorted(o) and o[0] == 0
    covered = np.zeros(length, bool)
    for v in o:
        covered[v: v + T] = True
    assert covered.all()                                                      # every pixel is under a tile
    if length <= T:
        assert o == [0]                                                       # one tile
    else:
        assert o[-1] + T == length                                            # the last tile ends at the border
        assert all(a + T - b >= overlap for a, b in zip(o, o[1:]))            # neighbours share at least `overlap` pixels
        assert len(set(o)) == len(o) or o[-1] == o[-2]                        # (only a clamped last tile may coincide with its neighbour)


def test_plan_tiles_is_row_major_and_covers_the_image(tiling):
    for h, w in [(64, 64), (100, 70), (65, 200), (40, 30), (3, 150), (64, 129)]:
        p = tiling.plan_tiles(h, w, 64, 64, 16)
        assert p == R.plan(h, w, 64, 64, 16)
        ys, xs = tiling.axis_origins(h, 64, 16), tiling.axis_origins(w, 64, 16)
        assert p == [(y, x) for y in ys for x in xs]                          # jy outer, jx inner
        seen = np.zeros((h, w), np.int64)
        for y0, x0 in p:
            seen[y0: y0 + 64, x0: x0 + 64] += 1
        assert seen.min() >= 1
    assert tiling.plan_tiles(40, 30, 64, 64, 16) == [(0, 0)] and tiling.plan_tiles(64, 64, 64, 64, 16) == [(0, 0)]
    assert tiling.plan_tiles(100, 70, 64, 64, 16) == [(0, 0), (0, 6), (36, 0), (36, 6)]      # two per axis, the last clamped
    # 161 = two strides + 1 past the tile: the clamped last tile starts one pixel behind its neighbour, and three tiles share pixels
    assert tiling.axis_origins(161, 64, 16) == [0, 48, 96, 97]


@pytest.mark.parametrize("overlap", [-1, 33, 1.5, "8", None, True])
def test_an_overlap_outside_0_to_half_a_tile_is_refused(tiling, overlap):
    with pytest.raises(ValueError):
        tiling.plan_tiles(100, 100, 64, 64, overlap)
    with pytest.raises(ValueError):
        tiling.plan_batch([(100, 100)], 64, 64, overlap, 8)


def test_the_overlap_bound_holds_on_both_axes(tiling):
    assert len(tiling.plan_tiles(100, 100, 64, 64, 0)) == 4 and len(tiling.plan_tiles(100, 100, 64, 64, 32)) == 9      # the bounds themselves pass
    with pytest.raises(ValueError):
        tiling.plan_tiles(100, 100, 64, 32, 17)                               # T_w / 2 = 16
    assert tiling.plan_tiles(100, 100, 64, 32, 16)
    with pytest.raises(ValueError):
        tiling.plan_tiles(100, 100, 2048, 64, 16)                             # a tile side beyond the blend's exact range


def test_plan_batch_concatenates_the_plans_and_pads_to_the_forward_batch(tiling):
    sizes = [(64, 64), (100, 70), (65, 200), (40, 30), (3, 150), (64, 129)]
    tiles, images = tiling.plan_batch(sizes, 64, 64, 16, 8)
    assert tiles.dtype == tiling.TILE_DTYPE and tiles.dtype.itemsize == 16 and images.dtype.itemsize == 16
    plans = [R.plan(h, w, 64, 64, 16) for h, w in sizes]
    real = sum(len(p) for p in plans)
    assert real == 1 + 4 + 8 + 1 + 3 + 3 and len(tiles) == 24 and len(tiles) % 8 == 0
    first = 0
    for i, p in enumerate(plans):
        assert tuple(images[i])[:3] == (first, len(R.axis_origins(sizes[i][0], 64, 16)), len(R.axis_origins(sizes[i][1], 64, 16)))
        for j, (y0, x0) in enumerate(p):
            assert tuple(tiles[first + j]) == (i, y0, x0, first)
        first += len(p)
    assert (tiles["image"][real:] == -1).all() and (tiles["image"][:real] >= 0).all()
    t7, _ = tiling.plan_batch(sizes, 64, 64, 16, 7)
    assert len(t7) == 21 and (t7["image"][20:] == -1).all()
    t1, _ = tiling.plan_batch([(64, 64)], 64, 64, 16, 8)
    assert len(t1) == 8 and t1["image"].tolist() == [0] + [-1] * 7
    with pytest.raises(ValueError):
        tiling.plan_batch([], 64, 64, 16, 8)
    with pytest.raises(ValueError):
        tiling.plan_batch(sizes, 64, 64, 16, 0)
    assert tiling.table_tensor(tiles).numel() == 16 * 24 and tiling.table_tensor(images).numel() == 16 * 6


def test_the_reflected_crop_is_borderinterpolate_101():
    assert R.reflect101(np.arange(-7, 12), 4).tolist() == [1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1]
    assert R.reflect101(np.arange(-3, 5), 1).tolist() == [0] * 8
    assert R.reflect101(np.arange(0, 6), 2).tolist() == [0, 1, 0, 1, 0, 1]
    img = np.arange(3 * 5 * 2, dtype=np.uint8).reshape(3, 5, 2)
    c = R.crop(img, 0, 0, 8, 8)
    assert c.shape == (8, 8, 2) and np.array_equal(c[:3, :5], img)
    assert np.array_equal(c[3], c[1]) and np.array_equal(c[4], c[0]) and np.array_equal(c[5], c[1])       # rows 0 1 2 1 0 1 2 1
    assert np.array_equal(c[:, 5], c[:, 3]) and np.array_equal(c[:, 7], c[:, 1])                          # columns 0 1 2 3 4 3 2 1
    assert np.array_equal(R.crop(img, 1, 2, 2, 3), img[1:3, 2:5])                                         # inside the image: a plain crop


@pytest.mark.parametrize("h,w", [(64, 64), (100, 70), (65, 200), (40, 30), (3, 150), (64, 129), (161, 161)])
def test_constant_tile_logits_blend_to_that_constant_exactly(h, w):
    """every w_k * c and every partial sum is an integer multiple of c below 2^24 c, so for a c of few mantissa bits the whole chain is
    exact and the quotient is c; a c of full mantissa need not come back bit for bit, which is why the rule passes single tiles through"""
    n = len(R.plan(h, w, 64, 64, 16))
    for c in (0.0, 1.0, -2.5, 0.375, 1024.0):
        out = R.blend(np.full((n, 64, 64), c, np.float32), h, w, 64, 64, 16)
        assert out.shape == (h, w) and out.dtype == np.float32 and (out == np.float32(c)).all(), (h, w, c)


def test_a_pixel_under_one_tile_is_passed_through_bit_for_bit():
    rng = np.random.default_rng(3)
    h, w = 100, 70                                                            # tiles at y 0 / 36, x 0 / 6
    lg = rng.normal(0, 3, (4, 64, 64)).astype(np.float32)
    lg[0, 0, 0] = np.float32(1e-41)                                           # a subnormal, and a value whose product with a weight rounds
    lg[3, 63, 63] = np.float32(np.pi)
    out = R.blend(lg, h, w, 64, 64, 16)
    assert np.array_equal(out[:36, :6].view(np.int32), lg[0, :36, :6].view(np.int32))                     # under tile (0, 0) alone
    assert np.array_equal(out[64:, 64:].view(np.int32), lg[3, 28:, 58:].view(np.int32))                   # under tile (1, 1) alone
    # under two tiles: the stated chain, by hand
    y, x = 10, 30                                                             # tiles (0, 0) and (0, 1): tx = 30 and 24
    w0, w1 = np.float32(11 * 31), np.float32(11 * 25)
    want = (w0 * lg[0, y, 30] + w1 * lg[1, y, 24]) / (w0 + w1)
    assert out[y, x].view(np.int32) == np.float32(want).view(np.int32)
    one = R.blend(lg[:1, :40, :30].copy().reshape(1, 40, 30), 40, 30, 40, 30, 0)
    assert np.array_equal(one.view(np.int32), lg[0, :40, :30].view(np.int32))


def test_the_blend_of_161_sums_three_tiles_in_plan_order():
    """len 161: origins 0, 48, 96, 97 -> column 100 lies under tiles 1, 2 and 3"""
    rng = np.random.default_rng(5)
    lg = rng.normal(0, 3, (4, 64, 64)).astype(np.float32)
    out = R.blend(lg, 64, 161, 64, 64, 16)
    f = np.float32
    ws = [f(1 * min(100 - o + 1, 64 - (100 - o))) for o in (48, 96, 97)]      # wy = 1 in row 0
    acc = ws[0] * lg[1, 0, 52]
    acc = acc + ws[1] * lg[2, 0, 4]
    acc = acc + ws[2] * lg[3, 0, 3]
    assert out[0, 100].view(np.int32) == f(acc / (ws[0] + ws[1] + ws[2])).view(np.int32)


# ------------------------------------------------------------------------------------------------ the library and the command line
@pytest.fixture(scope="module")
def L():
    from unet_watermark_amd import _lib
    return _lib


def test_the_header_declares_the_tiled_entries_and_the_binding_knows_them(L):
    header = open(os.path.join(ROOT, "include", "uwm.h")).read()
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES and hasattr(L.lib(), name), name
        assert f" {name}(" in header, name
    assert "uwm_tile_desc" in header and "uwm_tile_image" in header
    assert "tile_u8.hip" in L.SOURCES


def test_the_tiled_entries_check_their_arguments_before_any_launch(L):
    """no device is needed: every bad call returns non-zero with a message that names the call"""
    lib = L.lib()
    f3 = (C.c_float * 3)(0.5, 0.5, 0.5)
    z3 = (C.c_float * 3)(0.5, 0.0, 0.5)
    g = dict(src=0x10000, sb=4096, descs=0x20000, n=2, tiles=0x30000, K=8, C=3, Th=64, Tw=64, mean=f3, std=f3, out=0x40000)
    bad = [(dict(src=0), "null"), (dict(K=0), "K must be"), (dict(Th=2048), "tile sides"), (dict(C=5), "C must be"), (dict(n=0), "num_images"),
           (dict(src=0x10001), "4-byte"), (dict(descs=0x20004), "aligned"), (dict(out=0x40008), "16-byte"), (dict(std=z3), "std[1]")]
    for kw, word in bad:
        v = {**g, **kw}
        rc = lib.uwm_op_tile_norm_u8_nhwc4(v["src"], v["sb"], v["descs"], v["n"], v["tiles"], v["K"], v["C"], v["Th"], v["Tw"], v["mean"], v["std"],
                                           v["out"], 0)
        msg = lib.uwm_last_error().decode()
        assert rc != 0 and "uwm_op_tile_norm_u8_nhwc4" in msg and word in msg, (kw, msg)
    b = dict(store=0x10000, K=8, plans=0x20000, n=2, Th=64, Tw=64, ov=16, ind=0, sb=0, C=3, outd=0x30000, thr=0.5, mask=0x40000, mb=4096, lo=0)
    bad = [(dict(store=0), "null"), (dict(plans=0), "null"), (dict(ov=-1), "overlap"), (dict(ov=33), "overlap"), (dict(Tw=0), "tile sides"),
           (dict(mb=0), "mask_bytes"), (dict(thr=float("nan")), "finite"), (dict(outd=0x30004), "8-byte"), (dict(ind=0x50000, C=0), "C must be"),
           (dict(lo=0x60001), "4-byte"), (dict(n=1 << 30), "too many images")]
    for kw, word in bad:
        v = {**b, **kw}
        rc = lib.uwm_tile_blend_threshold_ragged(v["store"], v["K"], v["plans"], v["n"], v["Th"], v["Tw"], v["ov"], v["ind"], v["sb"], v["C"],
                                                 v["outd"], v["thr"], 0, v["mask"], v["mb"], v["lo"], 0)
        msg = lib.uwm_last_error().decode()
        assert rc != 0 and "uwm_tile_blend_threshold_ragged" in msg and word in msg, (kw, msg)
    assert lib.uwm_predict_tiled_workspace_bytes(None, 8, 0, 64, 64) == 0 and b"uwm_predict_tiled_workspace_bytes" in lib.uwm_last_error()
    rc = lib.uwm_predict_tiled_u8(None, 0x10000, 4096, 0x20000, 2, 0x30000, 8, 0x20000, 64, 64, 16, f3, f3, 0.5, 0, 0x30000, 0x40000, 4096, 0,
                                  0x50000, 1 << 20, 8, 0)
    assert rc != 0 and b"uwm_predict_tiled_u8: null argument" in lib.uwm_last_error()


def test_the_parser_takes_tile_and_predict_refuses_it_without_the_device_path_or_with_text_enhance(tmp_path):
    from unet_watermark_amd.cli import build_parser, predict_command
    base = ["predict", "--input", str(tmp_path), "--output", str(tmp_path / "out"), "--model", "none.pth"]
    d = build_parser().parse_args(base)
    assert d.tile is False and d.tile_overlap == 64                           # the defaults: nothing new is asked for
    args = build_parser().parse_args(base + ["--resize", "device", "--tile", "--tile-overlap", "32", "--mask-type", "text"])
    assert args.tile is True and args.tile_overlap == 32 and args.resize == "device"
    with pytest.raises(ValueError, match="--tile needs --resize device"):
        predict_command(build_parser().parse_args(base + ["--tile"]))
    with pytest.raises(ValueError, match="--tile needs --resize device"):
        predict_command(build_parser().parse_args(base + ["--resize", "host", "--tile"]))
    with pytest.raises(ValueError, match="--tile cannot be combined with --text-enhance"):
        predict_command(build_parser().parse_args(base + ["--resize", "device", "--tile", "--text-enhance"]))
    assert not (tmp_path / "out").exists()          # refused before anything was made


def test_the_predictor_has_no_cpu_fallback_for_the_tiled_path():
    from unet_watermark_amd.predict import WatermarkPredictor
    assert callable(getattr(WatermarkPredictor, "predict_images_tiled"))
    with pytest.raises(RuntimeError, match="HIP device"):
        WatermarkPredictor(device="cpu")
