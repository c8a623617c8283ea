"""Test-time augmentation, the part that needs no device: the view codes and sets (unet_watermark_amd/tta.py) against numpy's flips and
quarter turns, the host restatement of the merge, the slot table, the argument checks of the new C entries (made before any launch) and
the command line."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("uwm_view_stage_bytes", "uwm_op_resize_norm_view_u8_nhwc4", "uwm_op_tile_norm_view_u8_nhwc4", "uwm_op_view_merge",
               "uwm_predict_images_tta_workspace_bytes", "uwm_predict_images_tta_u8", "uwm_predict_tiled_tta_workspace_bytes",
               "uwm_predict_tiled_tta_u8")


@pytest.fixture(scope="module")
def T():
    from unet_watermark_amd import tta
    return tta


@pytest.fixture(scope="module")
def L():
    from unet_watermark_amd import _lib
    return _lib


def np_view(a, code):
    """the rule of include/uwm.h in numpy: the horizontal flip first, then r counter-clockwise quarter turns"""
    r, f = code & 3, code >> 2
    return np.rot90(np.flip(a, 1) if f else a, r)


def test_the_header_declares_the_entries_and_the_binding_knows_them(L):
    header = open(os.path.join(ROOT, "include", "uwm.h")).read()
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES and hasattr(L.lib(), name), name
        assert f" {name}(" in header, name
    assert "tta.hip" in L.SOURCES
    assert "mean of the LOGITS" in header


def test_apply_view_is_the_flip_then_the_quarter_turns(T):
    a = np.arange(25, dtype=np.float32).reshape(5, 5)
    for c in range(8):
        got = T.apply_view(torch.from_numpy(a), c).numpy()
        assert np.array_equal(got, np_view(a, c)), c
        assert np.array_equal(T.invert_view(torch.from_numpy(got), c).numpy(), a), c
    assert len({T.apply_view(torch.from_numpy(a), c).numpy().tobytes() for c in range(8)}) == 8      # eight different planes
    one = T.apply_view(torch.from_numpy(a), 1).numpy()                        # one turn of a square of side S: out[i][j] = in[j][S - 1 - i]
    assert all(one[i][j] == a[j][4 - i] for i in range(5) for j in range(5))
    b = np.arange(24, dtype=np.float32).reshape(4, 6)
    for c in (0, 2, 4, 6):
        got = T.apply_view(torch.from_numpy(b), c).numpy()
        assert np.array_equal(got, np_view(b, c)), c
        assert np.array_equal(T.invert_view(torch.from_numpy(got), c).numpy(), b), c
    for c in (1, 3, 5, 7):
        with pytest.raises(ValueError, match="H == W"):
            T.apply_view(torch.from_numpy(b), c)
    assert np.array_equal(T.apply_view(torch.from_numpy(b), 4).numpy(), b[:, ::-1])      # the horizontal flip
    assert np.array_equal(T.apply_view(torch.from_numpy(b), 6).numpy(), b[::-1])         # code 6 is the vertical flip
    assert np.array_equal(T.apply_view(torch.from_numpy(b), 2).numpy(), b[::-1, ::-1])   # the half turn
    x = torch.arange(2 * 3 * 25, dtype=torch.float32).view(2, 3, 5, 5)                   # leading dimensions ride along
    assert torch.equal(T.apply_view(x, 5)[1, 2], T.apply_view(x[1, 2], 5))


def test_the_named_sets_and_their_codes(T):
    assert [T.view_mask(n) for n in ("none", "hflip", "flips", "d4")] == [0x01, 0x11, 0x55, 0xFF]
    assert T.view_mask(None) == 1 and T.view_mask(0x26) == 0x26
    assert T.view_codes("hflip") == [0, 4] and T.view_codes("flips") == [0, 2, 4, 6] and T.view_codes("d4") == list(range(8))
    assert T.view_codes(0x26) == [1, 2, 5]
    for bad in (0, 256, -1, "all", 1.5, True):
        with pytest.raises(ValueError):
            T.view_mask(bad)


def test_composing_d4_with_a_fixed_view_permutes_the_set(T):
    """what the equivariance test on the device rests on: {view_c o view_g : c in d4} is d4 again, for every g"""
    a = torch.arange(25, dtype=torch.float32).view(5, 5)
    planes = {T.apply_view(a, c).numpy().tobytes(): c for c in range(8)}
    for g in range(8):
        seen = sorted(planes[T.apply_view(T.apply_view(a, g), c).numpy().tobytes()] for c in range(8))
        assert seen == list(range(8)), g
    hf = {T.apply_view(a, c).numpy().tobytes() for c in (0, 4)}               # hflip is no such set: a quarter turn leaves it
    assert {T.apply_view(T.apply_view(a, 1), c).numpy().tobytes() for c in (0, 4)} != hf


def test_merge_views_is_the_stated_chain(T):
    rng = np.random.default_rng(7)
    p = torch.from_numpy(rng.normal(0, 3, (1, 5, 5)).astype(np.float32))
    assert np.array_equal(T.merge_views(p, 0x01).numpy().view(np.int32), p[0].numpy().view(np.int32))      # k = 1 returns its input
    q = torch.from_numpy(rng.normal(0, 3, (3, 5, 5)).astype(np.float32))
    codes = T.view_codes(0x26)
    back = [T.invert_view(q[j], codes[j]).numpy() for j in range(3)]
    want = ((back[0] + back[1]) + back[2]) / np.float32(3)                    # k = 3 divides by 3
    assert np.array_equal(T.merge_views(q, 0x26).numpy().view(np.int32), want.view(np.int32))
    assert T.merge_views(q, 0x26).dtype == torch.float32
    assert torch.equal(T.merge_views(torch.stack([q, q]), 0x26)[1], T.merge_views(q, 0x26))      # a batch of sets
    with pytest.raises(ValueError):
        T.merge_views(q, "d4")                                                # 3 planes for 8 views


def test_the_order_of_the_sum_shows_in_the_bits(T):
    """planes of very different magnitude: summed from the other end the mean differs in at least one bit, so a test that compares
    the device's merge bit for bit pins the order"""
    rng = np.random.default_rng(11)
    mag = np.float32(10.0) ** rng.uniform(-6, 3, (4, 16, 16)).astype(np.float32)
    p = torch.from_numpy((mag * rng.choice([-1.0, 1.0], mag.shape)).astype(np.float32))
    up = T.merge_views(p, "flips")
    codes = T.view_codes("flips")
    acc = T.invert_view(p[3], codes[3])
    for j in (2, 1, 0):
        acc = acc + T.invert_view(p[j], codes[j])
    down = acc / torch.tensor(4.0)
    assert (up.view(torch.int32) != down.view(torch.int32)).any()
    assert torch.allclose(up, down, rtol=1e-3, atol=1e-3)


def test_plan_slots_pads_to_the_batch_and_lets_a_set_straddle_chunks(T):
    table, chunks = T.plan_slots(3, "d4", 3)                                  # k = 8, batch 3: 24 slots, every set straddles chunks
    assert chunks == 8 and table.shape == (24, 2) and table.dtype == np.int32
    assert table[:, 0].tolist() == [i for i in range(3) for _ in range(8)] and table[:, 1].tolist() == list(range(8)) * 3
    assert {int(table[s, 0]) for s in range(3, 9)} == {0, 1}                  # chunks 1 and 2 hold views of two images
    table, chunks = T.plan_slots(3, "hflip", 4)                               # 6 slots -> 8
    assert chunks == 2 and table[:, 0].tolist() == [0, 0, 1, 1, 2, 2, -1, -1] and table[:, 1].tolist() == [0, 4, 0, 4, 0, 4, 0, 0]
    table, chunks = T.plan_slots(5, "none", 8)
    assert chunks == 1 and table[:, 0].tolist() == [0, 1, 2, 3, 4, -1, -1, -1]
    table, chunks = T.plan_slots(2, 0x26, 2)
    assert chunks == 3 and table.tolist() == [[0, 1], [0, 2], [0, 5], [1, 1], [1, 2], [1, 5]]
    for num, batch in ((0, 4), (3, 0)):
        with pytest.raises(ValueError):
            T.plan_slots(num, "d4", batch)


def _handle(L):
    desc = L.uwm_unet_desc(L.ENC["resnet18"], 3, 1, (C.c_int * 5)(256, 128, 64, 32, 16), 1e-5, 0.1, 0)
    h = C.c_void_p()
    L.check(L.lib().uwm_create(C.byref(desc), C.byref(h)))
    return h


def test_the_entries_check_their_arguments_before_any_launch(L):
    """no device is needed: every bad call returns non-zero with a message that names the call (pointers are fake, never followed; the
    handle of the model-level calls is a real one that was never bound, which is the last thing they check)"""
    lib = L.lib()
    f3 = (C.c_float * 3)(0.5, 0.5, 0.5)

    def refused(fn, rc, word):
        msg = lib.uwm_last_error().decode()
        assert rc != 0 and fn in msg and word in msg, (fn, word, msg)
    assert lib.uwm_view_stage_bytes(0xFF, 4, 64, 64) == 2 * 64 * 64 * 16      # k = 8: four slots touch at most two images
    assert lib.uwm_view_stage_bytes(0x01, 4, 64, 64) == 4 * 64 * 64 * 16 and lib.uwm_view_stage_bytes(0x11, 4, 4, 6) == 3 * 4 * 6 * 16
    assert lib.uwm_view_stage_bytes(0, 4, 64, 64) == 0 and b"uwm_view_stage_bytes" in lib.uwm_last_error()
    assert lib.uwm_view_stage_bytes(0x02, 4, 4, 6) == 0 and b"H == W" in lib.uwm_last_error()
    # the viewed resize + Normalize
    g = dict(src=0x10000, sb=4096, descs=0x20000, n=2, C=3, H=64, W=64, views=0xFF, s0=0, ns=4, stage=0x100000, stb=1 << 20, out=0x400000)
    bad = [(dict(src=0), "null"), (dict(stage=0), "null"), (dict(views=0), "views must be 1..255"), (dict(views=256), "views must be 1..255"),
           (dict(views=0x02, H=4, W=6), "H == W"), (dict(out=0x400008), "16-byte"), (dict(stage=0x100004), "16-byte"), (dict(descs=0x20004), "aligned"),
           (dict(s0=-1), "slot0"), (dict(ns=0), "num_slots"), (dict(s0=2 ** 31 - 2), "overflows"), (dict(stb=64), "stage too small"), (dict(C=5), "C must be")]
    for kw, word in bad:
        v = {**g, **kw}
        rc = lib.uwm_op_resize_norm_view_u8_nhwc4(v["src"], v["sb"], v["descs"], v["n"], v["C"], v["H"], v["W"], f3, f3, v["views"], v["s0"], v["ns"],
                                                  v["stage"], v["stb"], v["out"], 0)
        refused("uwm_op_resize_norm_view_u8_nhwc4", rc, word)
    # the viewed tile gather
    g = dict(src=0x10000, sb=4096, descs=0x20000, n=2, tiles=0x30000, K=8, C=3, Th=64, Tw=64, views=0x55, s0=0, ns=4, stage=0x100000, stb=1 << 20,
             out=0x400000)
    bad = [(dict(tiles=0), "null"), (dict(out=0), "null"), (dict(views=0), "views must be 1..255"), (dict(views=256), "views must be 1..255"),
           (dict(views=0x80, Th=64, Tw=32), "H == W"), (dict(out=0x400004), "16-byte"), (dict(tiles=0x30002), "aligned"), (dict(K=0), "K must be"),
           (dict(Th=2048), "tile sides"), (dict(stb=0), "stage too small")]
    for kw, word in bad:
        v = {**g, **kw}
        rc = lib.uwm_op_tile_norm_view_u8_nhwc4(v["src"], v["sb"], v["descs"], v["n"], v["tiles"], v["K"], v["C"], v["Th"], v["Tw"], f3, f3, v["views"],
                                                v["s0"], v["ns"], v["stage"], v["stb"], v["out"], 0)
        refused("uwm_op_tile_norm_view_u8_nhwc4", rc, word)
    # the merge
    g = dict(lg=0x10000, ld=4, H=64, W=64, views=0xFF, s0=0, ns=4, items=3, store=0x40000)
    bad = [(dict(lg=0), "null"), (dict(store=0), "null"), (dict(views=0), "views must be 1..255"), (dict(views=256), "views must be 1..255"),
           (dict(views=0x08, H=4, W=6), "H == W"), (dict(store=0x40002), "4-byte"), (dict(lg=0x10001), "4-byte"), (dict(ld=0), "ld must be"),
           (dict(items=0), "item count"), (dict(items=2 ** 30), "overflows")]
    for kw, word in bad:
        v = {**g, **kw}
        rc = lib.uwm_op_view_merge(v["lg"], v["ld"], v["H"], v["W"], v["views"], v["s0"], v["ns"], v["items"], v["store"], 0)
        refused("uwm_op_view_merge", rc, word)
    # the model-level calls
    h = _handle(L)
    try:
        plain = lib.uwm_predict_workspace_bytes(h, 4, 64, 64, 1)
        need = lib.uwm_predict_images_tta_workspace_bytes(h, 4, 64, 64, 3, 0xFF)
        assert plain > 0 and need == (plain + 255) // 256 * 256 + 2 * 64 * 64 * 16 + 3 * 64 * 64 * 4      # forward, two staged planes, three merged
        assert need < plain + 4 * 64 * 64 * 16                                # never k copies of the batch's input
        tneed = lib.uwm_predict_tiled_tta_workspace_bytes(h, 4, 8, 64, 64, 0x55)
        assert tneed == (plain + 255) // 256 * 256 + 2 * 64 * 64 * 16 + 8 * 64 * 64 * 4      # k = 4: four slots touch at most two tiles
        for q, args in ((lib.uwm_predict_images_tta_workspace_bytes, (4, 64, 64, 3)), (lib.uwm_predict_tiled_tta_workspace_bytes, (4, 8, 64, 64))):
            assert q(None, *args, 0xFF) == 0 and b"null" in lib.uwm_last_error()
            assert q(h, *args, 0) == 0 and b"views must be 1..255" in lib.uwm_last_error()
            assert q(h, *args, 256) == 0 and b"views must be 1..255" in lib.uwm_last_error()
        assert lib.uwm_predict_images_tta_workspace_bytes(h, 4, 64, 96, 3, 0x22) == 0 and b"H == W" in lib.uwm_last_error()
        g = dict(h=h, src=0x10000, descs=0x20000, n=3, views=0xFF, od=0x28000, mask=0x30000, merged=0, ws=0x100000, N=4, H=64, W=64)
        bad = [(dict(h=None), "null"), (dict(mask=0), "null"), (dict(views=0), "views must be 1..255"), (dict(views=256), "views must be 1..255"),
               (dict(views=0x02, H=64, W=96), "H == W"), (dict(ws=0x100008), "16-byte"), (dict(src=0x10001), "4-byte"), (dict(od=0x28004), "8-byte"),
               (dict(merged=0x50002), "4-byte"), (dict(n=0), "item count"), ({}, "uwm_bind")]
        for kw, word in bad:
            v = {**g, **kw}
            rc = lib.uwm_predict_images_tta_u8(v["h"], v["src"], 4096, v["descs"], v["n"], v["views"], f3, f3, 0.5, 0, v["od"], v["mask"], 4096,
                                               v["merged"], v["ws"], 1 << 30, v["N"], v["H"], v["W"], 0)
            refused("uwm_predict_images_tta_u8", rc, word)
        g = dict(h=h, src=0x10000, descs=0x20000, n=2, tiles=0x30000, K=8, plans=0x38000, T=64, Tw=64, ov=16, od=0x28000, mask=0x40000, lo=0,
                 ws=0x100000, N=4, views=0x55)
        bad = [(dict(h=None), "null"), (dict(tiles=0), "null"), (dict(views=0), "views must be 1..255"), (dict(views=256), "views must be 1..255"),
               (dict(views=0x20, Tw=96), "H == W"), (dict(ws=0x100004), "16-byte"), (dict(tiles=0x30001), "4-byte"), (dict(ov=40), "overlap"),
               (dict(lo=0x60001), "4-byte"), ({}, "uwm_bind")]
        for kw, word in bad:
            v = {**g, **kw}
            rc = lib.uwm_predict_tiled_tta_u8(v["h"], v["src"], 4096, v["descs"], v["n"], v["tiles"], v["K"], v["plans"], v["T"], v["Tw"], v["ov"], f3, f3,
                                              0.5, 0, v["od"], v["mask"], 4096, v["lo"], v["ws"], 1 << 30, v["N"], v["views"], 0)
            refused("uwm_predict_tiled_tta_u8", rc, word)
    finally:
        lib.uwm_destroy(h)


def test_the_parser_takes_tta_and_predict_refuses_it_without_the_device_path(tmp_path):
    from unet_watermark_amd.cli import build_parser, predict_command
    base = ["predict", "--input", str(tmp_path), "--output", str(tmp_path / "out"), "--model", "none.pth"]
    assert build_parser().parse_args(base).tta == "none"                      # the default: nothing new is asked for
    args = build_parser().parse_args(base + ["--resize", "device", "--tta", "d4", "--tile", "--mask-type", "text"])
    assert args.tta == "d4" and args.tile is True
    for choice in ("none", "hflip", "flips", "d4"):
        assert build_parser().parse_args(base + ["--resize", "device", "--tta", choice]).tta == choice
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--tta", "rot"])
    with pytest.raises(ValueError, match="--tta needs --resize device"):
        predict_command(build_parser().parse_args(base + ["--tta", "d4"]))
    with pytest.raises(ValueError, match="--tta needs --resize device"):
        predict_command(build_parser().parse_args(base + ["--resize", "host", "--tta", "hflip"]))
    assert not (tmp_path / "out").exists()          # refused before anything was made
    ev = ["evaluate", "--data-dir", str(tmp_path), "--model", "none.pth"]
    assert build_parser().parse_args(ev).tta == "none" and build_parser().parse_args(ev + ["--tta", "d4"]).tta == "d4"


def test_evaluate_records_the_choice(tmp_path):
    from unet_watermark_amd.evaluate import Evaluator, check_settings
    (tmp_path / "watermarked").mkdir(); (tmp_path / "masks").mkdir()
    res = Evaluator(tmp_path / "watermarked", tmp_path / "masks", scorer=lambda *a: [], log=None, tta="flips").run()
    assert res["settings"]["tta"] == "flips"
    assert Evaluator(tmp_path / "watermarked", tmp_path / "masks", scorer=lambda *a: [], log=None).settings["tta"] == "none"
    with pytest.raises(ValueError):
        check_settings(tta="rot")


def test_the_predictor_takes_tta_on_its_three_entries():
    import inspect
    from unet_watermark_amd.predict import WatermarkPredictor
    for name in ("predict_images", "predict_images_tiled", "score_images"):
        assert inspect.signature(getattr(WatermarkPredictor, name)).parameters["tta"].default is None, name
