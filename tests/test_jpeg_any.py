"""The JPEG save of the synthesis chain at any image size, the parts that need no device: the numpy restatement of libjpeg's edge rule
(tests/jpeg_any_ref.py) against Pillow's libjpeg-turbo, bit for bit and with no exempted case; the refusals of device_jpeg_ragged, of
the C ABI and of the command line; the defaults that keep every existing command what it was."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_any_ref as A  # noqa: E402
import jpeg_ref as J  # noqa: E402

_SIDES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 18, 23, 24, 31, 32, 33, 40]
SIZES = [(h, w) for h in _SIDES for w in _SIDES if w != 32] + [(100, 75), (75, 100), (64, 2), (2, 64), (65, 3), (3, 65), (129, 131), (130, 66)]
QUALITIES = [95, 30, 1, 100]


def _pillow():
    pytest.importorskip("PIL")
    from PIL import Image, features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("Pillow without libjpeg-turbo")
    return Image


def _pillow_roundtrip(Image, img, q):
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=q)          # Pillow's defaults: baseline, 4:2:0, islow DCT; decode: fancy up-sampling
    b.seek(0)
    return np.asarray(Image.open(b).convert("RGB"))


def _images(h, w):
    with np.errstate(divide="ignore"):                       # (the 'ramps' kind of a 1 x 1 image divides by zero, to 0)
        return J.sample_images(h, w)


def test_reference_equals_pillow_bit_for_bit_at_every_size():
    """350 sizes x 5 image kinds x 4 qualities; a condition, not a tolerance"""
    Image = _pillow()
    assert len(SIZES) == 350
    wrong, cases = [], 0
    for h, w in SIZES:
        for kind, img in _images(h, w).items():
            for q in QUALITIES:
                cases += 1
                if not np.array_equal(_pillow_roundtrip(Image, img, q), A.roundtrip_any(img, q)):
                    wrong.append((h, w, kind, q))
    assert cases == 7000 and not wrong, wrong[:20]


def test_reference_equals_the_fixed_shape_reference_at_multiples_of_16():
    for h, w in [(16, 16), (16, 48), (48, 32), (64, 96)]:
        for kind, img in _images(h, w).items():
            for q in QUALITIES:
                assert np.array_equal(A.roundtrip_any(img, q), J.roundtrip(img, q)), (h, w, kind, q)


def test_reference_quality_zero_and_refusals():
    for h, w in [(1, 1), (5, 4), (17, 33)]:
        img = _images(h, w)["noise"]
        out = A.roundtrip_any(img, 0)
        assert np.array_equal(out, img) and out is not img
    img = _images(9, 17)["noise"]
    got = A.roundtrip_ragged([img, img, img[:5, :4]], [0, 30, 95])
    assert np.array_equal(got[0], img) and np.array_equal(got[1], A.roundtrip_any(img, 30)) and got[2].shape == (5, 4, 3)
    for bad in (img[..., :1], img.astype(np.int32), img[:0]):
        with pytest.raises(ValueError):
            A.roundtrip_any(bad, 50)
    with pytest.raises(ValueError):
        A.roundtrip_any(img, 101)
    with pytest.raises(ValueError):
        A.roundtrip_ragged([img], [95, 95])


def test_every_dct_operand_stays_inside_int32_at_the_edges():
    J.STATS["max_abs"] = 0
    for h, w in [(1, 1), (5, 4), (9, 17), (24, 24)]:
        for kind in ("noise01", "stripes", "checker8"):
            for q in (1, 100):
                A.roundtrip_any(_images(h, w)[kind], q)
    assert 0 < J.STATS["max_abs"] < 1 << 31


# ------------------------------------------------------------------------------------------------ the wrapper's refusals on the host
def test_device_jpeg_ragged_refusals_on_the_host():
    from unet_watermark_amd import data as D
    imgs = [np.zeros((5, 4, 3), np.uint8), np.zeros((9, 17, 3), np.uint8)]
    packed, descs, _ = D.pack_images(imgs)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            D.device_jpeg_ragged(packed, descs, [95, 0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.device_jpeg_ragged(packed.float(), descs, [95, 0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.device_jpeg_ragged(packed.view(-1, 4), descs, [95, 0])
    with pytest.raises(ValueError, match=r"0 \(the image stays\) or 1\.\.100"):
        D.device_jpeg_ragged(packed, descs, [95, 101])
    with pytest.raises(ValueError, match=r"0 \(the image stays\) or 1\.\.100"):
        D.device_jpeg_ragged(packed, descs, [-1, 95])
    with pytest.raises(ValueError, match="one per image"):
        D.device_jpeg_ragged(packed, descs, [95])
    with pytest.raises(ValueError, match="one per image"):
        D.device_jpeg_ragged(packed, descs, [95.0, 30.0])
    with pytest.raises(ValueError, match="DESC_DTYPE"):
        D.device_jpeg_ragged(packed, np.zeros(2, np.int64), [95, 0])
    far = descs.copy(); far["offset"][1] += 4
    with pytest.raises(ValueError, match="leaves the packed buffer"):
        D.device_jpeg_ragged(packed, far, [95, 0])
    flat = descs.copy(); flat["h"][0] = 0
    with pytest.raises(ValueError, match="h, w >= 1"):
        D.device_jpeg_ragged(packed, flat, [95, 0])
    assert D.SYNTH_JPEG_QUALITY == 95
    for bad in (-1, 101, 95.0, True, "95"):
        with pytest.raises(ValueError, match="1..100"):
            D.check_jpeg_quality(bad)
    assert D.check_jpeg_quality(0) == 0 and D.check_jpeg_quality(np.int32(95)) == 95


# ------------------------------------------------------------------------------------------------ the C ABI
def _lib():
    import __graft_entry__ as g
    g.build()
    from unet_watermark_amd import _lib
    return _lib.lib()


def test_abi_entry_checks_arguments_before_any_launch():
    """uwm_jpeg_ragged_u8's refusals, in the words of the other ragged entry points.  The pointers are host memory, so no launch is
    reached."""
    lib = _lib()
    buf = (C.c_uint8 * 8192)()
    p = C.c_void_p(C.addressof(buf) + (-C.addressof(buf)) % 16)
    o, w = C.c_void_p(p.value + 1024), C.c_void_p(p.value + 2048)      # in, out and the workspace: 1024 bytes each, apart
    d, q = C.c_void_p(p.value + 4096), C.c_void_p(p.value + 4096 + 256)
    odd1, odd4 = C.c_void_p(p.value + 1), C.c_void_p(p.value + 4100)

    def bad(rc, word):
        assert rc != 0
        assert word in lib.uwm_last_error().decode(), lib.uwm_last_error().decode()

    size = lib.uwm_jpeg_ragged_workspace_bytes
    assert size(1, 1) == 1 and size(13, 12345) == 12345 and size(65535, 1 << 42) == 1 << 42
    for n, b, word in ((0, 100, "N must be 1 .. 65535"), (-1, 100, "N must be"), (65536, 100, "N must be"), (1, 0, "bytes must be 1 .. 2^42"),
                       (1, (1 << 42) + 1, "bytes must be")):
        assert size(n, b) == 0
        assert word in lib.uwm_last_error().decode()
    f = lib.uwm_jpeg_ragged_u8
    bad(f(None, o, 1024, d, q, 2, 3, 1000, w, 1024, None), "null argument")
    bad(f(p, None, 1024, d, q, 2, 3, 1000, w, 1024, None), "null argument")
    bad(f(p, o, 1024, None, q, 2, 3, 1000, w, 1024, None), "null argument")
    bad(f(p, o, 1024, d, None, 2, 3, 1000, w, 1024, None), "null argument")
    bad(f(p, o, 1024, d, q, 2, 3, 1000, None, 1024, None), "null argument")
    bad(f(p, o, 1024, d, q, 2, 1, 1000, w, 1024, None), "C must be 3")
    bad(f(p, o, 1024, d, q, 2, 4, 1000, w, 1024, None), "C must be 3")
    bad(f(p, o, 1024, d, q, 0, 3, 1000, w, 1024, None), "N must be 1 .. 65535")
    bad(f(p, o, 0, d, q, 2, 3, 1000, w, 1024, None), "bytes must be 1 .. 2^42")
    bad(f(p, o, 1024, d, q, 2, 3, 0, w, 1024, None), "max_pixels must be >= 1")
    bad(f(p, o, 1024, d, q, 2, 3, (1 << 31) - 1, w, 1024, None), "max_pixels too large")
    bad(f(p, C.c_void_p(p.value + 512), 1024, d, q, 2, 3, 1000, w, 1024, None), "out must be in itself or not overlap it")
    bad(f(odd1, o, 1023, d, q, 2, 3, 1000, w, 1024, None), "in and out must be 4-byte aligned")
    bad(f(p, C.c_void_p(o.value + 2), 1022, d, q, 2, 3, 1000, w, 1024, None), "in and out must be 4-byte aligned")
    bad(f(p, o, 1024, d, C.c_void_p(q.value + 2), 2, 3, 1000, w, 1024, None), "quality must be 4-byte aligned")
    bad(f(p, o, 1024, odd4, q, 2, 3, 1000, w, 1024, None), "descriptors and the workspace must be 8-byte aligned")
    bad(f(p, o, 1020, d, q, 2, 3, 1000, C.c_void_p(w.value + 4), 1020, None), "descriptors and the workspace must be 8-byte aligned")
    bad(f(p, o, 1024, d, q, 2, 3, 1000, w, 1023, None), "workspace too small")
    bad(f(p, o, 1024, d, q, 2, 3, 1000, C.c_void_p(o.value + 512), 1024, None), "workspace must not overlap out")
    bad(f(p, p, 1024, d, q, 2, 3, 1000, C.c_void_p(p.value + 512), 1024, None), "workspace must not overlap")


# ------------------------------------------------------------------------------------------------ the command line and the dataset
def test_parser_takes_the_quality_flags_and_their_defaults_are_zero():
    from unet_watermark_amd import cli
    parser = cli.build_parser()
    assert parser.parse_args(["train"]).synth_jpeg_quality == 0
    assert parser.parse_args(["train", "--synthesize", "--synth-jpeg-quality", "95"]).synth_jpeg_quality == 95
    base = ["synth", "--clean-dir", "c", "--output-dir", "o", "--count", "1"]
    assert parser.parse_args(base).jpeg_quality == 0 and parser.parse_args(base + ["--jpeg-quality", "95"]).jpeg_quality == 95
    with pytest.raises(SystemExit):
        parser.parse_args(["train", "--synth-jpeg-quality", "high"])
    for sub, flag in (("train", "--synth-jpeg-quality"), ("synth", "--jpeg-quality")):
        text = " ".join(parser._subparsers._group_actions[0].choices[sub].format_help().split())
        assert flag in text and "reference's value is 95" in text, sub


def test_command_lines_refuse_a_quality_outside_0_100_before_any_device_work(tmp_path):
    """both refusals come before a directory is read or a device is asked for: the paths do not exist"""
    from unet_watermark_amd import cli
    parser = cli.build_parser()
    missing = str(tmp_path / "missing")
    for bad in ("101", "-1"):
        a = parser.parse_args(["train", "--synthesize", "--augment", "basic", "--clean-dir", missing, "--logos-dir", missing,
                               "--synth-jpeg-quality", bad])
        with pytest.raises(ValueError, match="--synth-jpeg-quality must be 0"):
            cli._check_synthesize(a, "basic")
        s = parser.parse_args(["synth", "--clean-dir", missing, "--logos-dir", missing, "--output-dir", str(tmp_path / "out"), "--count", "1",
                               "--jpeg-quality", bad])
        with pytest.raises(ValueError, match="--jpeg-quality must be 0"):
            cli.synth_command(s)
    assert not os.path.exists(str(tmp_path / "out"))
    with pytest.raises(ValueError, match="give --synthesize as well"):
        cli._check_synthesize(parser.parse_args(["train", "--synth-jpeg-quality", "95"]), "basic")
    cli._check_synthesize(parser.parse_args(["train"]), "none")                      # a command without the flags: nothing to refuse
    ok = parser.parse_args(["train", "--synthesize", "--clean-dir", missing, "--logos-dir", missing, "--synth-jpeg-quality", "95"])
    cli._check_synthesize(ok, "basic")


def _dataset(root, rng):
    from PIL import Image
    os.makedirs(f"{root}/clean"); os.makedirs(f"{root}/logos")
    for i, (h, w) in enumerate([(40, 56), (33, 47), (64, 64)]):
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(f"{root}/clean/im{i}.png")
    for i, (h, w) in enumerate([(10, 14), (8, 8)]):
        a = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8); a[..., 3] = 255
        Image.fromarray(a, "RGBA").save(f"{root}/logos/l{i}.png")
    return f"{root}/clean", f"{root}/logos"


def test_dataset_with_quality_zero_yields_what_it_yields_today(tmp_path):
    from unet_watermark_amd.data import RawSynthDataset
    clean_dir, logos_dir = _dataset(str(tmp_path), np.random.default_rng(5))
    plain = RawSynthDataset(clean_dir, logos_dir, seed=3, mask_threshold=15)
    assert plain.jpeg_quality == 0
    for q in (0, 95):                                        # the quality never changes an item: it is the pipeline's
        ds = RawSynthDataset(clean_dir, logos_dir, seed=3, mask_threshold=15, jpeg_quality=q)
        assert ds.jpeg_quality == q and len(ds) == len(plain)
        for i in range(len(ds)):
            a, b = plain[i], ds[i]
            assert len(a) == len(b) == 3 and np.array_equal(a[0], b[0]) and a[2].tobytes() == b[2].tobytes()
            assert len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
    for bad in (-1, 101, 95.5, "95"):
        with pytest.raises(ValueError, match="jpeg_quality must be 0"):
            RawSynthDataset(clean_dir, logos_dir, jpeg_quality=bad)
