"""The membrane fill on the CPU: the numpy restatement tests/inpaint_ref.py against the exact solution of the level-0 linear system
(scipy, float64), its exact properties, and the host logic of `main.py repair`.

Convergence.  The bar is derived, not guessed: below 0.5 grey level before rounding, the stored byte is within one level of the rounded
exact membrane.  DEFAULT_CYCLES is the smallest count at which the eight cases of the issue are under it.  The figures of the
restatement (max |u - exact| over the hole after the push and after cycles 1 .. 8; DESIGN.md 8v has the whole table):
    corner 97 x 131     29.1 | 13.7  7.36  3.80  1.96  1.00  0.514  0.263  0.135          <- the slowest: under 0.5 from cycle 7 on
    corner 200 x 264    34.4 | 12.3  6.19  2.29  1.14  0.434 0.208  0.0815 0.0382
    rect   97 x 131     21.0 | 2.96  0.663 0.190 0.0566 ...
    strokes 97 x 131    15.4 | 1.51  0.220 0.0331 ... 4.5e-05 4.5e-05                      <- float32's floor
The error falls from each cycle to the next until it reaches the resolution of float32: an iterate near 255 has an ulp of 2^-16 =
1.5e-05, a V-cycle's own rounding is a few of them, so below FLOOR = 2^-13 (eight ulp) a step may stall; the test asks for a strict
fall above FLOOR and for staying at or below it afterwards."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inpaint_ref as R  # noqa: E402

FLOOR = 2.0 ** -13
SIZES = ((97, 131), (200, 264))


def conv_image(h, w):
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:h, 0:w]
    return np.clip(128 + 60 * np.sin(x / 17) + 50 * np.cos(y / 11) + rng.normal(0, 25, (h, w)), 0, 255).round().astype(np.uint8)


def conv_masks(h, w):
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(1)
    return {
        "rect": (abs(y - h // 2) < h // 4) & (abs(x - w // 2) < w // 4),                 # centred, half the sides
        "corner": (y >= h - h // 3) & (x >= w - w // 3),                                 # lower right, a third of the sides
        "disc": (y - h / 2) ** 2 + (x - w / 2) ** 2 < (0.4 * min(h, w)) ** 2,
        "strokes": ((y % 16 < 3) & (y > 10) & (y < h - 10) & (x > 8) & (x < w - 8)) | ((x % 13 < 2) & (y > 20) & (y < h / 2)),
        "random": (rng.random((h, w)) < 0.5) | ((y < h // 2) & (x < w // 2)),            # reported, not held to the bar
    }


_errors = {}


def errors(size, name):
    """max |u - exact| over the hole after the push and after each of 8 cycles, computed once"""
    if (size, name) not in _errors:
        img, m = conv_image(*size), conv_masks(*size)[name]
        exact = R.exact_membrane(img.astype(np.float64), m)
        trace = []
        R.solve_plane(img.astype(np.float32), R.Hierarchy(m), 8, trace)
        _errors[(size, name)] = [float(np.abs(u.astype(np.float64) - exact)[m].max()) for u in trace]
    return _errors[(size, name)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ("rect", "corner", "disc", "strokes", "random"))
def test_convergence_against_the_exact_membrane(size, name):
    from unet_watermark_amd.inpaint import DEFAULT_CYCLES
    e = errors(size, name)
    print(f"{name} {size[0]} x {size[1]}: push {e[0]:.3g} | cycles 1..8 " + " ".join(f"{v:.3g}" for v in e[1:]))
    if name == "random":
        return
    assert e[DEFAULT_CYCLES] < 0.5
    for k in range(8):
        assert e[k + 1] < e[k] or e[k + 1] <= FLOOR, (k, e)


def test_default_cycles_is_the_smallest_count_under_the_bar():
    from unet_watermark_amd.inpaint import DEFAULT_CYCLES
    worst = [max(errors(s, n)[k] for s in SIZES for n in ("rect", "corner", "disc", "strokes")) for k in range(9)]
    assert worst[DEFAULT_CYCLES] < 0.5 <= worst[DEFAULT_CYCLES - 1], worst


# ---------------------------------------------------------------- exact properties of the restatement
def _some_masks(h, w, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    return [rng.random((h, w)) < 0.5, (y > h // 3) & (x > w // 4), (y + x) % 2 == 0, ~((y == 1) & (x == 2)), (y == h // 2) & (x == w // 2)]


@pytest.mark.parametrize("size", ((3, 5), (17, 30), (33, 65)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_constant_image_comes_back_constant(size):
    for value in (0, 7, 200, 255):
        img = np.full(size + (2,), value, np.uint8)
        for m in _some_masks(*size):
            out, stats = R.inpaint_ref(img, m.astype(np.uint8), 3)
            assert (out == value).all() and stats[1] == 0


def test_known_pixels_are_kept_and_cycles_0_is_the_rounded_push():
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (37, 50, 3), dtype=np.uint8)
    for m in _some_masks(37, 50):
        hier = R.Hierarchy(m)
        for cycles in (0, 2):
            out, stats = R.inpaint_ref(img, m.astype(np.uint8) * 255, cycles)
            assert np.array_equal(out[~m], img[~m]) and stats == [int(m.sum()), 0, hier.levels_with_unknowns, 0]
        out0, _ = R.inpaint_ref(img, m.astype(np.uint8), 0)
        for c in range(3):
            g = R.pull_push(img[:, :, c].astype(np.float32), hier)
            assert np.array_equal(out0[:, :, c][m], np.rint(np.clip(g, 0, 255))[m].astype(np.uint8))


def test_empty_and_full_masks():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (9, 14, 3), dtype=np.uint8)
    out, stats = R.inpaint_ref(img, np.zeros((9, 14), np.uint8), 7)
    assert np.array_equal(out, img) and stats == [0, 1, 0, 0]
    out, stats = R.inpaint_ref(img, np.full((9, 14), 3, np.uint8), 7)
    assert np.array_equal(out, img) and stats == [9 * 14, 2, 0, 0]


def test_channels_are_independent():
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (41, 29, 3), dtype=np.uint8)
    m = _some_masks(41, 29)[1].astype(np.uint8)
    out, _ = R.inpaint_ref(img, m, 4)
    for c in range(3):
        one, _ = R.inpaint_ref(img[:, :, c:c + 1], m, 4)
        assert np.array_equal(one[:, :, 0], out[:, :, c])


def test_level_rules():
    assert [R.num_levels(h, w) for h, w in ((1, 1), (1, 2), (2, 2), (3, 5), (64, 64), (65, 3), (150, 203))] == [0, 1, 1, 3, 6, 7, 8]
    c = np.arange(6, dtype=np.float32).reshape(2, 3)
    u = R.up(c, 3, 5)
    assert u.shape == (3, 5) and u[0, 0] == c[0, 0]                                     # clamped taps at the rim: 9 + 3 + 3 + 1 of one value
    assert u[1, 1] == ((9 * c[0, 0] + 3 * c[0, 1]) + (3 * c[1, 0] + c[1, 1])) * 0.0625
    hier = R.Hierarchy(np.ones((4, 6), bool) & (np.mgrid[0:4, 0:6][1] < 4))
    assert hier.H[1].tolist() == [[True, True, False], [True, True, False]] and hier.H[2].tolist() == [[True, False]]


# ---------------------------------------------------------------- host logic of `repair`
def _parse(argv):
    from unet_watermark_amd.cli import build_parser
    return build_parser().parse_args(["repair"] + argv)


@pytest.mark.parametrize("argv, word", (
    (["--input", "i", "--output", "o"], "--model"),
    (["--input", "i", "--output", "o", "--model", "m", "--masks", "d"], "--model"),
    (["--input", "i", "--output", "o", "--model", "m", "--tile", "--text-enhance"], "--tile"),
    (["--input", "i", "--output", "o", "--model", "m", "--cycles", "33"], "cycles"),
    (["--input", "i", "--output", "o", "--model", "m", "--cycles", "-1"], "cycles"),
    (["--input", "i", "--output", "o", "--masks", "d", "--tile"], "--masks"),
    (["--input", "i", "--output", "o", "--model", "m", "--batch-size", "0"], "--batch-size"),
))
def test_repair_refusals_come_before_anything_is_created(tmp_path, monkeypatch, argv, word):
    from unet_watermark_amd.cli import repair_command
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        repair_command(_parse(argv))
    assert str(e.value).startswith("repair: ") and word in str(e.value)
    assert os.listdir(tmp_path) == []


def test_repair_parser_refuses_the_reference_flags_it_does_not_serve():
    for flag in ("--iopaint-model", "--ocr", "--video"):
        with pytest.raises(SystemExit):
            _parse(["--input", "i", "--output", "o", "--model", "m", flag, "x"])
    a = _parse(["--input", "i", "--output", "o", "--model", "m"])
    assert a.mask_type == "watermark" and a.cycles is None and a.tta == "none" and a.batch_size == 16 and a.seed == 0


def test_repair_pairs_by_stem_and_counts_errors(tmp_path):
    """--masks on a temporary folder with the device call replaced by the restatement"""
    from PIL import Image
    from unet_watermark_amd.inpaint import DEFAULT_CYCLES
    from unet_watermark_amd.repair import format_counts, repair_folder
    rng = np.random.default_rng(8)
    inp, msk, out, saved = (str(tmp_path / d) for d in ("in", "masks", "out", "saved"))
    os.makedirs(inp); os.makedirs(msk)
    images, masks = {}, {}
    for stem, ext, kind in (("a", ".png", "hole"), ("b", ".png", "empty"), ("c", ".png", "full"), ("d", ".png", "orphan"),
                            ("e", ".png", "size"), ("f", ".png", "broken"), ("g", ".bmp", "hole")):
        im = rng.integers(0, 256, (20, 31, 3), dtype=np.uint8)
        m = np.zeros((20, 31), np.uint8)
        if kind in ("hole", "broken"):
            m[5:12, 8:20] = 255 if stem == "a" else 1
        if kind == "full":
            m[:] = 255
        images[stem], masks[stem] = im, m
        Image.fromarray(im).save(os.path.join(inp, stem + ext))
        if kind == "size":
            Image.fromarray(np.zeros((20, 30), np.uint8)).save(os.path.join(msk, stem + ".png"))
        elif kind != "orphan":
            Image.fromarray(m).save(os.path.join(msk, stem + ".png"))
    with open(os.path.join(inp, "f.png"), "wb") as fh:
        fh.write(b"not an image")
    with open(os.path.join(inp, "notes.txt"), "w") as fh:
        fh.write("ignored")
    calls = []

    def fill(ims, mks, cycles):
        calls.append((len(ims), cycles))
        res = [R.inpaint_ref(i, m, cycles) for i, m in zip(ims, mks)]
        return [r[0] for r in res], [r[1] for r in res]

    log = []
    res = repair_folder(inp, out, masks_dir=msk, save_masks=saved, batch_size=3, fill=fill, log=log.append)
    assert {k: res[k] for k in ("repaired", "nothing_to_fill", "no_known_pixel", "errors")} == dict(repaired=2, nothing_to_fill=1,
                                                                                                  no_known_pixel=1, errors=3)
    assert sorted(os.path.basename(e["path"]) for e in res["error_details"]) == ["d.png", "e.png", "f.png"] and len(log) == 3
    assert all(c[1] == DEFAULT_CYCLES for c in calls) and sum(c[0] for c in calls) == 4
    assert sorted(os.listdir(out)) == ["a.png", "b.png", "c.png", "g.png"] and sorted(os.listdir(saved)) == sorted(os.listdir(out))
    for stem in ("a", "b", "c", "g"):
        want, _ = R.inpaint_ref(images[stem], masks[stem], DEFAULT_CYCLES)
        assert np.array_equal(np.asarray(Image.open(os.path.join(out, stem + ".png"))), want), stem
        assert np.array_equal(np.asarray(Image.open(os.path.join(saved, stem + ".png"))) != 0, masks[stem] != 0)
    assert not np.array_equal(np.asarray(Image.open(os.path.join(out, "a.png"))), images["a"])
    assert format_counts(res) == "repaired 2, nothing to fill 1, no known pixel 1, errors 3"
    assert repair_folder(inp, out, masks_dir=msk, limit=2, seed=0, fill=fill, log=log.append)["repaired"] <= 2
