"""Text-watermark synthesis, the CPU side: the numpy restatement (tests/textsynth_ref.py) against Pillow itself, bit for bit — the
COLOUR stage against ImageDraw.text, the whole chain against the literal Pillow chain of the reference's generate_text_watermark, the
two mask modes against Image.paste and Image.blend — and the host layer: the sampler, the dataset, the library's symbols and the
refusals.  Pillow's embedded scalable font is used throughout, so the tests need freetype and nothing else."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest
import torch
from PIL import Image, ImageDraw, ImageEnhance, ImageFilter, features

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import textsynth_ref as T  # noqa: E402

needs_freetype = pytest.mark.skipif(not features.check("freetype2"), reason="this Pillow has no freetype: no scalable font to draw with")
IMAGE_SIZES = [(96, 64), (64, 96), (200, 120), (33, 47)]                 # (W, H)
TEXTS = ["Proof Copy", "©2025 №47", "STOCK", "www.stockpix.io", ""]


@pytest.fixture(scope="module")
def D():
    import __graft_entry__ as g
    g.build()
    from unet_watermark_amd import data
    return data


@pytest.fixture(scope="module")
def fonts(D):
    return D.FontSet()


# ------------------------------------------------------------------------------------------------ stage A against ImageDraw.text
@needs_freetype
@pytest.mark.parametrize("text", ["Proof Copy", "©2025 №47", ""])
@pytest.mark.parametrize("size", [21, 38])
def test_colour_stage_equals_imagedraw_text(D, fonts, text, size):
    font = fonts.font(0, size)
    plane = D.render_text_plane(text, font)
    assert plane.dtype == np.uint8 and plane.ndim == 2
    if text == "":
        assert plane.shape == (40, 40) and not plane.any()
    else:
        assert plane.any() and 0 < plane[plane != 0].min() < 255                 # anti-aliased: partial coverage occurs
    for ink in D.TEXT_INKS:
        canvas = Image.new("RGBA", (plane.shape[1], plane.shape[0]), (0, 0, 0, 0))
        ImageDraw.Draw(canvas).text((20, 20), text, font=font, fill=ink + (255,))
        assert np.array_equal(T.colour(plane, ink), np.asarray(canvas)), (text, size, ink)


@needs_freetype
def test_colour_stage_on_a_canvas_that_clips_the_glyph_box(D, fonts):
    """the coverage plane is the glyph mask placed at the draw position and clipped; COLOUR of it is what ImageDraw.text draws"""
    font = fonts.font(0, 30)
    for size, at in [((50, 30), (20, 2)), ((60, 40), (-9, -6)), ((25, 70), (3, 50))]:
        cover = Image.new("L", size, 0)
        ImageDraw.Draw(cover).text(at, "Stock №7", font=font, fill=255)
        plane = np.asarray(cover)
        assert plane.any() and (plane[:, -1].any() or plane[-1].any() or plane[0].any() or plane[:, 0].any()), "the text is clipped"
        for ink in D.TEXT_INKS:
            canvas = Image.new("RGBA", size, (0, 0, 0, 0))
            ImageDraw.Draw(canvas).text(at, "Stock №7", font=font, fill=ink + (255,))
            assert np.array_equal(T.colour(plane, ink), np.asarray(canvas)), (size, ink)


# ------------------------------------------------------------------------------------------------ the whole chain against Pillow
def pillow_chain(rng, clean, text_img, transparent):
    """generate_text_watermark from its colour draw on and apply_text_effects, restated with Pillow's own operations and the
    script's draws in the script's order -> (watermarked RGB, mask L by the non-OCR rule, what happened, the sizes at each step)"""
    seen, sizes = {}, []
    W, H = clean.size
    seen["rotate"] = rng.random() < 0.7
    if seen["rotate"]:
        text_img = text_img.rotate(rng.uniform(-45, 45), expand=True, fillcolor=(0, 0, 0, 0))
        sizes.append(text_img.size)
    seen["scale"] = rng.random() < 0.6
    if seen["scale"]:
        sx, sy = rng.uniform(0.8, 1.4), rng.uniform(0.8, 1.4)
        text_img = text_img.resize((int(text_img.width * sx), int(text_img.height * sy)), Image.Resampling.LANCZOS)
        sizes.append(text_img.size)
    seen["blur"] = rng.random() < 0.3
    if seen["blur"]:
        text_img = text_img.filter(ImageFilter.GaussianBlur(radius=rng.uniform(0.5, 1.5)))
    alpha = rng.uniform(0.1, 0.5) if transparent else rng.uniform(0.3, 0.8)
    seen["brightness"] = rng.random() < 0.5
    if seen["brightness"]:
        text_img = ImageEnhance.Brightness(text_img).enhance(rng.uniform(0.6, 1.4))
    seen["contrast"] = rng.random() < 0.5
    if seen["contrast"]:
        text_img = ImageEnhance.Contrast(text_img).enhance(rng.uniform(0.7, 1.3))
    a = np.array(text_img)
    a[:, :, 3] = (a[:, :, 3] * alpha).astype(np.uint8)
    text_img = Image.fromarray(a)
    seen["fit_width"] = text_img.width > W * 0.8
    if seen["fit_width"]:
        s = (W * 0.8) / text_img.width
        text_img = text_img.resize((int(text_img.width * s), int(text_img.height * s)), Image.Resampling.LANCZOS)
        sizes.append(text_img.size)
    seen["fit_height"] = text_img.height > H * 0.8
    if seen["fit_height"]:
        s = (H * 0.8) / text_img.height
        text_img = text_img.resize((int(text_img.width * s), int(text_img.height * s)), Image.Resampling.LANCZOS)
        sizes.append(text_img.size)
    seen["fit_third"] = W - text_img.width <= 0 or H - text_img.height <= 0
    if seen["fit_third"]:
        s = min(W / text_img.width, H / text_img.height) * 0.8
        text_img = text_img.resize((int(text_img.width * s), int(text_img.height * s)), Image.Resampling.LANCZOS)
        sizes.append(text_img.size)
    x, y = rng.randint(0, max(0, W - text_img.width)), rng.randint(0, max(0, H - text_img.height))
    out = clean.copy()
    out.paste(text_img, (x, y), text_img)
    mask = Image.new("L", clean.size, 0)
    mask.paste(text_img.split()[3], (x, y), text_img.split()[3])
    return out, mask, seen, sizes


def job_sizes(job):
    s = [(int(job["w2"]), int(job["h2"]))] if job["rotate"] else []
    s += [(int(job["w3"]), int(job["h3"]))] if job["scale"] else []
    return s + [tuple(int(v) for v in f) for f in job["fit"][:int(job["nfit"])]]


@needs_freetype
def test_chain_equals_the_literal_pillow_chain(D, fonts):
    """32 seeded jobs on the four image sizes, font sizes 20..24: the job record that sample_text_job draws, run through the
    restatement, gives Pillow's image and mask; the sizes it derived are the sizes Pillow reports at each step.  Every effect is
    seen on and off, and the fit-width, the fit-height and the both-in-a-row branches are seen.  The script's third rescale ("no room
    left") cannot be reached from its own arithmetic — after the two fits the patch is at most 0.8 of each side — so no seed shows
    it; test_three_fit_resizes_equal_pillow covers stage G at three resizes with a job built by hand."""
    tally = {}
    both = 0
    for n, (W, H) in enumerate(IMAGE_SIZES):
        clean = np.random.default_rng(100 + n).integers(0, 256, (H, W, 3), dtype=np.uint8)
        for seed in range(8):
            rng_a, rng_b = random.Random(f"chain:{n}:{seed}"), random.Random(f"chain:{n}:{seed}")
            text, size = TEXTS[(n + seed) % len(TEXTS)], 20 + (seed + n) % 5
            font = fonts.font(0, size)
            plane = D.render_text_plane(text, font)
            job = D.sample_text_job(rng_a, (W, H), (plane.shape[1], plane.shape[0]), enhance_transparent=bool(seed % 2))
            assert job is not None and job["enabled"] == 1
            # the literal chain: the script's canvas, drawn by ImageDraw, the ink being the script's first draw of this part
            ink = rng_b.choice(D.TEXT_INKS)
            assert tuple(int(v) for v in job["ink"]) == ink
            canvas = Image.new("RGBA", (plane.shape[1], plane.shape[0]), (0, 0, 0, 0))
            ImageDraw.Draw(canvas).text((20, 20), text, font=font, fill=ink + (255,))
            want, want_mask, seen, sizes = pillow_chain(rng_b, Image.fromarray(clean), canvas, bool(seed % 2))
            assert rng_a.getstate() == rng_b.getstate(), "the same draws in the same order"
            assert job_sizes(job) == sizes, (n, seed)
            assert D.text_job_final_size(job, (plane.shape[1], plane.shape[0])) == (sizes[-1] if sizes else canvas.size)
            got, got_mask = T.synth_text_image(clean, np.zeros((H, W), np.uint8), [plane], [job], mask_mode=0)
            assert np.array_equal(got, np.asarray(want)), (n, seed, seen)
            assert np.array_equal(got_mask, np.asarray(want_mask)), (n, seed, seen)
            for k, v in seen.items():
                tally.setdefault(k, set()).add(bool(v))
            both += int(seen["fit_width"] and seen["fit_height"])
    for k in ("rotate", "scale", "blur", "brightness", "contrast", "fit_width", "fit_height"):
        assert tally[k] == {False, True}, (k, tally)
    assert both >= 1 and tally["fit_third"] == {False}


@needs_freetype
def test_three_fit_resizes_equal_pillow(D, fonts):
    """stage G at its full length: three LANCZOS resizes after the opacity step, one of them to the size the patch already has
    (Pillow's copy, not a resample round trip), and a result one pixel wide"""
    font = fonts.font(0, 24)
    plane = D.render_text_plane("Proof №7", font)
    cw, ch = plane.shape[1], plane.shape[0]
    for fits in ([(70, 33), (70, 33), (41, 20)], [(cw, 30), (1, 30), (1, 9)], [(cw, ch), (50, ch), (50, 21)]):
        job = D.empty_text_jobs(1)[0]
        job["enabled"], job["ink"], job["nfit"], job["x"], job["y"] = 1, (0, 255, 255), 3, 5, 7
        job["opacity"] = D.synth_opacity_lut(0.62)
        job["fit"] = fits
        canvas = Image.new("RGBA", (cw, ch), (0, 0, 0, 0))
        ImageDraw.Draw(canvas).text((20, 20), "Proof №7", font=font, fill=(0, 255, 255, 255))
        a = np.array(canvas)
        a[:, :, 3] = (a[:, :, 3] * 0.62).astype(np.uint8)
        img = Image.fromarray(a)
        for size in fits:
            img = img.resize(size, Image.Resampling.LANCZOS)
        assert np.array_equal(T.job_patch(plane, job), np.asarray(img)), fits
        assert D.text_job_needs(np.array([job]), np.array([(0, ch, cw)], D.DESC_DTYPE))[0] >= cw * ch


# ------------------------------------------------------------------------------------------------ the mask modes
def test_halving_is_blend_at_a_half():
    m = np.arange(256, dtype=np.uint8).reshape(16, 16)
    zero = Image.new("L", (16, 16), 0)
    want = Image.blend(zero.convert("RGB"), Image.fromarray(m).convert("RGB"), 0.5).convert("L")
    assert np.array_equal(T.halve(m), np.asarray(want))


def test_mask_modes_equal_pillow(D):
    rng = np.random.default_rng(7)
    H, W = 40, 56
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    logo_mask = rng.integers(0, 256, (H, W), dtype=np.uint8); logo_mask[:10] = 0
    planes = [rng.integers(0, 256, (18, 30), dtype=np.uint8), rng.integers(0, 256, (25, 12), dtype=np.uint8)]
    jobs = D.empty_text_jobs(2)
    for k, (x, y) in enumerate([(4, 6), (20, 1)]):                           # the two texts overlap; the second overhangs nothing
        jobs[k]["enabled"], jobs[k]["glyph"], jobs[k]["ink"], jobs[k]["x"], jobs[k]["y"] = 1, k, (255, 0, 0), x, y
        jobs[k]["opacity"] = D.synth_opacity_lut(0.7)
    patches = [Image.fromarray(T.job_patch(planes[k], jobs[k])) for k in range(2)]
    # mode 0: mask.paste(alpha, (x, y), alpha) over what the plane holds
    want_img, want0 = Image.fromarray(image), Image.fromarray(logo_mask)
    text_mask = Image.new("L", (W, H), 0)
    for k, p in enumerate(patches):
        at = (int(jobs[k]["x"]), int(jobs[k]["y"]))
        want_img.paste(p, at, p); want0.paste(p.split()[3], at, p.split()[3]); text_mask.paste(p.split()[3], at, p.split()[3])
    got_img, got0 = T.synth_text_image(image, logo_mask, planes, jobs, mask_mode=0)
    assert np.array_equal(got_img, np.asarray(want_img)) and np.array_equal(got0, np.asarray(want0))
    # mode 1: generate_mixed_watermark — the logos' mask blended at a half with black, then the maximum with the text's mask
    halved = Image.blend(Image.new("L", (W, H), 0).convert("RGB"), Image.fromarray(logo_mask).convert("RGB"), 0.5).convert("L")
    want1 = np.maximum(np.asarray(halved), np.asarray(text_mask))
    got_img1, got1 = T.synth_text_image(image, logo_mask, planes, jobs, mask_mode=1)
    assert np.array_equal(got_img1, got_img) and np.array_equal(got1, want1)
    assert not np.array_equal(got1, got0) and (got1[:10] == np.asarray(text_mask)[:10]).all()
    # an image without a text that runs keeps its mask in either mode
    off = jobs.copy(); off["enabled"] = 0
    for mode in (0, 1):
        i, m = T.synth_text_image(image, logo_mask, planes, off, mask_mode=mode)
        assert np.array_equal(i, image) and np.array_equal(m, logo_mask)


# ------------------------------------------------------------------------------------------------ the sampler and the dataset
def test_sample_synth_kind(D):
    rng = random.Random(5)
    state = rng.getstate()
    assert D.sample_synth_kind(rng, 0.0, 0.0) == "logo" and rng.getstate() == state, "no number is drawn at ratios 0"
    kinds = [D.sample_synth_kind(random.Random(s), 0.3, 0.2) for s in range(2000)]
    share = {k: kinds.count(k) / 2000 for k in D.SYNTH_KINDS}
    assert abs(share["text"] - 0.3) < 0.04 and abs(share["mixed"] - 0.2) < 0.04 and abs(share["logo"] - 0.5) < 0.04
    for s in range(50):                                                       # one draw, the script's two comparisons
        r = random.Random(s).random()
        assert D.sample_synth_kind(random.Random(s), 0.3, 0.2) == ("text" if r < 0.3 else "mixed" if r < 0.5 else "logo")
    assert all(D.sample_synth_kind(random.Random(s), 1.0, 0.0) == "text" for s in range(20))


def test_texts_and_fonts(D, tmp_path):
    assert D.load_texts() is D.DEFAULT_TEXTS and all(len(c) >= 1 for c in D.DEFAULT_TEXTS)
    kinds = "".join(t for c in D.DEFAULT_TEXTS for t in c)
    assert D.has_cjk(kinds) and "©" in kinds and "www." in kinds
    f = tmp_path / "texts.txt"
    f.write_text("ALPHA\n  beta gamma \n\n\n水印\n", encoding="utf-8")
    assert D.load_texts(str(f)) == (("ALPHA", "beta gamma"), ("水印",))
    assert D.sample_text(random.Random(1), (("only",),)) == "only"
    (tmp_path / "empty.txt").write_text("\n\n")
    with pytest.raises(ValueError, match="holds no text"):
        D.load_texts(str(tmp_path / "empty.txt"))
    with pytest.raises(ValueError, match="fonts directory not found"):
        D.FontSet(str(tmp_path / "nowhere"))
    with pytest.raises(ValueError, match="no .ttf"):
        D.FontSet(str(tmp_path))
    for W, H in IMAGE_SIZES + [(1280, 720)]:
        sizes = [D.sample_font_size(random.Random(s), (W, H)) for s in range(200)]
        assert min(sizes) >= max(20, int(min(W, H) * 0.03)) and max(sizes) <= max(60, int(min(W, H) * 0.15))


@needs_freetype
def test_font_probe_and_empty_text(D, fonts):
    assert fonts.paths == [None] and fonts.select("STOCK") == 0 and fonts.accepts(0, "STOCK") and not fonts.accepts(0, "")
    assert fonts.font(0, 24).layout_engine == 0                                   # ImageFont.Layout.BASIC
    plane = D.render_text_plane("", fonts.font(0, 50))
    job = D.sample_text_job(random.Random(2), (96, 64), (40, 40))
    image = np.full((64, 96, 3), 77, np.uint8)
    got, mask = T.synth_text_image(image, np.zeros((64, 96), np.uint8), [plane], [job])
    assert np.array_equal(got, image) and not mask.any(), "an empty text changes nothing"


def test_a_size_of_zero_drops_the_job(D):
    assert all(D.sample_text_job(random.Random(s), (1, 1), (50, 45)) is None for s in range(20))      # int(0.8 * 1) = 0
    assert D.sample_text_job(random.Random(0), (200, 120), (60, 45)) is not None


def _dataset(root, rng):
    os.makedirs(f"{root}/clean"); os.makedirs(f"{root}/logos")
    for i, (W, H) in enumerate(IMAGE_SIZES):
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(f"{root}/clean/im{i}.png")
    for i, (h, w) in enumerate([(20, 30), (16, 16), (24, 12)]):
        a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8); a[2:-2, 2:-2, 3] = 255
        Image.fromarray(a, "RGBA").save(f"{root}/logos/l{i}.png")
    return f"{root}/clean", f"{root}/logos"


def test_dataset_at_ratios_zero_is_todays(D, tmp_path):
    """32 (epoch, index) pairs: the three-tuple of today's call sequence, value for value"""
    clean_dir, logos_dir = _dataset(str(tmp_path), np.random.default_rng(11))
    ds = D.RawSynthDataset(clean_dir, logos_dir, seed=9)
    assert not ds.with_text
    for epoch in range(8):
        ds.set_epoch(epoch)
        for i in range(4):
            item = ds[i]
            assert isinstance(item, tuple) and len(item) == 3
            clean, logos, jobs = item
            rng = random.Random(f"uwm-synth:9:{epoch}:{i}")
            transparent, picked = D.sample_synth_choice(rng, 3, 0.6, 0.4, 3)
            want_logos = [np.asarray(Image.open(ds.logos[k]).convert("RGBA")) for k in picked]
            want = D.sample_synth_jobs(rng, (clean.shape[1], clean.shape[0]), [(a.shape[1], a.shape[0]) for a in want_logos], transparent)
            assert jobs.dtype == D.SYNTH_JOB_DTYPE and jobs.tobytes() == want.tobytes(), (epoch, i)
            assert len(logos) == len(want_logos) and all(np.array_equal(a, b) for a, b in zip(logos, want_logos))
            assert ds.draw(i, (clean.shape[1], clean.shape[0]))[:2] == (transparent, picked)


@needs_freetype
def test_dataset_with_text_is_a_function_of_seed_epoch_index(D, tmp_path):
    clean_dir, logos_dir = _dataset(str(tmp_path), np.random.default_rng(12))
    kw = dict(seed=4, text_watermark_ratio=0.4, mixed_watermark_ratio=0.3)
    a, b = D.RawSynthDataset(clean_dir, logos_dir, **kw), D.RawSynthDataset(clean_dir, logos_dir, **kw)
    kinds = set()
    for epoch in range(6):
        a.set_epoch(epoch); b.set_epoch(epoch)
        for i in range(4):
            x, y = a[i], b[i]
            assert len(x) == 5 and x[4].dtype == D.TEXT_JOB_DTYPE and x[4].shape == (1,)
            assert x[2].tobytes() == y[2].tobytes() and x[4].tobytes() == y[4].tobytes()
            assert len(x[3]) == len(y[3]) and all(np.array_equal(p, q) for p, q in zip(x[3], y[3]))
            kind = a.draw_sample(i, (x[0].shape[1], x[0].shape[0]))[4]
            kinds.add(kind)
            assert (len(x[3]) == 1) == (kind != "logo") and (len(x[1]) == 0) == (kind == "text")
            assert bool(x[2]["enabled"].any()) <= (kind != "text") and bool(x[4]["enabled"].any()) <= (kind != "logo")
            if kind == "mixed":
                assert 1 <= len(x[1]) <= 2
    assert kinds == set(D.SYNTH_KINDS)
    a.set_epoch(0); first = a[0]
    a.set_epoch(1); second = a[0]
    assert first[2].tobytes() != second[2].tobytes() or first[4].tobytes() != second[4].tobytes()
    only_text = D.RawSynthDataset(clean_dir, None, text_watermark_ratio=1.0)                  # no logos needed
    assert all(len(only_text[i][1]) == 0 and len(only_text[i][3]) == 1 for i in range(4))
    with pytest.raises(ValueError, match="need both"):
        D.RawSynthDataset(clean_dir, None, text_watermark_ratio=0.9)
    for t, m in [(-0.1, 0), (0.5, 1.1), (0.7, 0.4), (float("nan"), 0)]:
        with pytest.raises(ValueError, match="sum to at most 1"):
            D.RawSynthDataset(clean_dir, logos_dir, text_watermark_ratio=t, mixed_watermark_ratio=m)


# ------------------------------------------------------------------------------------------------ the library and the refusals
def test_abi_symbols_and_job_layout(D):
    from unet_watermark_amd import _lib as L
    lib = L.lib()
    for name in ("uwm_synth_text_workspace_bytes", "uwm_synth_text_u8", "uwm_op_text_patches"):
        assert name in L.SIGNATURES and getattr(lib, name) is not None
    assert "synth_text_u8.hip" in L.SOURCES and L.EXTRA_FLAGS["synth_text_u8.hip"] == ["-ffp-contract=off"]
    f = D.TEXT_JOB_DTYPE.fields
    assert D.TEXT_JOB_DTYPE.itemsize == 416 and f["ink"][1] == 8 and f["fit"][1] == 80 and f["x"][1] == 104 and f["rot"][1] == 112 and f["opacity"][1] == 160
    assert D.SYNTH_JOB_DTYPE.itemsize == 488                                          # the logo record is untouched
    assert lib.uwm_synth_text_workspace_bytes(2, 3, 1000, 50) == 6 * (8 * 1000 + 32 * 50 + 8 * 32)
    for bad in [(0, 1, 10, 10), (1, 9, 10, 10), (1, 1, 0, 10), (1, 1, 10, 0), (1, 1, (1 << 26) + 1, 10)]:
        assert lib.uwm_synth_text_workspace_bytes(*bad) == 0 and b"uwm_synth_text_workspace_bytes" in lib.uwm_last_error()


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """(the pointers are host memory that is never dereferenced: every call here must be refused)"""
    from unet_watermark_amd import _lib as L
    lib = L.lib()
    buf = (C.c_uint8 * 4096)()
    p = C.c_void_p(C.addressof(buf) // 8 * 8 + 8)
    odd = C.c_void_p(p.value + 2)
    need = int(lib.uwm_synth_text_workspace_bytes(1, 1, 16, 16))
    good = [p, 64, p, None, 0, None, 0, p, 64, p, 1, p, 1, 1, 16, 16, p, need, None]

    def refused(i, v):
        a = list(good); a[i] = v
        return lib.uwm_synth_text_u8(*a) != 0 and b"uwm_synth_text_u8" in lib.uwm_last_error()

    assert all(refused(i, None) for i in (0, 2, 7, 9, 11, 16))
    assert refused(6, 2) and refused(7, odd) and refused(2, odd) and refused(10, 0) and refused(8, 0) and refused(12, 0) and refused(13, 9)
    assert refused(14, 0) and refused(15, 0) and refused(17, need - 1) and refused(3, p)       # (masks without mask_descs)
    goodp = [p, 64, p, 1, p, 1, 16, 16, p, need, p, 64, None]
    for i, v in [(0, None), (10, None), (10, odd), (11, 63), (9, need - 1), (5, 0), (3, 0)]:
        a = list(goodp); a[i] = v
        assert lib.uwm_op_text_patches(*a) != 0 and b"uwm_op_text_patches" in lib.uwm_last_error(), i


def test_device_synth_text_refusals(D):
    pi, di, _ = D.pack_images([np.zeros((8, 9, 3), np.uint8), np.zeros((5, 5, 3), np.uint8)])
    pp, dp, _ = D.pack_images([np.zeros((4, 6, 1), np.uint8)])
    jobs = D.empty_text_jobs(2, 2)
    with pytest.raises(ValueError, match=r"\(N, K\)"):
        D.device_synth_text(pi, di, pp, dp, jobs[:1])
    with pytest.raises(ValueError, match=r"\(N, K\)"):
        D.device_synth_text(pi, di, pp, dp, D.empty_synth_jobs(2, 2))
    with pytest.raises(ValueError, match="DESC_DTYPE"):
        D.device_synth_text(pi, di, pp, dp[:0], jobs)
    with pytest.raises(ValueError, match="mask_mode"):
        D.device_synth_text(pi, di, pp, dp, jobs, mask_mode=2)
    bad = jobs.copy(); bad["enabled"][1, 1] = 1; bad["glyph"][1, 1] = 1
    with pytest.raises(ValueError, match="names a plane"):
        D.device_synth_text(pi, di, pp, dp, bad)
    bad = jobs.copy(); bad["enabled"][0, 0] = 1; bad["nfit"][0, 0] = 4
    with pytest.raises(ValueError, match="nfit"):
        D.device_synth_text(pi, di, pp, dp, bad)
    with pytest.raises(RuntimeError, match="masks must be"):
        D.device_synth_text(pi, di, pp, dp, jobs, masks=torch.zeros(10, dtype=torch.uint8))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            D.device_synth_text(pi, di, pp, dp, jobs)


def test_command_line_flags_and_refusals(D, tmp_path):
    from unet_watermark_amd import cli
    ap = cli.build_parser()
    for cmd in (["train"], ["synth", "--clean-dir", "c", "--output-dir", "o", "--count", "1"]):
        a = ap.parse_args(cmd)
        assert (a.text_watermark_ratio, a.mixed_watermark_ratio, a.fonts_dir, a.texts_file) == (0.0, 0.0, None, None)
    clean_dir, logos_dir = _dataset(str(tmp_path), np.random.default_rng(13))
    synth = ["synth", "--clean-dir", clean_dir, "--output-dir", str(tmp_path / "out"), "--count", "2"]
    train = ["train", "--synthesize", "--augment", "basic", "--clean-dir", clean_dir]
    for base in (synth, train):
        for t, m in [("1.5", "0"), ("-0.1", "0"), ("0.6", "0.6"), ("0", "1.01")]:
            with pytest.raises(ValueError, match="sum to at most 1"):
                cli.main(base + ["--logos-dir", logos_dir, "--text-watermark-ratio", t, "--mixed-watermark-ratio", m])
        with pytest.raises(ValueError, match="--logos-dir"):                       # a mixed sample needs logos
            cli.main(base + ["--text-watermark-ratio", "0.5", "--mixed-watermark-ratio", "0.25"])
        with pytest.raises(ValueError, match="--logos-dir"):
            cli.main(base)
    with pytest.raises(ValueError, match="fonts directory not found"):
        cli.main(synth + ["--text-watermark-ratio", "1", "--fonts-dir", str(tmp_path / "nofonts")])
    assert not os.path.exists(tmp_path / "out"), "refused before anything was written"
