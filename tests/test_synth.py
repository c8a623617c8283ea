"""Logo-watermark synthesis without a device: the numpy restatement (tests/synth_ref.py) against Pillow itself, bit for bit, for
every stage that is Pillow code (resize, rotate, blur, enhance, opacity, paste) and for the chain without shear; the host sampler's
invariants; the refusals of device_synth, of the C entry points (before any launch) and of the command line.  Every comparison is
exact.  The shear stage restates cv2.warpAffine from knowledge and is NOT run against cv2 (cv2 is not a dependency)."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_ref as S  # noqa: E402


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from unet_watermark_amd import _lib
    _lib.lib()
    return _lib


def rgba(rng, h, w):
    """random RGBA with alpha planes that hold 0, 255 and values between"""
    p = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    u = rng.random((h, w))
    p[..., 3][u < 0.25] = 0
    p[..., 3][u > 0.75] = 255
    return p


# ------------------------------------------------------------------------------------------------ the stages against Pillow
@pytest.mark.parametrize("H,W,w,h", [(37, 53, 11, 7), (40, 64, 90, 23), (128, 200, 31, 19), (17, 9, 9, 30), (20, 20, 20, 31), (20, 20, 7, 20),
                                     (12, 15, 15, 12)])
def test_resize_equals_pillow(H, W, w, h):
    Image = pytest.importorskip("PIL.Image")
    p = rgba(np.random.default_rng(H * W + w), H, W)
    assert set(np.unique(p[..., 3])) >= {0, 255} and len(np.unique(p[..., 3])) > 2
    want = np.asarray(Image.fromarray(p, "RGBA").resize((w, h), Image.Resampling.LANCZOS))
    assert np.array_equal(S.resize_rgba(p, w, h), want)


@pytest.mark.parametrize("H,W", [(13, 29), (9, 9), (30, 12)])
@pytest.mark.parametrize("angle", [0, 37.3, 45, 90, 123.456, 180, 301, 359.2])
def test_rotate_equals_pillow(H, W, angle):
    Image = pytest.importorskip("PIL.Image")
    p = rgba(np.random.default_rng(H + W), H, W)
    want = np.asarray(Image.fromarray(p, "RGBA").rotate(angle, expand=True, fillcolor=(0, 0, 0, 0)))
    if angle % 360 == 0:
        got = p                                               # the identity: the sampler leaves the stage off
    else:
        got = S.rotate_nearest(p, *S.rotate_setup(W, H, angle))
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("H,W", [(3, 4), (21, 33), (40, 5)])
@pytest.mark.parametrize("radius", [0.5, 1.3, 2.5])
def test_blur_equals_pillow(H, W, radius):
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageFilter
    p = rgba(np.random.default_rng(H * 7 + W), H, W)
    want = np.asarray(Image.fromarray(p, "RGBA").filter(ImageFilter.GaussianBlur(radius=radius)))
    assert np.array_equal(S.gaussian_blur(p, *S.blur_params(radius)), want)


@pytest.mark.parametrize("f", [0.4, 0.77, 1.0, 1.3, 1.8])
def test_enhance_equals_pillow(f):
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageEnhance
    p = rgba(np.random.default_rng(5), 19, 23)
    im = Image.fromarray(p, "RGBA")
    assert np.array_equal(S.brightness(p, f), np.asarray(ImageEnhance.Brightness(im).enhance(f)))
    assert np.array_equal(S.contrast(p, f), np.asarray(ImageEnhance.Contrast(im).enhance(f)))
    assert np.array_equal(S.color(p, f), np.asarray(ImageEnhance.Color(im).enhance(f)))


def test_contrast_mean_that_lands_on_a_half():
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageEnhance
    p = np.zeros((1, 2, 4), np.uint8)
    p[0, 0] = (10, 10, 10, 0); p[0, 1] = (11, 11, 11, 200)     # L = 10 and 11: mean 10.5 -> 11, the transparent pixel included
    assert S.luma(p).tolist() == [[10, 11]] and S.contrast_mean(p) == 11
    for f in (0.5, 1.6):
        assert np.array_equal(S.contrast(p, f), np.asarray(ImageEnhance.Contrast(Image.fromarray(p, "RGBA")).enhance(f)))


@pytest.mark.parametrize("alpha", [0.08, 0.3, 0.45, 0.85])
def test_opacity_equals_the_scripts_numpy_line(alpha):
    p = rgba(np.random.default_rng(6), 9, 11)
    want = p.copy(); want[:, :, 3] = (want[:, :, 3] * alpha).astype(np.uint8)
    assert np.array_equal(S.opacity(p, S.opacity_lut(alpha)), want)


def _pil_paste(img, patches):
    from PIL import Image
    base = Image.fromarray(img.copy(), "RGB"); m = Image.new("L", base.size, 0)
    for p, x, y in patches:
        pim = Image.fromarray(p, "RGBA"); al = pim.split()[3]
        m.paste(al, (x, y), al); base.paste(pim, (x, y), pim)
    return np.asarray(base), np.asarray(m)


def test_paste_equals_pillow():
    pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)
    a, b = rgba(rng, 19, 23), rgba(rng, 12, 30)
    cases = [[(a, 0, 0)], [(a, 50 - 23, 40 - 19)], [(a, 40, 30)], [(a, 10, 5), (b, 20, 12)], [(b, 20, 12), (a, 10, 5)]]
    for patches in cases:                                      # origin, far corner, overhanging right and bottom, two overlapping in both orders
        gi, gm = img.copy(), np.zeros((40, 50), np.uint8)
        for p, x, y in patches:
            S.paste(gi, gm, p, x, y)
        wi, wm = _pil_paste(img, patches)
        assert np.array_equal(gi, wi) and np.array_equal(gm, wm)


def _job(**kw):
    from unet_watermark_amd import data as D
    j = D.empty_synth_jobs(1)
    j["enabled"] = 1
    for k, v in kw.items():
        j[k][0] = v
    return j[0]


def test_chain_without_shear_equals_pillow():
    """apply_watermark_effects with fixed parameters, shear left out, and the two pastes, in Pillow and in the restatement"""
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageEnhance, ImageFilter
    from unet_watermark_amd import data as D
    rng = np.random.default_rng(8)
    logo = rgba(rng, 40, 64)
    img = rng.integers(0, 256, (61, 80, 3), dtype=np.uint8)
    angle, radius, alpha, (fb, fc, fs) = 123.456, 1.3, 0.6, (1.4, 0.7, 1.2)
    m, w2, h2 = D.synth_rotate_setup(30, 19, angle)
    w3, h3 = int(w2 * 0.8), int(h2 * 1.3)
    defects = np.zeros((3, 4), np.int32); defects[0] = (2, 3, 5, 4); defects[1] = (w3 - 3, h3 - 2, 3, 2)
    j = _job(w1=30, h1=19, rotate=1, rot=m, w2=w2, h2=h2, stretch=1, w3=w3, h3=h3, blur=1, ndefects=2, defects=defects, enhance=1,
             brightness=fb, contrast=fc, color=fs, opacity=D.synth_opacity_lut(alpha), x=55, y=40)
    j["blur_r"], j["blur_ww"], j["blur_fw"] = D.synth_blur_params(radius)
    wm = Image.fromarray(logo, "RGBA").resize((30, 19), Image.Resampling.LANCZOS).rotate(angle, expand=True, fillcolor=(0, 0, 0, 0))
    assert wm.size == (w2, h2)
    wm = wm.resize((w3, h3), Image.Resampling.LANCZOS).filter(ImageFilter.GaussianBlur(radius=radius))
    arr = np.array(wm)
    for x, y, dw, dh in defects[:2]:
        arr[y:y + dh, x:x + dw, 3] = 0
    wm = Image.fromarray(arr)
    wm = ImageEnhance.Color(ImageEnhance.Contrast(ImageEnhance.Brightness(wm).enhance(fb)).enhance(fc)).enhance(fs)
    arr = np.array(wm); arr[:, :, 3] = (arr[:, :, 3] * alpha).astype(np.uint8)
    assert np.array_equal(S.job_patch(logo, j), arr)
    want_img, want_mask = _pil_paste(img, [(arr, 55, 40)])                 # overhangs the right and bottom edges
    got_img, got_mask = S.synth_image(img, [logo], [j])
    assert np.array_equal(got_img, want_img) and np.array_equal(got_mask, want_mask) and got_mask.any()


def test_lanczos_table_rows():
    """the identity-scale table is the unit tap; a table's rows sum to 2^22 within rounding; taps stay inside the source"""
    t = S.lanczos_table(9, 9)
    assert t.shape == (9, 2 + 7)
    for (i, o) in [(53, 11), (64, 90), (200, 31), (9, 30)]:
        t = S.lanczos_table(i, o)
        assert t.shape == (o, 2 + S.lanczos_ksize(i, o))
        assert (t[:, 0] >= 0).all() and (t[:, 0] + t[:, 1] <= i).all() and (t[:, 1] <= t.shape[1] - 2).all()
        assert np.abs(t[:, 2:].sum(1) - (1 << 22)).max() <= t.shape[1]


def test_shear_is_the_identity_at_zero_and_reads_zero_outside():
    p = rgba(np.random.default_rng(9), 11, 14)
    assert np.array_equal(S.shear(p, S.shear_inverse(0.0, 0.0)), p)
    out = S.shear(np.full((8, 8, 4), 200, np.uint8), S.shear_inverse(0.4, -0.4))
    assert out.min() == 0 and out.max() == 200                              # BORDER_CONSTANT 0, not a reflection


# ------------------------------------------------------------------------------------------------ the host sampler
def test_host_helpers_equal_the_restatement():
    from unet_watermark_amd import data as D
    for w, h, a in [(29, 13, 37.3), (9, 9, 45.0), (12, 30, 301.0), (5, 70, 90.0)]:
        assert D.synth_rotate_setup(w, h, a) == S.rotate_setup(w, h, a)
    for r in (0.5, 0.9, 1.3, 2.0, 2.5):
        assert D.synth_blur_params(r) == S.blur_params(r)
    assert D.synth_shear_inverse(0.31, -0.12) == S.shear_inverse(0.31, -0.12)
    assert np.array_equal(D.synth_opacity_lut(0.37), S.opacity_lut(0.37))


def test_sampler_invariants():
    Image = pytest.importorskip("PIL.Image")
    from unet_watermark_amd import data as D
    rng = random.Random(11)
    seen = dict(rotate=0, stretch=0, shear=0, blur=0, defects=0, plain=0, multi=0, dropped=0)
    for trial in range(600):
        W, H = rng.randint(40, 700), rng.randint(40, 500)
        sizes = [(rng.randint(8, 300), rng.randint(8, 300)) for _ in range(rng.randint(1, 3))]
        transparent = trial % 2 == 0
        jobs = D.sample_synth_jobs(rng, (W, H), sizes, transparent)
        assert jobs.shape == (D.SYNTH_SLOTS,) and jobs.dtype == D.SYNTH_JOB_DTYPE
        placed = []
        for k, j in enumerate(jobs):
            if k >= len(sizes):
                assert not j["enabled"]
                continue
            if not j["enabled"]:
                seen["dropped"] += 1
                continue
            lw, lh = sizes[k]
            w, h = int(j["w1"]), int(j["h1"])
            assert w >= 1 and h >= 1 and w <= 0.35 * W + 1 and h <= 0.35 * H + 1
            plain = not j["enhance"]
            if plain:                                           # resize_watermark(.., 0.02, 0.12): stage 1 only, opacity untouched
                seen["plain"] += 1
                assert not (j["rotate"] or j["stretch"] or j["shear"] or j["blur"] or j["ndefects"])
                assert np.array_equal(j["opacity"], np.arange(256)) and w <= 0.12 * W + 1 and h <= 0.12 * H + 1
            else:
                assert 0.4 <= j["brightness"] <= 1.8 and 0.5 <= j["contrast"] <= 1.6 and 0.5 <= j["color"] <= 1.5
                lo, hi = (0.08, 0.45) if transparent else (0.25, 0.85)
                assert int(255 * lo) <= int(j["opacity"][255]) <= int(255 * hi) and j["opacity"][0] == 0
            if j["rotate"]:
                seen["rotate"] += 1
                im = Image.new("RGBA", (w, h)).rotate(0.0 + _angle_of(j["rot"]), expand=True)
                assert im.size == (int(j["w2"]), int(j["h2"]))                   # the derived size is Pillow's
                w, h = im.size
            if j["stretch"]:
                seen["stretch"] += 1; seen["shear"] += int(j["shear"])
                assert 0.6 * w - 1 <= j["w3"] <= 1.6 * w and 0.6 * h - 1 <= j["h3"] <= 1.6 * h and j["w3"] >= 1 and j["h3"] >= 1
                w, h = int(j["w3"]), int(j["h3"])
            else:
                assert not j["shear"]
            if j["blur"]:
                seen["blur"] += 1
                assert 0 <= j["blur_r"] <= 2 and (2 * int(j["blur_r"]) + 1) * int(j["blur_ww"]) + 2 * int(j["blur_fw"]) in ((1 << 24) - 1, 1 << 24)
            assert 0 <= j["ndefects"] <= 3
            for x, y, dw, dh in j["defects"][:int(j["ndefects"])]:
                seen["defects"] += 1
                assert int(w * 0.05) <= dw <= int(w * 0.2) and int(h * 0.05) <= dh <= int(h * 0.2) and 0 <= x <= max(0, w - dw) and 0 <= y <= max(0, h - dh)
            x, y = int(j["x"]), int(j["y"])
            assert 0 <= x and 0 <= y and (x + w <= W and y + h <= H or not placed)      # (only a forced first logo may overhang)
            region = (x, y, x + w, y + h)
            for r in placed:                                                            # the 30 % rule
                ix, iy = min(region[2], r[2]) - max(region[0], r[0]), min(region[3], r[3]) - max(region[1], r[1])
                assert (ix * iy if ix > 0 and iy > 0 else 0) / (w * h) < 0.3
            placed.append(region)
        seen["multi"] += len(placed) > 1
    assert all(v > 0 for k, v in seen.items() if k != "dropped"), seen


def _angle_of(rot):
    """the angle whose Image.rotate matrix is rot (cos a, sin a with a = -radians(angle))"""
    import math
    return (-math.degrees(math.atan2(rot[1], rot[0]))) % 360.0


def test_sampler_drops_a_zero_size_job_and_falls_back_to_a_plain_job():
    from unet_watermark_amd import data as D
    # a logo 400 times as wide as high: int(lh * w / lw) is 0 at every scale -> the job is dropped, nothing is pasted
    for seed in range(20):
        jobs = D.sample_synth_jobs(random.Random(seed), (100, 100), [(4000, 10)], True)
        assert not jobs["enabled"].any()
    # a wide image and a wide logo: rotated towards 90 degrees the patch is higher than the image -> the plain fallback, which fits
    plain = 0
    for seed in range(200):
        jobs = D.sample_synth_jobs(random.Random(seed), (600, 40), [(300, 30)], False)
        j = jobs[0]
        if j["enabled"] and not j["enhance"]:
            plain += 1
            assert 1 <= j["h1"] <= int(40 * 0.12) and 1 <= j["w1"] <= 0.12 * 600 and j["x"] + j["w1"] <= 600 and j["y"] + j["h1"] <= 40
    assert plain > 0
    with pytest.raises(ValueError, match="slots"):
        D.sample_synth_jobs(random.Random(0), (100, 100), [(10, 10)] * 4, True)


def test_choice_and_dataset_are_functions_of_seed_epoch_index(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from unet_watermark_amd import data as D
    rng = np.random.default_rng(12)
    for i, (h, w) in enumerate([(40, 50), (33, 61), (64, 64)]):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(tmp_path / f"c{i}.png")
    os.makedirs(tmp_path / "logos" / "combined"); os.makedirs(tmp_path / "logos" / "car_logo"); os.makedirs(tmp_path / "flat")
    Image.fromarray(rgba(rng, 20, 30), "RGBA").save(tmp_path / "logos" / "combined" / "a.png")
    Image.fromarray(rgba(rng, 16, 16), "RGBA").save(tmp_path / "logos" / "car_logo" / "b.png")
    Image.fromarray(rgba(rng, 9, 12), "RGBA").save(tmp_path / "flat" / "f.png")
    assert [os.path.basename(p) for p in D.list_logos(str(tmp_path / "logos"))] == ["a.png", "b.png"]
    assert [os.path.basename(p) for p in D.list_logos(str(tmp_path / "flat"))] == ["f.png"]
    a, b = (D.RawSynthDataset(str(tmp_path), str(tmp_path / "logos"), seed=3, cache=1) for _ in range(2))
    assert len(a) == 3
    for i in range(3):
        ca, la, ja = a[i]; cb, lb, jb = b[i]
        assert np.array_equal(ca, cb) and ja.tobytes() == jb.tobytes() and len(la) == len(lb) and all(x.shape[2] == 4 for x in la)
    first = [a[i][2].tobytes() for i in range(3)]
    a.set_epoch(1)
    assert [a[i][2].tobytes() for i in range(3)] != first                  # a new epoch draws new samples
    a.set_epoch(0)
    assert [a[i][2].tobytes() for i in range(3)] == first
    counts = [len(D.sample_synth_choice(random.Random(s), 5)[1]) for s in range(300)]
    assert set(counts) == {1, 2, 3}
    assert all(len(D.sample_synth_choice(random.Random(s), 1)[1]) == 1 for s in range(50))
    with pytest.raises(ValueError, match="need both"):
        D.RawSynthDataset(str(tmp_path / "logos"), str(tmp_path / "logos"))
    with pytest.raises(ValueError, match="max_watermarks"):
        D.RawSynthDataset(str(tmp_path), str(tmp_path / "logos"), max_watermarks=4)


def test_job_needs_cover_every_intermediate():
    from unet_watermark_amd import data as D
    ld = np.zeros(1, D.DESC_DTYPE); ld["h"], ld["w"] = 40, 64
    j = D.empty_synth_jobs(1, 1)
    assert D.synth_job_needs(j, ld) == (1, 1)                              # nothing enabled
    j["enabled"], j["w1"], j["h1"] = 1, 90, 23
    P, T = D.synth_job_needs(j, ld)
    assert P == 90 * 40 and T == max(90 * (S.lanczos_ksize(64, 90) + 2), 23 * (S.lanczos_ksize(40, 23) + 2))
    j["rotate"], j["w2"], j["h2"], j["stretch"], j["w3"], j["h3"] = 1, 93, 93, 1, 140, 60
    P, T = D.synth_job_needs(j, ld)
    assert P == 140 * 93 and T == 140 * (S.lanczos_ksize(93, 140) + 2)


# ------------------------------------------------------------------------------------------------ refusals
def test_device_synth_refuses_on_the_host(L):
    import torch
    from unet_watermark_amd import data as D
    pi, di, _ = D.pack_images([np.zeros((8, 9, 3), np.uint8), np.zeros((5, 5, 3), np.uint8)])
    pl, dl, _ = D.pack_images([np.zeros((4, 6, 4), np.uint8)])
    jobs = D.empty_synth_jobs(2, 3)
    with pytest.raises(ValueError, match=r"\(N, K\)"):
        D.device_synth(pi, di, pl, dl, jobs[:1])
    with pytest.raises(ValueError, match=r"\(N, K\)"):
        D.device_synth(pi, di, pl, dl, D.empty_synth_jobs(2, 9))
    with pytest.raises(ValueError, match=r"\(N, K\)"):
        D.device_synth(pi, di, pl, dl, np.zeros((2, 3), np.int32))
    with pytest.raises(ValueError, match="DESC_DTYPE"):
        D.device_synth(pi, di[:0], pl, dl, jobs)
    bad = jobs.copy(); bad["enabled"][1, 2] = 1; bad["logo"][1, 2] = 1
    with pytest.raises(ValueError, match="names a logo"):
        D.device_synth(pi, di, pl, dl, bad)
    off = dl.copy(); off["offset"] = 2
    with pytest.raises(ValueError, match="multiple of 4"):
        D.device_synth(pi, di, pl, off, jobs)
    with pytest.raises(RuntimeError, match="flat uint8"):
        D.device_synth(pi.view(-1, 1), di, pl, dl, jobs)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            D.device_synth(pi, di, pl, dl, jobs)


def test_entry_points_check_arguments_before_any_launch(L):
    """nulls, counts, sizes, a workspace that is too small, misaligned pointers: every such call returns non-zero with a message and
    none reaches a launch (the pointers are host memory)"""
    lib = L.lib()
    buf = (C.c_uint8 * (1 << 16))()
    p = C.c_void_p(C.addressof(buf) + (-C.addressof(buf)) % 16)
    odd2, odd4 = C.c_void_p(p.value + 2), C.c_void_p(p.value + 4)
    need = lib.uwm_synth_workspace_bytes(2, 3, 100, 50)
    assert need == 2 * 3 * (8 * 100 + 16 * 50 + 8 * 32)
    for args in ((0, 3, 100, 50), (2, 0, 100, 50), (2, 9, 100, 50), (2, 3, 0, 50), (2, 3, 100, 0), (2, 3, 1 << 27, 50), (1 << 24, 8, 100, 50)):
        assert lib.uwm_synth_workspace_bytes(*args) == 0 and "uwm_synth_workspace_bytes" in lib.uwm_last_error().decode()
    base = dict(images=p, image_bytes=64, idesc=p, masks=p, mask_bytes=64, mdesc=p, logos=p, logo_bytes=64, ldesc=p, num_logos=1, jobs=p, N=2, K=3,
                P=100, T=50, ws=p, ws_bytes=need, st=None)

    def bad(word, **kw):
        rc = lib.uwm_synth_u8(*[kw.get(k, v) for k, v in base.items()])
        msg = lib.uwm_last_error().decode()
        assert rc != 0 and "uwm_synth_u8" in msg and word in msg, (kw, msg)

    for k in ("images", "idesc", "logos", "ldesc", "jobs", "ws"):
        bad("null", **{k: None})
    bad("mask_descs", mdesc=None); bad("mask_descs", mask_bytes=0); bad("mask_descs", mdesc=odd4)
    bad(">= 1", num_logos=0); bad(">= 1", logo_bytes=0); bad(">= 1", image_bytes=0)
    for kw in (dict(N=0), dict(K=0), dict(K=9), dict(P=0), dict(T=0), dict(N=1 << 24, K=8)):
        bad("need N >= 1", **kw)
    bad("workspace of", ws_bytes=need - 1)
    bad("aligned", logos=odd2); bad("aligned", ldesc=odd4); bad("aligned", jobs=odd4); bad("aligned", ws=odd4); bad("aligned", idesc=odd4)
    pbase = dict(logos=p, logo_bytes=64, ldesc=p, num_logos=1, jobs=p, J=6, P=100, T=50, ws=p, ws_bytes=need, out=p, out_bytes=6 * 100 * 4, st=None)
    for word, kw in (("null", dict(out=None)), ("null", dict(jobs=None)), ("aligned", dict(out=odd2)), ("out of", dict(out_bytes=6 * 100 * 4 - 1)),
                     ("workspace of", dict(ws_bytes=8)), ("need N >= 1", dict(J=0))):
        rc = lib.uwm_op_synth_patches(*[kw.get(k, v) for k, v in pbase.items()])
        assert rc != 0 and "uwm_op_synth_patches" in lib.uwm_last_error().decode() and word in lib.uwm_last_error().decode(), kw
    assert lib.uwm_lanczos_table_ints(53, 11) == 11 * (S.lanczos_ksize(53, 11) + 2) and lib.uwm_lanczos_table_ints(0, 5) == 0
    for word, a in (("null", (53, 11, None, 1000, None)), ("1..32767", (0, 11, p, 1000, None)), ("1..32767", (53, 40000, p, 10 ** 7, None)),
                    ("aligned", (53, 11, odd2, 1000, None)), ("need", (53, 11, p, 10, None))):
        assert lib.uwm_op_lanczos_table(*a) != 0 and word in lib.uwm_last_error().decode(), a


def test_parser_flags_and_refusals(tmp_path):
    from unet_watermark_amd import cli
    ap = cli.build_parser()
    a = ap.parse_args(["train", "--synthesize", "--clean-dir", "c", "--logos-dir", "l", "--augment", "basic"])
    assert (a.synthesize, a.transparent_ratio, a.multi_watermark_ratio, a.synth_max_watermarks, a.synth_mask, a.synth_seed) == (True, 0.6, 0.4, 3, "pair", 42)
    a = ap.parse_args(["train", "--synthesize", "--clean-dir", "c", "--logos-dir", "l", "--synth-mask", "alpha", "--synth-seed", "7",
                       "--transparent-ratio", "0.2", "--multi-watermark-ratio", "0.9", "--synth-max-watermarks", "2"])
    assert (a.transparent_ratio, a.multi_watermark_ratio, a.synth_max_watermarks, a.synth_mask, a.synth_seed) == (0.2, 0.9, 2, "alpha", 7)
    assert not ap.parse_args(["train"]).synthesize
    with pytest.raises(SystemExit):
        ap.parse_args(["train", "--synth-mask", "ocr"])
    s = ap.parse_args(["synth", "--clean-dir", "c", "--logos-dir", "l", "--output-dir", "o", "--count", "5", "--generate-mask", "--seed", "9"])
    assert (s.command, s.count, s.generate_mask, s.seed) == ("synth", 5, True, 9)
    with pytest.raises(SystemExit):
        ap.parse_args(["synth", "--clean-dir", "c", "--logos-dir", "l", "--count", "5"])
    common = ["train", "--synthesize", "--clean-dir", str(tmp_path), "--logos-dir", str(tmp_path)]
    with pytest.raises(ValueError, match="--augment basic or --augment config"):          # the default is --augment none
        cli.main(common)
    with pytest.raises(ValueError, match="toy generator"):
        cli.main(common + ["--augment", "basic", "--synthetic", "8"])
    with pytest.raises(ValueError, match="needs --clean-dir"):
        cli.main(["train", "--synthesize", "--augment", "basic"])
