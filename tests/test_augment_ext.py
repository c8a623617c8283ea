"""The enhanced recipe's stages, host side: properties of the rule itself (tests/augment_ext_ref.py, which csrc/augment_ext_u8.hip must
equal bit for bit — tests/test_augment_ext_gpu.py), the library's tables against the reference's, the accuracy of the integer
lightness rule, the noise distribution, and the sampler / descriptor layout / refusals of unet_watermark_amd.data.  No GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ext_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Measured on the CPU when the rule was written (see test_lightness_rule_against_float64_lab): the largest difference between the
# integer lightness rule and the float64 CIE Lab model over the 33^3 lattice was 5.95 / 9.21 / 1.95 grey levels at L8 shifts
# -40 / 0 / +40 (mean 0.20 / 0.28 / 0.22), rounded up to the next whole level.  The worst cases are saturated colours with one dark
# channel, where L8 rounds the other way in the two computations.  DESIGN.md 8e carries the same number.
LIGHTNESS_BOUND = 10.0
# 1 - the variance of the quantile table's own distribution (tails stop at +-3.4871 sigma, chords inside the cells): include/uwm.h
NOISE_VARIANCE_DEFICIT = 1.0 - 0.99908


def _data():
    from unet_watermark_amd import data
    return data


def _lib():
    import __graft_entry__ as g
    g.build()
    from unet_watermark_amd import _lib
    return _lib.lib()


def _image(h, w, c=3, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, c), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ layout
def _header_struct(name):
    text = open(os.path.join(ROOT, "include", "uwm.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = {"int": 4, "double": 8, "unsigned char": 1, "unsigned long long": 8}
    off, fields, align = 0, {}, 1
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.match(r"(unsigned long long|unsigned char|int|double)\s+(.*)", decl)
        for nm in (s.strip() for s in m.group(2).split(",")):
            cnt = re.match(r"(\w+)(?:\[(\d+)\])?$", nm)
            a = size[m.group(1)]
            off = (off + a - 1) // a * a
            fields[cnt.group(1)] = (off, a * int(cnt.group(2) or 1))
            off += a * int(cnt.group(2) or 1)
            align = max(align, a)
    return (off + align - 1) // align * align, fields


def test_ext_descriptor_layout_equals_the_header():
    D = _data()
    total, fields = _header_struct("uwm_aug_ext_desc")
    assert total == 296 == D.AUG_EXT_DTYPE.itemsize == R.EXT_DTYPE.itemsize and total % 8 == 0
    assert {k: v[0] for k, v in fields.items()} == {"tone": 0, "clahe_clip": 4, "noise_sigma": 8, "blur": 12, "blur_w": 16, "seed": 32, "lut2": 40}
    for name, (o, nbytes) in fields.items():
        for dtype in (D.AUG_EXT_DTYPE, R.EXT_DTYPE):
            dt, fo = dtype.fields[name][:2]
            assert fo == o and dt.itemsize == nbytes, name
    assert _header_struct("uwm_aug_desc")[0] == 320 == D.AUG_DESC_DTYPE.itemsize            # the basic descriptor is as it was
    e = D.identity_aug_ext_params(3)
    assert e.dtype == D.AUG_EXT_DTYPE and not e["tone"].any() and not e["noise_sigma"].any() and not e["blur"].any()
    img = _image(9, 11)
    assert np.array_equal(R.ext_stages(img, e[0]), img)


# ------------------------------------------------------------------------------------------------ gamma
def test_gamma_table_is_the_formula_and_gamma_one_is_the_identity():
    D = _data()
    assert np.array_equal(D.gamma_lut(1.0), np.arange(256))
    for g in (0.8, 0.93, 1.2):
        t = D.gamma_lut(g)
        want = [int(((i / 255.0) ** g) * 255) for i in range(256)]
        assert t.dtype == np.uint8 and t.tolist() == want and np.array_equal(t, R.gamma_lut(g))
        assert t[0] == 0 and t[255] == 255 and (np.diff(t.astype(int)) >= 0).all()
    assert (D.gamma_lut(0.8).astype(int) >= np.arange(256)).all() and (D.gamma_lut(1.2).astype(int) <= np.arange(256)).all()


# ------------------------------------------------------------------------------------------------ blur
def _all_motion_kernels():
    D = _data()
    pts = [(x, y) for y in range(3) for x in range(3)]
    return {bytes(D.motion_kernel(a, b)): (a, b) for a in pts for b in pts if a != b}


def test_gaussian_blur_equals_scipy_convolve_mirror():
    from scipy import ndimage
    w = np.outer([1, 2, 1], [1, 2, 1]).astype(np.int64)
    for h, wd, c in ((9, 13, 3), (1, 7, 1), (2, 2, 4), (5, 1, 3)):
        img = _image(h, wd, c, seed=h)
        want = np.stack([(ndimage.convolve(img[..., k].astype(np.int64), w, mode="mirror") + 8) >> 4 for k in range(c)], -1)
        assert np.array_equal(R.gaussian_blur3(img), want.astype(np.uint8)), (h, wd, c)


def test_motion_kernels_have_two_or_three_taps_and_blurs_keep_a_constant_image():
    from scipy import ndimage
    D = _data()
    kernels = _all_motion_kernels()
    assert len(kernels) > 20
    const = np.full((6, 7, 3), 93, dtype=np.uint8)
    img = _image(7, 9, 3, seed=5)
    for kb, (a, b) in kernels.items():
        k = np.frombuffer(kb, dtype=np.uint8)
        assert set(k.tolist()) <= {0, 1} and k.sum() in (2, 3), (a, b)
        assert k[3 * a[1] + a[0]] == 1 and k[3 * b[1] + b[0]] == 1
        assert np.array_equal(D.motion_kernel(a, b), R.motion_kernel(a, b)) and np.array_equal(D.motion_kernel(b, a), k)
        assert np.array_equal(R.motion_blur3(const, k), const)
        # correlation with the 0/1 taps, mean rounded half to even
        s = np.stack([ndimage.correlate(img[..., c].astype(np.int64), k.reshape(3, 3).astype(np.int64), mode="mirror") for c in range(3)], -1)
        assert np.array_equal(R.motion_blur3(img, k), np.rint(s / float(k.sum())).astype(np.uint8)), (a, b)
    assert np.array_equal(R.gaussian_blur3(const), const)
    assert D.motion_kernel((0, 0), (2, 2)).tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1] and D.motion_kernel((0, 1), (1, 1)).sum() == 2
    with pytest.raises(ValueError):
        D.motion_kernel((1, 1), (1, 1))


# ------------------------------------------------------------------------------------------------ CLAHE
def _clahe_loops(plane, clip):
    """OpenCV's CLAHE on 8 x 8 tiles with plain loops, written independently of augment_ext_ref"""
    H, W = plane.shape
    Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
    pad = np.zeros((Hp, Wp), dtype=np.int64)
    for y in range(Hp):
        for x in range(Wp):
            sy = y if y < H else 2 * (H - 1) - y
            sx = x if x < W else 2 * (W - 1) - x
            pad[y, x] = plane[sy, sx]
    th, tw = Hp // 8, Wp // 8
    scale = np.float32(255.0) / np.float32(th * tw)
    luts = [[None] * 8 for _ in range(8)]
    for ty in range(8):
        for tx in range(8):
            hist = [0] * 256
            for y in range(ty * th, (ty + 1) * th):
                for x in range(tx * tw, (tx + 1) * tw):
                    hist[pad[y, x]] += 1
            clipped = 0
            for i in range(256):
                if hist[i] > clip:
                    clipped += hist[i] - clip
                    hist[i] = clip
            batch = clipped // 256
            residual = clipped - batch * 256
            for i in range(256):
                hist[i] += batch
            if residual:
                step = max(256 // residual, 1)
                i = 0
                while i < 256 and residual > 0:
                    hist[i] += 1
                    i += step
                    residual -= 1
            lut, s = [], 0
            for i in range(256):
                s += hist[i]
                lut.append(min(max(int(np.rint(np.float32(s) * scale)), 0), 255))
            luts[ty][tx] = lut
    out = np.zeros((H, W), dtype=np.uint8)
    one = np.float32(1)
    for y in range(H):
        tyf = np.float32(y) * (one / np.float32(th)) - np.float32(0.5)
        ty1 = int(np.floor(tyf)); ya = tyf - np.float32(ty1); ya1 = one - ya
        ty2 = min(ty1 + 1, 7); ty1 = max(ty1, 0)
        for x in range(W):
            txf = np.float32(x) * (one / np.float32(tw)) - np.float32(0.5)
            tx1 = int(np.floor(txf)); xa = txf - np.float32(tx1); xa1 = one - xa
            tx2 = min(tx1 + 1, 7); tx1 = max(tx1, 0)
            v = int(plane[y, x])
            f = np.float32
            res = (f(luts[ty1][tx1][v]) * xa1 + f(luts[ty1][tx2][v]) * xa) * ya1 + (f(luts[ty2][tx1][v]) * xa1 + f(luts[ty2][tx2][v]) * xa) * ya
            out[y, x] = min(max(int(np.rint(res)), 0), 255)
    return out


@pytest.mark.parametrize("h,w,clip", [(32, 32, 1), (32, 32, 3), (20, 36, 2), (8, 8, 1), (19, 9, 1), (24, 40, 15)])
def test_clahe_equals_a_plain_loop_implementation(h, w, clip):
    plane = _image(h, w, 1, seed=h * w)[..., 0]
    plane[: h // 2, : w // 2] //= 4                                 # a dark quarter: tiles with different tables
    assert np.array_equal(R.clahe_plane(plane, clip), _clahe_loops(plane, clip))


def test_clahe_with_a_loose_clip_is_tile_histogram_equalisation_and_a_constant_plane_takes_the_residual_path():
    plane = _image(32, 48, 1, seed=2)[..., 0]
    th, tw = 4, 6
    luts = R.clahe_luts(plane, th * tw)                             # clip limit >= tileArea: nothing is clipped
    for ty in (0, 3, 7):
        for tx in (0, 5, 7):
            cdf = np.cumsum(np.bincount(plane[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].ravel(), minlength=256))
            assert np.array_equal(luts[ty, tx], np.rint(cdf.astype(np.float32) * (np.float32(255) / np.float32(th * tw))).astype(np.uint8))
    assert np.array_equal(R.clahe_luts(plane, 10 ** 6), luts)
    # a constant plane: one bin holds the tile (24), clip 1 -> excess 23 < 256 -> no batch, residual 23 at stride 11 from bin 0
    const = np.full((32, 48), 77, dtype=np.uint8)
    lut = R.clahe_luts(const, 1)[4, 4].astype(int)
    hist = np.zeros(256, dtype=int); hist[77] = 1; hist[np.arange(0, 256, 11)[:23]] += 1
    assert hist.sum() == 24 and np.array_equal(lut, np.rint(np.cumsum(hist).astype(np.float32) * (np.float32(255) / np.float32(24))).astype(int))
    out = R.clahe_plane(const, 1)
    assert (out == out[0, 0]).all() and out[0, 0] == lut[77]
    # padded size: the tables come from the reflected plane
    odd = _image(20, 36, 1, seed=3)[..., 0]
    pad = np.pad(odd, ((0, 4), (0, 4)), mode="reflect")
    assert np.array_equal(R.clahe_luts(odd, 2), R.clahe_luts(pad, 2))
    D = _data()
    assert D.clahe_clip_limit(2.0, 512, 512) == 32 and D.clahe_clip_limit(1.0, 512, 512) == 16 and D.clahe_clip_limit(2.0, 20, 36) == 1
    assert D.clahe_clip_limit(1.5, 100, 100) == max(1, int(1.5 * 13 * 13 / 256.0))


# ------------------------------------------------------------------------------------------------ lightness
def _library_tables():
    lib = _lib()
    out = []
    for which, dt in enumerate([np.int32, np.uint16, np.int32, np.uint8, np.int32]):
        d, n, b = C.c_void_p(), C.c_int(), C.c_int()
        assert lib.uwm_aug_lab_tables(which, C.byref(d), C.byref(n), C.byref(b)) == 0
        assert b.value == np.dtype(dt).itemsize
        out.append(np.frombuffer((C.c_char * (n.value * b.value)).from_address(d.value), dtype=dt).astype(np.int64))
    d, n, b = C.c_void_p(), C.c_int(), C.c_int()
    assert lib.uwm_aug_lab_tables(5, C.byref(d), C.byref(n), C.byref(b)) != 0 and b"0..4" in lib.uwm_last_error()
    return out


def test_library_tables_equal_the_reference_tables():
    lin, f, finv, gam, qn = _library_tables()
    rl, rf, rfinv, rgam = R.lab_tables()
    assert np.array_equal(lin, rl) and np.array_equal(f, rf) and np.array_equal(finv, rfinv) and np.array_equal(gam, rgam)
    assert np.array_equal(qn, R.normal_table())
    assert lin[0] == 0 and lin[255] == 16384 and f[16384] == 32768 and finv[8192] == 16384 and gam[16384] == 255 and (np.diff(gam) >= 0).all()
    assert qn[512] == 0 and np.array_equal(qn, -qn[::-1]) and (np.diff(qn) > 0).all() and abs(qn[0] / 4096.0 + 3.4871) < 1e-3
    # the equality does not hang on libm's last bit: the pow() and quantile entries are far from a rounding boundary (the cube
    # root and the linear pieces are decided by integer comparisons on both sides)
    from scipy.special import ndtri
    v = np.arange(11, 256)
    i = np.arange(52, 16385)
    for val in (16384.0 * ((v / 255.0 + 0.055) / 1.055) ** 2.4, 269.025 * (i / 16384.0) ** (1.0 / 2.4) - 14.025,
                4096.0 * ndtri(np.arange(1, 1024) / 1024.0), np.array([4096.0 * ndtri(1.0 / 4096.0)])):
        assert np.abs(val - np.floor(val) - 0.5).min() > 1e-5


def _lattice():
    g = np.rint(np.linspace(0, 255, 33)).astype(np.uint8)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def test_lightness_rule_against_float64_lab():
    lat = _lattice()
    l8 = R.rgb_to_l8(lat)
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    gl8 = R.rgb_to_l8(grey)
    assert (np.diff(gl8) >= 0).all() and gl8[0] == 0 and gl8[255] == 255
    for shift in (-40, 0, 40):
        got = R.l8_replace(lat, np.clip(l8 + shift, 0, 255)).astype(np.float64)
        d = np.abs(got - R.float_l8_shift(lat, shift))
        print("L8 shift", shift, "max", d.max(), "mean", d.mean())
        assert d.max() <= LIGHTNESS_BOUND and d.mean() < 0.5
        # greys stay grey, and where they should be
        g = R.l8_replace(grey, np.clip(gl8 + shift, 0, 255)).astype(np.float64)
        assert (g.max(1) - g.min(1)).max() <= LIGHTNESS_BOUND
        assert np.abs(g - R.float_l8_shift(grey, shift)).max() <= LIGHTNESS_BOUND
    back = R.l8_replace(grey, gl8).astype(int)
    assert (back.max(1) == back.min(1)).all() and np.abs(back[:, 0] - np.arange(256)).max() <= 1


# ------------------------------------------------------------------------------------------------ noise
def test_noise_distribution_and_determinism():
    n = 1 << 20
    sigma_q8 = int(round(np.sqrt(30.0) * 256.0))
    sigma = sigma_q8 / 256.0
    g = R.normal_q14(12345, np.arange(n, dtype=np.uint64)).astype(np.float64) * sigma_q8 / float(1 << 22)
    print("noise mean", g.mean(), "var", g.var(), "sigma^2", sigma * sigma, "max |g| / sigma", np.abs(g).max() / sigma)
    assert abs(g.mean()) <= 5 * sigma / np.sqrt(n)
    assert abs(g.var() - sigma * sigma) <= sigma * sigma * (5 * np.sqrt(2.0 / n) + NOISE_VARIANCE_DEFICIT)
    assert np.abs(g).max() <= 3.4872 * sigma                          # where the tails stop
    q = R.normal_table() / 4096.0
    a, b = q[:-1], q[1:]
    assert abs(((a * a + a * b + b * b) / 3).mean() - (1.0 - NOISE_VARIANCE_DEFICIT)) < 2e-5     # the documented variance of the table
    img = _image(16, 24, 3, seed=4)
    a1, a2, b1 = R.add_noise(img, 7, sigma_q8), R.add_noise(img, 7, sigma_q8), R.add_noise(img, 8, sigma_q8)
    assert np.array_equal(a1, a2) and not np.array_equal(a1, b1) and not np.array_equal(a1, img)
    assert np.array_equal(R.add_noise(img, 7, 0), img)
    off = R.noise_offsets(7, sigma_q8, 16, 24, 3)
    assert not np.array_equal(off[..., 0], off[..., 1])              # independent per channel
    mid = np.full((64, 64, 3), 128, dtype=np.uint8)
    assert np.array_equal(R.add_noise(mid, 9, sigma_q8).astype(int) - 128, R.noise_offsets(9, sigma_q8, 64, 64, 3))


# ------------------------------------------------------------------------------------------------ sampler
def test_enhanced_sampler_frequencies_ranges_and_identities():
    D = _data()
    n, h, w = 4000, 64, 64
    p, e = D.sample_aug_recipe(n, h, w, torch.Generator().manual_seed(0), "enhanced")
    assert p.dtype == D.AUG_DESC_DTYPE and e.dtype == D.AUG_EXT_DTYPE and len(p) == len(e) == n
    aff = (p["minv"] != np.array(D.IDENTITY_MINV)).any(1)
    lut = (p["lut"] != np.arange(256)).any(1)
    hsv = (p["hue"] != 0) | (p["sat"] != 0) | (p["val"] != 0)
    tone, noise, blur = e["tone"] != 0, e["noise_sigma"] != 0, e["blur"] != 0
    hsv_p = 0.4 * (1 - 1 / (25 * 51 * 31))
    for name, on, prob in (("hflip", (p["flags"] & 1) != 0, 0.5), ("vflip", (p["flags"] & 2) != 0, 0.2), ("rot90", (p["flags"] >> 2) != 0, 0.3),
                           ("affine", aff, 0.3), ("lut", lut, 0.6), ("hsv", hsv, hsv_p), ("tone", tone, 0.3), ("clahe", e["tone"] == 1, 0.15),
                           ("gamma", e["tone"] == 2, 0.15), ("noise", noise, 0.2), ("blur", blur, 0.15), ("motion", e["blur"] == 1, 0.075),
                           ("gauss", e["blur"] == 2, 0.075)):
        print(name, on.mean(), prob)
        assert abs(on.mean() - prob) <= 5 * np.sqrt(prob * (1 - prob) / n), (name, on.mean())
    # ranges
    assert np.abs(p["hue"]).max() == 12 and np.abs(p["sat"]).max() == 25 and np.abs(p["val"]).max() == 15
    lo, hi = D.brightness_contrast_lut(0.75, -0.25).astype(int), D.brightness_contrast_lut(1.25, 0.25).astype(int)
    t = p["lut"][lut].astype(int)
    assert (t >= np.minimum(lo, hi)[None]).all() and (t <= hi[None]).all()
    s = e["noise_sigma"][noise] / 256.0
    assert s.min() >= np.sqrt(5.0) - 1 / 256 and s.max() <= np.sqrt(30.0) + 1 / 256 and s.max() - s.min() > 2.5
    g = e["lut2"][e["tone"] == 2].astype(int)
    assert (g >= D.gamma_lut(1.2).astype(int)[None]).all() and (g <= D.gamma_lut(0.8).astype(int)[None]).all()
    taps = (e["blur_w"][e["blur"] == 1] != 0).sum(1)
    assert set(taps.tolist()) == {2, 3} and e["blur_w"].max() == 1
    assert len({bytes(k) for k in e["blur_w"][e["blur"] == 1]}) > 15
    assert (e["clahe_clip"] >= 1).all()
    _, big = D.sample_aug_recipe(n, 512, 512, torch.Generator().manual_seed(1), "enhanced")
    cl = big["clahe_clip"][big["tone"] == 1]
    assert cl.min() >= 16 and cl.max() <= 32 and cl.max() - cl.min() >= 12
    # skipped stages are exact identities
    ident = D.identity_aug_ext_params(1)[0]
    assert (e["lut2"][e["tone"] != 2] == np.arange(256)).all() and (e["clahe_clip"][e["tone"] != 1] == ident["clahe_clip"]).all()
    assert not e["seed"][~noise].any() and not e["blur_w"][e["blur"] != 1].any()
    assert (p["minv"][~aff] == np.array(D.IDENTITY_MINV)).all() and not p["hue"][~hsv].any()
    assert len(np.unique(e["seed"][noise])) == noise.sum()
    D._check_aug_params(p, n, h, w, 3)
    D._check_aug_ext_params(e, n, h, w, 3)
    # a non-square size draws no rot90
    q, _ = D.sample_aug_recipe(200, 48, 64, torch.Generator().manual_seed(0), "enhanced")
    assert not (q["flags"] >> 2).any()


def test_sampler_is_deterministic_and_basic_is_sample_aug_params():
    D = _data()
    a = D.sample_aug_recipe(64, 32, 32, torch.Generator().manual_seed(7), "enhanced")
    b = D.sample_aug_recipe(64, 32, 32, torch.Generator().manual_seed(7), "enhanced")
    c = D.sample_aug_recipe(64, 32, 32, torch.Generator().manual_seed(8), "enhanced")
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[0].tobytes() != c[0].tobytes() and a[1].tobytes() != c[1].tobytes()
    p, e = D.sample_aug_recipe(64, 32, 32, torch.Generator().manual_seed(7), "basic")
    assert e is None and p.tobytes() == D.sample_aug_params(64, 32, 32, torch.Generator().manual_seed(7)).tobytes()
    with pytest.raises(ValueError, match="transparent_watermark"):
        D.sample_aug_recipe(4, 32, 32, recipe="transparent_watermark")


# ------------------------------------------------------------------------------------------------ refusals
def test_host_refusals_need_no_device():
    D = _data()
    ok = D.identity_aug_ext_params(2)
    assert D._check_aug_ext_params(ok, 2, 8, 12, 3) is not None

    def bad(match, h=8, w=12, c=3, **kw):
        e = ok.copy()
        for k, v in kw.items():
            e[k][1] = v
        with pytest.raises(ValueError, match=match):
            D._check_aug_ext_params(e, 2, h, w, c)

    bad("1-channel or 3-channel", c=4, tone=1)
    bad("1-channel or 3-channel", c=2, tone=1)
    bad(">= 8", h=7, tone=1)
    bad(">= 8", w=5, tone=1)
    bad("clip limit", tone=1, clahe_clip=0)
    bad("empty motion kernel", blur=1)
    bad("unknown tone", tone=3)
    bad("unknown tone", tone=-1)
    bad("unknown blur", blur=3)
    bad("noise_sigma", noise_sigma=-1)
    bad("noise_sigma", noise_sigma=16384)
    with pytest.raises(ValueError, match="one descriptor per image"):
        D._check_aug_ext_params(ok, 3, 8, 12, 3)
    with pytest.raises(TypeError):
        D._check_aug_ext_params(D.identity_aug_params(2), 2, 8, 12, 3)
    e = ok.copy(); e["tone"][0] = 1; e["blur"][1] = 1; e["blur_w"][1, 4] = 1; e["tone"][1] = 2
    assert D._check_aug_ext_params(e, 2, 8, 8, 1) is not None and D._check_aug_ext_params(e, 2, 64, 8, 3) is not None
    e = ok.copy(); e["tone"][:] = 2; e["noise_sigma"][:] = 900; e["blur"][:] = 2
    assert D._check_aug_ext_params(e, 2, 1, 7, 4) is not None       # gamma, noise and blur need no minimum size or channel count
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.device_augment(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), None, D.identity_aug_params(2), ext=ok)


def test_abi_entry_checks_arguments_before_any_launch():
    """uwm_augment_u8's checks with its words, plus the workspace: null, too small, misaligned.  The pointers are host memory, so no
    launch is reached."""
    lib = _lib()
    buf = (C.c_uint8 * 8192)()
    p = C.c_void_p(C.addressof(buf) + (-C.addressof(buf)) % 16)
    odd = C.c_void_p(p.value + 4)
    mean = (C.c_float * 4)(0.5, 0.5, 0.5, 0.5); std = (C.c_float * 4)(0.25, 0.25, 0.25, 0.25); std0 = (C.c_float * 4)(0.25, 0.0, 0.25, 0.25)

    def bad(rc, word):
        assert rc != 0
        assert word in lib.uwm_last_error().decode(), lib.uwm_last_error().decode()

    need = lib.uwm_augment_ext_workspace_bytes(1, 8, 8, 3)
    assert need == 256 + 64 * 256 and lib.uwm_augment_ext_workspace_bytes(2, 20, 36, 1) == 1536 + 2 * 64 * 256
    assert lib.uwm_augment_ext_workspace_bytes(0, 8, 8, 3) == 0 and lib.uwm_augment_ext_workspace_bytes(1, 8, 8, 5) == 0
    f = lib.uwm_augment_ext_u8
    for ext in (None, p):
        bad(f(None, None, p, ext, 1, 8, 8, 3, mean, std, 127, p, need, p, None, None, None), "null")
        bad(f(p, None, None, ext, 1, 8, 8, 3, mean, std, 127, p, need, p, None, None, None), "null")
        bad(f(p, None, p, ext, 1, 8, 8, 3, mean, std, 127, p, need, None, None, None, None), "null")
        bad(f(p, None, p, ext, 1, 8, 8, 3, None, std, 127, p, need, p, None, None, None), "null")
        bad(f(p, p, p, ext, 1, 8, 8, 3, mean, std, 127, p, need, p, None, None, None), "together")
        bad(f(p, None, p, ext, 1, 8, 8, 3, mean, std, 127, p, need, p, p, None, None), "together")
        bad(f(p, None, p, ext, 1, 8, 8, 5, mean, std, 127, p, need, p, None, None, None), "1..4")
        bad(f(p, None, p, ext, 1, 0, 8, 3, mean, std, 127, p, need, p, None, None, None), ">= 1")
        bad(f(p, None, p, ext, 0, 8, 8, 3, mean, std, 127, p, need, p, None, None, None), ">= 1")
        bad(f(p, None, odd, ext, 1, 8, 8, 3, mean, std, 127, p, need, p, None, None, None), "aligned")
        bad(f(p, None, p, ext, 1, 8, 8, 3, mean, std0, 127, p, need, p, None, None, None), "positive")
    bad(f(p, None, p, odd, 1, 8, 8, 3, mean, std, 127, p, need, p, None, None, None), "aligned")
    bad(f(p, None, p, p, 1, 8, 8, 3, mean, std, 127, None, need, p, None, None, None), "null workspace")
    bad(f(p, None, p, p, 1, 8, 8, 3, mean, std, 127, p, need - 1, p, None, None, None), "too small")
    bad(f(p, None, p, p, 1, 8, 8, 3, mean, std, 127, odd, need, p, None, None, None), "16-byte aligned")


def test_parser_takes_the_config_route_and_transparent_watermark_is_refused_by_name():
    from unet_watermark_amd import cli
    from unet_watermark_amd.config import get_cfg_defaults
    a = cli.build_parser().parse_args(["train", "--augment", "config", "--augmentation-type", "enhanced"])
    assert a.augment == "config" and a.augmentation_type == "enhanced"
    assert cli.build_parser().parse_args(["train"]).augmentation_type is None
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["train", "--augmentation-type", "jpeg"])
    cfg = get_cfg_defaults()
    assert cfg.DATA.AUGMENTATION_TYPE == "transparent_watermark"
    with pytest.raises(ValueError, match="ImageCompression"):
        cli._served_recipe("config", cfg)
    # through the command itself: refused before any device work (this machine may have no device at all)
    with pytest.raises(ValueError, match="ImageCompression"):
        cli.main(["train", "--synthetic", "8", "--augment", "config", "--augmentation-type", "transparent_watermark"])
    with pytest.raises(ValueError, match="ImageCompression"):
        cli.main(["train", "--synthetic", "8", "--augment", "config"])
    cfg.DATA.AUGMENTATION_TYPE = "enhanced"
    assert cli._served_recipe("config", cfg)[0] == "enhanced" and cli._served_recipe("basic", cfg)[0] == "basic"
    assert "NOT applied" in cli._served_recipe("basic", cfg)[1] and cli._served_recipe("none", cfg) == ("none", "")
    cfg.DATA.AUGMENTATION_TYPE = "basic"
    assert cli._served_recipe("config", cfg)[0] == "basic" and cli._served_recipe("basic", cfg) == ("basic", "")
    cfg.DATA.AUGMENTATION_TYPE = "text_watermark"                    # the reference's else branch
    assert cli._served_recipe("config", cfg)[0] == "basic"
