"""Logo-watermark synthesis on the device (csrc/synth_u8.hip) against the numpy restatement (tests/synth_ref.py, which
tests/test_synth.py holds to Pillow): the LANCZOS tables, every stage through uwm_op_synth_patches, the whole chain on a ragged
batch, misfit jobs, guard bands, reproducibility, one captured graph for every batch, and the pipeline and command line built on it.
Everything is integers: every comparison is exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairmask_ref as P  # noqa: E402
import resize_ref as R  # noqa: E402
import synth_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0xA5
GUARD = 256


def _lib():
    from unet_watermark_amd import _lib as L
    return L, L.lib()


def _P(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


def rgba(rng, h, w):
    p = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    u = rng.random((h, w))
    p[..., 3][u < 0.25] = 0
    p[..., 3][u > 0.75] = 255
    return p


def make_job(logo, size, w1, h1, angle=None, stretch=None, shear=None, radius=None, defects=(), enhance=None, alpha=None, x=0, y=0):
    """one enabled job on logo index `logo` of size (w, h) -> (record, final (w, h))"""
    from unet_watermark_amd import data as D
    j = D.empty_synth_jobs(1)
    w, h = w1, h1
    j["enabled"], j["logo"], j["w1"], j["h1"], j["x"], j["y"] = 1, logo, w1, h1, x, y
    if angle is not None:
        m, w, h = D.synth_rotate_setup(w, h, angle)
        j["rotate"], j["rot"][0], j["w2"], j["h2"] = 1, m, w, h
    if stretch is not None:
        w, h = stretch
        j["stretch"], j["w3"], j["h3"] = 1, w, h
        if shear is not None:
            j["shear"], j["shear_minv"][0] = 1, D.synth_shear_inverse(*shear)
    if radius is not None:
        j["blur"] = 1
        j["blur_r"], j["blur_ww"], j["blur_fw"] = D.synth_blur_params(radius)
    for d, rect in enumerate(defects):
        j["defects"][0, d] = rect
    j["ndefects"] = len(defects)
    if enhance is not None:
        j["enhance"], j["brightness"], j["contrast"], j["color"] = 1, *enhance
    if alpha is not None:
        j["opacity"][0] = D.synth_opacity_lut(alpha)
    return j[0], (w, h)


def _pack(arrays, rng, guard=GUARD):
    """arrays back to back at 4-byte-aligned offsets with random bytes in front, between and behind -> (buffer, descs)"""
    from unet_watermark_amd.data import DESC_DTYPE
    descs = np.zeros(len(arrays), DESC_DTYPE)
    off = guard
    for i, a in enumerate(arrays):
        descs[i] = (off, a.shape[0], a.shape[1])
        off = (off + a.size + 3) // 4 * 4 + 4 * int(rng.integers(1, 8))
    buf = rng.integers(0, 256, size=off + guard, dtype=np.uint8)
    for a, d in zip(arrays, descs):
        buf[d["offset"]: d["offset"] + a.size] = a.reshape(-1)
    return buf, descs


def _workspace(dev, lib, n, k, Pp, T):
    """a workspace of exactly the needed bytes between two guard bands -> (tensor, needed bytes)"""
    need = int(lib.uwm_synth_workspace_bytes(n, k, Pp, T))
    assert need > 0
    return torch.full((need + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev), need


def _patches(dev, logos, jobs, rng):
    """uwm_op_synth_patches on J jobs -> the J finished patches (None where the device wrote nothing)"""
    from unet_watermark_amd import data as D
    L, lib = _lib()
    lbuf, ld = _pack(logos, rng)
    jobs = np.ascontiguousarray(jobs)
    Pp, T = D.synth_job_needs(jobs, ld)
    J = len(jobs)
    ws, need = _workspace(dev, lib, J, 1, Pp, T)
    out = torch.full((J * Pp * 4 + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
    lt, dt = torch.from_numpy(lbuf).to(dev), D.descs_tensor(ld, dev)
    jt = torch.from_numpy(jobs.view(np.uint8).copy()).to(dev)
    L.check(lib.uwm_op_synth_patches(_P(lt), lt.numel(), _P(dt), len(ld), _P(jt), J, Pp, T, _P(ws, GUARD), need, _P(out, GUARD), J * Pp * 4,
                                     C.c_void_p(L.stream_ptr(dev))))
    torch.cuda.synchronize(dev)
    o, w = out.cpu().numpy(), ws.cpu().numpy()
    assert (o[:GUARD] == FILL).all() and (o[-GUARD:] == FILL).all() and (w[:GUARD] == FILL).all() and (w[-GUARD:] == FILL).all()
    return o[GUARD:-GUARD].reshape(J, Pp * 4), Pp


def _check_patches(dev, logos, specs, seed):
    """specs: (logo index, make_job keywords) -> every device patch equals the restatement's"""
    jobs, sizes = zip(*(make_job(k, (logos[k].shape[1], logos[k].shape[0]), **kw) for k, kw in specs))
    got, Pp = _patches(dev, logos, np.array(jobs), np.random.default_rng(seed))
    for i, (j, (w, h)) in enumerate(zip(jobs, sizes)):
        want = S.job_patch(logos[int(j["logo"])], j)
        assert want.shape == (h, w, 4), (i, specs[i])
        assert np.array_equal(got[i, :w * h * 4].reshape(h, w, 4), want), (i, specs[i])
        assert (got[i, w * h * 4:] == FILL).all(), (i, specs[i])                  # nothing behind the patch


# ------------------------------------------------------------------------------------------------ the tables
@pytest.mark.parametrize("n_in,n_out", [(53, 11), (37, 7), (64, 90), (40, 23), (200, 31), (128, 19), (9, 9), (17, 30), (9, 10), (600, 38), (1, 5), (7, 1)])
def test_lanczos_table_equals_the_restatement(cuda, n_in, n_out):
    L, lib = _lib()
    want = S.lanczos_table(n_in, n_out)
    n = int(lib.uwm_lanczos_table_ints(n_in, n_out))
    assert n == want.size
    t = torch.full((n + 64,), -7, dtype=torch.int32, device=cuda)
    L.check(lib.uwm_op_lanczos_table(n_in, n_out, _P(t, 128), n, C.c_void_p(L.stream_ptr(cuda))))
    torch.cuda.synchronize(cuda)
    got = t.cpu().numpy()
    assert (got[:32] == -7).all() and (got[32 + n:] == -7).all()
    assert np.array_equal(got[32:32 + n].reshape(want.shape), want)


# ------------------------------------------------------------------------------------------------ the stages, one at a time
def test_resize_stage(cuda):
    rng = np.random.default_rng(31)
    logos = [rgba(rng, 37, 53), rgba(rng, 40, 64), rgba(rng, 128, 200), rgba(rng, 17, 9), rgba(rng, 20, 20)]
    specs = [(0, dict(w1=11, h1=7)), (1, dict(w1=90, h1=23)), (2, dict(w1=31, h1=19)), (3, dict(w1=9, h1=30)),
             (4, dict(w1=20, h1=31)), (4, dict(w1=7, h1=20)), (4, dict(w1=20, h1=20)), (3, dict(w1=1, h1=1))]      # one axis only; a copy; one pixel
    _check_patches(cuda, logos, specs, 32)


def test_rotate_stage(cuda):
    rng = np.random.default_rng(33)
    logos = [rgba(rng, 13, 29), rgba(rng, 9, 9), rgba(rng, 30, 12)]
    specs = [(k, dict(w1=a.shape[1], h1=a.shape[0], angle=ang)) for k, a in enumerate(logos) for ang in (37.3, 45, 90, 123.456, 180, 301, 359.2)]
    _check_patches(cuda, logos, specs, 34)


def test_stretch_and_shear_stage(cuda):
    rng = np.random.default_rng(35)
    logos = [rgba(rng, 21, 33), rgba(rng, 12, 30)]
    specs = [(0, dict(w1=33, h1=21, stretch=(40, 15))), (0, dict(w1=33, h1=21, stretch=(33, 30))),
             (0, dict(w1=33, h1=21, stretch=(33, 21), shear=(0.4, -0.4))), (1, dict(w1=30, h1=12, stretch=(45, 9), shear=(-0.31, 0.17))),
             (1, dict(w1=30, h1=12, stretch=(19, 19), shear=(0.0, 0.0))), (1, dict(w1=30, h1=12, stretch=(19, 19), shear=(0.05, 0.4)))]
    _check_patches(cuda, logos, specs, 36)


def test_blur_stage(cuda):
    rng = np.random.default_rng(37)
    logos = [rgba(rng, 3, 4), rgba(rng, 21, 33), rgba(rng, 40, 5)]
    specs = [(k, dict(w1=a.shape[1], h1=a.shape[0], radius=r)) for k, a in enumerate(logos) for r in (0.5, 1.3, 2.5)]
    _check_patches(cuda, logos, specs, 38)


def test_defects_enhance_and_opacity_stages(cuda):
    rng = np.random.default_rng(39)
    half = np.zeros((1, 2, 4), np.uint8); half[0, 0] = (10, 10, 10, 0); half[0, 1] = (11, 11, 11, 200)      # a contrast mean of 10.5
    logos = [rgba(rng, 19, 23), half, rgba(rng, 70, 131)]                                                  # (the last: more than one workgroup's stride of pixels)
    specs = [(0, dict(w1=23, h1=19, enhance=e)) for e in ((0.4, 1.0, 1.0), (1.8, 1.0, 1.0), (1.0, 0.5, 1.0), (1.0, 1.6, 1.0), (1.0, 1.0, 0.5),
                                                       (1.0, 1.0, 1.5), (0.77, 1.3, 0.9), (1.0, 1.0, 1.0))]
    specs += [(1, dict(w1=2, h1=1, enhance=(1.0, f, 1.0))) for f in (0.5, 1.6)]
    specs += [(2, dict(w1=131, h1=70, enhance=(1.2, 0.6, 1.4), alpha=0.33))]
    specs += [(0, dict(w1=23, h1=19, alpha=a)) for a in (0.08, 0.45, 0.85)]
    specs += [(0, dict(w1=23, h1=19, defects=[(0, 0, 4, 3), (20, 17, 3, 2), (5, 6, 1, 1)])), (0, dict(w1=23, h1=19, defects=[(22, 18, 9, 9)]))]
    _check_patches(cuda, logos, specs, 40)


# ------------------------------------------------------------------------------------------------ the whole chain on a ragged batch
SHAPES = [(61, 47), (64, 96), (33, 40)]


@pytest.fixture(scope="module")
def batch():
    """3 images x 3 slots: an empty slot, a plain job, a job with every stage on, one with every optional stage off, a patch that
    overhangs the right and bottom edges, overlapping logos; the reference result is computed once"""
    rng = np.random.default_rng(41)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SHAPES]
    logos = [rgba(rng, 40, 64), rgba(rng, 17, 9), rgba(rng, 25, 25)]
    sz = lambda k: (logos[k].shape[1], logos[k].shape[0])      # noqa: E731
    from unet_watermark_amd import data as D
    jobs = D.empty_synth_jobs(3, 3)
    full = dict(w1=30, h1=19, angle=123.456, stretch=(28, 40), shear=(0.3, -0.2), radius=1.3, defects=[(2, 3, 5, 4), (20, 30, 6, 8)],
                enhance=(1.4, 0.7, 1.2), alpha=0.6, x=5, y=8)
    jobs[0, 0] = make_job(0, sz(0), **full)[0]                                           # every stage on
    jobs[0, 2] = make_job(1, sz(1), w1=12, h1=22, x=10, y=20)[0]                         # a plain job, over the first (slot 1 stays empty)
    jobs[1, 0] = make_job(2, sz(2), w1=25, h1=25, enhance=(0.9, 1.2, 0.8), alpha=0.7, x=0, y=0)[0]      # every optional stage off, a copy at (0, 0)
    jobs[1, 1] = make_job(0, sz(0), w1=50, h1=31, angle=37.3, enhance=(1.1, 1.0, 1.3), alpha=0.8, x=70, y=40)[0]      # overhangs right and bottom
    jobs[1, 2] = make_job(2, sz(2), w1=31, h1=19, radius=2.5, enhance=(1.0, 1.5, 1.0), alpha=0.3, x=60, y=35)[0]      # over the second
    jobs[2, 0] = make_job(1, sz(1), w1=9, h1=30, stretch=(14, 20), enhance=(1.7, 0.6, 0.6), alpha=0.12, x=40 - 14, y=33 - 20)[0]      # the far corner, low opacity
    jobs[2, 1] = make_job(0, sz(0), w1=11, h1=7, angle=301, x=1, y=1)[0]
    want = [S.synth_image(images[n], logos, jobs[n]) for n in range(3)]
    assert all(m.any() for _, m in want) and all(not np.array_equal(w[0], im) for w, im in zip(want, images))
    return dict(images=images, logos=logos, jobs=jobs, want=want)


def _synth(dev, images, logos, jobs, seed, with_mask=True, needs=None):
    """uwm_synth_u8 with guard bands around the image buffer, the mask buffer and the workspace -> (images, masks or None)"""
    from unet_watermark_amd import data as D
    L, lib = _lib()
    rng = np.random.default_rng(seed)
    ibuf, idesc = _pack(images, rng)
    lbuf, ldesc = _pack(logos, rng)
    n, k = jobs.shape
    Pp, T = needs or D.synth_job_needs(jobs, ldesc)
    md = D.mask_descs_for(idesc); md["offset"] += GUARD + 3                            # masks at an odd offset
    mbytes = int((md["h"].astype(np.int64) * md["w"]).sum())
    ws, need = _workspace(dev, lib, n, k, Pp, T)
    it, lt = torch.from_numpy(ibuf).to(dev), torch.from_numpy(lbuf).to(dev)
    mt = torch.full((mbytes + 2 * GUARD + 3,), FILL, dtype=torch.uint8, device=dev)
    dt = D.descs_tensor(np.concatenate([idesc, md, ldesc]), dev)
    jt = torch.from_numpy(np.ascontiguousarray(jobs).reshape(-1).view(np.uint8).copy()).to(dev)
    step = n * D.DESC_DTYPE.itemsize
    L.check(lib.uwm_synth_u8(_P(it), it.numel(), _P(dt), _P(mt) if with_mask else None, mt.numel() if with_mask else 0, _P(dt, step), _P(lt), lt.numel(),
                             _P(dt, 2 * step), len(ldesc), _P(jt), n, k, Pp, T, _P(ws, GUARD), need, C.c_void_p(L.stream_ptr(dev))))
    torch.cuda.synchronize(dev)
    got, w, m = it.cpu().numpy(), ws.cpu().numpy(), mt.cpu().numpy()
    assert (w[:GUARD] == FILL).all() and (w[-GUARD:] == FILL).all(), "the workspace's guard bands"
    assert (m[:GUARD + 3] == FILL).all() and (m[GUARD + 3 + mbytes:] == FILL).all(), "the mask buffer's guard bands"
    keep = np.ones(ibuf.size, bool)
    for d in idesc:
        keep[d["offset"]: d["offset"] + d["h"] * d["w"] * 3] = False
    assert np.array_equal(got[keep], ibuf[keep]), "bytes around the images"
    assert np.array_equal(lt.cpu().numpy(), lbuf), "the logos are read only"
    outs = [got[d["offset"]: d["offset"] + d["h"] * d["w"] * 3].reshape(d["h"], d["w"], 3) for d in idesc]
    masks = [m[d["offset"]: d["offset"] + d["h"] * d["w"]].reshape(d["h"], d["w"]) for d in md] if with_mask else None
    return outs, masks


def test_ragged_batch_equals_the_restatement(cuda, batch):
    from unet_watermark_amd import data as D
    outs, masks = _synth(cuda, batch["images"], batch["logos"], batch["jobs"], 42)
    for n, (wi, wm) in enumerate(batch["want"]):
        assert np.array_equal(outs[n], wi), n
        assert np.array_equal(masks[n], wm), n                                          # mask source 'alpha'
    outs2, none = _synth(cuda, batch["images"], batch["logos"], batch["jobs"], 43, with_mask=False)      # other offsets, no mask: the same images
    assert none is None and all(np.array_equal(a, b) for a, b in zip(outs, outs2))
    # mask source 'pair': uwm_pair_mask_u8 on (synthesized, clean) = the reference's dataset rule on the restatement's images
    pi, di, _ = D.pack_images(batch["images"])
    pl, dl, _ = D.pack_images(batch["logos"])
    clean = pi.to(cuda)
    synth, alpha = D.device_synth(clean, di, pl.to(cuda), dl, batch["jobs"], with_mask=True)
    pm = D.device_pair_mask(synth, di, clean, di, 15).cpu().numpy()
    for n, (d, m) in enumerate(zip(di, D.mask_descs_for(di))):
        h, w = int(d["h"]), int(d["w"])
        assert np.array_equal(synth.cpu().numpy()[d["offset"]: d["offset"] + h * w * 3].reshape(h, w, 3), batch["want"][n][0])
        assert np.array_equal(alpha.cpu().numpy()[m["offset"]: m["offset"] + h * w].reshape(h, w), batch["want"][n][1])
        want = P.pair_mask(batch["want"][n][0], batch["images"][n], 15)
        assert np.array_equal(pm[m["offset"]: m["offset"] + h * w].reshape(h, w), want) and want.any()
    assert torch.equal(clean.cpu(), pi) and synth.data_ptr() != clean.data_ptr()        # device_synth works on a copy


def test_two_runs_are_bit_identical(cuda, batch):
    a = _synth(cuda, batch["images"], batch["logos"], batch["jobs"], 44)
    b = _synth(cuda, batch["images"], batch["logos"], batch["jobs"], 44)
    assert all(np.array_equal(x, y) for x, y in zip(a[0] + a[1], b[0] + b[1]))


def test_a_misfit_job_costs_only_itself(cuda, batch):
    """a logo index outside the logos, a patch above max_patch_pixels, a table above max_taps, a side of 0, a non-finite matrix, a
    negative defect: each leaves its image as it would be without that job, and every other job is served"""
    from unet_watermark_amd import data as D
    _, ldesc = _pack(batch["logos"], np.random.default_rng(45))
    needs = D.synth_job_needs(batch["jobs"], ldesc)
    cases = []
    j = batch["jobs"].copy(); j["logo"][0, 0] = 3; cases.append((j, (0, 0)))
    j = batch["jobs"].copy(); j["logo"][1, 2] = -1; cases.append((j, (1, 2)))
    j = batch["jobs"].copy(); j["w2"][1, 1], j["h2"][1, 1] = 300, 300; cases.append((j, (1, 1)))      # 90000 pixels > max_patch_pixels
    j = batch["jobs"].copy(); j["w1"][2, 0] = 0; cases.append((j, (2, 0)))
    j = batch["jobs"].copy(); j["rot"][2, 1, 2] = np.nan; cases.append((j, (2, 1)))
    j = batch["jobs"].copy(); j["defects"][0, 0, 1, 0] = -1; cases.append((j, (0, 0)))
    j = batch["jobs"].copy(); j["blur_r"][1, 2] = 33; cases.append((j, (1, 2)))
    assert needs[0] < 90000
    for jobs, (n, k) in cases:
        outs, masks = _synth(cuda, batch["images"], batch["logos"], jobs, 46, needs=needs)
        for i in range(3):
            wi, wm = S.synth_image(batch["images"][i], batch["logos"], batch["jobs"][i], skip={k} if i == n else ())
            assert np.array_equal(outs[i], wi) and np.array_equal(masks[i], wm), (n, k, i)
    # too few taps: every job that resamples is skipped, the copy at (0, 0) of image 1 is not
    outs, masks = _synth(cuda, batch["images"], batch["logos"], batch["jobs"], 47, needs=(needs[0], 8))
    assert np.array_equal(outs[0], batch["images"][0]) and not masks[0].any()
    wi, wm = S.synth_image(batch["images"][1], batch["logos"], batch["jobs"][1], skip={1, 2})
    assert np.array_equal(outs[1], wi) and np.array_equal(masks[1], wm) and wm.any()


def test_one_captured_graph_serves_every_batch(cuda, batch):
    from unet_watermark_amd import data as D
    L, lib = _lib()
    rng = np.random.default_rng(48)
    logos2 = [rgba(rng, 30, 12), rgba(rng, 21, 33)]
    images2 = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(40, 50), (70, 33), (20, 90)]]
    jobs2 = D.empty_synth_jobs(3, 3)
    jobs2[0, 1] = make_job(1, (33, 21), w1=20, h1=13, angle=45, radius=0.5, enhance=(1.3, 1.3, 0.7), alpha=0.5, x=3, y=4)[0]
    jobs2[1, 0] = make_job(0, (12, 30), w1=12, h1=30, stretch=(20, 25), shear=(0.2, 0.1), enhance=(0.6, 0.9, 1.1), alpha=0.85, x=10, y=40)[0]
    jobs2[2, 2] = make_job(0, (12, 30), w1=6, h1=15, x=80, y=10)[0]
    sets = [(batch["images"], batch["logos"], batch["jobs"], batch["want"]),
            (images2, logos2, jobs2, [S.synth_image(images2[n], logos2, jobs2[n]) for n in range(3)])]
    packed = [(_pack(im, rng), _pack(lg, rng)) for im, lg, _, _ in sets]
    needs = [D.synth_job_needs(j, p[1][1]) for (_, _, j, _), p in zip(sets, packed)]
    Pp, T = max(a for a, _ in needs), max(b for _, b in needs)
    it = torch.zeros(max(p[0][0].size for p in packed), dtype=torch.uint8, device=cuda)
    lt = torch.zeros(max(p[1][0].size for p in packed), dtype=torch.uint8, device=cuda)
    mt = torch.zeros(max(sum(a.shape[0] * a.shape[1] for a in s[0]) for s in sets), dtype=torch.uint8, device=cuda)
    dt = torch.zeros((3 + 3 + 3) * D.DESC_DTYPE.itemsize, dtype=torch.uint8, device=cuda)
    jt = torch.zeros(9 * D.SYNTH_JOB_DTYPE.itemsize, dtype=torch.uint8, device=cuda)
    ws, need = _workspace(cuda, lib, 3, 3, Pp, T)
    step = 3 * D.DESC_DTYPE.itemsize

    def call():
        L.check(lib.uwm_synth_u8(_P(it), it.numel(), _P(dt), _P(mt), mt.numel(), _P(dt, step), _P(lt), lt.numel(), _P(dt, 2 * step), 3, _P(jt), 3, 3,
                                 Pp, T, _P(ws, GUARD), need, C.c_void_p(L.stream_ptr(cuda))))

    def load(k):
        (ibuf, idesc), (lbuf, ldesc) = packed[k]
        ld3 = np.zeros(3, D.DESC_DTYPE); ld3[:len(ldesc)] = ldesc
        it[:ibuf.size].copy_(torch.from_numpy(ibuf)); lt[:lbuf.size].copy_(torch.from_numpy(lbuf)); mt.fill_(FILL)
        dt.copy_(D.descs_tensor(np.concatenate([idesc, D.mask_descs_for(idesc), ld3])))
        jt.copy_(torch.from_numpy(np.ascontiguousarray(sets[k][2]).reshape(-1).view(np.uint8).copy()))

    def check(k, what):
        torch.cuda.synchronize()
        got, m = it.cpu().numpy(), mt.cpu().numpy()
        idesc = packed[k][0][1]
        for n, (d, md) in enumerate(zip(idesc, D.mask_descs_for(idesc))):
            h, w = int(d["h"]), int(d["w"])
            assert np.array_equal(got[d["offset"]: d["offset"] + h * w * 3].reshape(h, w, 3), sets[k][3][n][0]), (what, n)
            assert np.array_equal(m[md["offset"]: md["offset"] + h * w].reshape(h, w), sets[k][3][n][1]), (what, n)

    load(0)
    call()                                                   # eager, and the warm-up of the capture
    check(0, "eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for k in (1, 0):
        load(k)
        graph.replay()
        check(k, f"replay on batch {k}")


# ------------------------------------------------------------------------------------------------ the pipeline and the command line
def _dataset(root, rng):
    from PIL import Image
    os.makedirs(f"{root}/clean"); os.makedirs(f"{root}/logos/combined"); os.makedirs(f"{root}/logos/independent")
    for i, (h, w) in enumerate([(128, 128), (100, 140), (180, 122), (128, 192), (66, 94), (142, 142)]):
        base = rng.integers(0, 256, size=(h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8)
        Image.fromarray(base).resize((w, h), Image.BILINEAR).save(f"{root}/clean/im{i}.png")
    for i, (h, w) in enumerate([(20, 30), (16, 16), (24, 12)]):
        a = rgba(rng, h, w); a[..., :3] = a[..., :3] // 4 * (i + 1); a[2:-2, 2:-2, 3] = 255
        Image.fromarray(a, "RGBA").save(f"{root}/logos/{'combined' if i < 2 else 'independent'}/l{i}.png")
    return f"{root}/clean", f"{root}/logos"


def test_pipeline_synthesizes_what_the_restatement_does(cuda, tmp_path):
    """items of RawSynthDataset through DeviceInputPipeline.to_u8 = restatement -> pair mask -> cv2-convention resize, for both mask
    sources; normal-opacity samples have non-empty masks"""
    from unet_watermark_amd.data import DeviceInputPipeline, RawSynthDataset
    clean_dir, logos_dir = _dataset(str(tmp_path), np.random.default_rng(49))
    for source in ("pair", "alpha"):
        ds = RawSynthDataset(clean_dir, logos_dir, seed=5, transparent_ratio=0.0, mask_threshold=15, mask_source=source)
        pipe = DeviceInputPipeline(32, cuda, source=ds)
        items = [ds[i] for i in range(len(ds))]
        x, m = pipe.to_u8(items)
        assert x.shape == (6, 32, 32, 3) and m.shape == (6, 32, 32)
        filled = 0
        for k, (clean, logos, jobs) in enumerate(items):
            wi, wa = S.synth_image(clean, logos, jobs)
            wm = P.pair_mask(wi, clean, 15) if source == "pair" else wa
            assert jobs["enabled"].any(), k
            filled += int(wm.any())
            assert np.array_equal(x[k].cpu().numpy(), R.resize_u8_linear(wi, 32, 32)), (source, k)
            assert np.array_equal(m[k].cpu().numpy(), R.resize_u8_nearest(wm, 32, 32)), (source, k)
        assert filled >= 4, source                                                      # (a logo of two or three pixels does not survive the opening)


def test_train_synthesize_two_epochs(cuda, tmp_path, capsys):
    from unet_watermark_amd import cli
    from unet_watermark_amd.config import get_cfg_defaults
    from unet_watermark_amd.data import DeviceInputPipeline
    clean_dir, logos_dir = _dataset(str(tmp_path), np.random.default_rng(50))
    argv = ["train", "--synthesize", "--clean-dir", clean_dir, "--logos-dir", logos_dir, "--augment", "basic", "--epochs", "2", "--batch-size", "2",
            "--lr", "0.002", "--no-early-stopping", "--img-size", "64", "--encoder", "resnet18", "--model", "Unet", "--workers", "0",
            "--transparent-ratio", "0.0", "--model-save-path", str(tmp_path / "m.pth"), "--checkpoint-dir", str(tmp_path / "ck")]
    hist = cli.main(argv)
    assert "synthesis: 6 clean images x 3 logos" in capsys.readouterr().out
    assert len(hist) == 2 and all(np.isfinite(h["train_loss"]) and np.isfinite(h["val_loss"]) for h in hist)
    # the same datasets the command built: validation batches are the same in epoch 0 and epoch 1, training batches are not
    args = cli.build_parser().parse_args(argv)
    cfg = get_cfg_defaults()
    tr, va = cli._synth_datasets(cfg, args)
    assert len(tr) + len(va) == 6 and len(va) >= 1
    pipe = DeviceInputPipeline(64, cuda, source=tr.dataset)
    runs = []
    for epoch in (0, 1):
        tr.dataset.set_epoch(epoch)
        xv, mv = pipe.val_batch([va[i] for i in range(len(va))])
        xt, mt = pipe.to_u8([tr[i] for i in range(len(tr))])
        assert bool(mt.flatten(1).any(1).all())                                         # normal opacity: no empty mask
        runs.append((xv.cpu(), mv.cpu(), xt.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert not torch.equal(runs[0][2], runs[1][2])


def test_main_synth_output_is_read_by_the_pair_dataset(cuda, tmp_path, capsys):
    from PIL import Image
    from unet_watermark_amd import cli
    from unet_watermark_amd.data import RawPairDataset
    clean_dir, logos_dir = _dataset(str(tmp_path / "src"), np.random.default_rng(51))
    out = str(tmp_path / "out")
    res = cli.main(["synth", "--clean-dir", clean_dir, "--logos-dir", logos_dir, "--output-dir", out, "--count", "5", "--batch-size", "2", "--seed", "3"])
    assert res["written"] == 5 and "wrote 5 samples" in capsys.readouterr().out
    assert sorted(os.listdir(f"{out}/watermarked")) == sorted(os.listdir(f"{out}/clean")) and not os.path.exists(f"{out}/masks")
    ds = RawPairDataset([out], 15)
    assert len(ds) == 5 and ds.missing_masks() == list(range(5))
    changed = 0
    for i in range(5):
        img, m, clean = ds[i]
        assert m is None and clean is not None and clean.shape == img.shape
        changed += int(not np.array_equal(img, clean))
    assert changed >= 4                                                                 # (a sample whose every logo was dropped stays clean)
    out2 = str(tmp_path / "out2")
    cli.main(["synth", "--clean-dir", clean_dir, "--logos-dir", logos_dir, "--output-dir", out2, "--count", "5", "--seed", "3", "--generate-mask"])
    assert sorted(os.listdir(f"{out2}/masks")) == sorted(os.listdir(f"{out}/watermarked"))
    for f in os.listdir(f"{out}/watermarked"):                                          # the batch size does not change a sample
        assert np.array_equal(np.asarray(Image.open(f"{out}/watermarked/{f}")), np.asarray(Image.open(f"{out2}/watermarked/{f}")))
    assert RawPairDataset([out2], 15).missing_masks() == []
