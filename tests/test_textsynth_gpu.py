"""Text-watermark synthesis on the device (csrc/synth_text_u8.hip) against the numpy restatement (tests/textsynth_ref.py, which
tests/test_textsynth.py holds to Pillow): every stage through uwm_op_text_patches, the whole chain on a ragged batch in both mask
modes, a disabled slot and a misfit job, guard bands, reproducibility, one captured graph for every batch, logos and texts on the same
images, and the command lines built on it.  Everything is integers: every comparison is exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
from PIL import features

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_ref as S  # noqa: E402
import test_synth_gpu as G  # noqa: E402  (its packing helpers, guard constants and logo jobs)
import textsynth_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu
needs_freetype = pytest.mark.skipif(not features.check("freetype2"), reason="this Pillow has no freetype: no scalable font to draw with")
FILL, GUARD = G.FILL, G.GUARD
SHAPES = [(64, 96), (96, 64), (120, 200), (47, 33)]                    # (h, w): the image sizes of the CPU chain test
_P = G._P


def coverage(rng, h, w, empty=False):
    """a coverage plane as a rasterised text leaves it: a margin of 20 zeros, and inside it zeros, partial and full coverage"""
    p = np.zeros((h, w), np.uint8)
    if not empty:
        inner = rng.integers(1, 256, (h - 40, w - 40), dtype=np.uint8)
        u = rng.random(inner.shape)
        inner[u < 0.5] = 0; inner[u > 0.8] = 255
        p[20:-20, 20:-20] = inner
    return p


def make_job(glyph, size, ink=(255, 0, 0), angle=None, scale=None, radius=None, brightness=None, contrast=None, alpha=None, fits=(), x=0, y=0):
    """one enabled job on plane `glyph` of size (w, h) -> the record"""
    from unet_watermark_amd import data as D
    j = D.empty_text_jobs(1)
    w, h = size
    j["enabled"], j["glyph"], j["ink"], j["x"], j["y"] = 1, glyph, ink, x, y
    if angle is not None:
        m, w, h = D.synth_rotate_setup(w, h, angle)
        j["rotate"], j["rot"][0], j["w2"], j["h2"] = 1, m, w, h
    if scale is not None:
        j["scale"], j["w3"], j["h3"] = 1, *scale
    if radius is not None:
        j["blur"] = 1
        j["blur_r"], j["blur_ww"], j["blur_fw"] = D.synth_blur_params(radius)
    if brightness is not None:
        j["brighten"], j["brightness"] = 1, brightness
    if contrast is not None:
        j["recontrast"], j["contrast"] = 1, contrast
    if alpha is not None:
        j["opacity"][0] = D.synth_opacity_lut(alpha)
    j["nfit"] = len(fits)
    for f, s in enumerate(fits):
        j["fit"][0, f] = s
    return j[0]


def _workspace(dev, lib, n, k, Pp, Tt):
    need = int(lib.uwm_synth_text_workspace_bytes(n, k, Pp, Tt))
    assert need > 0
    return torch.full((need + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev), need


# ------------------------------------------------------------------------------------------------ stages A-G, job by job
def test_text_patches_equal_the_restatement(cuda):
    """12 jobs: every stage on and off, every fit count 0..3, a fit to the size the patch already has, a result one pixel wide, the
    empty text, planes from 40 x 40 to 200 x 70, a patch of more pixels than one launch's threads"""
    from unet_watermark_amd import data as D
    L, lib = G._lib()
    rng = np.random.default_rng(61)
    planes = [coverage(rng, 40, 40, empty=True), coverage(rng, 45, 61), coverage(rng, 70, 200), coverage(rng, 58, 133), coverage(rng, 41, 43)]
    sz = lambda k: (planes[k].shape[1], planes[k].shape[0])      # noqa: E731
    inks = D.TEXT_INKS
    jobs = [
        make_job(0, sz(0), inks[0], angle=30.0, scale=(50, 44), radius=1.0, brightness=1.2, contrast=0.8, alpha=0.4),      # the empty text
        make_job(1, sz(1), inks[1]),                                                                             # COLOUR alone
        make_job(1, sz(1), inks[2], angle=-45.0),
        make_job(1, sz(1), inks[3], angle=17.25, alpha=0.5),
        make_job(2, sz(2), inks[4], scale=(163, 97), alpha=0.31, fits=[(76, 45)]),
        make_job(2, sz(2), inks[5], scale=(200, 56), radius=0.5, fits=[(160, 44), (100, 27)]),                   # one axis only
        make_job(2, sz(2), inks[6], angle=44.9, scale=(280, 250), radius=1.5, brightness=0.6, contrast=1.3, alpha=0.8,
                 fits=[(160, 142), (86, 76), (51, 45)]),                                                         # everything, > 8192 * 8 pixels
        make_job(3, sz(3), inks[7], brightness=1.4, alpha=0.1),
        make_job(3, sz(3), inks[8], contrast=0.7, alpha=0.45),
        make_job(3, sz(3), inks[0], brightness=0.77, contrast=1.21, fits=[(133, 58), (1, 58), (1, 9)]),          # a copy; one pixel wide
        make_job(4, sz(4), inks[8], radius=1.2, contrast=1.3, fits=[(43, 20), (43, 20), (20, 20)]),
        make_job(4, sz(4), inks[2], angle=-3.0, scale=(36, 57), brightness=1.0, contrast=1.0, alpha=1.0),
    ]
    jobs = np.array(jobs)
    assert {int(j["nfit"]) for j in jobs} == {0, 1, 2, 3}
    for name in ("rotate", "scale", "blur", "brighten", "recontrast"):
        assert {bool(v) for v in jobs[name]} == {False, True}, name
    pbuf, pd = G._pack(planes, rng)
    Pp, Tt = D.text_job_needs(jobs, pd)
    J = len(jobs)
    ws, need = _workspace(cuda, lib, J, 1, Pp, Tt)
    out = torch.full((J * Pp * 4 + 2 * GUARD,), FILL, dtype=torch.uint8, device=cuda)
    pt, dt = torch.from_numpy(pbuf).to(cuda), D.descs_tensor(pd, cuda)
    jt = torch.from_numpy(jobs.view(np.uint8).copy()).to(cuda)
    L.check(lib.uwm_op_text_patches(_P(pt), pt.numel(), _P(dt), len(pd), _P(jt), J, Pp, Tt, _P(ws, GUARD), need, _P(out, GUARD), J * Pp * 4,
                                    C.c_void_p(L.stream_ptr(cuda))))
    torch.cuda.synchronize(cuda)
    o, w = out.cpu().numpy(), ws.cpu().numpy()
    assert (o[:GUARD] == FILL).all() and (o[-GUARD:] == FILL).all() and (w[:GUARD] == FILL).all() and (w[-GUARD:] == FILL).all()
    assert np.array_equal(pt.cpu().numpy(), pbuf), "the planes are read only"
    got = o[GUARD:-GUARD].reshape(J, Pp * 4)
    for i, j in enumerate(jobs):
        want = T.job_patch(planes[int(j["glyph"])], j)
        h, wd = want.shape[:2]
        assert (wd, h) == D.text_job_final_size(j, sz(int(j["glyph"]))), i
        assert np.array_equal(got[i, :wd * h * 4].reshape(h, wd, 4), want), i
        assert (got[i, wd * h * 4:] == FILL).all(), i                          # nothing behind the patch
    assert T.job_patch(planes[3], jobs[9]).shape[1] == 1 and not T.job_patch(planes[0], jobs[0])[..., 3].any()


# ------------------------------------------------------------------------------------------------ the whole chain on a ragged batch
@pytest.fixture(scope="module")
def batch():
    """4 images x 2 slots: a disabled slot, overlapping texts, a text that overhangs the right and bottom edges, one with every
    stage, one with none; masks that already hold something (the logos' planes of a mixed sample).  References are computed once."""
    rng = np.random.default_rng(62)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SHAPES]
    masks = [rng.integers(0, 256, (h, w), dtype=np.uint8) for h, w in SHAPES]
    planes = [coverage(rng, 45, 61), coverage(rng, 52, 101), coverage(rng, 40, 40, empty=True), coverage(rng, 44, 48)]
    sz = lambda k: (planes[k].shape[1], planes[k].shape[0])      # noqa: E731
    from unet_watermark_amd import data as D
    jobs = D.empty_text_jobs(4, 2)
    jobs[0, 0] = make_job(0, sz(0), (255, 255, 0), angle=-21.0, alpha=0.45, x=10, y=3)
    jobs[0, 1] = make_job(3, sz(3), (0, 0, 255), radius=0.8, contrast=1.25, alpha=0.7, x=30, y=20)                # over the first
    jobs[1, 1] = make_job(1, sz(1), (255, 255, 255), scale=(90, 60), brightness=1.3, alpha=0.6, fits=[(51, 34)], x=2, y=50)      # slot 0 stays empty
    jobs[2, 0] = make_job(1, sz(1), (0, 255, 0), angle=40.0, scale=(150, 130), radius=1.5, brightness=0.7, contrast=0.75, alpha=0.35,
                          fits=[(160, 138), (110, 95)], x=95, y=30)                                               # every stage; overhangs right and bottom
    jobs[2, 1] = make_job(2, sz(2), (128, 128, 128), alpha=0.5, x=0, y=0)                                        # the empty text
    jobs[3, 0] = make_job(3, sz(3), (0, 0, 0), fits=[(26, 23)], x=33 - 26, y=47 - 23)                            # the far corner
    jobs[3, 1] = make_job(0, sz(0), (255, 0, 255), x=-20, y=-20)                                                 # no optional stage; overhangs left and top
    want = {mode: [T.synth_text_image(images[n], masks[n], planes, jobs[n], mask_mode=mode) for n in range(4)] for mode in (0, 1)}
    assert all(not np.array_equal(w[0], im) for w, im in zip(want[0], images))
    assert all(not np.array_equal(a[1], b[1]) for a, b in zip(want[0], want[1]))
    return dict(images=images, masks=masks, planes=planes, jobs=jobs, want=want)


def _synth_text(dev, images, masks, planes, jobs, mode, seed, plane_descs=None, needs=None):
    """uwm_synth_text_u8 with guard bands around the image buffer, the mask buffer and the workspace -> (images, masks or None)"""
    from unet_watermark_amd import data as D
    L, lib = G._lib()
    rng = np.random.default_rng(seed)
    ibuf, idesc = G._pack(images, rng)
    pbuf, pdesc = G._pack(planes, rng)
    if plane_descs is not None:
        pdesc = plane_descs(pdesc, pbuf.size)
    n, k = jobs.shape
    Pp, Tt = needs or D.text_job_needs(jobs, pdesc)
    md = D.mask_descs_for(idesc); md["offset"] += GUARD + 3                            # masks at an odd offset
    mbytes = int((md["h"].astype(np.int64) * md["w"]).sum())
    ws, need = _workspace(dev, lib, n, k, Pp, Tt)
    it, pt = torch.from_numpy(ibuf).to(dev), torch.from_numpy(pbuf).to(dev)
    mbuf = np.full(mbytes + 2 * GUARD + 3, FILL, np.uint8)
    if masks is not None:
        for d, m in zip(md, masks):
            mbuf[d["offset"]: d["offset"] + m.size] = m.reshape(-1)
    mt = torch.from_numpy(mbuf).to(dev)
    dt = D.descs_tensor(np.concatenate([idesc, md, pdesc]), dev)
    jt = torch.from_numpy(np.ascontiguousarray(jobs).reshape(-1).view(np.uint8).copy()).to(dev)
    step = n * D.DESC_DTYPE.itemsize
    with_mask = masks is not None
    L.check(lib.uwm_synth_text_u8(_P(it), it.numel(), _P(dt), _P(mt) if with_mask else None, mt.numel() if with_mask else 0, _P(dt, step), mode,
                                  _P(pt), pt.numel(), _P(dt, 2 * step), len(pdesc), _P(jt), n, k, Pp, Tt, _P(ws, GUARD), need,
                                  C.c_void_p(L.stream_ptr(dev))))
    torch.cuda.synchronize(dev)
    got, w, m = it.cpu().numpy(), ws.cpu().numpy(), mt.cpu().numpy()
    assert (w[:GUARD] == FILL).all() and (w[-GUARD:] == FILL).all(), "the workspace's guard bands"
    assert (m[:GUARD + 3] == FILL).all() and (m[GUARD + 3 + mbytes:] == FILL).all(), "the mask buffer's guard bands"
    keep = np.ones(ibuf.size, bool)
    for d in idesc:
        keep[d["offset"]: d["offset"] + d["h"] * d["w"] * 3] = False
    assert np.array_equal(got[keep], ibuf[keep]), "bytes around the images"
    assert np.array_equal(pt.cpu().numpy(), pbuf), "the planes are read only"
    outs = [got[d["offset"]: d["offset"] + d["h"] * d["w"] * 3].reshape(d["h"], d["w"], 3) for d in idesc]
    mouts = [m[d["offset"]: d["offset"] + d["h"] * d["w"]].reshape(d["h"], d["w"]) for d in md] if with_mask else None
    return outs, mouts


@pytest.mark.parametrize("mode", [0, 1])
def test_ragged_batch_equals_the_restatement(cuda, batch, mode):
    outs, masks = _synth_text(cuda, batch["images"], batch["masks"], batch["planes"], batch["jobs"], mode, 63)
    for n, (wi, wm) in enumerate(batch["want"][mode]):
        assert np.array_equal(outs[n], wi), n
        assert np.array_equal(masks[n], wm), n
    again = _synth_text(cuda, batch["images"], batch["masks"], batch["planes"], batch["jobs"], mode, 63)      # a second run is bit-identical
    assert all(np.array_equal(a, b) for a, b in zip(outs + masks, again[0] + again[1]))
    outs2, none = _synth_text(cuda, batch["images"], None, batch["planes"], batch["jobs"], mode, 64)          # other offsets, no mask: the same images
    assert none is None and all(np.array_equal(a, b) for a, b in zip(outs, outs2))


@pytest.mark.parametrize("mode", [0, 1])
def test_a_misfit_job_costs_only_itself(cuda, batch, mode):
    """a plane descriptor that leaves its buffer: the job that names it is skipped by every stage, its neighbour in the same image
    and every other image are served.  Likewise a patch above max_patch_pixels, a side of 0, a non-finite matrix, nfit of 4, an ink of
    256; and an image whose only job misfits keeps its mask, in mode 1 too."""
    from unet_watermark_amd import data as D

    def leave(pdesc, nbytes):                                    # plane 3 now claims rows behind the end of the buffer
        d = pdesc.copy()
        d["h"][3] = (nbytes - int(d["offset"][3])) // int(d["w"][3]) + 1
        return d

    needs = (max(D.text_job_needs(batch["jobs"], np.array([(0, p.shape[0], p.shape[1]) for p in batch["planes"]], D.DESC_DTYPE))[0], 1 << 16), 1 << 12)
    outs, masks = _synth_text(cuda, batch["images"], batch["masks"], batch["planes"], batch["jobs"], mode, 65, plane_descs=leave, needs=needs)
    for n in range(4):
        skip = {k for k in range(2) if batch["jobs"][n, k]["enabled"] and batch["jobs"][n, k]["glyph"] == 3}
        wi, wm = T.synth_text_image(batch["images"][n], batch["masks"][n], batch["planes"], batch["jobs"][n], mask_mode=mode, skip=skip)
        assert np.array_equal(outs[n], wi) and np.array_equal(masks[n], wm), n
    cases = []
    j = batch["jobs"].copy(); j["w2"][2, 0], j["h2"][2, 0] = 400, 400; cases.append((j, (2, 0)))      # 160000 pixels > max_patch_pixels
    j = batch["jobs"].copy(); j["fit"][1, 1, 0, 0] = 0; cases.append((j, (1, 1)))                      # image 1 is left without a text
    j = batch["jobs"].copy(); j["rot"][0, 0, 2] = np.inf; cases.append((j, (0, 0)))
    j = batch["jobs"].copy(); j["nfit"][3, 0] = 4; cases.append((j, (3, 0)))
    j = batch["jobs"].copy(); j["ink"][0, 1, 1] = 256; cases.append((j, (0, 1)))
    assert needs[0] < 160000
    for jobs, (n, k) in cases:
        outs, masks = _synth_text(cuda, batch["images"], batch["masks"], batch["planes"], jobs, mode, 66, needs=needs)
        for i in range(4):
            wi, wm = T.synth_text_image(batch["images"][i], batch["masks"][i], batch["planes"], batch["jobs"][i], mask_mode=mode,
                                        skip={k} if i == n else ())
            assert np.array_equal(outs[i], wi) and np.array_equal(masks[i], wm), (n, k, i)


def test_one_captured_graph_serves_every_batch(cuda, batch):
    from unet_watermark_amd import data as D
    L, lib = G._lib()
    rng = np.random.default_rng(67)
    planes2 = [coverage(rng, 50, 77), coverage(rng, 41, 90)]
    images2 = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(40, 50), (70, 33), (20, 90), (55, 55)]]
    masks2 = [rng.integers(0, 256, im.shape[:2], dtype=np.uint8) for im in images2]
    jobs2 = D.empty_text_jobs(4, 2)
    jobs2[0, 1] = make_job(1, (90, 41), (0, 255, 255), angle=12.5, radius=1.1, contrast=0.9, alpha=0.5, fits=[(40, 19)], x=3, y=4)
    jobs2[1, 0] = make_job(0, (77, 50), (255, 0, 0), scale=(62, 60), brightness=0.8, alpha=0.75, fits=[(26, 25)], x=4, y=40)
    jobs2[3, 0] = make_job(0, (77, 50), (0, 0, 0), x=-10, y=20)
    jobs2[3, 1] = make_job(1, (90, 41), (255, 255, 255), angle=-33.0, alpha=0.2, x=0, y=0)
    sets = [(batch["images"], batch["masks"], batch["planes"], batch["jobs"], batch["want"][1]),
            (images2, masks2, planes2, jobs2, [T.synth_text_image(images2[n], masks2[n], planes2, jobs2[n], mask_mode=1) for n in range(4)])]
    packed = [(G._pack(im, rng), G._pack(pl, rng)) for im, _, pl, _, _ in sets]
    needs = [D.text_job_needs(s[3], p[1][1]) for s, p in zip(sets, packed)]
    Pp, Tt = max(a for a, _ in needs), max(b for _, b in needs)
    it = torch.zeros(max(p[0][0].size for p in packed), dtype=torch.uint8, device=cuda)
    pt = torch.zeros(max(p[1][0].size for p in packed), dtype=torch.uint8, device=cuda)
    mt = torch.zeros(max(sum(a.shape[0] * a.shape[1] for a in s[0]) for s in sets), dtype=torch.uint8, device=cuda)
    dt = torch.zeros((4 + 4 + 4) * D.DESC_DTYPE.itemsize, dtype=torch.uint8, device=cuda)
    jt = torch.zeros(8 * D.TEXT_JOB_DTYPE.itemsize, dtype=torch.uint8, device=cuda)
    ws, need = _workspace(cuda, lib, 4, 2, Pp, Tt)
    step = 4 * D.DESC_DTYPE.itemsize

    def call():
        L.check(lib.uwm_synth_text_u8(_P(it), it.numel(), _P(dt), _P(mt), mt.numel(), _P(dt, step), 1, _P(pt), pt.numel(), _P(dt, 2 * step), 4, _P(jt),
                                      4, 2, Pp, Tt, _P(ws, GUARD), need, C.c_void_p(L.stream_ptr(cuda))))

    def load(k):
        (ibuf, idesc), (pbuf, pdesc) = packed[k]
        pd4 = np.zeros(4, D.DESC_DTYPE); pd4[:len(pdesc)] = pdesc
        it[:ibuf.size].copy_(torch.from_numpy(ibuf)); pt[:pbuf.size].copy_(torch.from_numpy(pbuf))
        mflat = np.concatenate([m.reshape(-1) for m in sets[k][1]])
        mt.fill_(FILL); mt[:mflat.size].copy_(torch.from_numpy(mflat))
        dt.copy_(D.descs_tensor(np.concatenate([idesc, D.mask_descs_for(idesc), pd4])))
        jt.copy_(torch.from_numpy(np.ascontiguousarray(sets[k][3]).reshape(-1).view(np.uint8).copy()))

    def check(k, what):
        torch.cuda.synchronize()
        got, m = it.cpu().numpy(), mt.cpu().numpy()
        idesc = packed[k][0][1]
        for n, (d, md) in enumerate(zip(idesc, D.mask_descs_for(idesc))):
            h, w = int(d["h"]), int(d["w"])
            assert np.array_equal(got[d["offset"]: d["offset"] + h * w * 3].reshape(h, w, 3), sets[k][4][n][0]), (what, n)
            assert np.array_equal(m[md["offset"]: md["offset"] + h * w].reshape(h, w), sets[k][4][n][1]), (what, n)

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


# ------------------------------------------------------------------------------------------------ logos and texts on the same images
def test_logos_then_texts_equal_both_restatements(cuda, batch):
    """a mixed batch through the wrappers: device_synth, then device_synth_text with the mixed mask rule on the planes device_synth
    wrote; image 1 carries logos only (its text job is off) and keeps its unhalved mask, image 3 a text only"""
    from unet_watermark_amd import data as D
    rng = np.random.default_rng(68)
    logos = [G.rgba(rng, 20, 31), G.rgba(rng, 17, 9)]
    lj = D.empty_synth_jobs(4, 2)
    lj[0, 0] = G.make_job(0, (31, 20), w1=25, h1=16, angle=33.0, enhance=(1.2, 0.9, 1.1), alpha=0.8, x=5, y=6)[0]
    lj[1, 0] = G.make_job(1, (9, 17), w1=12, h1=22, alpha=0.9, x=20, y=30)[0]
    lj[1, 1] = G.make_job(0, (31, 20), w1=31, h1=20, radius=1.0, alpha=0.6, x=15, y=40)[0]
    lj[2, 1] = G.make_job(0, (31, 20), w1=60, h1=40, stretch=(70, 35), enhance=(0.8, 1.3, 0.7), alpha=0.7, x=100, y=40)[0]
    tj = batch["jobs"].copy()
    tj["enabled"][1] = 0
    pi, di, _ = D.pack_images(batch["images"])
    pl, dl, _ = D.pack_images(logos)
    pp, dp, _ = D.pack_images([p[..., None] for p in batch["planes"]])
    clean = pi.to(cuda)
    a, am = D.device_synth(clean, di, pl.to(cuda), dl, lj, with_mask=True)
    b, bm = D.device_synth_text(a, di, pp.to(cuda), dp, tj, masks=am, mask_mode=1)
    assert b.data_ptr() != a.data_ptr() and bm.data_ptr() != am.data_ptr(), "copies unless inplace"
    c, cm = D.device_synth_text(a.clone(), di, pp, dp, tj, masks=True, mask_mode=0, inplace=True)            # text masks alone, on zeroed planes
    for n, (d, m) in enumerate(zip(di, D.mask_descs_for(di))):
        h, w = int(d["h"]), int(d["w"])
        li, lm = S.synth_image(batch["images"][n], logos, lj[n])
        wi, wm = T.synth_text_image(li, lm, batch["planes"], tj[n], mask_mode=1)
        assert np.array_equal(b.cpu().numpy()[d["offset"]: d["offset"] + h * w * 3].reshape(h, w, 3), wi), n
        assert np.array_equal(bm.cpu().numpy()[m["offset"]: m["offset"] + h * w].reshape(h, w), wm), n
        _, tm = T.synth_text_image(li, np.zeros((h, w), np.uint8), batch["planes"], tj[n], mask_mode=0)
        assert np.array_equal(c.cpu().numpy()[d["offset"]: d["offset"] + h * w * 3].reshape(h, w, 3), wi), n
        assert np.array_equal(cm.cpu().numpy()[m["offset"]: m["offset"] + h * w].reshape(h, w), tm), n
        if n == 1:
            assert np.array_equal(wm, lm) and lm.any() and not tm.any()
    assert torch.equal(clean.cpu(), pi)


# ------------------------------------------------------------------------------------------------ the command lines
@needs_freetype
def test_main_synth_writes_text_and_mixed_samples(cuda, tmp_path, capsys):
    from PIL import Image
    from unet_watermark_amd import cli
    clean_dir, logos_dir = G._dataset(str(tmp_path / "src"), np.random.default_rng(69))
    runs = []
    for out in ("out", "out2"):
        out = str(tmp_path / out)
        res = cli.main(["synth", "--clean-dir", clean_dir, "--logos-dir", logos_dir, "--output-dir", out, "--count", "8", "--seed", "4",
                        "--text-watermark-ratio", "0.5", "--mixed-watermark-ratio", "0.25", "--generate-mask", "--batch-size", "3" if out.endswith("2") else "8"])
        assert res["written"] == 8
        names = sorted(os.listdir(f"{out}/watermarked"))
        assert names == sorted(os.listdir(f"{out}/masks")) == sorted(os.listdir(f"{out}/clean")) and len(names) == 8
        runs.append({f"{sub}/{f}": open(f"{out}/{sub}/{f}", "rb").read() for sub in ("watermarked", "masks") for f in names})
    assert runs[0] == runs[1], "the same seed writes the same bytes, whatever the batch size"
    kinds = {"text": 0, "mixed": 0, "logo": 0}
    for f in names:
        kind = "text" if f.startswith(("text_trans_", "text_norm_")) else "mixed" if f.startswith(("mixed_trans_", "mixed_norm_")) else "logo"
        assert kind != "logo" or f.startswith(("trans_", "norm_", "multi_trans_", "multi_norm_")), f
        kinds[kind] += 1
        mask = np.asarray(Image.open(str(tmp_path / "out" / "masks" / f)))
        img, clean = (np.asarray(Image.open(str(tmp_path / "out" / sub / f))) for sub in ("watermarked", "clean"))
        assert mask.shape == img.shape[:2]
        if kind == "text":
            assert mask.any() and not np.array_equal(img, clean), f
    assert kinds["text"] >= 1 and kinds["mixed"] >= 1, kinds
    assert "wrote 8 samples" in capsys.readouterr().out


@needs_freetype
def test_train_synthesize_with_text_and_mixed_samples(cuda, tmp_path, capsys):
    from unet_watermark_amd import cli
    clean_dir, logos_dir = G._dataset(str(tmp_path), np.random.default_rng(70))
    hist = cli.main(["train", "--synthesize", "--clean-dir", clean_dir, "--logos-dir", logos_dir, "--augment", "basic", "--epochs", "1",
                     "--batch-size", "2", "--lr", "0.002", "--no-early-stopping", "--img-size", "64", "--encoder", "resnet18", "--model", "Unet",
                     "--workers", "0", "--text-watermark-ratio", "0.3", "--mixed-watermark-ratio", "0.2",
                     "--model-save-path", str(tmp_path / "m.pth"), "--checkpoint-dir", str(tmp_path / "ck")])
    out = capsys.readouterr().out
    assert "synthesis: 6 clean images x 3 logos" in out and "text watermarks on 0.3 of the samples" in out
    assert len(hist) == 1 and np.isfinite(hist[0]["train_loss"]) and np.isfinite(hist[0]["val_loss"])


@needs_freetype
def test_pipeline_pastes_texts_as_the_restatement_does(cuda, tmp_path):
    """items of a RawSynthDataset with text and mixed samples through DeviceInputPipeline.to_u8 = both restatements -> pair mask or
    alpha rule -> cv2-convention resize; a dataset at ratios 0 goes the way it always went"""
    import pairmask_ref as P
    import resize_ref as R
    from unet_watermark_amd.data import DeviceInputPipeline, RawSynthDataset
    clean_dir, logos_dir = G._dataset(str(tmp_path), np.random.default_rng(71))
    for source in ("pair", "alpha"):
        ds = RawSynthDataset(clean_dir, logos_dir, seed=6, transparent_ratio=0.0, mask_threshold=15, mask_source=source,
                             text_watermark_ratio=0.4, mixed_watermark_ratio=0.3)
        pipe = DeviceInputPipeline(32, cuda, source=ds)
        items = [ds[i] for i in range(len(ds))]
        kinds = {ds.draw_sample(i, (items[i][0].shape[1], items[i][0].shape[0]))[4] for i in range(len(ds))}
        assert len(kinds) >= 2, kinds
        x, m = pipe.to_u8(items)
        for k, (clean, logos, jobs, planes, text_jobs) in enumerate(items):
            li, la = S.synth_image(clean, logos, jobs)
            wi, wa = T.synth_text_image(li, la, planes, text_jobs, mask_mode=1)
            wm = P.pair_mask(wi, clean, 15) if source == "pair" else wa
            assert np.array_equal(x[k].cpu().numpy(), R.resize_u8_linear(wi, 32, 32)), (source, k)
            assert np.array_equal(m[k].cpu().numpy(), R.resize_u8_nearest(wm, 32, 32)), (source, k)
    only = RawSynthDataset(clean_dir, None, seed=6, transparent_ratio=0.0, mask_threshold=15, mask_source="alpha", text_watermark_ratio=1.0)
    items = [only[i] for i in range(3)]                                                   # a batch without any logo
    x, m = DeviceInputPipeline(32, cuda, source=only).to_u8(items)
    for k, (clean, _, _, planes, text_jobs) in enumerate(items):
        wi, wa = T.synth_text_image(clean, np.zeros(clean.shape[:2], np.uint8), planes, text_jobs, mask_mode=0)
        assert np.array_equal(x[k].cpu().numpy(), R.resize_u8_linear(wi, 32, 32)) and np.array_equal(m[k].cpu().numpy(), R.resize_u8_nearest(wa, 32, 32))
