"""uwm_jpeg_ragged_u8 on the device against the numpy restatement (tests/jpeg_any_ref.py, itself held to Pillow bit for bit by
test_jpeg_any.py): ragged batches at the sizes where libjpeg's edge rule bites, aliasing, quality 0, the fixed-shape kernel at
multiples of 16, one captured graph for two batches, and the synthesis pipeline with the flag on and off.  Everything is bit-equality:
the arithmetic is integer."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
from PIL import features

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_any_ref as A  # noqa: E402
import jpeg_ref as J  # noqa: E402
import test_synth_gpu as G  # noqa: E402  (its packing helper, guard constants and the tiny clean / logo fixture)

pytestmark = pytest.mark.gpu
needs_freetype = pytest.mark.skipif(not features.check("freetype2"), reason="this Pillow has no freetype: no scalable font to draw with")
FILL, GUARD = G.FILL, G.GUARD
_P = G._P
# (h, w).  5x4: wc = 2, the replication branch; 6x5: wc = 3, the smallest size with the triangle filter; 24x24: even H, rows replicated
# behind the down-sampling; 17x33: both sides odd, across MCU borders; 100x75: several MCU groups to one workgroup
SIZES = [(1, 1), (1, 9), (2, 2), (5, 4), (6, 5), (8, 8), (9, 17), (15, 16), (16, 16), (24, 24), (17, 33), (23, 40), (100, 75)]
QUALITIES = [95, 30, 1, 100, 0]
_REF = {}


def _images(kind, sizes=SIZES, seed=0):
    with np.errstate(divide="ignore"):
        return [J.sample_images(h, w, seed)[kind] for h, w in sizes]


def _want(kind, shift):
    """the reference of the SIZES batch with the qualities rotated by `shift`, computed once"""
    key = (kind, shift)
    if key not in _REF:
        q = [QUALITIES[(i + shift) % 5] for i in range(len(SIZES))]
        _REF[key] = (q, A.roundtrip_ragged(_images(kind), q))
    return _REF[key]


def _call(dev, images, quality, alias, seed, max_pixels=None):
    """the C entry point on a packed buffer with random bytes around every image, a workspace of exactly `bytes` bytes between guard
    bands -> the images of `out`; every byte outside them must be what it was"""
    L, lib = G._lib()
    rng = np.random.default_rng(seed)
    buf, descs = G._pack(images, rng)
    src = torch.from_numpy(buf).to(dev)
    fill = rng.integers(0, 256, size=buf.size, dtype=np.uint8)
    out = src if alias else torch.from_numpy(fill).to(dev)
    n, nbytes = len(images), buf.size
    assert int(lib.uwm_jpeg_ragged_workspace_bytes(n, nbytes)) == nbytes
    ws = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
    dd = torch.from_numpy(descs.view(np.uint8).copy()).to(dev)
    qd = torch.tensor(list(quality), dtype=torch.int32, device=dev)
    mp = int(max(a.shape[0] * a.shape[1] for a in images)) if max_pixels is None else max_pixels
    L.check(lib.uwm_jpeg_ragged_u8(_P(src), _P(out), nbytes, _P(dd), _P(qd), n, 3, mp, _P(ws, GUARD), nbytes, C.c_void_p(L.stream_ptr(dev))))
    torch.cuda.synchronize()
    got, w = out.cpu().numpy(), ws.cpu().numpy()
    assert (w[:GUARD] == FILL).all() and (w[GUARD + nbytes:] == FILL).all(), "a write left the workspace"
    if not alias:
        assert np.array_equal(src.cpu().numpy(), buf), "the input changed"
    outside = np.ones(nbytes, bool)
    res = []
    for a, d in zip(images, descs):
        o = int(d["offset"])
        outside[o: o + a.size] = False
        res.append(got[o: o + a.size].reshape(a.shape))
    assert np.array_equal(got[outside], (buf if alias else fill)[outside]), "a write left the images"
    return res


@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("kind", ["noise", "checker8"])
def test_ragged_batch_equals_the_restatement(cuda, kind, alias):
    """every size meets every quality of 95, 30, 1, 100 and 0: the vector is rotated five times"""
    images = _images(kind)
    for shift in range(5):
        q, want = _want(kind, shift)
        got = _call(cuda, images, q, alias, 80 + shift)
        for (h, w), qi, g, r, im in zip(SIZES, q, got, want, images):
            assert np.array_equal(g, r), (kind, alias, h, w, qi, int(np.abs(g.astype(int) - r).max()))
            if qi == 0:
                assert np.array_equal(g, im), (h, w)


def test_quality_zero_keeps_the_bytes_and_a_misfit_costs_only_itself(cuda):
    images = _images("noise")
    for alias in (False, True):
        got = _call(cuda, images, [0] * len(images), alias, 90)
        assert all(np.array_equal(g, im) for g, im in zip(got, images))
    # max_pixels below the largest image: that image is skipped (nothing of it is written), the others are served
    q = [95] * len(images)
    got = _call(cuda, images, q, True, 91, max_pixels=23 * 40)
    want = A.roundtrip_ragged(images, q)
    for (h, w), g, r, im in zip(SIZES, got, want, images):
        assert np.array_equal(g, im if h * w > 23 * 40 else r), (h, w)
    # qualities outside 0..100 are clamped by the kernels
    got = _call(cuda, images[:6], [-5, 250, 100, 1, 0, -1], False, 92)
    for g, r in zip(got, A.roundtrip_ragged(images[:6], [0, 100, 100, 1, 0, 0])):
        assert np.array_equal(g, r)


def test_wrapper_and_the_fixed_shape_kernel_at_multiples_of_16(cuda):
    from unet_watermark_amd import data as D
    sizes = [(32, 48), (16, 16)]
    images = _images("noise", sizes, seed=3)
    packed, descs, _ = D.pack_images(images)
    q = [30, 95]
    out = D.device_jpeg_ragged(packed, descs, q)
    assert out.device.type == "cuda" and out.shape == packed.shape
    same = D.device_jpeg_ragged(packed.to(cuda), descs, q, inplace=True)
    got = out.cpu().numpy()
    assert np.array_equal(got, same.cpu().numpy())
    for im, d, qi in zip(images, descs, q):
        o = int(d["offset"])
        _, u8 = D.device_jpeg(torch.from_numpy(im[None]).to(cuda), [qi], return_u8=True)
        assert np.array_equal(got[o: o + im.size].reshape(im.shape), u8[0].cpu().numpy()), im.shape
        assert np.array_equal(u8[0].cpu().numpy(), A.roundtrip_any(im, qi))
    src = packed.to(cuda)
    keep = src.clone()
    assert D.device_jpeg_ragged(src, descs, q).data_ptr() != src.data_ptr() and torch.equal(src, keep), "a copy unless inplace"
    assert D.device_jpeg_ragged(src, descs, q, inplace=True).data_ptr() == src.data_ptr()


def test_one_captured_graph_serves_every_batch(cuda):
    """the same N, other sizes and other qualities within the same `bytes` and `max_pixels`"""
    L, lib = G._lib()
    rng = np.random.default_rng(93)
    sets = [([(9, 17), (24, 24), (5, 4), (40, 23)], [95, 30, 0, 100]), ([(33, 17), (6, 5), (16, 48), (1, 9)], [1, 95, 30, 0])]
    batches = []
    for k, (sizes, q) in enumerate(sets):
        images = _images("noise", sizes, seed=10 + k)
        batches.append((images, q, G._pack(images, rng), A.roundtrip_ragged(images, q)))
    nbytes = max(b[2][0].size for b in batches)
    mp = max(h * w for sizes, _ in sets for h, w in sizes)
    it = torch.zeros(nbytes, dtype=torch.uint8, device=cuda)
    ws = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=cuda)
    dt = torch.zeros(4 * 16, dtype=torch.uint8, device=cuda)
    qt = torch.zeros(4, dtype=torch.int32, device=cuda)

    def call():
        L.check(lib.uwm_jpeg_ragged_u8(_P(it), _P(it), nbytes, _P(dt), _P(qt), 4, 3, mp, _P(ws, GUARD), nbytes, C.c_void_p(L.stream_ptr(cuda))))

    def load(k):
        buf, descs = batches[k][2]
        it.fill_(FILL); it[:buf.size].copy_(torch.from_numpy(buf))
        dt.copy_(torch.from_numpy(descs.view(np.uint8).copy())); qt.copy_(torch.tensor(batches[k][1], dtype=torch.int32))

    def check(k, what):
        torch.cuda.synchronize()
        got = it.cpu().numpy()
        for a, d, r in zip(batches[k][0], batches[k][2][1], batches[k][3]):
            o = int(d["offset"])
            assert np.array_equal(got[o: o + a.size].reshape(a.shape), r), (what, a.shape)

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
    w = ws.cpu().numpy()
    assert (w[:GUARD] == FILL).all() and (w[GUARD + nbytes:] == FILL).all()


# ------------------------------------------------------------------------------------------------ the synthesis pipeline
@needs_freetype
def test_pipeline_with_the_flag_equals_the_chain_of_restatements(cuda, tmp_path):
    """a logo sample, a text sample and a mixed sample through DeviceInputPipeline.to_u8 with jpeg_quality = 95: today's synthesis
    restatements, the round trip where the flag says (a mixed sample between its logos and its text, every sample behind the last
    stage), then the pair mask — of the compressed image — or the untouched alpha rule, then the cv2-convention resize"""
    import pairmask_ref as P
    import resize_ref as R
    import synth_ref as S
    import textsynth_ref as T
    from unet_watermark_amd.data import DeviceInputPipeline, RawSynthDataset
    clean_dir, logos_dir = G._dataset(str(tmp_path), np.random.default_rng(71))
    for source in ("pair", "alpha"):
        kw = dict(seed=6, transparent_ratio=0.0, mask_threshold=15, mask_source=source, text_watermark_ratio=0.4, mixed_watermark_ratio=0.3)
        ds = RawSynthDataset(clean_dir, logos_dir, jpeg_quality=95, **kw)
        items = [ds[i] for i in range(len(ds))]
        kinds = [ds.draw_sample(i, (items[i][0].shape[1], items[i][0].shape[0]))[4] for i in range(len(ds))]
        assert set(kinds) == {"logo", "text", "mixed"}, kinds
        x, m = DeviceInputPipeline(32, cuda, source=ds).to_u8(items)
        plain_x, plain_m = DeviceInputPipeline(32, cuda, source=RawSynthDataset(clean_dir, logos_dir, **kw)).to_u8(items)
        assert not torch.equal(x, plain_x)
        if source == "alpha":
            assert torch.equal(m, plain_m), "masks from the alpha planes are not affected"
        seen = set()
        for k, (clean, logos, jobs, planes, text_jobs) in enumerate(items):
            li, la = S.synth_image(clean, logos, jobs)
            mixed = len(planes) > 0 and bool((jobs["enabled"] != 0).any())
            assert not mixed or kinds[k] == "mixed", (k, kinds[k])
            seen.add((kinds[k], mixed))
            if mixed:
                li = A.roundtrip_any(li, 95)
            wi, wa = T.synth_text_image(li, la, planes, text_jobs, mask_mode=1)
            wi = A.roundtrip_any(wi, 95)
            wm = P.pair_mask(wi, clean, 15) if source == "pair" else wa
            assert np.array_equal(x[k].cpu().numpy(), R.resize_u8_linear(wi, 32, 32)), (source, k, kinds[k])
            assert np.array_equal(m[k].cpu().numpy(), R.resize_u8_nearest(wm, 32, 32)), (source, k, kinds[k])
        assert {("logo", False), ("text", False), ("mixed", True)} <= seen, seen


def test_pipeline_with_quality_zero_equals_the_argument_left_out(cuda, tmp_path):
    from unet_watermark_amd.data import DeviceInputPipeline, RawSynthDataset
    clean_dir, logos_dir = G._dataset(str(tmp_path), np.random.default_rng(72))
    for source in ("pair", "alpha"):
        kw = dict(seed=5, transparent_ratio=0.0, mask_threshold=15, mask_source=source)
        a, b = RawSynthDataset(clean_dir, logos_dir, **kw), RawSynthDataset(clean_dir, logos_dir, jpeg_quality=0, **kw)
        items = [a[i] for i in range(len(a))]
        xa, ma = DeviceInputPipeline(32, cuda, source=a).to_u8(items)
        xb, mb = DeviceInputPipeline(32, cuda, source=b).to_u8([b[i] for i in range(len(b))])
        assert torch.equal(xa, xb) and torch.equal(ma, mb), source


def test_main_synth_writes_the_round_tripped_pixels_as_png(cuda, tmp_path):
    """logo samples: every file written with --jpeg-quality 95 holds the round trip of the file written without the flag"""
    from PIL import Image
    from unet_watermark_amd import cli
    clean_dir, logos_dir = G._dataset(str(tmp_path / "src"), np.random.default_rng(73))
    base = ["synth", "--clean-dir", clean_dir, "--logos-dir", logos_dir, "--count", "4", "--seed", "4", "--batch-size", "3"]
    assert cli.main(base + ["--output-dir", str(tmp_path / "plain")])["written"] == 4
    assert cli.main(base + ["--output-dir", str(tmp_path / "jpeg"), "--jpeg-quality", "95"])["written"] == 4
    names = sorted(os.listdir(str(tmp_path / "plain" / "watermarked")))
    assert names == sorted(os.listdir(str(tmp_path / "jpeg" / "watermarked"))) and len(names) == 4 and all(f.endswith(".png") for f in names)
    for f in names:
        plain, jpeg = (np.asarray(Image.open(str(tmp_path / d / "watermarked" / f))) for d in ("plain", "jpeg"))
        assert np.array_equal(jpeg, A.roundtrip_any(plain, 95)), f
        assert np.array_equal(*(np.asarray(Image.open(str(tmp_path / d / "clean" / f))) for d in ("plain", "jpeg"))), f
