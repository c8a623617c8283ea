"""uwm_inpaint_ragged on the device against the numpy restatement tests/inpaint_ref.py: every result byte-equal, every stats row
equal.  Shapes are the smallest at which the kernels can go wrong: odd sides at every level, level counts from 1 to 8, sizes on both
sides of the 32-pixel tile and of LDS_SIDE = 64, the size up to which a level (and every level above it) runs in LDS in one workgroup
(kLds of csrc/inpaint.hip): 64 x 64 runs wholly there, 33 x 65 has one tiled level below it, 150 x 203 two."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inpaint_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

LDS_SIDE = 64
SIZES = ((1, 7), (7, 1), (2, 2), (3, 5), (31, 33), (33, 65), (64, 64), (97, 131), (150, 203))
FILL, GUARD = 0x5A, 256


@pytest.fixture(scope="module")
def U(cuda):
    import __graft_entry__ as g
    g.build()
    import unet_watermark_amd as U
    return U


def image(h, w, c, seed=0):
    rng = np.random.default_rng(seed + 1000 * h + w)
    y, x = np.mgrid[0:h, 0:w]
    planes = [np.clip(128 + 60 * np.sin(x / (7 + 3 * k)) + 50 * np.cos(y / (5 + 2 * k)) + rng.normal(0, 25, (h, w)), 0, 255) for k in range(c)]
    return np.stack(planes, 2).round().astype(np.uint8)


def masks_of(h, w):
    """the issue's masks at one size, in this order"""
    y, x = np.mgrid[0:h, 0:w]
    bh, bw = max(1, h // 5), max(1, w // 5)
    ey, ex = (y < bh) | (y >= h - bh), (x < bw) | (x >= w - bw)
    my, mx = abs(y - h // 2) <= bh // 2, abs(x - w // 2) <= bw // 2
    m = {
        "pixel": (y == h // 2) & (x == w // 2),
        "edges": (ey & ex) | (ey & mx) | (ex & my),                         # a hole at each corner and on each edge
        "wide": (y >= min(3, h // 3)) & (y < h - min(3, h // 3)) & (x >= min(5, w // 3)) & (x < w - min(5, w // 3)),   # wider than two tiles from 97 x 131 on
        "strokes": ((y % 4 == 1) | (x % 5 == 2)) & ((y < h - 1) | (h == 1)) & ((x < w - 1) | (w == 1)),   # one-pixel strokes: no coarse unknown at all
        "checker": (y + x) % 2 == 0,
        "all_but_one": ~((y == h // 2) & (x == w // 3)),
        "empty": np.zeros((h, w), bool),
        "full": np.ones((h, w), bool),
    }
    return {k: (v * np.uint8(255)).astype(np.uint8) for k, v in m.items()}


_want = {}


def want(im, mask, cycles):
    """inpaint_ref of one image, computed once and never changed"""
    key = (im.shape, im.tobytes(), mask.tobytes(), cycles)
    if key not in _want:
        out, stats = R.inpaint_ref(im, mask, cycles)
        out.setflags(write=False)
        _want[key] = (out, stats)
    return _want[key]


def check(res, stats, images, masks, cycles, names=None):
    for i, (im, mk) in enumerate(zip(images, masks)):
        out, st = want(im, mk, cycles)
        tag = (i, im.shape, names[i] if names else None)
        assert list(stats[i]) == st, tag
        got = res[i].cpu().numpy() if isinstance(res[i], torch.Tensor) else res[i]
        assert np.array_equal(got, out), (tag, int((got != out).sum()), int(np.abs(got.astype(int) - out).max()))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_mask_at_every_size(U, size):
    from unet_watermark_amd.inpaint import DEFAULT_CYCLES, inpaint_ragged
    h, w = size
    ms = masks_of(h, w)
    if h >= 97:
        assert (ms["wide"].any(0).sum() > 2 * 32) and ms["wide"][h // 2].sum() > 2 * 32
    if min(h, w) >= 3:
        assert R.Hierarchy(ms["strokes"] != 0).levels_with_unknowns == 1
    images = [image(h, w, 3, seed=k) for k in range(len(ms))]
    res, stats = inpaint_ragged(images, list(ms.values()), DEFAULT_CYCLES, return_stats=True)
    check(res, stats, images, list(ms.values()), DEFAULT_CYCLES, list(ms))


@pytest.mark.parametrize("cycles", (0, 1, 3))
def test_cycle_counts_one_channel(U, cycles):
    from unet_watermark_amd.inpaint import inpaint_ragged
    images, masks, names = [], [], []
    for h, w in ((3, 5), (33, 65), (97, 131)):
        for name, mk in masks_of(h, w).items():
            if name in ("pixel", "edges", "wide", "checker", "all_but_one"):
                images.append(image(h, w, 1, seed=7)); masks.append(mk); names.append(name)
    res, stats = inpaint_ragged(images, masks, cycles, return_stats=True)
    check(res, stats, images, masks, cycles, names)


def test_single_image_entry_point(U):
    from unet_watermark_amd.inpaint import DEFAULT_CYCLES, inpaint
    im, mk = image(31, 33, 1)[:, :, 0], masks_of(31, 33)["edges"]
    got, st = inpaint(im, mk, return_stats=True)
    out, stats = want(im[:, :, None], mk, DEFAULT_CYCLES)
    assert got.shape == im.shape and np.array_equal(got.cpu().numpy(), out[:, :, 0]) and list(st) == stats


# ---------------------------------------------------------------- the ABI on hand-laid buffers
def _layout(shapes, c, rng):
    """descriptors at ANY alignment with gaps of 1..7 bytes in front of, between and behind the regions -> (descs, total bytes)"""
    from unet_watermark_amd.data import DESC_DTYPE
    descs = np.zeros(len(shapes), DESC_DTYPE)
    off = int(rng.integers(1, 8))
    for i, (h, w) in enumerate(shapes):
        descs[i] = (off, h, w)
        off += h * w * c + int(rng.integers(1, 8))
    return descs, off


def _pack(arrays, descs, nbytes):
    buf = np.full(nbytes, FILL, np.uint8)
    for a, d in zip(arrays, descs):
        o = int(d["offset"])
        buf[o:o + a.size] = a.reshape(-1)
    return buf


def _abi(cuda, images, masks, idescs, ibytes, mdescs, mbytes, cycles, inplace=False, caps=None, expect_rc=0, call_descs=None):
    """uwm_inpaint_ragged on hand-laid buffers; out and the workspace sit between guard bytes, which must come back untouched -> (out
    host buffer, stats).  call_descs: the descriptors the call is given, where they differ from the ones the bytes were laid by"""
    from unet_watermark_amd import _lib as L
    from unet_watermark_amd.data import descs_tensor
    n, c = len(idescs), images[0].shape[2]
    hs, ws = idescs["h"].astype("int64"), idescs["w"].astype("int64")
    max_pixels, rows, max_side = caps or (int((hs * ws).max()), int(hs.sum()), int(max(hs.max(), ws.max())))
    ibuf = torch.from_numpy(_pack(images, idescs, ibytes)).to(cuda)
    mbuf = torch.from_numpy(_pack(masks, mdescs, mbytes)).to(cuda)
    need = L.lib().uwm_inpaint_workspace_bytes(n, ibytes, c, max_side)
    assert need > 0
    wsb = torch.full((GUARD + need + GUARD,), FILL, dtype=torch.uint8, device=cuda)
    outb = ibuf if inplace else torch.full((GUARD + ibytes + GUARD,), FILL, dtype=torch.uint8, device=cuda)
    out_ptr = outb.data_ptr() + (0 if inplace else GUARD)
    assert wsb.data_ptr() % 256 == 0
    stats = torch.full((n, 4), -7, dtype=torch.int64, device=cuda)
    call_i, call_m = call_descs or (idescs, mdescs)
    di, dm = descs_tensor(call_i).to(cuda), descs_tensor(call_m).to(cuda)
    rc = L.lib().uwm_inpaint_ragged(C.c_void_p(ibuf.data_ptr()), C.c_void_p(out_ptr), ibytes, C.c_void_p(di.data_ptr()),
                                    C.c_void_p(mbuf.data_ptr()), mbytes, C.c_void_p(dm.data_ptr()), n, c, cycles, max_pixels, rows, max_side,
                                    C.c_void_p(stats.data_ptr()), C.c_void_p(wsb.data_ptr() + GUARD), need, C.c_void_p(L.stream_ptr(cuda)))
    assert rc == expect_rc, L.lib().uwm_last_error()
    torch.cuda.synchronize()
    host_ws = wsb.cpu().numpy()
    assert (host_ws[:GUARD] == FILL).all() and (host_ws[GUARD + need:] == FILL).all()
    o = outb.cpu().numpy()
    if not inplace:
        assert (o[:GUARD] == FILL).all() and (o[GUARD + ibytes:] == FILL).all()
        o = o[GUARD:GUARD + ibytes]
    return o, stats.cpu().numpy()


def _region(buf, d, c):
    o, h, w = int(d["offset"]), int(d["h"]), int(d["w"])
    return buf[o:o + h * w * c].reshape(h, w, c)


RAGGED = ((33, 65), (3, 5), (97, 131), (64, 64), (1, 7))


def _ragged_batch(c=3):
    images = [image(h, w, c, seed=11 + i) for i, (h, w) in enumerate(RAGGED)]
    kinds = ("edges", "checker", "wide", "all_but_one", "pixel")
    masks = [masks_of(h, w)[k] for (h, w), k in zip(RAGGED, kinds)]
    return images, masks


@pytest.mark.parametrize("inplace", (False, True), ids=("out", "aliased"))
def test_ragged_batch_unaligned_and_one_per_call(U, cuda, inplace):
    from unet_watermark_amd.inpaint import DEFAULT_CYCLES
    rng = np.random.default_rng(5)
    images, masks = _ragged_batch()
    idescs, ibytes = _layout(RAGGED, 3, rng)
    mdescs, mbytes = _layout(RAGGED, 1, rng)
    assert any(int(o) % 4 for o in idescs["offset"]) and any(int(o) % 4 for o in mdescs["offset"])
    out, stats = _abi(cuda, images, masks, idescs, ibytes, mdescs, mbytes, DEFAULT_CYCLES, inplace=inplace)
    check([_region(out, d, 3) for d in idescs], stats, images, masks, DEFAULT_CYCLES)
    covered = np.zeros(ibytes, bool)
    for d in idescs:
        covered[int(d["offset"]): int(d["offset"]) + int(d["h"]) * int(d["w"]) * 3] = True
    assert (out[~covered] == FILL).all()                                   # the gaps between the images
    if not inplace:                                                        # the same images, one per call (other capacities, other launches)
        for i in range(len(RAGGED)):
            o1, s1 = _abi(cuda, images[i:i + 1], masks[i:i + 1], idescs[i:i + 1], ibytes, mdescs[i:i + 1], mbytes, DEFAULT_CYCLES)
            assert np.array_equal(_region(o1, idescs[i], 3), _region(out, idescs[i], 3)) and list(s1[0]) == list(stats[i])


def test_misfits_cost_the_others_nothing(U, cuda):
    """a descriptor that leaves the buffer and a mask of another size: status 3, nothing written there, the neighbours as alone; the
    guard bytes around out and the workspace are checked by _abi"""
    from unet_watermark_amd.inpaint import DEFAULT_CYCLES
    rng = np.random.default_rng(9)
    images, masks = _ragged_batch()
    idescs, ibytes = _layout(RAGGED, 3, rng)
    mdescs, mbytes = _layout(RAGGED, 1, rng)
    bad_i, bad_m = idescs.copy(), mdescs.copy()
    bad_i[1]["offset"] = ibytes - 10                                       # leaves the buffer
    bad_m[3]["w"] = 63                                                     # a mask of another size
    out, stats = _abi(cuda, images, masks, idescs, ibytes, mdescs, mbytes, DEFAULT_CYCLES, call_descs=(bad_i, bad_m))
    assert list(stats[1]) == [0, 3, 0, 0] and list(stats[3]) == [0, 3, 0, 0]
    for i in (0, 2, 4):
        ref, st = want(images[i], masks[i], DEFAULT_CYCLES)
        assert np.array_equal(_region(out, idescs[i], 3), ref) and list(stats[i]) == st, i
    for i in (1, 3):
        assert (_region(out, idescs[i], 3) == FILL).all(), i               # the misfits' regions are not written
    # the capacities: an image above max_pixels, above max_side, and the one whose rows leave `rows`
    for caps, misfit in (((97 * 131 - 1, 10 ** 6, 131), (2,)), ((97 * 131, 10 ** 6, 130), (2,)), ((97 * 131, 33 + 3 + 97, 131), (3, 4))):
        out, stats = _abi(cuda, images, masks, idescs, ibytes, mdescs, mbytes, 1, caps=caps)
        for i in range(5):
            if i in misfit:
                assert list(stats[i]) == [0, 3, 0, 0] and (_region(out, idescs[i], 3) == FILL).all(), (caps, i)
            else:
                assert np.array_equal(_region(out, idescs[i], 3), want(images[i], masks[i], 1)[0]), (caps, i)


def test_argument_refusals(U, cuda):
    from unet_watermark_amd import _lib as L
    lib = L.lib()
    assert lib.uwm_inpaint_workspace_bytes(0, 100, 3, 10) == 0 and lib.uwm_inpaint_workspace_bytes(1, 100, 5, 10) == 0
    assert lib.uwm_inpaint_workspace_bytes(1, 100, 3, 40000) == 0 and lib.uwm_inpaint_launch_count(33, 64) == 0
    assert lib.uwm_inpaint_launch_count(7, 64) == 3 + 6 + 1 + 0 + 7 * 1 + 1 and lib.uwm_inpaint_launch_count(7, 1280) == 98
    images, masks = [image(3, 5, 3)], [masks_of(3, 5)["pixel"]]
    rng = np.random.default_rng(2)
    idescs, ibytes = _layout([(3, 5)], 3, rng)
    mdescs, mbytes = _layout([(3, 5)], 1, rng)
    for caps in ((0, 3, 5), (15, 0, 5), (2 ** 30 + 1, 3, 5)):
        _abi(cuda, images, masks, idescs, ibytes, mdescs, mbytes, 1, caps=caps, expect_rc=1)
    for cycles in (-1, 33):
        _abi(cuda, images, masks, idescs, ibytes, mdescs, mbytes, cycles, expect_rc=1)


def test_one_graph_two_batches_and_repeatability(U, cuda):
    """one captured call replayed on two batches of different sizes under equal capacities; two eager runs are byte-equal"""
    from unet_watermark_amd.data import descs_tensor
    from unet_watermark_amd.inpaint import inpaint_buffers, inpaint_workspace
    cycles, c = 3, 3
    shapes_a, shapes_b = ((97, 131), (33, 65), (31, 33)), ((64, 64), (150, 80), (3, 5))
    caps = dict(max_pixels=150 * 131, rows=97 + 33 + 31 + 150, max_side=150)
    rng = np.random.default_rng(3)
    batches = []
    for shapes, kinds in ((shapes_a, ("wide", "edges", "checker")), (shapes_b, ("all_but_one", "edges", "pixel"))):
        images = [image(h, w, c, seed=21 + i) for i, (h, w) in enumerate(shapes)]
        masks = [masks_of(h, w)[k] for (h, w), k in zip(shapes, kinds)]
        idescs, ibytes = _layout(shapes, c, rng)
        mdescs, mbytes = _layout(shapes, 1, rng)
        batches.append((images, masks, idescs, ibytes, mdescs, mbytes))
    IB, MB = max(b[3] for b in batches), max(b[5] for b in batches)
    ibuf = torch.zeros(IB, dtype=torch.uint8, device=cuda); mbuf = torch.zeros(MB, dtype=torch.uint8, device=cuda)
    di = torch.zeros(48, dtype=torch.uint8, device=cuda); dm = torch.zeros(48, dtype=torch.uint8, device=cuda)
    out = torch.zeros(IB, dtype=torch.uint8, device=cuda); stats = torch.zeros((3, 4), dtype=torch.int64, device=cuda)
    ws = inpaint_workspace(cuda, 3, IB, c, caps["max_side"])

    def load(b):
        ibuf.copy_(torch.from_numpy(np.resize(_pack(b[0], b[2], b[3]), IB))); mbuf.copy_(torch.from_numpy(np.resize(_pack(b[1], b[4], b[5]), MB)))
        di.copy_(descs_tensor(b[2])); dm.copy_(descs_tensor(b[4]))

    def run():
        inpaint_buffers(ibuf, di, mbuf, dm, 3, c, cycles=cycles, out=out, stats=stats, workspace=ws, **caps)

    load(batches[0]); run(); torch.cuda.synchronize()
    first = out.cpu().numpy().copy()
    out.zero_(); run(); torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), first)                        # two eager runs
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for b in (batches[1], batches[0]):
        load(b); out.zero_(); g.replay(); torch.cuda.synchronize()
        o = out.cpu().numpy()
        check([_region(o, d, c) for d in b[2]], stats.cpu().numpy(), b[0], b[1], cycles)


# ---------------------------------------------------------------- the predictor
def test_remove_watermarks_is_the_fill_of_the_predicted_masks(U, cuda):
    import test_surface_gpu as S
    from unet_watermark_amd.inpaint import DEFAULT_CYCLES
    from unet_watermark_amd.predict import WatermarkPredictor
    pred = WatermarkPredictor(model=S._model(cuda), config=S._cfg(), device=cuda, precision="f32")
    images = S._images(((50, 70), (64, 64), (97, 130)), 61)[0]
    pred.threshold = S._median_logit(pred.model, images)
    for mask_type in ("watermark", None):
        before = [m.cpu().numpy() for m in pred.predict_images(images, mask_type=mask_type)]
        res, masks, stats = pred.remove_watermarks(images, mask_type=mask_type, return_masks=True, return_stats=True)
        after = [m.cpu().numpy() for m in pred.predict_images(images, mask_type=mask_type)]
        assert any(0 < (m != 0).sum() < m.size for m in before)
        for b, m, a in zip(before, masks, after):
            assert np.array_equal(b, m.cpu().numpy()) and np.array_equal(b, a)
        check(res, stats, images, before, DEFAULT_CYCLES)
    masks3 = [m.cpu().numpy() for m in pred.predict_images(images, mask_type="watermark")]
    res3, st3 = pred.remove_watermarks(images, cycles=3, return_stats=True)
    check(res3, st3, images, masks3, 3)
    with pytest.raises(ValueError):
        pred.remove_watermarks(images, tile=True, text_enhance=True)
    with pytest.raises(ValueError):
        pred.remove_watermarks(images, cycles=33)


def test_repair_command_with_a_mask_folder(U, cuda, tmp_path, capsys):
    """main.py repair --masks: no model is loaded, the files hold exactly the bytes of the restatement"""
    from PIL import Image
    from unet_watermark_amd.cli import main
    inp, msk, out = (str(tmp_path / d) for d in ("in", "masks", "out"))
    os.makedirs(inp); os.makedirs(msk)
    cases = {"a": ((50, 70), "edges"), "b": ((33, 65), "wide"), "c": ((31, 33), "empty"), "d": ((20, 9), "full")}
    for stem, ((h, w), kind) in cases.items():
        Image.fromarray(image(h, w, 3, seed=3)).save(os.path.join(inp, stem + ".png"))
        Image.fromarray(masks_of(h, w)[kind]).save(os.path.join(msk, stem + ".png"))
    Image.fromarray(image(8, 8, 3)).save(os.path.join(inp, "orphan.png"))
    res = main(["repair", "--input", inp, "--output", out, "--masks", msk, "--cycles", "3", "--batch-size", "3"])
    assert (res["repaired"], res["nothing_to_fill"], res["no_known_pixel"], res["errors"]) == (2, 1, 1, 1)
    assert "repaired 2, nothing to fill 1, no known pixel 1, errors 1" in capsys.readouterr().out
    for stem, ((h, w), kind) in cases.items():
        got = np.asarray(Image.open(os.path.join(out, stem + ".png")))
        assert np.array_equal(got, want(image(h, w, 3, seed=3), masks_of(h, w)[kind], 3)[0]), stem
