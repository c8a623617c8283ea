"""uwm_enhance_masks_ragged on the device: one ragged batch (tests/enhance_ref.py: images) at every parameter set of the issue
against the restatement enhance_reduced fed the library's own taps, in-place use, repeatability, a call without stats, misfits,
the Python entry points, a captured call replayed on another batch, and the command line.  Every comparison is byte equality.

The shape that overshoots the kernels' tile by one pixel in each direction is 65 x 65 (the tile is 64 x 64: kT of
csrc/mask_enhance.hip, enhance_ref.TILE)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import enhance_ref as E  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0x5A                                   # what gaps, guard band and untouched regions must keep
GUARD = 64


@pytest.fixture(scope="module")
def U(cuda):
    import __graft_entry__ as g
    g.build()
    import unet_watermark_amd as U
    return U


def _taps(blur_kernel):
    """what the restatement is fed: None for no blur, else the library's very taps"""
    from unet_watermark_amd import _lib as L
    if blur_kernel == 0:
        return None
    buf = (C.c_float * 63)()
    k = L.lib().uwm_enhance_gauss_taps(blur_kernel, buf)
    assert k == blur_kernel | 1
    return np.array(buf[:k], np.float32)


_want = {}


def want(im, params):
    """enhance_reduced of one image at one parameter set, computed once and never changed"""
    key = (im.shape, im.tobytes(), params)
    if key not in _want:
        _want[key] = E.enhance_reduced(im, _taps(params[1]), params[0], params[2])
        _want[key].setflags(write=False)
    return _want[key]


def _layout(shapes, rng):
    """mask descriptors at ANY alignment with gaps of 1..7 bytes in front of, between and behind the masks -> (descs, total bytes)"""
    from unet_watermark_amd.data import DESC_DTYPE
    descs = np.zeros(len(shapes), DESC_DTYPE)
    off = int(rng.integers(1, 8))
    for i, (h, w) in enumerate(shapes):
        descs[i] = (off, h, w)
        off += h * w + int(rng.integers(1, 8))
    return descs, off


def _pack(images, descs, nbytes):
    buf = np.full(nbytes + GUARD, FILL, np.uint8)
    for im, d in zip(images, descs):
        o = int(d["offset"])
        buf[o:o + im.size] = im.reshape(-1)
    return buf


def _region(buf, d):
    o, h, w = int(d["offset"]), int(d["h"]), int(d["w"])
    return buf[o:o + h * w].reshape(h, w)


def _call(cuda, buf, descs, nbytes, params, max_pixels=None, inplace=False, with_stats=True):
    """the ABI call on a host buffer of nbytes + GUARD bytes, of which the call is told nbytes -> (out buffer, stats (N, 4) or None)"""
    from unet_watermark_amd import _lib as L
    from unet_watermark_amd.data import descs_tensor
    lib = L.lib()
    n = len(descs)
    if max_pixels is None:
        max_pixels = int((descs["h"].astype(np.int64) * descs["w"]).max())
    src = torch.from_numpy(buf).to(cuda)
    dst = src if inplace else torch.full_like(src, FILL)
    dd = descs_tensor(descs, cuda)
    stats = torch.full((n, 4), -77, dtype=torch.int64, device=cuda) if with_stats else None
    need = lib.uwm_enhance_masks_workspace_bytes(n, nbytes)
    assert need > 0
    ws = torch.empty(need + 256, dtype=torch.uint8, device=cuda)
    ws[need:] = FILL
    L.check(lib.uwm_enhance_masks_ragged(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), nbytes, C.c_void_p(dd.data_ptr()), n,
                                         params[0], params[1], params[2], max_pixels, C.c_void_p(stats.data_ptr() if with_stats else 0),
                                         C.c_void_p(ws.data_ptr()), need, C.c_void_p(L.stream_ptr(cuda))))
    torch.cuda.synchronize(cuda)
    assert bool((ws[need:] == FILL).all()), "a write behind the workspace"
    if not inplace:
        assert torch.equal(src.cpu(), torch.from_numpy(buf)), "the input was written"
    return dst.cpu().numpy(), (stats.cpu().numpy() if with_stats else None)


def _untouched(out, descs, nbytes, skip=()):
    """everything outside the images' regions (gaps, guard band) and the regions of `skip` still hold the fill byte"""
    covered = np.zeros(len(out), bool)
    for i, d in enumerate(descs):
        if i not in skip:
            o = int(d["offset"])
            covered[o:o + int(d["h"]) * int(d["w"])] = True
    assert (out[~covered] == FILL).all(), "a write outside the masks"
    assert (out[nbytes:] == FILL).all(), "a write into the guard band"


def _row(im, res):
    return [int((im > 127).sum()), int((res > 127).sum()), im.size, 0]


@pytest.mark.parametrize("params", E.PARAMS)
def test_the_batch_equals_the_restatement(U, cuda, params):
    images = E.batch_for(params)
    descs, nbytes = _layout([im.shape for im in images], np.random.default_rng(51))
    buf = _pack(images, descs, nbytes)
    out, stats = _call(cuda, buf, descs, nbytes, params)
    _untouched(out, descs, nbytes)
    for i, (im, d) in enumerate(zip(images, descs)):
        res = want(im, params)
        got = _region(out, d)
        assert np.array_equal(got, res), (params, i, im.shape, int((got != res).sum()))
        assert stats[i].tolist() == _row(im, res), (params, i, im.shape)
    # in place, a second run, and a call without stats give the same bytes
    again, stats2 = _call(cuda, buf, descs, nbytes, params)
    assert np.array_equal(again, out) and np.array_equal(stats2, stats)
    inplace, stats3 = _call(cuda, buf, descs, nbytes, params, inplace=True)
    assert np.array_equal(inplace, out) and np.array_equal(stats3, stats)
    none, no_stats = _call(cuda, buf, descs, nbytes, params, with_stats=False)
    assert no_stats is None and np.array_equal(none, out)
    # max_pixels is a capacity: a generous one changes nothing
    big, stats4 = _call(cuda, buf, descs, nbytes, params, max_pixels=3_000_000)
    assert np.array_equal(big, out) and np.array_equal(stats4, stats)


def test_misfits_cost_only_themselves(U, cuda):
    from unet_watermark_amd.data import DESC_DTYPE
    params = (2, 4, 1)
    rng = np.random.default_rng(52)
    shapes = [(20, 30), (5, 5), (8, 8), (40, 50), (10, 10), (6, 7), (25, 8), (3, 3)]
    descs, nbytes = _layout(shapes, rng)
    images = [((rng.random(s) < 0.3) * rng.integers(100, 256, s)).astype(np.uint8) for s in shapes]
    buf = _pack(images, descs, nbytes)
    descs = descs.astype(DESC_DTYPE)
    descs[1]["h"] = 0                                        # a zero side
    descs[2]["offset"] = nbytes - 10                         # its region leaves [0, mask_bytes) (and would reach the guard band)
    descs[5]["offset"] = -4                                  # ... at the other end
    descs[6]["h"] = (1 << 30) + 1                            # an oversized side
    descs[7]["w"] = -3
    max_pixels = 1500                                        # image 3 has 2000 pixels
    misfit = [False, True, True, True, False, True, True, True]
    out, stats = _call(cuda, buf, descs, nbytes, params, max_pixels=max_pixels)
    assert (out[nbytes:] == FILL).all()
    covered = np.zeros(len(out), bool)
    for i, m in enumerate(misfit):
        if m:
            assert stats[i].tolist() == [0, 0, 0, 1], (i, stats[i].tolist())
        else:
            o = int(descs[i]["offset"])
            covered[o:o + images[i].size] = True
            res = want(images[i], params)
            assert np.array_equal(_region(out, descs[i]), res) and stats[i].tolist() == _row(images[i], res), i
    assert (out[~covered] == FILL).all(), "a misfit's bytes were written"
    # the same batch with room for image 3: only the malformed ones stay misfits
    out2, stats2 = _call(cuda, buf, descs, nbytes, params, max_pixels=2000)
    assert stats2[:, 3].tolist() == [0, 1, 1, 0, 0, 1, 1, 1]
    for i in (0, 3, 4):
        assert np.array_equal(_region(out2, descs[i]), want(images[i], params)), i


def test_python_entry_points(U, cuda):
    """the ragged result of each image equals postprocess.enhance_mask on that image alone; host descriptors, a new output buffer,
    the stats tensor, the (N, H, W) form, out = the input"""
    from unet_watermark_amd.postprocess import ENHANCE_STATS_FIELDS, enhance_mask, enhance_masks_ragged
    params = (10, 15, 2)
    images = E.images()
    descs, nbytes = _layout([im.shape for im in images], np.random.default_rng(53))
    buf = torch.from_numpy(_pack(images, descs, nbytes)[:nbytes].copy()).to(cuda)
    out, stats = enhance_masks_ragged(buf, descs, return_stats=True)
    assert out.data_ptr() != buf.data_ptr() and stats.shape == (len(images), 4) == (len(images), len(ENHANCE_STATS_FIELDS))
    host = out.cpu().numpy()
    for im, d, row in zip(images, descs, stats.cpu().numpy()):
        alone, row1 = enhance_mask(torch.from_numpy(im).to(cuda), return_stats=True)
        assert alone.shape == im.shape and np.array_equal(alone.cpu().numpy(), _region(host, d)), im.shape
        assert np.array_equal(_region(host, d), want(im, params)) and row.tolist() == row1.cpu().tolist() == _row(im, want(im, params))
    stack = torch.from_numpy(np.stack([images[5], images[5].T.copy(), 255 - images[5]])).to(cuda)
    res = enhance_mask(stack, 3, 7, 0)
    for k in range(3):
        assert np.array_equal(res[k].cpu().numpy(), want(stack[k].cpu().numpy(), (3, 7, 0))), k
    same = enhance_mask(stack, 3, 7, 0, out=stack)
    assert same.data_ptr() == stack.data_ptr() and torch.equal(stack, res)
    with pytest.raises(ValueError):
        enhance_masks_ragged(buf, descs, expand_pixels=32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enhance_masks_ragged(buf.cpu(), descs)


def test_a_captured_call_serves_another_batch(U, cuda):
    """descriptors on the device, capacities on the host: one torch.cuda.graph, replayed on a second batch of other sizes"""
    from unet_watermark_amd.data import descs_tensor
    from unet_watermark_amd.postprocess import enhance_masks_ragged
    params = (4, 9, 1)
    ims = E.images()
    batches = [[ims[4], ims[1], ims[7], ims[3]], [ims[5], ims[10], ims[0], ims[9]]]
    laid = [_layout([im.shape for im in b], np.random.default_rng(54 + k)) for k, b in enumerate(batches)]
    nbytes = max(nb for _, nb in laid)
    max_pixels = max(im.size for b in batches for im in b)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    out = torch.empty_like(buf)
    dd = torch.empty(16 * 4, dtype=torch.uint8, device=cuda)
    stats = torch.empty((4, 4), dtype=torch.int64, device=cuda)

    def load(k):
        buf.copy_(torch.from_numpy(_pack(batches[k], laid[k][0], nbytes)[:nbytes].copy()))
        dd.copy_(descs_tensor(laid[k][0]))
        out.fill_(FILL); stats.fill_(-1)

    def call():
        enhance_masks_ragged(buf, dd, *params, return_stats=True, out=out, n=4, max_pixels=max_pixels, stats=stats)

    def check(k, what):
        torch.cuda.synchronize()
        host = out.cpu().numpy()
        _untouched(np.concatenate([host, np.full(GUARD, FILL, np.uint8)]), laid[k][0], nbytes)
        for im, d, row in zip(batches[k], laid[k][0], stats.cpu().numpy()):
            assert np.array_equal(_region(host, d), want(im, params)) and row.tolist() == _row(im, want(im, params)), (what, im.shape)

    load(0)
    call()                                                   # eager: the first call allocates the workspace
    check(0, "eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for k in (1, 0):
        load(k)
        graph.replay()
        check(k, f"replay on batch {k}")


def test_command_line(U, cuda, tmp_path, capsys):
    from PIL import Image
    from unet_watermark_amd.cli import main
    ims = E.images()
    src, dst = tmp_path / "masks", tmp_path / "enhanced"
    src.mkdir()
    files = {"a.png": ims[5], "b.png": ims[4], "c.png": ims[7], "d.png": ims[10]}
    for name, im in files.items():
        Image.fromarray(im).save(src / name)
    (src / "notes.txt").write_text("not a mask")
    (src / "broken.png").write_bytes(b"not a png")
    res = main(["enhance-masks", "--mask-dir", str(src), "--output-dir", str(dst), "--expand-pixels", "3", "--blur-kernel", "7",
                "--smooth-iterations", "0", "--batch-size", "3"])
    assert res["written"] == 4 and res["unreadable"] == 1
    assert sorted(os.listdir(dst)) == sorted(files)
    text = capsys.readouterr().out
    for name, im in files.items():
        res_im = want(im, (3, 7, 0))
        assert np.array_equal(np.asarray(Image.open(dst / name)), res_im), name
        assert np.array_equal(np.asarray(Image.open(src / name)), im), name                     # the inputs stay
        assert f"{name}: foreground {(im > 127).mean():.4f} -> {(res_im > 127).mean():.4f}" in text
    with pytest.raises(SystemExit):                                                            # overwriting needs --in-place
        main(["enhance-masks", "--mask-dir", str(src), "--output-dir", str(src)])
    with pytest.raises(SystemExit):
        main(["enhance-masks", "--mask-dir", str(src)])
    capsys.readouterr()
    for name, im in files.items():
        assert np.array_equal(np.asarray(Image.open(src / name)), im), name
    res = main(["enhance-masks", "--mask-dir", str(src), "--in-place"])
    assert res["written"] == 4 and (src / "broken.png").read_bytes() == b"not a png"
    for name, im in files.items():
        assert np.array_equal(np.asarray(Image.open(src / name)), want(im, (10, 15, 2))), name
