"""uwm_edt_ragged and uwm_surface_distances_ragged on the device: one ragged, unaligned batch of the smallest shapes that can go
wrong under every mask kind, misfits, the record cases of DESIGN.md 8u, the sqrt sums (against numpy, run to run, eager against a
replayed graph), WatermarkPredictor.score_images(surface=True) on the three predict paths and `main.py evaluate --surface-distance`
end to end.  Squared distances are integers: every comparison but the sums' is equality with the restatement (tests/surface_ref.py)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import surface_ref as SF  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0x5A                                   # what guard bands must keep
GUARD = 64
UNWRITTEN = -7                                # what entries of d2 that no image covers must keep
SHAPES = ((1, 1), (1, 70), (70, 1), (5, 3), (17, 64), (9, 65), (33, 129), (40, 200), (130, 257), (3, 4100))
KINDS = ("sparse", "half", "dense", "set", "clear", "corner", "twins", "grey")


@pytest.fixture(scope="module")
def L(cuda):
    import __graft_entry__ as g
    g.build()
    from unet_watermark_amd import _lib
    _lib.lib()
    return _lib


def _mask(kind, h, w, rng):
    if kind in ("sparse", "half", "dense"):
        return ((rng.random((h, w)) < {"sparse": 0.01, "half": 0.5, "dense": 0.99}[kind]) * 255).astype(np.uint8)
    if kind == "set":
        return np.full((h, w), 255, np.uint8)
    m = np.zeros((h, w), np.uint8)
    if kind == "corner":                      # one set pixel in a corner: the far corner is the largest distance there is
        m[h - 1, 0] = 255
    elif kind == "twins":                     # two set pixels equidistant from the centre
        m[0, 0] = m[h - 1, w - 1] = 255
    elif kind == "grey":                      # grey values either side of the > 127 rule
        return rng.choice(np.array([126, 127, 128, 129], np.uint8), size=(h, w))
    return m


def _descs(shapes, first=0):
    """the masks back to back from byte `first` on, so most regions start unaligned -> (descs, total bytes)"""
    from unet_watermark_amd.data import DESC_DTYPE
    d = np.zeros(len(shapes), DESC_DTYPE)
    off = first
    for i, (h, w) in enumerate(shapes):
        d[i] = (off, h, w)
        off += h * w
    return d, off


def _pack(masks, descs, nbytes):
    buf = np.full(nbytes + GUARD, FILL, np.uint8)
    for m, d in zip(masks, descs):
        o = int(d["offset"])
        buf[o:o + m.size] = m.reshape(-1)
    return buf


def _caps(descs, max_pixels, rows):
    if max_pixels is None:
        max_pixels = int((descs["h"].astype(np.int64) * descs["w"]).max())
    if rows is None:
        rows = int(descs["h"].sum())
    return max_pixels, rows


def _edt(L, cuda, masks, descs, nbytes, max_pixels=None, rows=None):
    """uwm_edt_ragged on a host buffer of nbytes + GUARD bytes, of which the call is told nbytes -> d2 (nbytes,) with UNWRITTEN where
    nothing was written; checks that the input was not written and that the entries behind d2 and the workspace are intact"""
    from unet_watermark_amd.data import descs_tensor
    lib = L.lib()
    n = len(descs)
    max_pixels, rows = _caps(descs, max_pixels, rows)
    m = torch.from_numpy(masks).to(cuda)
    dd = descs_tensor(descs, cuda)
    d2 = torch.full((nbytes + GUARD,), UNWRITTEN, dtype=torch.int32, device=cuda)
    need = lib.uwm_edt_workspace_bytes(n, nbytes, rows)
    assert need > 0
    ws = torch.empty(need + 256, dtype=torch.uint8, device=cuda)
    ws[need:] = FILL
    L.check(lib.uwm_edt_ragged(C.c_void_p(m.data_ptr()), nbytes, C.c_void_p(dd.data_ptr()), n, max_pixels, rows, C.c_void_p(d2.data_ptr()),
                               C.c_void_p(ws.data_ptr()), need, C.c_void_p(L.stream_ptr(cuda))))
    torch.cuda.synchronize(cuda)
    assert bool((ws[need:] == FILL).all()), "a write behind the workspace"
    assert bool((d2[nbytes:] == UNWRITTEN).all()), "a write behind d2"
    assert np.array_equal(m.cpu().numpy(), masks), "the masks were written"
    assert np.array_equal(dd.cpu().numpy(), descs_tensor(descs).numpy()), "the descriptors were written"
    return d2[:nbytes].cpu().numpy()


def _surface(L, cuda, pred, truth, descs, nbytes, max_pixels=None, rows=None, alias=False):
    """uwm_surface_distances_ragged likewise -> (records (N, 10), sums (N, 2))"""
    from unet_watermark_amd.data import descs_tensor
    lib = L.lib()
    n = len(descs)
    max_pixels, rows = _caps(descs, max_pixels, rows)
    p = torch.from_numpy(pred).to(cuda)
    t = p if alias else torch.from_numpy(truth).to(cuda)
    dd = descs_tensor(descs, cuda)
    records = torch.full((n + 1, 10), -77, dtype=torch.int64, device=cuda)
    sums = torch.full((n + 1, 2), -77.0, dtype=torch.float64, device=cuda)
    need = lib.uwm_surface_distances_workspace_bytes(n, nbytes, rows)
    assert need > 0
    ws = torch.empty(need + 256, dtype=torch.uint8, device=cuda)
    ws[need:] = FILL
    L.check(lib.uwm_surface_distances_ragged(C.c_void_p(p.data_ptr()), C.c_void_p(t.data_ptr()), nbytes, C.c_void_p(dd.data_ptr()), n, max_pixels,
                                             rows, C.c_void_p(records.data_ptr()), C.c_void_p(sums.data_ptr()), C.c_void_p(ws.data_ptr()), need,
                                             C.c_void_p(L.stream_ptr(cuda))))
    torch.cuda.synchronize(cuda)
    assert bool((ws[need:] == FILL).all()), "a write behind the workspace"
    assert bool((records[n] == -77).all()) and bool((sums[n] == -77.0).all()), "a write behind the records or the sums"
    assert np.array_equal(p.cpu().numpy(), pred), "pred was written"
    if not alias:
        assert np.array_equal(t.cpu().numpy(), truth), "truth was written"
    assert np.array_equal(dd.cpu().numpy(), descs_tensor(descs).numpy()), "the descriptors were written"
    return records[:n].cpu().numpy(), sums[:n].cpu().numpy()


def _sums_close(got, want, rec):
    """one rounding per term and per addition: a relative (n + 2) * 2^-52 with n the terms of that sum"""
    for k in range(2):
        tol = (int(rec[k]) + 2) * 2.0 ** -52 * abs(want[k])
        assert abs(got[k] - want[k]) <= tol, (got[k], want[k], int(rec[k]))


def _images_of(d2, descs):
    return [d2[int(d["offset"]): int(d["offset"]) + int(d["h"]) * int(d["w"])].reshape(int(d["h"]), int(d["w"])) for d in descs]


# ---------------------------------------------------------------- the transform
def test_d2_of_one_ragged_batch_equals_the_restatement(L, cuda):
    """every shape under every mask kind: 80 images, laid out from byte 3 on"""
    rng = np.random.default_rng(2000)
    shapes = [s for s in SHAPES for _ in KINDS]
    masks = [_mask(k, h, w, rng) for (h, w) in SHAPES for k in KINDS]
    descs, nbytes = _descs(shapes, first=3)
    d2 = _edt(L, cuda, _pack(masks, descs, nbytes), descs, nbytes)
    assert (d2[:3] == UNWRITTEN).all()
    kinds = [k for _ in SHAPES for k in KINDS]
    for i, (got, m) in enumerate(zip(_images_of(d2, descs), masks)):
        want = SF.d2(SF.binary(m))
        assert np.array_equal(got, want), (i, shapes[i], kinds[i])
        if kinds[i] == "clear":
            assert (got == SF.EDT_NONE).all()
        if kinds[i] == "set":
            assert (got == 0).all()
        if kinds[i] == "corner":
            h, w = shapes[i]
            assert got[0, w - 1] == (h - 1) ** 2 + (w - 1) ** 2
    # the wrapper returns the same map
    from unet_watermark_amd.scoring import distance_transform_ragged
    buf = torch.from_numpy(_pack(masks, descs, nbytes)[:nbytes]).to(cuda)
    again = distance_transform_ragged(buf, descs).cpu().numpy()
    assert again.dtype == np.int32 and np.array_equal(again[3:], d2[3:])


def test_misfits_get_status_one_cost_the_others_nothing_and_are_not_written(L, cuda):
    from unet_watermark_amd.data import DESC_DTYPE
    rng = np.random.default_rng(11)
    good = [(17, 64), (33, 129), (32768, 1), (40, 200)]
    pairs = [(_mask("half", h, w, rng), _mask("sparse", h, w, rng)) for h, w in good]
    pairs[2][1][100, 0] = pairs[2][0][32767, 0] = 255
    gd, nbytes = _descs(good, first=5)
    assert nbytes > 32769 + 5
    descs = np.zeros(8, DESC_DTYPE)
    descs[0] = gd[0]
    descs[1] = (0, 0, 5)                          # a zero side
    descs[2] = gd[1]
    descs[3] = (0, 32769, 1)                      # a side above 32768 (it would fit the buffer and max_pixels)
    descs[4] = gd[2]                              # the longest side there is
    descs[5] = (nbytes - 3, 4, 5)                 # leaves the buffer
    descs[6] = (0, 1, 32769)
    descs[7] = gd[3]
    where = {0: 0, 2: 1, 4: 2, 7: 3}
    pred = _pack([p for p, _ in pairs], gd, nbytes)
    truth = _pack([t for _, t in pairs], gd, nbytes)
    rows = sum(h for h, _ in good)
    want = {i: SF.record(*pairs[k]) for i, k in where.items()}
    want_d2 = {i: SF.d2(SF.binary(pairs[k][0])) for i, k in where.items()}
    for short in (0, 1):                          # then a row capacity one short: the last one no longer fits
        rec, sums = _surface(L, cuda, pred, truth, descs, nbytes, max_pixels=40000, rows=rows - short)
        d2 = _edt(L, cuda, pred, descs, nbytes, max_pixels=40000, rows=rows - short)
        written = np.zeros(nbytes, bool)
        for i in range(8):
            if i in where and not (short and i == 7):
                assert rec[i].tolist() == want[i][0].tolist(), i
                _sums_close(sums[i], want[i][1], rec[i])
                o = int(descs[i]["offset"])
                assert np.array_equal(d2[o:o + want_d2[i].size].reshape(want_d2[i].shape), want_d2[i]), i
                written[o:o + want_d2[i].size] = True
            else:
                assert rec[i].tolist() == SF.MISFIT.tolist() and sums[i].tolist() == [0.0, 0.0], i
        assert (d2[~written] == UNWRITTEN).all()


# ---------------------------------------------------------------- the records
def _rect(h, w, y0, y1, x0, x1):
    m = np.zeros((h, w), np.uint8)
    m[y0:y1, x0:x1] = 255
    return m


_PAIRS = {}


def _pairs():
    """the record cases on pairs from SHAPES, with their reference records (computed once)"""
    if not _PAIRS:
        rng = np.random.default_rng(77)
        preds, truths, names = [], [], []

        def add(name, p, t):
            names.append(name); preds.append(p); truths.append(t)
        for h, w in SHAPES:
            add("random", _mask("half", h, w, rng), _mask("sparse" if h * w > 300 else "half", h, w, rng))
            add("dense", _mask("dense", h, w, rng), _mask("grey", h, w, rng))
            m = _mask("half", h, w, rng)
            add("identical", m, m.copy())
            add("both empty", _mask("clear", h, w, rng), _mask("clear", h, w, rng))
            add("pred empty", _mask("clear", h, w, rng), _mask("corner", h, w, rng))          # n = 1
            add("truth empty", _mask("half", h, w, rng) | _mask("corner", h, w, rng), _mask("clear", h, w, rng))
        for h, w in ((17, 64), (33, 129), (40, 200), (130, 257)):
            add("disjoint rectangles", _rect(h, w, 1, h // 2, 2, w // 3), _rect(h, w, h // 2 + 2, h, w // 2, w - 1))
            add("nested squares", _rect(h, w, 5, 12, 20, 27), _rect(h, w, 0, 17, 15, 32))
            add("touching the edges", _rect(h, w, 0, h, 0, w // 2), _rect(h, w, 3, h - 1, 1, w))
        add("n - 1 = 20", _rect(17, 64, 3, 4, 5, 16), _rect(17, 64, 9, 10, 30, 40))             # a line of 11 and a line of 10 border pixels
        add("single pixels", _rect(5, 3, 0, 1, 0, 1), _rect(5, 3, 4, 5, 2, 3))                  # n = 2
        shapes = [p.shape for p in preds]
        descs, nbytes = _descs(shapes, first=1)
        _PAIRS.update(names=names, preds=preds, truths=truths, shapes=shapes, descs=descs, nbytes=nbytes, want=SF.records(preds, truths))
    return _PAIRS


def test_surface_records_equal_the_restatement(L, cuda):
    b = _pairs()
    rec, sums = _surface(L, cuda, _pack(b["preds"], b["descs"], b["nbytes"]), _pack(b["truths"], b["descs"], b["nbytes"]), b["descs"], b["nbytes"])
    want, want_sums = b["want"]
    for i, name in enumerate(b["names"]):
        assert rec[i].tolist() == want[i].tolist(), (i, name, b["shapes"][i])
        _sums_close(sums[i], want_sums[i], rec[i])
    by = {n: want[[k for k, m in enumerate(b["names"]) if m == n]] for n in set(b["names"])}
    assert (by["identical"][:, [2, 3, 4, 5, 7]] == 0).all() and (by["identical"][:, 8] == 1).all()
    assert (by["both empty"] == [0] * 8 + [1, 0]).all()
    assert (by["pred empty"][:, :2] == [0, 1]).all() and (by["pred empty"][:, 7] == -1).all() and (by["pred empty"][:, 8] == 0).all()
    assert (by["truth empty"][:, 7] == 0).all() and (by["truth empty"][:, 2:6] == -1).all()
    assert by["n - 1 = 20"][0, :2].tolist() == [11, 10] and by["n - 1 = 20"][0, 6] == 0
    assert (by["nested squares"][:, 3] == 25 + 25).all()                       # the outer square's corner to the inner square's corner
    assert (by["disjoint rectangles"][:, 7] > 0).all() and len({tuple(r) for r in want.tolist()}) > 40


def test_pred_aliased_to_truth_and_identical_bits_on_every_run(L, cuda):
    b = _pairs()
    pred, truth = _pack(b["preds"], b["descs"], b["nbytes"]), _pack(b["truths"], b["descs"], b["nbytes"])
    one = _surface(L, cuda, pred, truth, b["descs"], b["nbytes"])
    two = _surface(L, cuda, pred, truth, b["descs"], b["nbytes"])
    assert np.array_equal(one[0], two[0]) and one[1].tobytes() == two[1].tobytes()
    same = _surface(L, cuda, pred, pred.copy(), b["descs"], b["nbytes"])
    alias = _surface(L, cuda, pred, None, b["descs"], b["nbytes"], alias=True)
    assert np.array_equal(same[0], alias[0]) and same[1].tobytes() == alias[1].tobytes()
    assert np.array_equal(same[0], SF.records(b["preds"], b["preds"])[0])
    assert (same[0][:, [2, 3, 4, 5, 7]] == 0).all() and (same[0][:, 8] == 1).all() and (same[1] == 0).all()


def test_a_captured_call_replays_with_the_eager_bits_on_a_batch_of_other_sizes(L, cuda):
    """one torch.cuda.graph capture at N = 4; bytes and descriptors are then overwritten with a batch of other sizes that fits the
    same capacities, and the replay gives the records and the bits of the sums of the eager call"""
    from unet_watermark_amd.data import descs_tensor
    lib = L.lib()
    rng = np.random.default_rng(5)
    n, nbytes, max_pixels, rows = 4, 24000, 8000, 400
    batches = []
    for shapes, first in ((((17, 64), (33, 129), (40, 200), (9, 65)), 0), (((60, 90), (1, 70), (33, 128), (130, 57)), 7)):
        preds = [_mask(k, h, w, rng) for k, (h, w) in zip(("half", "dense", "sparse", "grey"), shapes)]
        truths = [_mask(k, h, w, rng) for k, (h, w) in zip(("sparse", "half", "half", "half"), shapes)]
        descs, used = _descs(shapes, first)
        assert used <= nbytes and sum(h for h, _ in shapes) <= rows
        batches.append((preds, truths, descs))
    p = torch.zeros(nbytes, dtype=torch.uint8, device=cuda)
    t = torch.zeros(nbytes, dtype=torch.uint8, device=cuda)
    dd = torch.zeros(16 * n, dtype=torch.uint8, device=cuda)
    records = torch.zeros((n, 10), dtype=torch.int64, device=cuda)
    sums = torch.zeros((n, 2), dtype=torch.float64, device=cuda)
    need = lib.uwm_surface_distances_workspace_bytes(n, nbytes, rows)
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)

    def load(batch):
        preds, truths, descs = batch
        p.copy_(torch.from_numpy(_pack(preds, descs, nbytes)[:nbytes]))
        t.copy_(torch.from_numpy(_pack(truths, descs, nbytes)[:nbytes]))
        dd.copy_(descs_tensor(descs))

    def call():
        L.check(lib.uwm_surface_distances_ragged(C.c_void_p(p.data_ptr()), C.c_void_p(t.data_ptr()), nbytes, C.c_void_p(dd.data_ptr()), n,
                                                 max_pixels, rows, C.c_void_p(records.data_ptr()), C.c_void_p(sums.data_ptr()),
                                                 C.c_void_p(ws.data_ptr()), need, C.c_void_p(L.stream_ptr(cuda))))
    load(batches[0])
    call()
    torch.cuda.synchronize(cuda)
    assert records.cpu().numpy().tolist() == SF.records(*batches[0][:2])[0].tolist()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    load(batches[1])
    call()
    torch.cuda.synchronize(cuda)
    eager, eager_sums = records.cpu().numpy().copy(), sums.cpu().numpy().copy()
    records.fill_(-1); sums.fill_(-1.0)
    g.replay()
    torch.cuda.synchronize(cuda)
    assert np.array_equal(records.cpu().numpy(), eager) and sums.cpu().numpy().tobytes() == eager_sums.tobytes()
    want, want_sums = SF.records(*batches[1][:2])
    assert eager.tolist() == want.tolist()
    for i in range(n):
        _sums_close(eager_sums[i], want_sums[i], eager[i])


# ---------------------------------------------------------------- the predictor and the command
SIZES = ((50, 70), (64, 64), (97, 130), (150, 81))
_STATE = {}


def _model(dev):
    import unet_watermark_amd as U
    from oracle import unet_oracle as O
    m = U.Unet("resnet18").to(dev)
    m.load_state_dict(O.build("resnet18", seed=3).state_dict())
    xs, _ = O.synthetic_batch(2, 64, 64, seed=5)
    m.train()
    with torch.no_grad():                                          # representative running statistics
        for k in range(3):
            m(xs.to(dev) * (1.0 + 0.1 * k))
    return m.eval()


def _cfg():
    from unet_watermark_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults(); cfg.MODEL.NAME = "Unet"; cfg.MODEL.ENCODER_NAME = "resnet18"; cfg.DATA.IMG_SIZE = 64
    cfg.PREDICT.BATCH_SIZE = 4
    return cfg


def _images(shapes, seed):
    """smooth random images with a bright rectangle each, and random blob truths of the same sizes"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    images, truths = [], []
    for i, (h, w) in enumerate(shapes):
        base = rng.integers(0, 256, size=(h // 6 + 2, w // 6 + 2, 3), dtype=np.uint8)
        a = np.asarray(Image.fromarray(base).resize((w, h), Image.BILINEAR)).copy()
        a[h // 4: h // 4 + h // (2 + i % 3), w // 5: w // 5 + w // 2] = 255 - 40 * (i % 4)
        images.append(a)
        coarse = rng.integers(0, 256, size=(h // 9 + 2, w // 9 + 2), dtype=np.uint8)
        truths.append(np.asarray(Image.fromarray(coarse).resize((w, h), Image.BILINEAR)).copy())       # grey: binarised by the call
    return images, truths


def _median_logit(model, images):
    import unet_watermark_amd as U
    from unet_watermark_amd.constants import IMAGENET_MEAN, IMAGENET_STD
    packed, descs, _ = U.pack_images(images)
    _, lg = model.predict_u8(U.device_resize(packed, descs, 64, 3), IMAGENET_MEAN, IMAGENET_STD, 0.0, return_logits=True)
    return float(lg.median())


def _pred(cuda):
    if "pred" not in _STATE:
        import __graft_entry__ as g
        g.build()
        from unet_watermark_amd.predict import WatermarkPredictor
        pred = WatermarkPredictor(model=_model(cuda), config=_cfg(), device=cuda, precision="f32")
        pred.threshold = _median_logit(pred.model, _images(SIZES, 61)[0])
        _STATE["pred"] = pred
    return _STATE["pred"]


@pytest.mark.parametrize("case", ["plain", "watermark", "tiled"])
def test_score_images_with_surface_measures_the_masks_the_predict_paths_return(cuda, case):
    pred = _pred(cuda)
    images, truths = _images(SIZES, 61)
    kw = dict(tile=True, overlap=16) if case == "tiled" else dict(mask_type="watermark" if case == "watermark" else None)
    plain = pred.score_images(images, truths, **kw)
    counts, (rec, sums), masks = pred.score_images(images, truths, return_masks=True, surface=True, **kw)
    only_counts, (only_rec, only_sums) = pred.score_images(images, truths, surface=True, **kw)
    assert isinstance(plain, np.ndarray) and np.array_equal(plain, counts) and np.array_equal(plain, only_counts)
    assert rec.dtype == np.int64 and rec.shape == (4, 10) and sums.dtype == np.float64 and sums.shape == (4, 2)
    assert np.array_equal(rec, only_rec) and sums.tobytes() == only_sums.tobytes()
    want, want_sums = SF.records([m.cpu().numpy() for m in masks], truths)
    assert rec.tolist() == want.tolist()
    for i in range(4):
        _sums_close(sums[i], want_sums[i], rec[i])
    assert (rec[:, 9] == 0).all() and ((rec[:, 8] == 1).any() or case == "watermark")


def test_main_evaluate_surface_distance_end_to_end(cuda, tmp_path):
    from PIL import Image
    from unet_watermark_amd import cli
    from unet_watermark_amd.checkpoint import save_checkpoint
    from unet_watermark_amd.scoring import SURFACE_FIELDS, summarize_surface, surface_from_record
    pred = _pred(cuda)
    images, truths = _images(SIZES, 62)
    os.makedirs(tmp_path / "d" / "watermarked"); os.makedirs(tmp_path / "d" / "masks")
    for i, (a, t) in enumerate(zip(images, truths)):
        Image.fromarray(a).save(tmp_path / "d" / "watermarked" / f"im{i}.png")
        Image.fromarray(t).save(tmp_path / "d" / "masks" / f"im{i}.png")
    save_checkpoint(str(tmp_path / "m.pth"), pred.model, epoch=1)
    (tmp_path / "c.yaml").write_text(f"MODEL:\n  NAME: Unet\n  ENCODER_NAME: resnet18\nDATA:\n  IMG_SIZE: 64\nPREDICT:\n  THRESHOLD: {pred.threshold!r}\n")
    base = ["evaluate", "--data-dir", str(tmp_path / "d"), "--model", str(tmp_path / "m.pth"), "--config", str(tmp_path / "c.yaml"),
            "--batch-size", "3", "--per-image"]
    cli.main(base + ["--output", str(tmp_path / "plain.json")])
    cli.main(base + ["--output", str(tmp_path / "surface.json"), "--surface-distance"])
    plain, js = json.loads((tmp_path / "plain.json").read_text()), json.loads((tmp_path / "surface.json").read_text())
    assert set(plain) == {"settings", "images", "errors", "error_details", "micro", "imagewise", "per_image"}
    assert "surface_distance" not in plain["settings"] and all("surface" not in r for r in plain["per_image"])
    # without the flag: the report of the flagged run less what the flag adds
    less = {k: v for k, v in js.items() if k != "surface"}
    less["settings"] = {k: v for k, v in js["settings"].items() if k != "surface_distance"}
    less["per_image"] = [{k: v for k, v in r.items() if k != "surface"} for r in js["per_image"]]
    assert less == plain and js["settings"]["surface_distance"] is True and js["images"] == 4
    rows = np.array([[r["surface"]["record"][k] for k in SURFACE_FIELDS] for r in js["per_image"]], dtype=np.int64)
    sums = np.array([r["surface"]["sums"] for r in js["per_image"]], dtype=np.float64)
    assert js["surface"] == json.loads(json.dumps(summarize_surface(rows, sums)))
    for r, row, sm in zip(js["per_image"], rows, sums):
        assert {k: r["surface"][k] for k in ("hd", "hd95", "assd", "asd_pred_to_truth", "asd_truth_to_pred", "cover_radius")} == surface_from_record(row, sm)
    masks = [m.cpu().numpy() for m in pred.predict_images(images)]
    want, want_sums = SF.records(masks, truths)
    assert rows.tolist() == want.tolist()
    for i in range(4):
        _sums_close(sums[i], want_sums[i], rows[i])
