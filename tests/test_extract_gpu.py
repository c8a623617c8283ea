"""Watermark extraction on the device against the numpy / scipy / Pillow restatement (tests/extract_ref.py): stage 1 byte for byte and
integer for integer on one ragged batch of crafted and seeded pairs, stage 2 byte for byte, batch independence, and the tool end to
end.  Every comparison is exact.

The crafted marks are drawn on a coarse grid and enlarged three times, so that every cell is a 3 x 3 block: such shapes pass the
closing and the opening unchanged and reach the fill and the labelling as drawn.  (A one-pixel line cannot: the opening removes it,
which is how it is "dropped at every min_area"; the rule for degenerate polygons is held on the CPU, tests/test_extract.py.)"""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extract_ref as R  # noqa: E402
import resize_ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    import __graft_entry__ as g
    g.build()
    import unet_watermark_amd.extract as E
    return E


def _coarse(rows):
    return np.kron(np.array([[c == "#" for c in r] for r in rows]), np.ones((3, 3), bool))


def _spiral(n):
    """a one-cell-wide square spiral on an n x n grid: the longest chain a labelling has to follow"""
    g = np.zeros((n, n), bool)
    y = x = 0
    dy, dx = 0, 1
    g[0, 0] = True
    while True:
        ny, nx = y + dy, x + dx
        ahead = 0 <= ny < n and 0 <= nx < n and not g[ny, nx]
        ny2, nx2 = ny + dy, nx + dx
        if ahead and not (0 <= ny2 < n and 0 <= nx2 < n and g[ny2, nx2]):
            y, x = ny, nx
            g[y, x] = True
            continue
        dy, dx = dx, -dy                                   # turn right
        ny, nx = y + dy, x + dx
        ny2, nx2 = ny + dy, nx + dx
        if not (0 <= ny < n and 0 <= nx < n) or g[ny, nx] or (0 <= ny2 < n and 0 <= nx2 < n and g[ny2, nx2]):
            return g


def _place(shape, mark, at=(0, 0)):
    m = np.zeros(shape, bool)
    m[at[0]:at[0] + mark.shape[0], at[1]:at[1] + mark.shape[1]] = mark
    return m


def _pair(rng, mark):
    clean = rng.integers(0, 150, mark.shape + (3,), dtype=np.uint8)
    wm = clean.copy()
    wm[mark] += 100
    return wm, clean


def _crafted():
    rng = np.random.default_rng(11)
    diag = _coarse([".#.", "#.#", ".#."])                   # a ring closed only by diagonal links
    gap = _coarse(["###", "#..", "###"])                    # open through a 4-connected gap
    island = _coarse(["#####", "#...#", "#.#.#", "#...#", "#####"])
    rings = _coarse(["#########", "#.......#", "#.#####.#", "#.#...#.#", "#.#.#.#.#", "#.#...#.#", "#.#####.#", "#.......#", "#########"])
    lines = np.zeros((24, 40), bool)
    lines[4, 2:38] = True; lines[9:21, 5] = True; np.fill_diagonal(lines[9:21, 14:26], True)
    cross = np.zeros((33, 41), bool)
    cross[12:20, :] = True; cross[:, 15:24] = True          # touches all four borders
    many = np.kron(np.indices((17, 17)).sum(0) % 2 == 0, np.ones((3, 3), bool))      # 145 blocks that touch at corners: one region
    apart = np.zeros((102, 102), bool)
    apart[::6, ::6] = True
    apart = ndimage.binary_dilation(apart, np.ones((3, 3), bool))[:102, :102]          # 17 x 17 separate blocks
    marks = [
        ("3x3", np.ones((3, 3), bool)),
        ("strip", _place((3, 70), np.ones((3, 9), bool), (0, 30))),
        ("w63", _place((12, 63), _coarse(["##.##"]) , (4, 48))),
        ("w64", _place((12, 64), np.ones((6, 64), bool), (3, 0))),
        ("w65", _place((12, 65), np.ones((5, 7), bool), (7, 58))),
        ("borders", cross),
        ("diagonal ring", _place((15, 70), diag, (3, 59))),
        ("open ring", _place((14, 17), gap, (2, 4))),
        ("island", _place((21, 19), island, (3, 2))),
        ("ring in ring", _place((33, 31), rings, (3, 2))),
        ("lines", lines),
        ("spiral", _coarse(["".join("#" if v else "." for v in r) for r in _spiral(16)])),
        ("identical", np.zeros((9, 14), bool)),
        ("checker", many),
        ("289 blocks", apart),
        ("two far marks", _place((120, 160), np.ones((14, 18), bool), (5, 6)) | _place((120, 160), np.ones((15, 15), bool), (100, 140))),
    ]
    assert dict(marks)["spiral"].shape == (48, 48)
    pairs = [(name,) + _pair(rng, m) for name, m in marks]
    for k in range(6):                                      # seeded: blobs and speckle around the threshold
        h, w = (int(v) for v in rng.integers(20, 90, 2))
        clean = rng.integers(0, 200, (h, w, 3), dtype=np.uint8)
        f = ndimage.gaussian_filter(rng.standard_normal((h, w)), 2.5)
        noise = rng.integers(0, 56, (h, w, 1)) * ((f > np.quantile(f, 0.6)) | (rng.random((h, w)) < 0.15))[..., None]
        pairs.append((f"random{k}", (clean + noise).astype(np.uint8), clean))
    pairs.insert(len(pairs) // 2, ("misfit",) + _pair(rng, _place((10, 12), np.ones((4, 4), bool), (3, 3))))
    return pairs


@pytest.fixture(scope="module")
def batch(E, cuda):
    """the crafted batch on the device, with a misfit descriptor in the middle, run at min_area 0 and 100"""
    from unet_watermark_amd.data import pack_images
    pairs = _crafted()
    mid = [p[0] for p in pairs].index("misfit")
    wm_p, wd, _ = pack_images([p[1] for p in pairs])
    cl_p, cd, _ = pack_images([p[2] for p in pairs])
    cd = cd.copy()
    cd[mid]["h"] -= 1                                       # the clean image of pair `mid` is one row short: a misfit
    wm, cl = wm_p.to(cuda), cl_p.to(cuda)
    runs = {}
    for min_area in (0, 100):
        plane, pd, stats, table = E.extract_regions(wm, cl, wd, 30, min_area, clean_descs=cd)
        runs[min_area] = (plane.cpu().numpy(), pd, stats.cpu().numpy(), table.cpu().numpy())
    torch.cuda.synchronize()
    return dict(pairs=pairs, mid=mid, wm=wm, cl=cl, wd=wd, cd=cd, runs=runs)


@pytest.mark.parametrize("min_area", [0, 100])
def test_stage1_equals_the_restatement(batch, min_area):
    plane, pd, stats, table = batch["runs"][min_area]
    kept_total = 0
    for i, (name, wm, clean) in enumerate(batch["pairs"]):
        h, w = wm.shape[:2]
        o = int(pd[i]["offset"])
        got = plane[o:o + h * w].reshape(h, w)
        if i == batch["mid"]:
            assert stats[i].tolist() == [0, 0, 1, 0] and not table[i].any() and (got == 255).all(), name      # untouched (pre-filled 255)
            continue
        want = R.regions(wm, clean, 30, min_area)
        assert stats[i].tolist() == [want["found"], want["kept"], want["status"], h * w], name
        k = len(want["rows"])
        assert np.array_equal(table[i, :k], want["rows"]) and not table[i, k:].any(), name
        assert np.array_equal(got, want["plane"]), name
        kept_total += k
    by_name = {p[0]: i for i, p in enumerate(batch["pairs"])}
    # the crafted cases do what they were made for
    assert stats[by_name["identical"]].tolist()[:3] == [0, 0, 0] and stats[by_name["lines"]].tolist()[:3] == [0, 0, 0]
    assert stats[by_name["289 blocks"]].tolist()[:3] == ([289, 289, 2] if min_area == 0 else [289, 0, 0])
    assert stats[by_name["checker"]].tolist()[0] == 1 and stats[by_name["spiral"]].tolist()[0] == 1
    if min_area == 0:
        assert table[by_name["3x3"], 0].tolist() == [0, 8, 24, 24, 0, 0, 2, 2, 9]
        assert table[by_name["diagonal ring"], 0, 8] == 4 * 9 + 9 and table[by_name["open ring"], 0, 8] == 7 * 9       # filled / not filled
        assert table[by_name["island"], 0, 8] == 25 * 9 and table[by_name["ring in ring"], 0, 8] == 81 * 9 and stats[by_name["ring in ring"], 0] == 1
        assert table[by_name["borders"], 0, 4:8].tolist() == [0, 0, 40, 32] and stats[by_name["two far marks"], 1] == 2
    assert kept_total > 0


def test_stage1_one_image_alone_equals_it_inside_the_batch_and_runs_repeat(E, batch, cuda):
    from unet_watermark_amd.data import pack_images
    plane, pd, stats, table = batch["runs"][0]
    for name in ("spiral", "random3", "w65"):
        i = [p[0] for p in batch["pairs"]].index(name)
        _, wm, clean = batch["pairs"][i]
        wp, d, _ = pack_images([wm]); cp, _, _ = pack_images([clean])
        p1, _, s1, t1 = E.extract_regions(wp.to(cuda), cp.to(cuda), d, 30, 0)
        o, n = int(pd[i]["offset"]), wm.shape[0] * wm.shape[1]
        assert np.array_equal(p1.cpu().numpy()[:n], plane[o:o + n]) and np.array_equal(s1.cpu().numpy()[0], stats[i])
        assert np.array_equal(t1.cpu().numpy()[0], table[i])
    again = E.extract_regions(batch["wm"], batch["cl"], batch["wd"], 30, 0, clean_descs=batch["cd"])
    assert np.array_equal(again[0].cpu().numpy(), plane) and np.array_equal(again[2].cpu().numpy(), stats)
    assert np.array_equal(again[3].cpu().numpy(), table)


def test_stage1_capacities_make_misfits_not_faults(E, batch):
    sizes = batch["wd"]["h"].astype(np.int64) * batch["wd"]["w"]
    mid, full = batch["mid"], batch["runs"][0][2]
    assert mid > 10
    # an image above max_pixels is a misfit and costs the others nothing
    _, _, stats, _ = E.extract_regions(batch["wm"], batch["cl"], batch["wd"], 30, 0, clean_descs=batch["cd"], max_pixels=2000)
    stats = stats.cpu().numpy()
    big = (sizes > 2000) | (np.arange(len(sizes)) == mid)
    assert 1 < big.sum() < len(big) and np.array_equal(stats[:, 2] == 1, big) and np.array_equal(stats[~big], full[~big])
    # the working planes hold the first ten images only: the others are misfits
    _, _, stats, _ = E.extract_regions(batch["wm"], batch["cl"], batch["wd"], 30, 0, clean_descs=batch["cd"], total_pixels=int(sizes[:10].sum()))
    stats = stats.cpu().numpy()
    assert np.array_equal(stats[:10], full[:10]) and (stats[10:, 2] == 1).all() and not stats[10:, :2].any()


def test_stage2_cutouts_equal_pillow(E, cuda):
    from unet_watermark_amd.data import mask_descs_for, pack_images
    rng = np.random.default_rng(21)
    ims = [ndimage.gaussian_filter(rng.random((h, w, 3)) * 255, (1.5, 1.5, 0)).astype(np.uint8) for h, w in ((37, 53), (64, 65), (3, 3))]
    ims[1][::7] = 255; ims[1][:, ::5] = 0                  # saturating values: every clip of the three blends
    planes = [np.where(rng.random(a.shape[:2]) < 0.5, rng.integers(0, 3, a.shape[:2]), 255).astype(np.uint8) for a in ims]
    cuts = [(0, dict(x=0, y=0, w=53, h=37, members=[0, 2])),           # the whole image
            (0, dict(x=0, y=0, w=20, h=11, members=[1])),              # clipped at the left and top edges; the second job of image 0
            (1, dict(x=40, y=50, w=25, h=14, members=[0])),            # clipped at the right and bottom edges
            (1, dict(x=60, y=0, w=9, h=9, members=[0])),               # outside the image: a misfit between the others
            (1, dict(x=7, y=9, w=3, h=30, members=[1, 2])),
            (2, dict(x=0, y=0, w=3, h=3, members=[0, 1, 2])),
            (2, dict(x=0, y=0, w=2, h=3, members=[0]))]                # a side below 3: a misfit
    jobs, nbytes = E.cutout_jobs([[c for i, c in cuts if i == k] for k in range(3)])
    wp, wd, _ = pack_images(ims)
    pd = mask_descs_for(wd)
    plane = torch.from_numpy(np.concatenate([p.reshape(-1) for p in planes])).to(cuda)
    out, status = E.extract_cutouts(wp.to(cuda), wd, plane, pd, jobs, nbytes)
    out2, _ = E.extract_cutouts(wp.to(cuda), wd, plane, pd, jobs, nbytes)
    out, status = out.cpu().numpy(), status.cpu().numpy()
    assert status.tolist() == [0, 0, 0, 1, 0, 0, 1] and np.array_equal(out, out2.cpu().numpy())
    for j, (i, c) in zip(jobs, cuts):
        o, n = int(j["out_offset"]), c["w"] * c["h"] * 4
        got = out[o:o + n].reshape(c["h"], c["w"], 4)
        if c["x"] + c["w"] > ims[i].shape[1] or c["w"] < 3:
            assert not got.any()                           # nothing written
        else:
            assert np.array_equal(got, R.cutout(ims[i], planes[i], c)), c


def _folder_pairs():
    rng = np.random.default_rng(33)

    def smooth(h, w):
        return ndimage.gaussian_filter(rng.random((h, w, 3)) * 200, (3, 3, 0)).astype(np.uint8)
    pairs = []
    c = smooth(120, 160); w = c.copy()
    w[6:24, 8:40] = 250; w[95:115, 120:150] //= 4; w[95:115, 120:150] += 190           # two marks far apart: two parts
    pairs.append(("far", c, w))
    c = smooth(80, 90); w = c.copy()
    w[30:50, 20:60, 1] = 255 - w[30:50, 20:60, 1]; w[34:40, 30:40] = c[34:40, 30:40]   # one mark with a hole
    pairs.append(("one", c, w))
    c = smooth(100, 140); w = resize_ref.resize_u8_linear(c, 70, 100).copy()
    w[20:45, 30:70] = 240                                                              # the clean file is larger: both go to 70 x 100
    pairs.append(("sizes", c, w))
    c = smooth(40, 40)
    pairs.append(("nothing", c, c.copy()))
    return pairs


def test_extract_command_end_to_end(E, cuda, tmp_path, capsys):
    cdir, wdir, out = tmp_path / "clean", tmp_path / "watermarked", tmp_path / "out"
    cdir.mkdir(); wdir.mkdir()
    pairs = _folder_pairs()
    for stem, c, w in pairs:
        Image.fromarray(c).save(cdir / f"{stem}.png"); Image.fromarray(w).save(wdir / f"{stem}.png")
    Image.fromarray(c).save(cdir / "broken.png"); (wdir / "broken.png").write_bytes(b"not an image")
    Image.fromarray(c).save(cdir / "unpaired.png")
    from unet_watermark_amd.cli import main
    res = main(["extract", "--clean-dir", str(cdir), "--watermarked-dir", str(wdir), "--output-dir", str(out), "--batch-size", "3"])
    files, counts = R.predict_folder(pairs + [("broken", None, None)], 30, 100, E.plan_cutouts)
    assert res == counts == dict(processed=4, extracted=3, written=4, errors=1)
    assert sorted(os.listdir(out)) == sorted(files) == ["far_watermark_part1.png", "far_watermark_part2.png", "one_watermark.png", "sizes_watermark.png"]
    for name, want in files.items():
        assert np.array_equal(R.read_rgba(out / name), want), name
    assert "processed 4 pairs: 3 yielded cut-outs, 4 files written" in capsys.readouterr().out


def test_captured_calls_serve_another_batch(E, cuda):
    """descriptors and jobs on the device, capacities on the host: both calls in one torch.cuda.graph, replayed on a second batch of
    other sizes"""
    import ctypes as C
    from unet_watermark_amd import _lib as L
    from unet_watermark_amd.data import descs_tensor, pack_images
    by_name = {p[0]: p for p in _crafted()}
    batches = [[by_name[k] for k in names] for names in (("island", "w65", "random1"), ("two far marks", "3x3", "ring in ring"))]
    n, laid = 3, []
    for b in batches:
        wp, wd, pd = pack_images([p[1] for p in b])
        cp, _, _ = pack_images([p[2] for p in b])
        whole = [[dict(x=0, y=0, w=p[1].shape[1], h=p[1].shape[0], members=[0])] for p in b]
        laid.append((wp, cp, wd, pd, whole) + E.cutout_jobs(whole))
    sizes = [[p[1].shape[0] * p[1].shape[1] for p in b] for b in batches]
    img_bytes, total, max_pixels = max(x[0].numel() for x in laid), max(sum(s) for s in sizes), max(max(s) for s in sizes)
    out_bytes = max(x[6] for x in laid)
    wm, cl = (torch.empty(img_bytes, dtype=torch.uint8, device=cuda) for _ in range(2))
    plane, out = torch.empty(total, dtype=torch.uint8, device=cuda), torch.empty(out_bytes, dtype=torch.uint8, device=cuda)
    dd, dj = torch.empty(3 * n * 16, dtype=torch.uint8, device=cuda), torch.empty(n * 288, dtype=torch.uint8, device=cuda)
    stats, table = torch.empty((n, 4), dtype=torch.int64, device=cuda), torch.empty((n, 254, 9), dtype=torch.int64, device=cuda)
    status = torch.empty(n, dtype=torch.int32, device=cuda)
    lib = L.lib()
    ws = torch.empty(lib.uwm_extract_workspace_bytes(n, total, n), dtype=torch.uint8, device=cuda)

    def p(t, o=0):
        return C.c_void_p(t.data_ptr() + o)

    def load(k):
        wp, cp, wd, pd, _, jobs, _ = laid[k]
        wm[:wp.numel()].copy_(wp); cl[:cp.numel()].copy_(cp)
        dd.copy_(descs_tensor(np.concatenate([wd, wd, pd])))
        dj.copy_(torch.from_numpy(jobs.view(np.uint8).copy()))
        plane.fill_(7); out.fill_(7); stats.fill_(-1); table.fill_(-1); status.fill_(-1)

    def call():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        L.check(lib.uwm_extract_regions_ragged(p(wm), wm.numel(), p(dd), p(cl), cl.numel(), p(dd, n * 16), n, 3, 30, 0, max_pixels, total, p(plane),
                                               plane.numel(), p(dd, 2 * n * 16), p(stats), p(table), p(ws), ws.numel(), st))
        L.check(lib.uwm_extract_cutouts_ragged(p(wm), wm.numel(), p(dd), p(plane), plane.numel(), p(dd, 2 * n * 16), n, p(dj), n, max_pixels, p(out),
                                               out.numel(), p(status), p(ws), ws.numel(), st))

    def check(k, what):
        torch.cuda.synchronize()
        _, _, _, pd, whole, jobs, _ = laid[k]
        hp, ho, hs, ht = plane.cpu().numpy(), out.cpu().numpy(), stats.cpu().numpy(), table.cpu().numpy()
        assert status.cpu().tolist() == [0, 0, 0], what
        for i, (name, a, b) in enumerate(batches[k]):
            want = R.regions(a, b, 30, 0)
            h, w = a.shape[:2]
            o = int(pd[i]["offset"])
            assert hs[i].tolist() == [want["found"], want["kept"], 0, h * w] and np.array_equal(ht[i, :want["kept"]], want["rows"]), (what, name)
            assert np.array_equal(hp[o:o + h * w].reshape(h, w), want["plane"]), (what, name)
            o = int(jobs["out_offset"][i])
            assert np.array_equal(ho[o:o + h * w * 4].reshape(h, w, 4), R.cutout(a, want["plane"], whole[i][0])), (what, name)

    load(0)
    call()
    check(0, "eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for k in (1, 0):
        load(k)
        graph.replay()
        check(k, f"replay on batch {k}")
