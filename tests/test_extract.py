"""Watermark extraction, the part that needs no device: the rules the device kernels restate, held to literal implementations (a
border follower with the shoelace formulas, scipy's binary_fill_holes, sklearn's DBSCAN, Pillow's ImageEnhance), the host plan's
arithmetic, the command line, and the argument checks of the new entry points, which fail before any launch.  Every comparison is
exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extract_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from unet_watermark_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def E(L):
    import unet_watermark_amd.extract as E
    return E


# ------------------------------------------------------------------------------------------------ the restated OpenCV rules
def test_window_sums_equal_the_shoelace_sums_of_the_followed_outer_border_and_the_fill_is_fill_holes():
    rng = np.random.default_rng(20240)
    nregions = 0
    for k in range(300):
        m = R.random_mask(rng, smooth=k % 2 == 0)
        F = R.fill(m)
        assert np.array_equal(F, ndimage.binary_fill_holes(m))                       # B2, the whole image
        lab, ids = R.label_regions(F)
        comps, _ = ndimage.label(m, np.ones((3, 3), int))
        sums = R.window_sums(F, lab, len(ids))
        for r, rid in enumerate(ids):
            region = lab == r + 1
            comp = comps == comps.reshape(-1)[rid]                                   # the component of m the region grew from
            assert np.array_equal(ndimage.binary_fill_holes(comp), region)           # B2: filling the component's outer polygon
            assert R.shoelace(R.outer_border(comp)) == tuple(int(v) for v in sums[r])      # B4: contourArea, m10, m01
            nregions += 1
    assert nregions > 1000


def test_window_sums_of_known_shapes():
    F = np.zeros((9, 12), bool)
    F[2:6, 3:9] = True                                       # a 4 x 6 block: the polygon through the centres is 3 x 5
    lab, ids = R.label_regions(F)
    assert list(ids) == [2 * 12 + 3]
    a00, a10, a01 = (int(v) for v in R.window_sums(F, lab, 1)[0])
    assert a00 == 2 * 15 and a10 // (3 * a00) == 5 and a01 // (3 * a00) == 3 and a10 == 6 * 15 * 5.5 and a01 == 6 * 15 * 3.5
    line = np.zeros((5, 9), bool)
    line[2, 1:8] = True                                      # a one-pixel line encloses nothing
    lab, _ = R.label_regions(line)
    assert list(R.window_sums(line, lab, 1)[0]) == [0, 0, 0]


def test_fill_closes_diagonal_rings_and_leaves_open_ones():
    ring = np.zeros((7, 7), bool)
    for y, x in ((1, 3), (2, 2), (3, 1), (4, 2), (5, 3), (4, 4), (3, 5), (2, 4)):
        ring[y, x] = True                                    # closed by diagonal links only
    F = R.fill(ring)
    assert F.sum() == 8 + 5 and F[3, 3] and F[2, 3]
    gap = np.zeros((7, 7), bool)
    gap[1:6, 1:6] = True
    gap[2:5, 2:5] = False
    gap[1, 3] = False                                        # a 4-connected way out
    assert np.array_equal(R.fill(gap), gap)


# ------------------------------------------------------------------------------------------------ clustering
def test_clustering_equals_dbscan_up_to_renaming(E):
    from sklearn.cluster import DBSCAN
    rng = np.random.default_rng(7)
    cases = []
    for _ in range(60):
        h, w = (int(v) for v in rng.integers(20, 400, 2))
        n = int(rng.integers(2, 12))
        cases.append((h, w, [(int(rng.integers(0, w)), int(rng.integers(0, h))) for _ in range(n)]))
    # exactly eps apart: the diagonal of 12 x 16 is 20, eps 5.0; (3, 4) steps are at distance 5, (3, 5) steps beyond it
    cases.append((12, 16, [(0, 0), (3, 4), (6, 8), (9, 13), (15, 11)]))
    cases.append((300, 400, [(10, 10), (135, 10), (135, 135), (261, 135), (10, 136)]))      # eps 125.0
    for h, w, pts in cases:
        eps = R.reference_dbscan_eps(h, w)
        want = DBSCAN(eps=eps, min_samples=1).fit(np.array(pts)).labels_
        got = E.cluster_centres(pts, eps)
        assert len(set(zip(want.tolist(), got))) == len(set(want.tolist())) == len(set(got)), (h, w, pts)
        firsts = [got.index(k) for k in range(max(got) + 1)]
        assert firsts == sorted(firsts) and got[0] == 0                                # numbered by each cluster's first point
    assert E.cluster_centres([(0, 0), (3, 4), (6, 8), (9, 13), (15, 11)], 5.0) == [0, 0, 0, 1, 2]


# ------------------------------------------------------------------------------------------------ the host plan
def _row(rid, x0, y0, x1, y1):
    """a solid box as a table row"""
    w, h = x1 - x0, y1 - y0                                  # the polygon through the centres
    a00 = 2 * w * h
    return [rid, a00, 3 * a00 * (x0 + x1) // 2, 3 * a00 * (y0 + y1) // 2, x0, y0, x1, y1, (w + 1) * (h + 1)]


def test_plan_single_region_margins_clipping_and_name(E):
    H, W = 200, 300
    (c,), = E.plan_cutouts([(0, np.array([_row(5, 100, 80, 139, 99)]))], [(H, W)], ["pic"])
    assert c == dict(name="pic_watermark.png", x=80, y=60, w=80, h=60, members=[0])       # margins max(20, int(40*.15)) = 20 both ways
    (c,), = E.plan_cutouts([(0, np.array([_row(5, 0, 0, 199, 9)]))], [(H, W)], ["pic"])
    assert (c["x"], c["y"], c["w"], c["h"]) == (0, 0, 260, 50)          # int(200*.15) = 30: the cut left margin stays in the width
    (c,), = E.plan_cutouts([(0, np.array([_row(5, 250, 180, 299, 199)]))], [(H, W)], ["pic"])
    assert (c["x"], c["y"], c["w"], c["h"]) == (230, 160, 70, 40)       # clipped at the right and bottom edges
    (c,), = E.plan_cutouts([(0, np.array([_row(5, 10, 5, 59, 54)]))], [(H, W)], ["pic"])
    assert (c["x"], c["y"], c["w"], c["h"]) == (0, 0, 90, 90)           # the asymmetry: x = 0, w = 50 + 40, not 10 + 50 + 20


def test_plan_combined_and_parts(E):
    H, W = 400, 600
    near = [_row(1000, 100, 100, 139, 119), _row(2000, 160, 110, 199, 149)]
    (c,), = E.plan_cutouts([(0, np.array(near))], [(H, W)], ["a"])
    assert c == dict(name="a_watermark.png", x=75, y=75, w=150, h=100, members=[0, 1])     # the union box, margins max(25, 12 %)
    far = [_row(90000, 500, 300, 559, 359), _row(1000, 100, 100, 139, 119), _row(2000, 160, 110, 199, 149)]
    far.sort()
    cuts, = E.plan_cutouts([(0, np.array(far))], [(H, W)], ["a"])
    assert [c["name"] for c in cuts] == ["a_watermark_part1.png", "a_watermark_part2.png"]
    assert cuts[0]["members"] == [0, 1] and cuts[1]["members"] == [2]      # part 1 = the cluster of the lowest id
    assert (cuts[1]["x"], cuts[1]["y"], cuts[1]["w"], cuts[1]["h"]) == (475, 275, 110, 110)
    # one region takes the single branch (20 / 15 %), the same box among several the combined one (25 / 12 %)
    (s,), = E.plan_cutouts([(0, np.array(far[:1]))], [(H, W)], ["a"])
    assert (s["x"], s["y"], s["w"], s["h"]) == (80, 80, 80, 60) and (cuts[0]["x"], cuts[0]["y"]) == (75, 75)
    # centres truncate: a10 // (3 * a00)
    rows = np.array([[7, 10, 3 * 10 * 7 + 29, 3 * 10 * 9 + 1, 0, 0, 1, 1, 4], _row(9, 300, 300, 310, 310)])
    cuts, = E.plan_cutouts([(0, rows)], [(H, W)], ["a"])
    assert len(cuts) == 2


def test_plan_statuses_and_jobs(E):
    rows = np.array([_row(5, 100, 80, 139, 99)])
    plans = E.plan_cutouts([(1, rows[:0]), (2, rows[:0]), (0, rows[:0]), (0, rows)], [(50, 50)] * 3 + [(200, 300)])
    assert plans[:3] == [[], [], []] and plans[3][0]["name"] == "image3_watermark.png"
    stats = np.array([[0, 0, 1, 0], [400, 255, 2, 2500], [3, 1, 0, 60000]])
    table = np.zeros((3, E.MAX_REGIONS, 9), np.int64)
    table[2, 0] = rows[0]
    host = E.host_regions(stats, table)
    assert [s for s, _ in host] == [1, 2, 0] and [len(r) for _, r in host] == [0, 0, 1]
    with pytest.raises(ValueError):
        E.plan_cutouts([(0, np.zeros((255, 9), np.int64) + 1)], [(50, 50)])
    jobs, nbytes = E.cutout_jobs(plans)
    assert jobs.dtype.itemsize == 288 == C.sizeof(__import__("unet_watermark_amd")._lib.uwm_extract_job) and len(jobs) == 1
    assert nbytes == 80 * 60 * 4 and int(jobs["image"][0]) == 3 and jobs["member"][0].tolist() == [1] + [0] * 255


# ------------------------------------------------------------------------------------------------ the enhancement
def test_restated_enhancement_equals_pillow():
    rng = np.random.default_rng(3)
    for h, w, lo, hi in ((3, 3, 0, 256), (3, 17, 0, 256), (17, 3, 100, 256), (40, 55, 0, 256), (31, 29, 0, 40), (25, 33, 200, 256), (64, 64, 0, 256)):
        wm = rng.integers(lo, hi, (h, w, 3), dtype=np.uint8)
        plane = np.where(rng.random((h, w)) < 0.5, 0, 255).astype(np.uint8)
        want = R.cutout(wm, plane, dict(x=0, y=0, w=w, h=h, members=[0]))
        rgba = np.dstack([wm, np.where(plane == 0, 255, 0).astype(np.uint8)])
        assert np.array_equal(R.enhance_restated(rgba), want), (h, w)
    smooth = ndimage.gaussian_filter(rng.random((50, 60, 3)) * 255, (3, 3, 0)).astype(np.uint8)
    rgba = np.dstack([smooth, np.full((50, 60), 255, np.uint8)])
    assert np.array_equal(R.enhance_restated(rgba), R.cutout(smooth, np.zeros((50, 60), np.uint8), dict(x=0, y=0, w=60, h=50, members=[0])))


# ------------------------------------------------------------------------------------------------ command line and glue
def test_cli_parsing_and_defaults(L):
    from unet_watermark_amd.cli import build_parser
    a = build_parser().parse_args(["extract", "--clean-dir", "c", "--watermarked-dir", "w", "--output-dir", "o"])
    assert (a.command, a.threshold, a.min_area, a.limit, a.seed, a.batch_size) == ("extract", 30, 100, None, 0, 16)
    a = build_parser().parse_args(["extract", "--clean-dir", "c", "--watermarked-dir", "w", "--output-dir", "o", "--threshold", "12",
                                   "--min-area", "7", "--limit", "3", "--seed", "9", "--batch-size", "2"])
    assert (a.threshold, a.min_area, a.limit, a.seed, a.batch_size) == (12, 7, 3, 9, 2)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["extract", "--clean-dir", "c"])
    import unet_watermark_amd as U
    assert U.WatermarkExtractor is U.extract.WatermarkExtractor and U.plan_cutouts and U.extract_regions and U.extract_cutouts


def _write_pairs(tmp_path, n):
    rng = np.random.default_rng(0)
    (tmp_path / "clean").mkdir(); (tmp_path / "wm").mkdir()
    for i in range(n):
        a = rng.integers(0, 256, (8, 9, 3), dtype=np.uint8)
        Image.fromarray(a).save(tmp_path / "clean" / f"p{i:02d}.png")
        Image.fromarray(a).save(tmp_path / "wm" / (f"p{i:02d}.jpg" if i % 2 else f"p{i:02d}.png"))
    Image.fromarray(a).save(tmp_path / "clean" / "lonely.png")
    (tmp_path / "wm" / "notes.txt").write_text("x")


def test_pairs_by_stem_and_the_seeded_limit(E, tmp_path):
    _write_pairs(tmp_path, 10)
    pairs = E.list_pairs(str(tmp_path / "clean"), str(tmp_path / "wm"))
    assert [p[0] for p in pairs] == [f"p{i:02d}" for i in range(10)] and pairs[1][2].endswith("p01.jpg")
    a, b, c = E.sample_pairs(pairs, 4, 0), E.sample_pairs(pairs, 4, 0), E.sample_pairs(pairs, 4, 1)
    assert a == b and len(a) == 4 and len(set(a)) == 4 and a != c
    assert E.sample_pairs(pairs, None, 0) == pairs and E.sample_pairs(pairs, 10, 0) == pairs and E.sample_pairs(pairs, 99, 0) == pairs


def test_no_cpu_fallback(E, tmp_path):
    wm = torch.zeros(27, dtype=torch.uint8)
    d = np.zeros(1, E.DESC_DTYPE); d[0] = (0, 3, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        E.extract_regions(wm, wm, d)
    jobs = np.zeros(1, E.EXTRACT_JOB_DTYPE)
    with pytest.raises(RuntimeError, match="HIP device"):
        E.extract_cutouts(wm, d, torch.zeros(9, dtype=torch.uint8), d, jobs)
    if not torch.cuda.is_available():
        _write_pairs(tmp_path, 2)
        with pytest.raises(RuntimeError, match="HIP device"):
            E.WatermarkExtractor(tmp_path / "clean", tmp_path / "wm", tmp_path / "out").process_all_images()
        from unet_watermark_amd.cli import main
        with pytest.raises(SystemExit, match="HIP device"):
            main(["extract", "--clean-dir", str(tmp_path / "clean"), "--watermarked-dir", str(tmp_path / "wm"), "--output-dir", str(tmp_path / "o")])
    with pytest.raises(ValueError):
        E.WatermarkExtractor("a", "b", "c", threshold=300)


def test_entry_points_check_arguments_before_any_launch(L):
    lib = L.lib()
    P = C.c_void_p
    a = P(0x1000)                                            # never dereferenced: every call below fails its checks first

    def err():
        return lib.uwm_last_error().decode()
    assert lib.uwm_extract_workspace_bytes(0, 0, 0) == 0 and "N and J" in err()
    assert lib.uwm_extract_workspace_bytes(70000, 10, 0) == 0 and lib.uwm_extract_workspace_bytes(1, 0, 0) == 0 and "total_pixels" in err()
    need = lib.uwm_extract_workspace_bytes(2, 1000, 0)
    assert need >= 10 * 1000 and lib.uwm_extract_workspace_bytes(0, 0, 5) >= 5 * 8
    assert lib.uwm_extract_workspace_bytes(2, 1000, 5) == max(need, lib.uwm_extract_workspace_bytes(0, 0, 5))

    def regions(**kw):
        v = dict(wm=a, wm_bytes=100, wd=a, clean=a, clean_bytes=100, cd=a, N=1, C=3, thr=30, area=100, maxp=100, total=100, plane=a, plane_bytes=100,
                 pd=a, stats=a, table=a, ws=a, ws_bytes=1 << 30)
        v.update(kw)
        return lib.uwm_extract_regions_ragged(v["wm"], v["wm_bytes"], v["wd"], v["clean"], v["clean_bytes"], v["cd"], v["N"], v["C"], v["thr"],
                                              v["area"], v["maxp"], v["total"], v["plane"], v["plane_bytes"], v["pd"], v["stats"], v["table"],
                                              v["ws"], v["ws_bytes"], P(0))
    for kw, word in ((dict(wm=P(0)), "null"), (dict(table=P(0)), "null"), (dict(C=4), "C must be 3"), (dict(thr=256), "threshold"),
                     (dict(area=-1), "min_area"), (dict(N=0), ">= 1"), (dict(N=70000), "65535"), (dict(total=0), "total_pixels"),
                     (dict(maxp=0), "max_pixels"), (dict(maxp=(1 << 30) + 1), "max_pixels"), (dict(wd=P(0x1004)), "aligned"),
                     (dict(wm=P(0x1001)), "aligned"), (dict(ws_bytes=16), "workspace too small")):
        assert regions(**kw) == 1 and word in err(), (kw, err())

    def cutouts(**kw):
        v = dict(wm=a, wm_bytes=100, wd=a, plane=a, plane_bytes=100, pd=a, N=1, jobs=a, J=1, maxc=100, out=a, out_bytes=400, status=a, ws=a,
                 ws_bytes=1 << 20)
        v.update(kw)
        return lib.uwm_extract_cutouts_ragged(v["wm"], v["wm_bytes"], v["wd"], v["plane"], v["plane_bytes"], v["pd"], v["N"], v["jobs"], v["J"],
                                              v["maxc"], v["out"], v["out_bytes"], v["status"], v["ws"], v["ws_bytes"], P(0))
    for kw, word in ((dict(jobs=P(0)), "null"), (dict(J=0), ">= 1"), (dict(J=70000), "65535"), (dict(maxc=0), "max_crop_pixels"),
                     (dict(out=P(0x1002)), "aligned"), (dict(jobs=P(0x1004)), "aligned"), (dict(ws_bytes=8), "workspace too small")):
        assert cutouts(**kw) == 1 and word in err(), (kw, err())


def test_written_cutouts_serve_as_a_logos_dir(E, tmp_path):
    """what one extraction writes (here: the restatement's files, which the device test holds the tool to) is a --logos-dir"""
    from unet_watermark_amd.data import RawSynthDataset
    rng = np.random.default_rng(5)
    clean = ndimage.gaussian_filter(rng.random((90, 120, 3)) * 255, (4, 4, 0)).astype(np.uint8)
    wm = clean.copy()
    wm[20:50, 30:80] = 255 - wm[20:50, 30:80] // 2
    files, counts = R.predict_folder([("shot", clean, wm)], 30, 100, E.plan_cutouts)
    assert counts == dict(processed=1, extracted=1, written=1, errors=0) and list(files) == ["shot_watermark.png"]
    (tmp_path / "logos").mkdir(); (tmp_path / "clean").mkdir()
    for name, rgba in files.items():
        assert rgba.shape[2] == 4 and rgba[..., 3].max() == 255 and rgba[..., 3].min() == 0
        Image.fromarray(rgba).save(tmp_path / "logos" / name)
    Image.fromarray(clean).save(tmp_path / "clean" / "c0.png")
    ds = RawSynthDataset(str(tmp_path / "clean"), str(tmp_path / "logos"), seed=1)
    img, logos, jobs = ds[0]
    assert len(ds.logos) == 1 and logos and all(a.shape == files["shot_watermark.png"].shape for a in logos)
    assert np.array_equal(logos[0], files["shot_watermark.png"]) and int((jobs["enabled"] != 0).sum()) >= 1
