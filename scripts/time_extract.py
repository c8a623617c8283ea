#!/usr/bin/env python3
"""Device time of the watermark extraction (uwm_extract_regions_ragged, uwm_extract_cutouts_ragged) on 64 pairs of 720 x 1280 beside the
numpy / scipy / Pillow restatement (tests/extract_ref.py) on 16 processes of the same box.

The pairs: the seeded photographs of scripts/time_maskpost_ragged.py as clean images, and as marks the masks that script times
(tests/maskpost_ref.synth: blobs, strokes, 1 % noise), each mark pixel moved by 90 grey levels.  The cut-outs are those the host plan
(extract.plan_cutouts) asks for.

  (a) stage 1, one call          (b) stage 2, one call          (c) the restatement of both stages, 16 worker processes, host clock

2 warm-ups, then 7 windows of 20 calls each, HIP events around a window; the figure is the median of the windows with the least and
the greatest beside it.  The library is called with buffers made once, so no allocation or fill is inside a window.  (c) runs first,
before the device is touched, so its workers never hold it.  --profile: 3 calls of each stage and nothing else, for a run under
`rocprofv3 --kernel-trace --stats`, which gives the share of each kernel.

  python scripts/time_extract.py [--out profiles/extract_mi355x.txt] [--images 64] [--windows 7] [--no-cpu] [--profile]"""
import argparse, ctypes as C, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def make_pairs(n, h, w):
    import maskpost_ref
    from time_maskpost_ragged import photographs
    cleans = photographs(n, h, w, 9)
    pairs = []
    for i, c in enumerate(cleans):
        m = maskpost_ref.synth(h, w, 2000 + i)
        wm = c.copy()
        wm[m] = np.where(c[m] < 128, c[m] + 90, c[m] - 90)
        pairs.append((wm, c))
    return pairs


def cpu_one(args):
    """one pair through the restatement: regions, plan, cut-outs -> the number of cut-outs"""
    import extract_ref as R
    from unet_watermark_amd.extract import plan_cutouts
    wm, clean, thr, area = args
    r = R.regions(wm, clean, thr, area)
    cuts = plan_cutouts([(r["status"], r["rows"])], [wm.shape[:2]])[0]
    return len([R.cutout(wm, r["plane"], c) for c in cuts])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "extract_mi355x.txt"))
    ap.add_argument("--images", type=int, default=64); ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--no-cpu", action="store_true"); ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    n, h, w, thr, area = a.images, 720, 1280, 30, 100
    pairs = make_pairs(n, h, w)
    cpu_s = ncut_cpu = None
    if not a.no_cpu and not a.profile:
        import multiprocessing as mp
        with mp.get_context("spawn").Pool(16) as pool:
            pool.map(cpu_one, [p + (thr, area) for p in pairs[:16]])             # the workers' imports
            t0 = time.perf_counter()
            ncut_cpu = sum(pool.map(cpu_one, [p + (thr, area) for p in pairs], chunksize=1))
            cpu_s = time.perf_counter() - t0
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_extract needs a HIP device (a timing without one says nothing)")
    import unet_watermark_amd as U
    import unet_watermark_amd.extract as E
    from unet_watermark_amd import _lib as L
    from unet_watermark_amd.data import descs_tensor
    from time_maskpost_ragged import event_ms, fmt, windows
    dev = torch.device("cuda:0")
    wp, wd, pd = U.pack_images([p[0] for p in pairs])
    cp, _, _ = U.pack_images([p[1] for p in pairs])
    wm, cl = wp.to(dev), cp.to(dev)
    plane, _, stats, table = E.extract_regions(wm, cl, wd, thr, area)
    regions = E.host_regions(stats, table)
    plans = E.plan_cutouts(regions, [(h, w)] * n)
    jobs, nbytes = E.cutout_jobs(plans)
    out, status = E.extract_cutouts(wm, wd, plane, pd, jobs, nbytes)
    assert int(status.abs().sum()) == 0
    s = stats.cpu().numpy()
    say(f"scripts/time_extract.py : {torch.cuda.get_device_name(0)}, {n} pairs of {h} x {w}, threshold {thr}, min_area {area}")
    say(f"regions found {int(s[:, 0].sum())}, kept {int(s[:, 1].sum())}, statuses {sorted(set(s[:, 2].tolist()))}; {len(jobs)} cut-outs, "
        f"{nbytes / 4e6:.2f} M RGBA pixels (largest {int((jobs['w'].astype(np.int64) * jobs['h']).max())})")
    lib = L.lib()
    dd = descs_tensor(np.concatenate([wd, wd, pd]), dev)
    step = n * 16
    dj = torch.from_numpy(jobs.view(np.uint8).copy()).to(dev)
    total, maxc = n * h * w, int((jobs["w"].astype(np.int64) * jobs["h"]).max())
    ws = torch.empty(lib.uwm_extract_workspace_bytes(n, total, len(jobs)), dtype=torch.uint8, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t, o=0: C.c_void_p(t.data_ptr() + o)

    def stage1():
        L.check(lib.uwm_extract_regions_ragged(p(wm), wm.numel(), p(dd), p(cl), cl.numel(), p(dd, step), n, 3, thr, area, h * w, total, p(plane),
                                               plane.numel(), p(dd, 2 * step), p(stats), p(table), p(ws), ws.numel(), st))

    def stage2():
        L.check(lib.uwm_extract_cutouts_ragged(p(wm), wm.numel(), p(dd), p(plane), plane.numel(), p(dd, 2 * step), n, p(dj), len(jobs), maxc,
                                               p(out), out.numel(), p(status), p(ws), ws.numel(), st))
    if a.profile:
        for _ in range(3):
            stage1(); stage2()
        torch.cuda.synchronize()
        return
    ref = (plane.clone(), stats.clone(), table.clone(), out.clone())
    r = windows({"stage1": (stage1, 20), "stage2": (stage2, 20)}, a.windows, event_ms)
    same = all(torch.equal(x, y) for x, y in zip(ref, (plane, stats, table, out)))
    say(f"(a) stage 1, uwm_extract_regions_ragged, 18 launches   {fmt(r['stage1'])}")
    say(f"(b) stage 2, uwm_extract_cutouts_ragged, 3 launches    {fmt(r['stage2'])}")
    both = np.median(r["stage1"]) + np.median(r["stage2"])
    say(f"    both stages {both:.3f} ms = {1e3 * both / n:.1f} us per pair; stage 1 moves {total * 6 / 1e6:.0f} MB of pixels in: "
        f"{total * 6 / 1e6 / np.median(r['stage1']):.1f} GB/s of input")
    say(f"    results after {2 + 20 * a.windows} more calls equal the first call's bit for bit: {same}")
    if cpu_s is not None:
        say(f"(c) numpy / scipy / Pillow restatement, 16 processes    {1e3 * cpu_s:10.1f} ms for the {n} pairs ({ncut_cpu} cut-outs), host clock, one run")
        say(f"    (c) / ((a) + (b)) = {1e3 * cpu_s / both:.0f}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
