#!/usr/bin/env python3
"""Device time of the distance transform (uwm_edt_ragged) and of the surface-distance call (uwm_surface_distances_ragged) beside
uwm_score_masks_ragged on the same batches, on seeded blob + stroke + 1 % noise masks (tests/maskpost_ref.synth; the truth is the
prediction moved by (3, 5) pixels):

  workload 1: 64 pairs of 720 x 1280
  workload 2: 16 pairs of 2160 x 3840 (workload 1's masks enlarged three times)
  yardstick:  uwm_score_masks_ragged at the paper's radius (29 and 88) on each batch, in the same process
  host:       the numpy / scipy restatement (tests/surface_ref.py) of workload 1 on 16 processes, before the device is touched

2 warm-ups of every route, then 7 windows in which the routes alternate, timed with HIP events around the window's calls.  A
route's figure is the median of its 7 windows, with the least and the greatest beside it.  The records of every pair of workload 1
and of the first pair of workload 2, and the transform of the first mask of each, are compared with the restatement.

  python scripts/time_surface.py [--out profiles/surface_mi355x.txt] [--windows 7]"""
import argparse, os, sys, time
from concurrent.futures import ProcessPoolExecutor
import multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def _ref_record(args):
    import surface_ref as SF
    return SF.record(*args)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "surface_mi355x.txt"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=64, help="pairs of workload 1 (workload 2 takes a quarter)")
    ap.add_argument("--trace", action="store_true",
                    help="for a `rocprofv3 --kernel-trace --stats` run: 20 surface calls on workload 1 and nothing else")
    a = ap.parse_args()
    import maskpost_ref as R
    import surface_ref as SF
    from time_score import clocks, fmt
    n1, n2 = a.pairs, max(1, a.pairs // 4)
    pred1 = [R.synth(720, 1280, 2000 + i).astype(np.uint8) * 255 for i in range(n1)]
    truth1 = [np.roll(m, (3, 5), (0, 1)) for m in pred1]
    if a.trace:
        import torch
        from time_maskpost_ragged import ragged_batch
        from unet_watermark_amd.scoring import surface_distances_ragged
        dev = torch.device("cuda:0")
        pbuf, desc, _, caps = ragged_batch(pred1, dev)
        tbuf = ragged_batch(truth1, dev)[0]
        for _ in range(20):
            surface_distances_ragged(pbuf, tbuf, desc, **caps)
        torch.cuda.synchronize()
        return
    pred2 = [np.repeat(np.repeat(m, 3, 0), 3, 1) for m in pred1[:n2]]
    truth2 = [np.roll(m, (9, 15), (0, 1)) for m in pred2]
    with ProcessPoolExecutor(16, mp_context=mp.get_context("spawn")) as pool:      # the device is not initialised yet
        list(pool.map(_ref_record, [(pred1[0][:8, :8], truth1[0][:8, :8])] * 16))   # start the workers
        t0 = time.perf_counter()
        want1 = np.stack(list(pool.map(_ref_record, list(zip(pred1, truth1)))))
        host_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        want2 = np.stack(list(pool.map(_ref_record, [(pred2[0], truth2[0])])))
        host2_s = time.perf_counter() - t0
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_surface needs a HIP device (a timing without one says nothing)")
    from time_maskpost_ragged import event_ms, ragged_batch, windows
    from unet_watermark_amd.scoring import boundary_radius, distance_transform_ragged, score_masks_ragged, surface_distances_ragged
    dev = torch.device("cuda:0")
    say(f"scripts/time_surface.py : {torch.cuda.get_device_name(0)}, {a.windows} windows after 2 warm-ups of every route, routes alternating, "
        f"HIP events around 20 calls (10 on workload 2)")
    say(f"clocks before the windows: {clocks()}")
    say(f"workload 1: {n1} pairs of 720 x 1280, foreground {100 * float(np.mean([(m > 127).mean() for m in pred1])):.1f} %, "
        f"border pixels {100 * float(np.mean([SF.border(m > 127).mean() for m in pred1[:4]])):.1f} %;  workload 2: {n2} pairs of 2160 x 3840")
    ok = {}
    for name, preds, truths, reps, want in (("1", pred1, truth1, 20, want1), ("2", pred2, truth2, 10, want2)):
        n = len(preds)
        pbuf, desc, _, caps = ragged_batch(preds, dev)
        tbuf = ragged_batch(truths, dev)[0]
        d = boundary_radius(*preds[0].shape)
        counts = torch.empty((n, 8), dtype=torch.int64, device=dev)
        rad = torch.full((n,), d, dtype=torch.int32, device=dev)
        d2 = torch.zeros(pbuf.numel(), dtype=torch.int32, device=dev)
        out = (torch.empty((n, 10), dtype=torch.int64, device=dev), torch.empty((n, 2), dtype=torch.float64, device=dev))
        routes = {"edt (one mask each)": ((lambda: distance_transform_ragged(pbuf, desc, out=d2, **caps)), reps),
                  "surface distances": ((lambda: surface_distances_ragged(pbuf, tbuf, desc, out=out, **caps)), reps),
                  f"score d={d}": ((lambda: score_masks_ragged(pbuf, tbuf, desc, rad, out=counts, **caps)), reps)}
        r = windows(routes, a.windows, event_ms)
        say(f"--- workload {name}")
        for k, v in r.items():
            say(f"{k:<22}{fmt(v)}")
        base = np.median(r[f"score d={d}"])
        say(f"    edt / score = {np.median(r['edt (one mask each)']) / base:.1f},  surface / score = {np.median(r['surface distances']) / base:.1f},  "
            f"surface / edt = {np.median(r['surface distances']) / np.median(r['edt (one mask each)']):.2f} (three transforms and the reduction)")
        mp_ = pbuf.numel() / 1e6
        say(f"    {mp_:.0f} M pixels a mask buffer: {mp_ / 1e3 / (np.median(r['edt (one mask each)']) / 1e3):.1f} G pixels/s through the transform")
        rec = surface_distances_ragged(pbuf, tbuf, desc, **caps)[0].cpu().numpy()
        first = distance_transform_ragged(pbuf, desc, **caps)[: preds[0].size].cpu().numpy().reshape(preds[0].shape)
        ok[name] = (np.array_equal(rec[: len(want)], want), np.array_equal(first, SF.d2(preds[0] > 127)))
    say("--- the restatement on the host (scipy.ndimage: binary_erosion and three distance_transform_edt a pair), 16 processes")
    say(f"workload 1, {n1} pairs: {1e3 * host_s:9.1f} ms;  one pair of workload 2: {1e3 * host2_s:9.1f} ms (one process)")
    say(f"the device records equal the restatement: workload 1, all {n1} pairs: {ok['1'][0]};  workload 2, first pair: {ok['2'][0]};  "
        f"D2 of the first mask of each: {ok['1'][1]}, {ok['2'][1]}")
    say(f"clocks after the windows: {clocks()}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    if not all(all(v) for v in ok.values()):
        raise SystemExit("the device results differ from the restatement")


if __name__ == "__main__":
    main()
