#!/usr/bin/env python3
"""Device time of the mask scoring call (uwm_score_masks_ragged) beside uwm_optimize_masks_ragged on the same batches, on seeded
blob + stroke + 1 % noise masks (tests/maskpost_ref.synth; the truth is the prediction moved by (3, 5) pixels):

  workload 1: 64 pairs of 720 x 1280 at d = 29 (the paper's 2 % of the diagonal), and the same call at d = 1 and d = 300
  workload 2: 16 pairs of 2160 x 3840 at d = 88 (workload 1's masks enlarged three times)
  yardstick:  uwm_optimize_masks_ragged (mask_type watermark) on the predictions of each batch, in the same process
  host:       the numpy / scipy restatement (tests/score_ref.py) of workload 1 on 16 processes, before the device is touched

2 warm-ups of every route, then 7 windows in which the routes alternate, timed with HIP events around the window's calls.  A
route's figure is the median of its 7 windows, with the least and the greatest beside it.  The counts of every pair of workload 1
and of the first pair of workload 2 are compared with the restatement.

  python scripts/time_score.py [--out profiles/score_mi355x.txt] [--windows 7]"""
import argparse, os, subprocess, sys, time
from concurrent.futures import ProcessPoolExecutor
import multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def fmt(v):
    return f"median {np.median(v):8.3f} ms  (min {min(v):8.3f}, max {max(v):8.3f}, spread {max(v) - min(v):6.3f})"


def _ref_row(args):
    import score_ref as SR
    return SR.counts(*args)


def clocks():
    """the clock state as the system tool reports it (a query; nothing is set)"""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=30)
        keep = [ln.strip() for ln in r.stdout.decode(errors="replace").splitlines() if "sclk" in ln or "mclk" in ln]
        return "; ".join(keep) if keep else "not reported"
    except Exception as e:      # noqa: BLE001
        return f"not reported ({e.__class__.__name__})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "score_mi355x.txt"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=64, help="pairs of workload 1 (workload 2 takes a quarter)")
    ap.add_argument("--trace", action="store_true",
                    help="for a `rocprofv3 --kernel-trace --stats` run: 20 score calls on workload 1 at d = 29 and nothing else")
    a = ap.parse_args()
    import maskpost_ref as R
    n1, n2 = a.pairs, max(1, a.pairs // 4)
    pred1 = [R.synth(720, 1280, 2000 + i).astype(np.uint8) * 255 for i in range(n1)]
    truth1 = [np.roll(m, (3, 5), (0, 1)) for m in pred1]
    if a.trace:
        import torch
        from time_maskpost_ragged import ragged_batch
        from unet_watermark_amd.scoring import score_masks_ragged
        dev = torch.device("cuda:0")
        pbuf, desc, _, caps = ragged_batch(pred1, dev)
        tbuf = ragged_batch(truth1, dev)[0]
        rad = torch.full((n1,), 29, dtype=torch.int32, device=dev)
        for _ in range(20):
            score_masks_ragged(pbuf, tbuf, desc, rad, **caps)
        torch.cuda.synchronize()
        return
    pred2 = [np.repeat(np.repeat(m, 3, 0), 3, 1) for m in pred1[:n2]]
    truth2 = [np.roll(m, (9, 15), (0, 1)) for m in pred2]
    with ProcessPoolExecutor(16, mp_context=mp.get_context("spawn")) as pool:      # the device is not initialised yet
        list(pool.map(_ref_row, [(pred1[0][:8, :8], truth1[0][:8, :8], 1)] * 16))   # start the workers
        t0 = time.perf_counter()
        want1 = np.stack(list(pool.map(_ref_row, [(p, t, 29) for p, t in zip(pred1, truth1)])))
        host_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        want2 = np.stack(list(pool.map(_ref_row, [(pred2[0], truth2[0], 88)])))
        host2_s = time.perf_counter() - t0
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_score needs a HIP device (a timing without one says nothing)")
    from time_maskpost_ragged import event_ms, ragged_batch, windows
    from unet_watermark_amd.postprocess import optimize_masks_ragged
    from unet_watermark_amd.scoring import boundary_radius, score_masks_ragged
    dev = torch.device("cuda:0")
    say(f"scripts/time_score.py : {torch.cuda.get_device_name(0)}, {a.windows} windows after 2 warm-ups of every route, routes alternating, "
        f"HIP events around 100 calls (50 on workload 2)")
    say(f"clocks before the windows: {clocks()}")
    assert boundary_radius(720, 1280) == 29 and boundary_radius(2160, 3840) == 88
    say(f"workload 1: {n1} pairs of 720 x 1280, foreground {100 * float(np.mean([(m > 127).mean() for m in pred1])):.1f} %;  "
        f"workload 2: {n2} pairs of 2160 x 3840")
    res = {}
    for name, preds, truths, d, reps in (("1", pred1, truth1, 29, 100), ("2", pred2, truth2, 88, 50)):
        n = len(preds)
        pbuf, desc, _, caps = ragged_batch(preds, dev)
        tbuf = ragged_batch(truths, dev)[0]
        obuf = torch.empty_like(pbuf)
        counts = torch.empty((n, 8), dtype=torch.int64, device=dev)
        rad = {k: torch.full((n,), k, dtype=torch.int32, device=dev) for k in ((d, 1, 300) if name == "1" else (d,))}
        routes = {f"score d={k}": ((lambda k=k: score_masks_ragged(pbuf, tbuf, desc, rad[k], out=counts, **caps)), reps) for k in rad}
        routes["optimize watermark"] = ((lambda: optimize_masks_ragged(pbuf, desc, "watermark", out=obuf, **caps)), reps)
        r = windows(routes, a.windows, event_ms)
        say(f"--- workload {name}")
        for k, v in r.items():
            say(f"{k:<22}{fmt(v)}")
        base = np.median(r["optimize watermark"])
        say("    score / optimize = " + ", ".join(f"{np.median(v) / base:.3f} ({k})" for k, v in r.items() if k.startswith("score")))
        got = score_masks_ragged(pbuf, tbuf, desc, rad[d], **caps).cpu().numpy()
        res[name] = got
        mb = 2 * pbuf.numel() / 1e6
        say(f"    the two byte buffers are {mb:.0f} MB: {mb / 1e3 / (np.median(r[f'score d={d}']) / 1e3):.0f} GB/s of mask bytes at d = {d}")
    say("--- the restatement on the host (scipy.ndimage.binary_erosion, iterations = d), 16 processes")
    say(f"workload 1, {n1} pairs at d = 29: {1e3 * host_s:9.1f} ms;  one pair of workload 2 at d = 88: {1e3 * host2_s:9.1f} ms (one process)")
    ok1, ok2 = np.array_equal(res["1"], want1), np.array_equal(res["2"][:1], want2)
    say(f"the device counts equal the restatement: workload 1, all {n1} pairs: {ok1};  workload 2, first pair: {ok2}")
    say(f"clocks after the windows: {clocks()}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    if not (ok1 and ok2):
        raise SystemExit("the device counts differ from the restatement")


if __name__ == "__main__":
    main()
