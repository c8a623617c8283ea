#!/usr/bin/env python3
"""Device time of the mask enhancement (uwm_enhance_masks_ragged: one call per batch) on seeded blob + stroke masks (tight
segmentation masks: the shapes of tests/maskpost_ref.synth without its noise, which a dilation by 10 turns into a full plane),
beside the bytes its stages move and the time those bytes take at the measured copy rate of the device (6.29 TB/s, float4 copy),
and beside the numpy restatement (tests/enhance_ref.enhance_reduced) on 16 worker processes:

  64 masks of 720 x 1280 at (expand_pixels, blur_kernel, smooth_iterations) = (10, 15, 2) and (15, 21, 2)
  16 masks of 512 x 512  at the same two

Every stage is one launch that reads one byte and writes one byte per pixel (the halo re-reads of a tile come from cache and are
not counted): 3 morphology stages (2 when expand_pixels = 0), the blur, one per two smoothing rounds; the call here carries no
stats.  2 warm-ups of every run, then 7 windows in which the runs alternate, HIP events around a window's calls (about 0.1 s of work per
window).  A run's figure is the median of its 7 windows, with the least and the greatest beside it.  The first --check masks of
every run are compared with the restatement byte for byte; the restatement's time is taken on 16 masks, one per process, and
scaled to the batch (reported only).

  python scripts/time_enhance.py [--out profiles/enhance_mi355x.txt] [--windows 7] [--check 2] [--cpu-masks 16]"""
import argparse, ctypes as C, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

COPY_RATE = 6.29e12                      # bytes / s: the device's measured float4 copy
RUNS = ((64, 720, 1280, (10, 15, 2)), (64, 720, 1280, (15, 21, 2)), (16, 512, 512, (10, 15, 2)), (16, 512, 512, (15, 21, 2)))
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def fmt(v):
    return f"median {np.median(v):8.3f} ms  (min {min(v):8.3f}, max {max(v):8.3f})"


def lib_taps(k):
    from unet_watermark_amd import _lib as L
    if k == 0:
        return None
    buf = (C.c_float * 63)()
    n = L.lib().uwm_enhance_gauss_taps(k, buf)
    return np.array(buf[:n], np.float32)


def tight_mask(h, w, seed):
    """1 to 4 filled ellipses and up to 11 two-pixel strokes, some touching the border -> uint8 {0,255}"""
    g = np.random.default_rng(seed)
    m = np.zeros((h, w), bool)
    yy, xx = np.mgrid[:h, :w]
    for _ in range(int(g.integers(1, 5))):
        cy, cx = g.integers(0, h), g.integers(0, w)
        ry, rx = g.integers(3, max(4, h // 5)), g.integers(3, max(4, w // 5))
        m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
    for _ in range(int(g.integers(0, 12))):
        y, x = g.integers(0, h), g.integers(0, w)
        if g.random() < .5:
            m[y:y + 2, x:x + int(g.integers(4, 30))] = True
        else:
            m[y:y + int(g.integers(4, 30)), x:x + 2] = True
    return m.astype(np.uint8) * 255


def _cpu_one(job):
    import enhance_ref as E
    mask, taps, e, s = job
    return E.enhance_reduced(mask, taps, e, s)


def cpu_seconds(masks, params, procs=16):
    """wall time of enhance_reduced on `masks`, one worker process each (at most `procs` at a time)"""
    import multiprocessing as mp
    jobs = [(m, lib_taps(params[1]), params[0], params[2]) for m in masks]
    with mp.get_context("fork").Pool(min(procs, len(jobs))) as pool:
        pool.map(abs, range(4 * procs))                     # the workers are up
        t0 = time.perf_counter()
        res = pool.map(_cpu_one, jobs, chunksize=1)
        return time.perf_counter() - t0, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "enhance_mi355x.txt"))
    ap.add_argument("--windows", type=int, default=7); ap.add_argument("--check", type=int, default=2)
    ap.add_argument("--cpu-masks", type=int, default=16, help="masks the restatement is timed on (0: leave it out)")
    a = ap.parse_args()
    from unet_watermark_amd.data import DESC_DTYPE, descs_tensor
    from unet_watermark_amd.postprocess import enhance_masks_ragged
    cpu = {}
    if a.cpu_masks:                                        # the worker processes come and go before this process opens the device
        for n, h, w, params in RUNS:
            masks = [tight_mask(h, w, 4000 + i) for i in range(min(n, a.cpu_masks))]
            cpu[(n, h, w, params)] = cpu_seconds(masks, params)
    if not torch.cuda.is_available():
        raise SystemExit("time_enhance needs a HIP device (a timing without one says nothing)")
    dev = torch.device("cuda:0")
    say(f"scripts/time_enhance.py : {torch.cuda.get_device_name(0)}, {a.windows} windows after 2 warm-ups of every run, runs alternating")
    runs = {}
    for n, h, w, params in RUNS:
        masks = [tight_mask(h, w, 4000 + i) for i in range(n)]
        descs = np.zeros(n, DESC_DTYPE)
        descs["offset"], descs["h"], descs["w"] = np.arange(n, dtype=np.int64) * (h * w), h, w
        buf = torch.from_numpy(np.stack(masks).reshape(-1)).to(dev)
        out = torch.empty_like(buf)
        dd = descs_tensor(descs, dev)
        fn = (lambda buf=buf, dd=dd, out=out, n=n, hw=h * w, p=params: enhance_masks_ragged(buf, dd, *p, out=out, n=n, max_pixels=hw))
        stages = (3 if params[0] else 2) + 1 + (params[2] + 1) // 2
        one = np.median([event_ms(fn, 3) for _ in range(2)])                       # (also the warm-ups)
        runs[(n, h, w, params)] = dict(fn=fn, reps=max(3, int(100.0 / max(one, 1e-3))), ms=[], out=out, masks=masks, stages=stages,
                                       fg=float(np.mean([(m > 127).mean() for m in masks])))
    for _ in range(a.windows):
        for r in runs.values():
            r["ms"].append(event_ms(r["fn"], r["reps"]))
    for key, r in runs.items():
        n, h, w, params = key
        r["fn"](); torch.cuda.synchronize()
        got = r["out"].view(n, h, w).cpu().numpy()
        want = cpu[key][1] if key in cpu else []
        same = all(np.array_equal(got[i], want[i]) for i in range(min(a.check, len(want))))
        moved = 2.0 * r["stages"] * n * h * w
        floor = 1e3 * moved / COPY_RATE
        med = float(np.median(r["ms"]))
        say(f"--- {n} masks of {h} x {w} at {params}: foreground in {100 * r['fg']:.1f} %, out {100 * float((got > 127).mean()):.1f} %")
        say(f"one call, {r['reps']} calls per window        {fmt(r['ms'])}")
        say(f"    {r['stages']} launches x 2 bytes per pixel = {moved / 1e6:.1f} MB; at 6.29 TB/s {floor:.3f} ms; the call takes {med / floor:.1f} x that "
            f"({moved / med / 1e6:.0f} GB/s of stage traffic)")
        if key in cpu:
            sec, k = cpu[key][0], len(cpu[key][1])
            say(f"    enhance_reduced (numpy) on {k} masks, one process each: {sec:.2f} s -> {sec * n / k:.2f} s for the batch on 16 cores (scaled, reported only); "
                f"the first {min(a.check, k)} masks equal the device's: {same}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
