#!/usr/bin/env python3
"""Device time of the membrane fill (uwm_inpaint_ragged: one call per batch) at the default cycle count, beside the same call with no
cycle (prep, pull, push and store alone), the numpy restatement (tests/inpaint_ref.inpaint_ref) on 16 worker processes, and the
predict_images call the fill follows in `repair` (Unet-resnet34 at 512, mask_type watermark, the same 64 images):

  corner   64 images of 720 x 1280, a logo rectangle in the lower right corner (about 3 % of the pixels)
  centre   the same images, the `watermark` chain's dilated mask of a centred 300 x 400 logo
  4k       16 images of 2160 x 3840, the corner rectangle at the same share

Images: a smooth seeded field plus noise, three channels.  2 warm-ups of every run, then --windows windows in which the runs
alternate, HIP events around a window's calls (about 0.1 s of work per window).  A run's figure is the median of its windows, with the
least and the greatest beside it.  The first --check images of the 720 x 1280 runs are compared with the restatement byte for byte;
the restatement's time is taken on --cpu-images images, one per process, and scaled to the batch (reported only).  The share of
each kernel comes from a run of its own: `rocprofv3 --kernel-trace --stats -- python scripts/time_inpaint.py --profile corner`.

  python scripts/time_inpaint.py [--out profiles/inpaint_mi355x.txt] [--windows 5] [--check 2] [--cpu-images 16] [--no-predict]"""
import argparse, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

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
    return f"median {np.median(v):9.3f} ms  (min {min(v):9.3f}, max {max(v):9.3f})"


def field(h, w, seed):
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    planes = [np.clip(128 + 60 * np.sin(x / (17 + 5 * k) + seed) + 50 * np.cos(y / (11 + 3 * k)) + g.normal(0, 25, (h, w)), 0, 255) for k in range(3)]
    return np.stack(planes, 2).round().astype(np.uint8)


def corner_mask(h, w):
    m = np.zeros((h, w), np.uint8)
    m[h - int(h * 0.15):h - int(h * 0.02), w - int(w * 0.26):w - int(w * 0.02)] = 255          # 13 % x 24 % of the sides: 3.1 %
    return m


def centre_logo(h, w):
    m = np.zeros((h, w), np.uint8)
    m[h // 2 - 150:h // 2 + 150, w // 2 - 200:w // 2 + 200] = 255
    return m


def _cpu_one(job):
    import inpaint_ref as R
    return R.inpaint_ref(*job)[0]


def cpu_seconds(images, masks, cycles, procs=16):
    import multiprocessing as mp
    jobs = [(i, m, cycles) for i, m in zip(images, masks)]
    with mp.get_context("fork").Pool(min(procs, len(jobs))) as pool:
        pool.map(abs, range(4 * procs))                     # the workers are up
        t0 = time.perf_counter()
        res = pool.map(_cpu_one, jobs, chunksize=1)
        return time.perf_counter() - t0, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "inpaint_mi355x.txt"))
    ap.add_argument("--windows", type=int, default=5); ap.add_argument("--check", type=int, default=2)
    ap.add_argument("--cpu-images", type=int, default=16, help="images the restatement is timed on (0: leave it out)")
    ap.add_argument("--no-predict", action="store_true", help="leave out the predict_images call")
    ap.add_argument("--profile", type=str, default=None, choices=["corner", "centre", "4k"],
                    help="for a `rocprofv3 --kernel-trace --stats` run: 5 calls of this run at the default cycles and nothing else")
    a = ap.parse_args()
    from unet_watermark_amd.data import DESC_DTYPE, descs_tensor
    from unet_watermark_amd.inpaint import DEFAULT_CYCLES, inpaint_buffers, inpaint_workspace, launch_count
    base = [field(720, 1280, 100 + i) for i in range(4)]               # four distinct images, repeated: the time does not depend on the bytes
    cpu = {}
    if a.profile:
        a.cpu_images, a.no_predict = 0, True
    if a.cpu_images:                                       # the worker processes come and go before this process opens the device
        k = min(64, a.cpu_images)
        cpu["corner"] = cpu_seconds([base[i % 4] for i in range(k)], [corner_mask(720, 1280)] * k, DEFAULT_CYCLES)
    if not torch.cuda.is_available():
        raise SystemExit("time_inpaint needs a HIP device (a timing without one says nothing)")
    dev = torch.device("cuda:0")
    say(f"scripts/time_inpaint.py : {torch.cuda.get_device_name(0)}, {a.windows} windows after 2 warm-ups of every run, runs alternating, "
        f"default cycles = {DEFAULT_CYCLES}")
    from unet_watermark_amd.postprocess import optimize_mask
    dil = optimize_mask(torch.from_numpy(centre_logo(720, 1280))[None].to(dev), "watermark")[0].cpu().numpy()
    specs = (("corner", 64, 720, 1280, corner_mask(720, 1280)), ("centre", 64, 720, 1280, dil), ("4k", 16, 2160, 3840, corner_mask(2160, 3840)))
    runs = {}
    for name, n, h, w, mask in specs:
        if a.profile and name != a.profile:
            continue
        one = np.stack([base[i % 4] for i in range(4)]) if h == 720 else np.stack([np.tile(base[i % 4], (3, 3, 1)) for i in range(4)])
        buf = torch.from_numpy(one.reshape(-1)).to(dev).repeat(n // 4)
        mbuf = torch.from_numpy(mask.reshape(-1)).to(dev).repeat(n)
        descs, mdescs = np.zeros(n, DESC_DTYPE), np.zeros(n, DESC_DTYPE)
        descs["offset"], descs["h"], descs["w"] = np.arange(n, dtype=np.int64) * (h * w * 3), h, w
        mdescs["offset"], mdescs["h"], mdescs["w"] = np.arange(n, dtype=np.int64) * (h * w), h, w
        di, dm = descs_tensor(descs, dev), descs_tensor(mdescs, dev)
        out = torch.empty_like(buf)
        ws = inpaint_workspace(dev, n, buf.numel(), 3, max(h, w))
        caps = dict(max_pixels=h * w, rows=n * h, max_side=max(h, w))
        for cyc in (DEFAULT_CYCLES, 0):
            fn = (lambda buf=buf, di=di, mbuf=mbuf, dm=dm, n=n, out=out, ws=ws, caps=caps, cyc=cyc:
                  inpaint_buffers(buf, di, mbuf, dm, n, 3, cycles=cyc, out=out, workspace=ws, **caps))
            t = np.median([event_ms(fn, 2) for _ in range(2)])                         # (also the warm-ups)
            runs[(name, cyc)] = dict(fn=fn, reps=max(2, int(100.0 / max(t, 1e-3))), ms=[], n=n, h=h, w=w, out=out, mask=mask,
                                     launches=launch_count(cyc, max(h, w)), ws=ws.numel())
    if a.profile:
        for _ in range(5):
            runs[(a.profile, DEFAULT_CYCLES)]["fn"]()
        torch.cuda.synchronize()
        return
    pred = None
    if not a.no_predict:
        import unet_watermark_amd as U
        from unet_watermark_amd.config import get_cfg_defaults
        from unet_watermark_amd.predict import WatermarkPredictor
        cfg = get_cfg_defaults(); cfg.MODEL.NAME = "Unet"; cfg.MODEL.ENCODER_NAME = "resnet34"; cfg.DATA.IMG_SIZE = 512
        torch.manual_seed(0)
        pred = WatermarkPredictor(model=U.Unet("resnet34").to(dev), config=cfg, device=dev, freeze=True)
        imgs = [base[i % 4] for i in range(64)]
        fn = lambda: pred.predict_images(imgs, mask_type="watermark")
        fn(); fn(); torch.cuda.synchronize()

        def wall(reps=2):
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / reps
        runs[("predict", -1)] = dict(fn=None, ms=[], wall=wall)
    for _ in range(a.windows):
        for r in runs.values():
            r["ms"].append(r["wall"]() if r["fn"] is None else event_ms(r["fn"], r["reps"]))
    for (name, cyc), r in runs.items():
        if name == "predict":
            say(f"--- predict_images(mask_type='watermark') of the 64 images of 720 x 1280, Unet-resnet34 at 512, frozen, graph replay; wall time with "
                f"packing, upload and the masks' clone")
            say(f"one call                                 {fmt(r['ms'])}")
            continue
        n, h, w = r["n"], r["h"], r["w"]
        med = float(np.median(r["ms"]))
        if cyc:
            say(f"--- {name}: {n} images of {h} x {w} x 3, hole pixels {100 * float((r['mask'] != 0).mean()):.2f} %, workspace {r['ws'] / 2 ** 20:.0f} MiB "
                f"({r['ws'] / (n * h * w):.1f} bytes per pixel)")
        say(f"cycles {cyc}: {r['launches']:3d} launches, {r['reps']} calls per window   {fmt(r['ms'])}   {1e3 * med / n:8.1f} us per image")
        if cyc and name in cpu:
            r["fn"](); torch.cuda.synchronize()
            got = r["out"].view(n, h, w, 3).cpu().numpy()
            sec, res = cpu[name]
            same = all(np.array_equal(got[i], res[i]) for i in range(min(a.check, len(res))))
            say(f"    inpaint_ref (numpy) on {len(res)} images, one process each: {sec:.2f} s -> {sec * n / len(res):.2f} s for the batch on 16 cores "
                f"(scaled, reported only); the first {min(a.check, len(res))} images equal the device's: {same}")
    for name in ("corner", "centre", "4k"):
        full, zero = np.median(runs[(name, DEFAULT_CYCLES)]["ms"]), np.median(runs[(name, 0)]["ms"])
        say(f"{name}: pull + push + store {zero:.3f} ms, one V-cycle {(full - zero) / DEFAULT_CYCLES:.3f} ms")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
