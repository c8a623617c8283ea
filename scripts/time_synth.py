#!/usr/bin/env python3
"""Device time of uwm_synth_u8 on a batch of `--n` images of `--size` with three `--logo`-sized logos each (jobs drawn by
data.sample_synth_jobs from a seed), beside the same jobs done by Pillow on `--procs` CPU processes (gen_data.py's calls: resize
LANCZOS, rotate, GaussianBlur, ImageEnhance, paste; the shear stage is left off on both sides since cv2 is not a dependency).

  python scripts/time_synth.py [--n 16] [--size 720 1280] [--logo 600] [--reps 7] [--calls 10] [--procs 16]
      total time: HIP events around `calls` calls after warm-ups, the median over `reps` such windows; the Pillow figure is the
      wall time of one pass over the batch, median over `reps` passes, taken BEFORE the device is opened (the pool forks)
  rocprofv3 --kernel-trace --stats ... -- python scripts/time_synth.py --trace
      a short run for the per-kernel table (resample = stages 1 and 3a, four passes; blur = six passes)
  python scripts/time_synth.py --write-data DIR [--n 128]
      no timing: the batch's clean images into DIR/clean and its three logos into DIR/logos, for `main.py train --synthesize` against
      `main.py synth` + `main.py train --data-dir` on the same files"""
import argparse, ctypes as C, os, random, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def make_batch(n, h, w, logo, seed):
    from unet_watermark_amd import data as D
    rng = np.random.default_rng(seed)
    images = []
    for _ in range(n):
        base = rng.integers(0, 256, (h // 16 + 1, w // 16 + 1, 3), dtype=np.uint8)
        images.append(np.ascontiguousarray(np.kron(base, np.ones((16, 16, 1), np.uint8))[:h, :w]))
    yy, xx = np.mgrid[0:logo, 0:logo]
    logos = []
    for k in range(3):
        a = rng.integers(0, 256, (logo, logo, 4), dtype=np.uint8)
        a[..., 3] = np.where((yy - logo / 2) ** 2 + (xx - logo / 2) ** 2 < (logo * (0.3 + 0.07 * k)) ** 2, 255, rng.integers(0, 120))
        logos.append(a)
    class Recorder(random.Random):                            # Pillow wants the angle and the radius themselves, which a job does not hold
        log = []

        def uniform(self, a, b):
            v = super().uniform(a, b); self.log.append((a, b, v)); return v

    r = Recorder(seed)
    jobs, drawn = [], []
    for _ in range(n):
        r.log = []
        jobs.append(D.sample_synth_jobs(r, (w, h), [(logo, logo)] * 3, False))
        per, cur = [], None
        for a, b, v in r.log:
            if (a, b) == (0.03, 0.35):                        # the first draw of apply_watermark_effects: a new logo
                cur = {}; per.append(cur)
            elif (a, b) == (0, 360):
                cur["angle"] = v
            elif (a, b) == (0.5, 2.5):
                cur["radius"] = v
        drawn.append(per)
    jobs = np.stack(jobs)
    jobs["shear"] = 0
    for k in range(3):
        jobs["logo"][:, k] = k
    return images, logos, jobs, drawn


def pillow_one(arg):
    """gen_data.py's calls with one image's jobs"""
    from PIL import Image, ImageEnhance, ImageFilter
    image, logos, jobs, drawn = arg
    out = Image.fromarray(image); mask = Image.new("L", out.size, 0)
    for j, d in zip(jobs, drawn):
        if not j["enabled"]:
            continue
        wm = Image.fromarray(logos[int(j["logo"])], "RGBA").resize((int(j["w1"]), int(j["h1"])), Image.Resampling.LANCZOS)
        if j["rotate"]:
            wm = wm.rotate(d["angle"], expand=True, fillcolor=(0, 0, 0, 0))
        if j["stretch"]:
            wm = wm.resize((int(j["w3"]), int(j["h3"])), Image.Resampling.LANCZOS)
        if j["blur"]:
            wm = wm.filter(ImageFilter.GaussianBlur(radius=d["radius"]))
        arr = np.array(wm)
        for x, y, dw, dh in j["defects"][:int(j["ndefects"])]:
            arr[y:y + dh, x:x + dw, 3] = 0
        wm = Image.fromarray(arr)
        if j["enhance"]:
            wm = ImageEnhance.Color(ImageEnhance.Contrast(ImageEnhance.Brightness(wm).enhance(float(j["brightness"]))).enhance(float(j["contrast"]))).enhance(float(j["color"]))
        arr = np.array(wm); arr[:, :, 3] = j["opacity"][arr[:, :, 3]]
        wm = Image.fromarray(arr); al = wm.split()[3]
        mask.paste(al, (int(j["x"]), int(j["y"])), al); out.paste(wm, (int(j["x"]), int(j["y"])), wm)
    return np.asarray(out), np.asarray(mask)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16); ap.add_argument("--size", type=int, nargs=2, default=(720, 1280)); ap.add_argument("--logo", type=int, default=600)
    ap.add_argument("--reps", type=int, default=7); ap.add_argument("--calls", type=int, default=10); ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--trace", action="store_true"); ap.add_argument("--write-data", type=str, default=None)
    a = ap.parse_args()
    (h, w), n = a.size, a.n
    images, logos, jobs, drawn = make_batch(n, h, w, a.logo, 0)
    if a.write_data:
        from PIL import Image
        os.makedirs(os.path.join(a.write_data, "clean"), exist_ok=True); os.makedirs(os.path.join(a.write_data, "logos"), exist_ok=True)
        for i, im in enumerate(images):
            Image.fromarray(im).save(os.path.join(a.write_data, "clean", f"c{i:04d}.png"))
        for i, lg in enumerate(logos):
            Image.fromarray(lg, "RGBA").save(os.path.join(a.write_data, "logos", f"l{i}.png"))
        return
    from unet_watermark_amd import data as D
    pil_t, pil_out = [], None
    if not a.trace:
        import multiprocessing as mp
        with mp.get_context("fork").Pool(a.procs) as pool:
            args = [(images[i], logos, jobs[i], drawn[i]) for i in range(n)]
            pool.map(pillow_one, args)                       # warm-up
            for _ in range(a.reps):
                t0 = time.perf_counter(); pil_out = pool.map(pillow_one, args); pil_t.append((time.perf_counter() - t0) * 1e3)
    import torch
    from unet_watermark_amd import _lib as L
    assert torch.cuda.is_available(), "time_synth.py measures on a HIP device"
    dev = torch.device("cuda:0")
    pi, di, _ = D.pack_images(images); pl, dl, _ = D.pack_images(logos)
    Pp, T = D.synth_job_needs(jobs, dl)
    lib, st = L.lib(), C.c_void_p(L.stream_ptr(dev))
    clean, lt = pi.to(dev), pl.to(dev)
    it = clean.clone()
    md = D.mask_descs_for(di)
    mt = torch.empty(int((md["h"].astype(np.int64) * md["w"]).sum()), dtype=torch.uint8, device=dev)
    dt = D.descs_tensor(np.concatenate([di, md, dl]), dev)
    jt = torch.from_numpy(jobs.reshape(-1).view(np.uint8).copy()).to(dev)
    ws = torch.empty(int(lib.uwm_synth_workspace_bytes(n, 3, Pp, T)), dtype=torch.uint8, device=dev)
    step = n * D.DESC_DTYPE.itemsize
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)      # noqa: E731

    def call():
        L.check(lib.uwm_synth_u8(ptr(it), it.numel(), ptr(dt), ptr(mt), mt.numel(), ptr(dt, step), ptr(lt), lt.numel(), ptr(dt, 2 * step), 3, ptr(jt), n, 3,
                                 Pp, T, ptr(ws), ws.numel(), st))

    call(); torch.cuda.synchronize()
    exact = None
    if pil_out is not None:                                  # the first call ran on the clean batch: compare it with Pillow's result
        got, gm = it.cpu().numpy(), mt.cpu().numpy()
        exact = all(np.array_equal(got[d["offset"]: d["offset"] + h * w * 3].reshape(h, w, 3), pil_out[i][0]) and
                    np.array_equal(gm[m["offset"]: m["offset"] + h * w].reshape(h, w), pil_out[i][1]) for i, (d, m) in enumerate(zip(di, md)))
    for _ in range(2 if a.trace else 3):
        call()
    torch.cuda.synchronize()
    if a.trace:
        return
    ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            call()
        e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / a.calls)
    on = int((jobs["enabled"] != 0).sum())
    px = sum(int(j["w3"] * j["h3"]) if j["stretch"] else int(j["w2"] * j["h2"]) if j["rotate"] else int(j["w1"] * j["h1"]) for j in jobs.reshape(-1) if j["enabled"])
    print(f"synthesis, {n} images of {h}x{w}x3, three {a.logo}x{a.logo} logos each: {on} jobs enabled, {px / max(on, 1):.0f} patch pixels per job on average, "
          f"max_patch_pixels {Pp}, max_taps {T}, workspace {ws.numel() / 2 ** 20:.1f} MiB | equals Pillow on the same jobs (shear off): {exact}")
    v = sorted(ts)
    print(f"uwm_synth_u8 (16 launches)          {v[len(v) // 2]:8.3f} ms/batch median of {a.reps} x {a.calls} calls (min {v[0]:.3f}, max {v[-1]:.3f})")
    v = sorted(pil_t)
    print(f"Pillow chain, {a.procs} processes         {v[len(v) // 2]:8.3f} ms/batch median of {a.reps} passes (min {v[0]:.3f}, max {v[-1]:.3f}); "
          "images and logos pickled to the workers, results back")


if __name__ == "__main__":
    main()
