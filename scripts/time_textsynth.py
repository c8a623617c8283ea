#!/usr/bin/env python3
"""Device time of uwm_synth_text_u8 on a batch of `--n` images of `--size` with one text each (texts, font sizes and jobs drawn by
data.sample_text_item from a seed, Pillow's embedded font), beside the same jobs done by Pillow on `--procs` CPU processes
(gen_data.py's calls from the drawn canvas on: rotate, resize LANCZOS, GaussianBlur, ImageEnhance, the alpha scale, the fit resizes,
paste), and the host's rasterisation time per text (data.render_text_plane), which both routes need.

  python scripts/time_textsynth.py [--n 16] [--size 720 1280] [--reps 7] [--calls 10] [--procs 16]
      total time: HIP events around `calls` calls after warm-ups, the median over `reps` such windows; the Pillow figure is the
      wall time of one pass over the batch, median over `reps` passes, taken BEFORE the device is opened (the pool forks)
  rocprofv3 --kernel-trace --stats ... -- python scripts/time_textsynth.py --trace
      a short run for the per-kernel table (resample = the SCALE and FIT passes, eight launches; blur = six passes)"""
import argparse, ctypes as C, os, random, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


class Recorder(random.Random):                                # Pillow wants the angle and the radius themselves, which a job does not hold
    log = []

    def uniform(self, a, b):
        v = super().uniform(a, b); self.log.append((a, b, v)); return v


def make_batch(n, h, w, seed):
    from unet_watermark_amd import data as D
    rng = np.random.default_rng(seed)
    images = []
    for _ in range(n):
        base = rng.integers(0, 256, (h // 16 + 1, w // 16 + 1, 3), dtype=np.uint8)
        images.append(np.ascontiguousarray(np.kron(base, np.ones((16, 16, 1), np.uint8))[:h, :w]))
    fonts, r = D.FontSet(), Recorder(seed)
    planes, jobs, drawn, raster = [], D.empty_text_jobs(n, 1), [], []
    for i in range(n):
        r.log = []
        text, size = D.sample_text(r, D.DEFAULT_TEXTS), D.sample_font_size(r, (w, h))
        font = fonts.font(fonts.select(text), size)
        D.render_text_plane(text, font)                       # (the first call of a size loads the font)
        t0 = time.perf_counter(); plane = D.render_text_plane(text, font); raster.append((time.perf_counter() - t0) * 1e3)
        job = D.sample_text_job(r, (w, h), (plane.shape[1], plane.shape[0]), i % 2 == 0, glyph=i)
        assert job is not None
        planes.append(plane); jobs[i, 0] = job
        drawn.append({{(-45, 45): "angle", (0.5, 1.5): "radius"}[(a, b)]: v for a, b, v in r.log if (a, b) in ((-45, 45), (0.5, 1.5))})
    return images, planes, jobs, drawn, raster


def pillow_one(arg):
    """gen_data.py's calls with one image's job, from the canvas ImageDraw.text leaves"""
    from PIL import Image, ImageEnhance, ImageFilter
    image, plane, j, d = arg
    a = np.zeros(plane.shape + (4,), np.uint8)
    a[..., :3] = np.where((plane != 0)[..., None], j["ink"].astype(np.uint8), 0); a[..., 3] = plane
    t = Image.fromarray(a, "RGBA")
    if j["rotate"]:
        t = t.rotate(d["angle"], expand=True, fillcolor=(0, 0, 0, 0))
    if j["scale"]:
        t = t.resize((int(j["w3"]), int(j["h3"])), Image.Resampling.LANCZOS)
    if j["blur"]:
        t = t.filter(ImageFilter.GaussianBlur(radius=d["radius"]))
    if j["brighten"]:
        t = ImageEnhance.Brightness(t).enhance(float(j["brightness"]))
    if j["recontrast"]:
        t = ImageEnhance.Contrast(t).enhance(float(j["contrast"]))
    arr = np.array(t); arr[:, :, 3] = j["opacity"][arr[:, :, 3]]
    t = Image.fromarray(arr)
    for fw, fh in j["fit"][:int(j["nfit"])]:
        t = t.resize((int(fw), int(fh)), Image.Resampling.LANCZOS)
    out = Image.fromarray(image); mask = Image.new("L", out.size, 0)
    al = t.split()[3]
    mask.paste(al, (int(j["x"]), int(j["y"])), al); out.paste(t, (int(j["x"]), int(j["y"])), t)
    return np.asarray(out), np.asarray(mask)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16); ap.add_argument("--size", type=int, nargs=2, default=(720, 1280))
    ap.add_argument("--reps", type=int, default=7); ap.add_argument("--calls", type=int, default=10); ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    (h, w), n = a.size, a.n
    images, planes, jobs, drawn, raster = make_batch(n, h, w, 0)
    from unet_watermark_amd import data as D
    pil_t, pil_out = [], None
    if not a.trace:
        import multiprocessing as mp
        with mp.get_context("fork").Pool(a.procs) as pool:
            args = [(images[i], planes[i], jobs[i, 0], drawn[i]) for i in range(n)]
            pool.map(pillow_one, args)                       # warm-up
            for _ in range(a.reps):
                t0 = time.perf_counter(); pil_out = pool.map(pillow_one, args); pil_t.append((time.perf_counter() - t0) * 1e3)
    import torch
    from unet_watermark_amd import _lib as L
    assert torch.cuda.is_available(), "time_textsynth.py measures on a HIP device"
    dev = torch.device("cuda:0")
    pi, di, _ = D.pack_images(images); pp, dp, _ = D.pack_images([p[..., None] for p in planes])
    Pp, T = D.text_job_needs(jobs, dp)
    lib, st = L.lib(), C.c_void_p(L.stream_ptr(dev))
    it, pt = pi.to(dev), pp.to(dev)
    md = D.mask_descs_for(di)
    mt = torch.zeros(int((md["h"].astype(np.int64) * md["w"]).sum()), dtype=torch.uint8, device=dev)
    dt = D.descs_tensor(np.concatenate([di, md, dp]), dev)
    jt = torch.from_numpy(jobs.reshape(-1).view(np.uint8).copy()).to(dev)
    ws = torch.empty(int(lib.uwm_synth_text_workspace_bytes(n, 1, Pp, T)), dtype=torch.uint8, device=dev)
    step = n * D.DESC_DTYPE.itemsize
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)      # noqa: E731

    def call():
        L.check(lib.uwm_synth_text_u8(ptr(it), it.numel(), ptr(dt), ptr(mt), mt.numel(), ptr(dt, step), 0, ptr(pt), pt.numel(), ptr(dt, 2 * step), n,
                                      ptr(jt), n, 1, Pp, T, ptr(ws), ws.numel(), st))

    call(); torch.cuda.synchronize()
    exact = None
    if pil_out is not None:                                  # the first call ran on the clean batch and zeroed masks: compare it with Pillow's result
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
    sizes = [D.text_job_final_size(jobs[i, 0], (planes[i].shape[1], planes[i].shape[0])) for i in range(n)]
    print(f"text synthesis, {n} images of {h}x{w}x3, one text each: planes of {np.mean([p.size for p in planes]):.0f} pixels and pasted patches of "
          f"{np.mean([s[0] * s[1] for s in sizes]):.0f} pixels on average, {int(jobs['nfit'].sum())} fit resizes, max_patch_pixels {Pp}, max_taps {T}, "
          f"workspace {ws.numel() / 2 ** 20:.1f} MiB | equals Pillow on the same jobs: {exact}")
    v = sorted(ts)
    print(f"uwm_synth_text_u8 (20 launches)     {v[len(v) // 2]:8.3f} ms/batch median of {a.reps} x {a.calls} calls (min {v[0]:.3f}, max {v[-1]:.3f})")
    v = sorted(pil_t)
    print(f"Pillow chain, {a.procs} processes         {v[len(v) // 2]:8.3f} ms/batch median of {a.reps} passes (min {v[0]:.3f}, max {v[-1]:.3f}); "
          "images and canvases pickled to the workers, results back")
    v = sorted(raster)
    print(f"host rasterisation (render_text_plane) {v[len(v) // 2]:6.3f} ms/text median of {n} texts (min {v[0]:.3f}, max {v[-1]:.3f}), one process")


if __name__ == "__main__":
    main()
