#!/usr/bin/env python3
"""Device time of the JPEG save of the synthesis chain (uwm_jpeg_ragged_u8: the block pass + the pixel pass, out beside in) on packed ragged
batches: 16 and 64 images of 720 x 1280 at quality 95 and a batch of mixed sizes; beside it uwm_jpeg_u8 (uint8 output only) on the same
720 x 1280 images — both sides are multiples of 16, so the fixed-shape kernel is the yardstick — Pillow's encode + decode of the same
images on 16 threads (libjpeg releases the GIL), and one DeviceInputPipeline._synth_u8 batch with the flag on against off (host clock
around the call and a synchronise: packing and uploads included).  GB/s is against the traffic floor of the two passes, 9 bytes per
pixel: 3 read, 1.5 written and 1.5 read for the planes, 3 written.  HIP events around 20 calls after 5 warm-ups, repeated 15 times; the
median and the spread are printed.

  python scripts/time_jpeg_ragged.py [--quality 95] [--out profiles/jpeg_ragged_mi355x.txt]"""
import argparse, ctypes as C, io, os, sys, tempfile, time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

MIXED_SIZES = [(720, 1280), (1080, 1920), (480, 640), (333, 500), (1000, 667), (512, 512), (97, 1201), (768, 1024)] * 2      # (h, w)


def median_ms(fn, warm=5, calls=20, runs=15):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record(); torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) / calls)
    t = np.sort(np.asarray(t))
    return float(np.median(t)), float(t[0]), float(t[-1])


def photo(rng, h, w):
    """a smooth image with noise on it, like a photograph: flat fields would make every quantised block trivial"""
    yy, xx = np.mgrid[0:h, 0:w]
    return (128 + 100 * np.sin(xx / 37.0)[..., None] * np.cos(yy / 23.0)[..., None] + rng.normal(0, 12, size=(h, w, 3))).clip(0, 255).astype(np.uint8)


def pillow_ms(images, q, threads=16, runs=3):
    from PIL import Image

    def one(a):
        b = io.BytesIO()
        Image.fromarray(a).save(b, "JPEG", quality=q)
        b.seek(0)
        return np.asarray(Image.open(b).convert("RGB"))

    t = []
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(one, images[:threads]))
        for _ in range(runs):
            t0 = time.perf_counter()
            list(pool.map(one, images))
            t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quality", type=int, default=95); ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_jpeg_ragged.py measures on a HIP device"
    from unet_watermark_amd import _lib as L, data as D
    from unet_watermark_amd.constants import IMAGENET_MEAN, IMAGENET_STD
    dev = torch.device("cuda:0")
    lib, st = L.lib(), C.c_void_p(L.stream_ptr(dev))
    P = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    rng = np.random.default_rng(0)
    lines = []

    def say(s=""):
        print(s, flush=True); lines.append(s)

    say(f"# uwm_jpeg_ragged_u8, quality {a.quality}, out beside in; median (min .. max) of 15 runs of 20 calls, HIP events, 5 warm-up calls")

    def ragged(images, label):
        packed, descs, _ = D.pack_images(images)
        buf = packed.to(dev)
        keep = buf.clone()
        dd = D.descs_tensor(descs, dev)
        qd = torch.full((len(images),), a.quality, dtype=torch.int32, device=dev)
        ws = torch.empty(int(lib.uwm_jpeg_ragged_workspace_bytes(len(images), buf.numel())), dtype=torch.uint8, device=dev)
        pixels = int(sum(im.shape[0] * im.shape[1] for im in images)); mp = int(max(im.shape[0] * im.shape[1] for im in images))

        def call():
            L.check(lib.uwm_jpeg_ragged_u8(P(keep), P(buf), buf.numel(), P(dd), P(qd), len(images), 3, mp, P(ws), ws.numel(), st))

        t = median_ms(call)
        say(f"{label}: {pixels / 1e6:.1f} Mpixel\n    {t[0]:8.3f} ms ({t[1]:.3f} .. {t[2]:.3f}) = {9 * pixels / t[0] / 1e6:7.1f} GB/s of the "
            f"9 B/pixel floor, {t[0] * 1e9 / pixels:.2f} ps/pixel")
        return t[0]

    for n in (16, 64):
        base = [photo(rng, 720, 1280) for _ in range(16)]
        images = (base * (n // 16))[:n]
        t_r = ragged(images, f"ragged, {n} x 720x1280")
        x = torch.from_numpy(np.stack(images)).to(dev)
        u8 = torch.empty_like(x)
        q = torch.full((n,), a.quality, dtype=torch.int32, device=dev)
        ws = torch.empty(int(lib.uwm_jpeg_workspace_bytes(n, 720, 1280)), dtype=torch.uint8, device=dev)
        mc, sc = (C.c_float * 3)(*IMAGENET_MEAN), (C.c_float * 3)(*IMAGENET_STD)
        t_f = median_ms(lambda: L.check(lib.uwm_jpeg_u8(P(x), P(q), n, 720, 1280, mc, sc, P(ws), ws.numel(), None, P(u8), st)))
        say(f"uwm_jpeg_u8 (fixed shape, uint8 output only), the same {n} images\n    {t_f[0]:8.3f} ms ({t_f[1]:.3f} .. {t_f[2]:.3f}); "
            f"ragged / fixed = {t_r / t_f[0]:.2f}")
        del x, u8, ws
        if n == 16:
            t_p = pillow_ms(images, a.quality)
            say(f"Pillow save(quality={a.quality}) + reload of the same 16 images on 16 threads\n    {t_p[0]:8.1f} ms ({t_p[1]:.1f} .. {t_p[2]:.1f}) = "
                f"{t_p[0] / t_r:.0f} x the ragged call")
    ragged([photo(rng, h, w) for h, w in MIXED_SIZES], f"ragged, {len(MIXED_SIZES)} images of mixed sizes (97x1201 .. 1080x1920)")

    # one _synth_u8 batch, flag on against off
    from PIL import Image
    with tempfile.TemporaryDirectory() as root:
        os.makedirs(f"{root}/clean"); os.makedirs(f"{root}/logos")
        for i in range(16):
            Image.fromarray(photo(rng, 720, 1280)).save(f"{root}/clean/im{i:02d}.png")
        for i, (h, w) in enumerate([(120, 300), (200, 200), (90, 160)]):
            g = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8); g[..., 3] = 200
            Image.fromarray(g, "RGBA").save(f"{root}/logos/l{i}.png")
        res = {}
        for quality in (0, a.quality) * 3:                          # alternating
            ds = D.RawSynthDataset(f"{root}/clean", f"{root}/logos", seed=1, mask_threshold=30, jpeg_quality=quality)
            pipe = D.DeviceInputPipeline(512, dev, source=ds)
            items = [ds[i] for i in range(16)]
            for _ in range(3):
                pipe.to_u8(items)
            torch.cuda.synchronize()
            t = []
            for _ in range(20):
                t0 = time.perf_counter()
                pipe.to_u8(items); torch.cuda.synchronize()
                t.append(1e3 * (time.perf_counter() - t0))
            res.setdefault(quality, []).append(float(np.median(t)))
        off, on = res[0], res[a.quality]
        say(f"DeviceInputPipeline._synth_u8, 16 logo samples of 720x1280 -> 512x512, masks from pairs; host clock to a synchronise, median of "
            f"20, three alternating rounds\n    flag off {' / '.join(f'{v:.2f}' for v in off)} ms, jpeg_quality {a.quality} "
            f"{' / '.join(f'{v:.2f}' for v in on)} ms: {np.mean(on) - np.mean(off):+.2f} ms")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
