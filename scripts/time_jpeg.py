#!/usr/bin/env python3
"""Device time of ImageCompression (uwm_jpeg_u8: the block pass + the pixel pass) at N x S x S x 3: every image compressed (qualities
60..100), the transparent_watermark recipe's mix (30 % of the images), no image (all pass through), and beside them the augment call
in front of it (uwm_augment_ext_u8 with the recipe's descriptors, image + mask + uint8 output) and a device uint8 copy of the batch.
HIP events around 20 calls after 5 warm-ups, repeated 25 times; the median and the spread of the 25 are printed.

  python scripts/time_jpeg.py [--n 16] [--size 512] [--step-ms 13.6]"""
import argparse, ctypes as C, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch


def median_us(fn, warm=5, calls=20, runs=25):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record(); torch.cuda.synchronize()
        t.append(1e3 * e0.elapsed_time(e1) / calls)
    t = np.sort(np.asarray(t))
    return float(np.median(t)), float(t[0]), float(t[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16); ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--step-ms", type=float, default=13.6)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_jpeg.py measures on a HIP device"
    from unet_watermark_amd import _lib as L, data as D
    from unet_watermark_amd.predict import IMAGENET_MEAN, IMAGENET_STD
    dev = torch.device("cuda:0")
    n, s = a.n, a.size
    rng = np.random.default_rng(0)
    # a smooth image with noise on it, like a photograph: flat fields would make every quantised block trivial
    yy, xx = np.mgrid[0:s, 0:s]
    base = (128 + 100 * np.sin(xx / 37.0)[None, :, :, None] * np.cos(yy / 23.0)[None, :, :, None]
            + rng.normal(0, 12, size=(n, s, s, 3))).clip(0, 255).astype(np.uint8)
    x = torch.from_numpy(base).to(dev)
    m = torch.from_numpy(rng.integers(0, 256, size=(n, s, s), dtype=np.uint8)).to(dev)
    out = torch.empty((n, 3, s, s), dtype=torch.float32, device=dev); mo = torch.empty((n, s, s), dtype=torch.uint8, device=dev)
    u8 = torch.empty_like(x)
    mc, sc = (C.c_float * 3)(*IMAGENET_MEAN), (C.c_float * 3)(*IMAGENET_STD)
    lib, st = L.lib(), C.c_void_p(L.stream_ptr(dev))
    ws = torch.empty(int(lib.uwm_jpeg_workspace_bytes(n, s, s)), dtype=torch.uint8, device=dev)
    ews = torch.empty(int(lib.uwm_augment_ext_workspace_bytes(n, s, s, 3)), dtype=torch.uint8, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    up = lambda arr: torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).to(dev)
    print(f"# N = {n}, {s}x{s}x3; median (min .. max) of 25 runs of 20 calls, HIP events, 5 warm-up calls")
    cb = torch.empty_like(x)
    us_copy = median_us(lambda: cb.copy_(x))
    print(f"device uint8 copy of the batch ({x.numel() / 1e6:.1f} MB read, as much written): {us_copy[0]:8.1f} us ({us_copy[1]:.1f} .. {us_copy[2]:.1f})")

    def report(label, t):
        print(f"{label}\n    {t[0]:8.1f} us ({t[1]:.1f} .. {t[2]:.1f}) = {100 * t[0] / (a.step_ms * 1e3):5.2f} % of a {a.step_ms} ms train step; "
              f"{t[0] / us_copy[0]:5.2f} x the uint8 copy's time")

    def jpeg_call(qd, of, ou):
        return lambda: L.check(lib.uwm_jpeg_u8(P(x), P(qd), n, s, s, mc, sc, P(ws), ws.numel(), P(of), P(ou), st))

    q_all = torch.from_numpy(rng.integers(60, 101, size=n).astype(np.int32)).to(dev)
    report("uwm_jpeg_u8, every image compressed (quality 60..100), fp32 output only (what the training path asks for)",
           median_us(jpeg_call(q_all, out, None)))
    report("uwm_jpeg_u8, every image compressed, fp32 and uint8 outputs", median_us(jpeg_call(q_all, out, u8)))
    p, e, q = D.sample_transparent_recipe(n, s, s, torch.Generator().manual_seed(1))
    report(f"uwm_jpeg_u8, the recipe's mix ({int((q != 0).sum())} of {n} images compressed), fp32 output only",
           median_us(jpeg_call(torch.from_numpy(q).to(dev), out, None)))
    report("uwm_jpeg_u8, no image compressed (the pixel pass copies and normalises), fp32 output only",
           median_us(jpeg_call(torch.zeros(n, dtype=torch.int32, device=dev), out, None)))
    dd, ed = up(p), up(e)
    report(f"uwm_augment_ext_u8 in front of it, the recipe's mix (noise/motion/gauss on {int((e['noise_sigma'] > 0).sum())}/"
           f"{int((e['blur'] == 1).sum())}/{int((e['blur'] == 2).sum())} images), image + mask + uint8 output",
           median_us(lambda: L.check(lib.uwm_augment_ext_u8(P(x), P(m), P(dd), P(ed), n, s, s, 3, mc, sc, 127, P(ews), ews.numel(), P(out),
                                                            P(mo), P(u8), st))))
    full = D.identity_aug_ext_params(n)
    full["noise_sigma"] = 1402; full["seed"] = np.arange(n, dtype=np.uint64) + np.uint64(11); full["blur"] = D.BLUR_GAUSS
    fd = up(full)
    report("uwm_augment_ext_u8, every image noise + Gaussian blur (the recipe's enhanced stages, all on)",
           median_us(lambda: L.check(lib.uwm_augment_ext_u8(P(x), P(m), P(dd), P(fd), n, s, s, 3, mc, sc, 127, P(ews), ews.numel(), P(out),
                                                            P(mo), P(u8), st))))


if __name__ == "__main__":
    main()
