#!/usr/bin/env python3
"""Device time of the enhanced recipe's call (uwm_augment_ext_u8: stage pass + CLAHE tile tables + apply pass) at N x S x S x 3,
image + mask, by the method of scripts/time_augment.py (HIP events around 50 calls after 5 warm-ups): with the enhanced recipe's
parameter mix (data.sample_aug_recipe), with every stage on for every image (CLAHE + noise + Gaussian blur, and gamma + noise +
motion blur), with ext = NULL, beside uwm_augment_u8 with the basic recipe's mix (augment_u8.hip is unchanged, so this is the basic
call as it was), a device copy of the image call's byte count (the copy ceiling), and each as a share of the train step.

  python scripts/time_augment_ext.py [--n 16] [--size 512] [--step-ms 13.6]"""
import argparse, ctypes as C, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from time_augment import events


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16); ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--step-ms", type=float, default=13.6)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_augment_ext.py measures on a HIP device"
    from unet_watermark_amd import _lib as L, data as D
    from unet_watermark_amd.predict import IMAGENET_MEAN, IMAGENET_STD
    dev = torch.device("cuda:0")
    n, s = a.n, a.size
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.integers(0, 256, size=(n, s, s, 3), dtype=np.uint8)).to(dev)
    m = torch.from_numpy(rng.integers(0, 256, size=(n, s, s), dtype=np.uint8)).to(dev)
    out = torch.empty((n, 3, s, s), dtype=torch.float32, device=dev); mo = torch.empty((n, s, s), dtype=torch.uint8, device=dev)
    mc, sc = (C.c_float * 3)(*IMAGENET_MEAN), (C.c_float * 3)(*IMAGENET_STD)
    lib, st = L.lib(), C.c_void_p(L.stream_ptr(dev))
    ws = torch.empty(int(lib.uwm_augment_ext_workspace_bytes(n, s, s, 3)), dtype=torch.uint8, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    up = lambda arr: torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).to(dev)
    img_b, mask_b = n * s * s * 3 * (1 + 4), n * s * s * 2
    ca, cb = torch.empty(img_b // 2, dtype=torch.uint8, device=dev), torch.empty(img_b // 2, dtype=torch.uint8, device=dev)
    us_copy = events(lambda: cb.copy_(ca))
    print(f"device copy of the image call's {img_b / 1e6:.1f} MB (read + written): {us_copy:8.1f} us = {img_b / us_copy / 1e3:7.1f} GB/s   (the copy ceiling)")

    def report(label, us):
        print(f"{label}\n    image + mask {us:8.1f} us = {100 * us / (a.step_ms * 1e3):5.2f} % of a {a.step_ms} ms train step; "
              f"{us / us_copy:5.2f} x the copy ceiling's time")

    basic = D.sample_aug_params(n, s, s, torch.Generator().manual_seed(1))
    dd = up(basic)
    report(f"uwm_augment_u8, {n} x {s}x{s}x3, basic recipe's parameter mix",
           events(lambda: L.check(lib.uwm_augment_u8(P(x), P(m), P(dd), n, s, s, 3, mc, sc, 127, P(out), P(mo), None, st))))

    def ext_call(dd, ed):
        return lambda: L.check(lib.uwm_augment_ext_u8(P(x), P(m), P(dd), P(ed), n, s, s, 3, mc, sc, 127, P(ws), ws.numel(), P(out), P(mo), None, st))

    report("uwm_augment_ext_u8, ext = NULL, the same descriptors", events(ext_call(dd, None)))
    p, e = D.sample_aug_recipe(n, s, s, torch.Generator().manual_seed(1), "enhanced")
    D._check_aug_ext_params(e, n, s, s, 3)
    report(f"uwm_augment_ext_u8, enhanced recipe's parameter mix (CLAHE/gamma/noise/motion/gauss on {int((e['tone'] == 1).sum())}/"
           f"{int((e['tone'] == 2).sum())}/{int((e['noise_sigma'] > 0).sum())}/{int((e['blur'] == 1).sum())}/{int((e['blur'] == 2).sum())} images)",
           events(ext_call(up(p), up(e))))
    report("uwm_augment_ext_u8, identity ext descriptors (stage pass + two launches that leave at once)",
           events(ext_call(dd, up(D.identity_aug_ext_params(n)))))
    full = D.identity_aug_ext_params(n)
    full["tone"] = D.TONE_CLAHE; full["clahe_clip"] = D.clahe_clip_limit(2.0, s, s)
    full["noise_sigma"] = 1402; full["seed"] = np.arange(n, dtype=np.uint64) + np.uint64(11); full["blur"] = D.BLUR_GAUSS
    report("uwm_augment_ext_u8, every image CLAHE + noise + Gaussian blur (9 recomputed taps)", events(ext_call(dd, up(full))))
    full["tone"] = D.TONE_TABLE; full["lut2"] = D.gamma_lut(0.9); full["blur"] = D.BLUR_MOTION
    full["blur_w"] = D.motion_kernel((0, 0), (2, 2))
    report("uwm_augment_ext_u8, every image gamma + noise + motion blur (3 taps)", events(ext_call(dd, up(full))))
    full["blur"] = D.BLUR_NONE; full["noise_sigma"] = 0; full["tone"] = D.TONE_CLAHE
    report("uwm_augment_ext_u8, every image CLAHE only", events(ext_call(dd, up(full))))


if __name__ == "__main__":
    main()
