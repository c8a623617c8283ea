#!/usr/bin/env python3
"""Device time of uwm_optimize_mask on seeded blob + stroke + 1 % noise masks (tests/maskpost_ref.synth), per mask type and batch
size, beside the host time of the numpy restatement (tests/maskpost_ref.py — a restatement of the specification, NOT OpenCV) on
the same masks.  HIP events around 20 calls after 3 warm-ups.

  python scripts/time_maskpost.py [--size 768 1024] [--batches 1 8 64] [--ref-images 4]"""
import argparse, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=(768, 1024)); ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--ref-images", type=int, default=4)
    a = ap.parse_args()
    import maskpost_ref as R
    import unet_watermark_amd as U
    h, w = a.size
    masks = np.stack([R.synth(h, w, 1000 + i) for i in range(max(a.batches))]).astype(np.uint8) * 255
    dev = torch.from_numpy(masks).cuda()
    print(f"masks {h} x {w}, foreground {100 * float((masks > 127).mean()):.1f} %")
    for t in R.MASK_TYPES:
        t0 = time.perf_counter()
        refs = [R.optimize_mask(masks[i], t)[0] for i in range(a.ref_images)]
        ref_ms = 1e3 * (time.perf_counter() - t0) / a.ref_images
        for n in a.batches:
            x = dev[:n].contiguous()
            out = torch.empty_like(x)
            for _ in range(3):
                U.optimize_mask(x, t, out=out)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                U.optimize_mask(x, t, out=out)
            e1.record(); torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / 20
            k = min(n, a.ref_images)
            same = all(np.array_equal(out[i].cpu().numpy(), refs[i]) for i in range(k))
            print(f"{t:9s} bs{n:<3d} device {ms:8.3f} ms per batch = {1e3 * ms / n:8.1f} us per image | numpy restatement on this host {ref_ms:7.1f} ms per image"
                  f" | first {k} equal the restatement: {same}")


if __name__ == "__main__":
    main()
