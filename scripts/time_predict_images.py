#!/usr/bin/env python3
"""Host-clocked time of WatermarkPredictor.predict_images on one GPU: 200 calls of eight 512 x 384 images (Unet-resnet34, fp16x3), one
synchronise at the end, three times; prints one JSON line.  The call replays a captured graph, so what differs between two checkouts
of this repository is the host layer around the replay: run it from each, alternating, and compare the medians.
usage: time_predict_images.py [--mask-type watermark|text|mixed]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mask-type", choices=["watermark", "text", "mixed"], default=None)
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    from unet_watermark_amd.config import get_cfg_defaults
    from unet_watermark_amd.predict import WatermarkPredictor
    cfg = get_cfg_defaults(); cfg.MODEL.NAME = "Unet"; cfg.MODEL.ENCODER_NAME = "resnet34"
    torch.manual_seed(42)
    pred = WatermarkPredictor(config=cfg, device="cuda", precision="f16x3")
    rng = np.random.default_rng(7)
    imgs = [rng.integers(0, 256, (512, 384, 3), dtype=np.uint8) for _ in range(8)]
    kw = {} if a.mask_type is None else {"mask_type": a.mask_type}
    for _ in range(5):
        pred.predict_images(imgs, **kw)
    torch.cuda.synchronize()
    reps = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(a.calls):
            m = pred.predict_images(imgs, **kw)
        torch.cuda.synchronize()
        reps.append(time.perf_counter() - t0)
    print(json.dumps({"mask_type": a.mask_type, "calls": a.calls, "seconds": [round(r, 4) for r in reps],
                      "ms_per_call_median": round(1000 * sorted(reps)[1] / a.calls, 4), "checksum": int(sum(int(x.sum()) for x in m) % 1000003)}))


if __name__ == "__main__":
    main()
