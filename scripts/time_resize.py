#!/usr/bin/env python3
"""Device time of the fused resize + Normalize kernel (uwm_op_resize_norm_u8_nhwc4) on a batch of equal-sized photographs, in us and
in GB/s of the bytes it actually touches (the source rows some output row reads, once, + the fp32 NHWC4 output), beside a device
copy of the same byte count on the same machine (the copy ceiling scripts/hbm_floor.py quotes is 6.3 TB/s); then, end to end,
WatermarkPredictor.predict_images on those images against the host-resize path (PIL resize -> preprocess -> logits -> resize_threshold
per image), both in images per second, alternating, masks left on the device.  HIP events / a host clock around synchronised work,
after warm-ups.

  python scripts/time_resize.py [--n 64] [--src 720 1280] [--size 512] [--encoder resnet34] [--reps 3]"""
import argparse, ctypes as C, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch


def events(fn, warm=3, calls=20):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record(); torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / calls          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64); ap.add_argument("--src", type=int, nargs=2, default=(720, 1280))
    ap.add_argument("--size", type=int, default=512); ap.add_argument("--encoder", default="resnet34"); ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--e2e-calls", type=int, default=4)
    a = ap.parse_args()
    import resize_ref as R
    import unet_watermark_amd as U
    from unet_watermark_amd import _lib as L
    from unet_watermark_amd.config import get_cfg_defaults
    from unet_watermark_amd.data import descs_tensor
    from unet_watermark_amd.predict import WatermarkPredictor, IMAGENET_MEAN, IMAGENET_STD
    assert torch.cuda.is_available(), "time_resize.py measures on a HIP device"
    dev = torch.device("cuda:0")
    h, w = a.src
    s, n = a.size, a.n
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for _ in range(n)]

    # ---- the kernel alone
    packed, descs, _ = U.pack_images(imgs)
    src, dd = packed.to(dev), descs_tensor(descs, dev)
    out = torch.empty((n, s, s, 4), dtype=torch.float32, device=dev)
    mc, sc = (C.c_float * 3)(*IMAGENET_MEAN), (C.c_float * 3)(*IMAGENET_STD)
    lib, st = L.lib(), C.c_void_p(L.stream_ptr(dev))
    fused = lambda: L.check(lib.uwm_op_resize_norm_u8_nhwc4(C.c_void_p(src.data_ptr()), src.numel(), C.c_void_p(dd.data_ptr()), n, 3, s, s,
                                                           mc, sc, C.c_void_p(out.data_ptr()), st))
    sy, sy1, _, _ = R.taps(s, h)
    rows = len(set(sy.tolist()) | set(sy1.tolist()))
    read_b, write_b = n * rows * w * 3, n * s * s * 16
    us = events(fused)
    want = U.device_preprocess(U.device_resize(src, dd, s, 3)).permute(0, 2, 3, 1)
    same = torch.equal(out[..., :3], want)
    a_, b_ = torch.empty((read_b + write_b) // 2, dtype=torch.uint8, device=dev), torch.empty((read_b + write_b) // 2, dtype=torch.uint8, device=dev)
    us_copy = events(lambda: b_.copy_(a_))
    print(f"fused resize + normalize, {n} x {h}x{w}x3 -> {s}x{s}: {us:8.1f} us = {(read_b + write_b) / us / 1e3:7.1f} GB/s "
          f"({read_b / 1e6:.1f} MB of {rows}/{h} source rows read + {write_b / 1e6:.1f} MB written) | equals resize_u8 -> preprocess: {same}")
    print(f"device copy of the same {(read_b + write_b) / 1e6:.1f} MB (read + written):   {us_copy:8.1f} us = {(read_b + write_b) / us_copy / 1e3:7.1f} GB/s")

    # ---- end to end, alternating
    from PIL import Image
    cfg = get_cfg_defaults(); cfg.MODEL.NAME = "Unet"; cfg.MODEL.ENCODER_NAME = a.encoder; cfg.DATA.IMG_SIZE = s
    pred = WatermarkPredictor(config=cfg, device="cuda", precision="f16x3", freeze=True)
    pils = [Image.fromarray(im) for im in imgs]

    def host_path():                                   # predict_command's default path, without the PNG writes
        arr = np.stack([np.asarray(im.resize((s, s), Image.BILINEAR), dtype=np.uint8) for im in pils])
        logits = pred.logits(pred.preprocess(torch.from_numpy(arr)), use_graph=True)
        return [U.resize_threshold(logits[k:k + 1], (h, w), pred.threshold, False) for k in range(n)]

    def device_path():
        return pred.predict_images(imgs, use_graph=True)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.e2e_calls):
            fn()
        torch.cuda.synchronize()
        return n * a.e2e_calls / (time.perf_counter() - t0)

    host_path(); device_path(); host_path(); device_path()
    res = {"host": [], "device": []}
    for _ in range(a.reps):
        res["host"].append(clock(host_path)); res["device"].append(clock(device_path))
    for k, label in (("host", "PIL resize -> preprocess -> logits -> resize_threshold per image"), ("device", "predict_images (one graph replay per batch)")):
        v = res[k]
        print(f"end to end, {n} images {h}x{w} -> {a.encoder} Unet at {s}, f16x3 frozen: {label:66s} {np.mean(v):8.1f} img/s (runs: {', '.join(f'{x:.1f}' for x in v)})")


if __name__ == "__main__":
    main()
