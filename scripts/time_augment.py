#!/usr/bin/env python3
"""Device time of the augmentation kernels (uwm_augment_u8) at N x S x S x 3, with the parameter mix of the basic recipe
(data.sample_aug_params) and with every stage switched on for every image, in us and in GB/s of the bytes the call has to move (the
uint8 image read once + the fp32 NCHW output written; the mask read + written), beside a device copy of the same byte count on the
same machine (the copy ceiling) and as a share of the train step.  Then, end to end, `main.py train --augment none` against
`--augment basic` on a folder of generated PNGs of mixed sizes that this script writes (fresh processes, alternating; img/s of the
epochs after the first, as the trainer reports them).  HIP events around repeated calls after warm-ups.

  python scripts/time_augment.py [--n 16] [--size 512] [--images 320] [--epochs 3] [--workers 8] [--encoder resnet34] [--reps 2]
                                 [--step-ms 13.6] [--skip-e2e]"""
import argparse, ctypes as C, json, os, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch


def events(fn, warm=5, calls=50):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record(); torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / calls          # us per call


def kernel_times(a):
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
    g = torch.Generator().manual_seed(1)
    mix = D.sample_aug_params(n, s, s, g)
    full = D.identity_aug_params(n)
    full["flags"] = D.random_aug_flags(n, g).numpy() | 1
    for i in range(n):
        full["minv"][i] = D.affine_inverse(s, s, 15.0 - 2.0 * i, 0.9 + 0.0125 * i, 0.1 - 0.0125 * i, -0.1 + 0.0125 * i)
        full["lut"][i] = D.brightness_contrast_lut(1.2 - 0.025 * i, -0.2 + 0.025 * i)
        full["hue"][i], full["sat"][i], full["val"][i] = 10 - i, 20 - 2 * i, i - 5
    img_b, mask_b = n * s * s * 3 * (1 + 4), n * s * s * 2
    ca, cb = torch.empty(img_b // 2, dtype=torch.uint8, device=dev), torch.empty(img_b // 2, dtype=torch.uint8, device=dev)
    us_copy = events(lambda: cb.copy_(ca))
    print(f"device copy of the image call's {img_b / 1e6:.1f} MB (read + written): {us_copy:8.1f} us = {img_b / us_copy / 1e3:7.1f} GB/s   (the copy ceiling)")
    P = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    for label, p in (("basic recipe's parameter mix", mix), ("every stage on, every image", full)):
        D._check_aug_params(p, n, s, s, 3)
        dd = torch.from_numpy(p.view(np.uint8).reshape(-1).copy()).to(dev)
        stages = [int((p["minv"] != np.array(D.IDENTITY_MINV)).any(1).sum()), int((p["lut"] != np.arange(256)).any(1).sum()),
                  int(((p["hue"] != 0) | (p["sat"] != 0) | (p["val"] != 0)).sum())]
        image = lambda: L.check(lib.uwm_augment_u8(P(x), None, P(dd), n, s, s, 3, mc, sc, 127, P(out), None, None, st))
        both = lambda: L.check(lib.uwm_augment_u8(P(x), P(m), P(dd), n, s, s, 3, mc, sc, 127, P(out), P(mo), None, st))
        us_i, us_b = events(image), events(both)
        print(f"uwm_augment_u8, {n} x {s}x{s}x3, {label} (affine/table/hsv on {stages[0]}/{stages[1]}/{stages[2]} images):")
        print(f"    image launch        {us_i:8.1f} us = {img_b / us_i / 1e3:7.1f} GB/s of {img_b / 1e6:.1f} MB = {100 * us_copy / us_i:5.1f} % of the copy ceiling")
        print(f"    image + mask launch {us_b:8.1f} us = {(img_b + mask_b) / us_b / 1e3:7.1f} GB/s of {(img_b + mask_b) / 1e6:.1f} MB; "
              f"{100 * us_b / (a.step_ms * 1e3):.2f} % of a {a.step_ms} ms train step")
    flags = torch.from_numpy(mix["flags"].copy()).to(dev)
    us_p = events(lambda: D.device_preprocess(x, m, flags))
    print(f"for scale: device_preprocess (flips / rot90 + Normalize, image + mask, with its allocations) {us_p:8.1f} us")


def write_folder(root, count, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "watermarked")); os.makedirs(os.path.join(root, "masks"))
    for i in range(count):
        h, w = int(rng.integers(300, 900)), int(rng.integers(300, 900))
        base = rng.integers(0, 256, size=(h // 16 + 1, w // 16 + 1, 3), dtype=np.uint8)
        img = np.asarray(Image.fromarray(base).resize((w, h), Image.BILINEAR)).copy()
        mk = np.zeros((h, w), dtype=np.uint8)
        y0, x0 = int(rng.integers(0, h // 2)), int(rng.integers(0, w // 2))
        mk[y0: y0 + h // 3, x0: x0 + w // 3] = 255
        img[mk > 0] = (img[mk > 0].astype(np.int32) * 6 // 10 + 100).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(root, "watermarked", f"im{i:04d}.png"))
        Image.fromarray(mk).save(os.path.join(root, "masks", f"im{i:04d}.png"))


def end_to_end(a):
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "data")
        write_folder(root, a.images)
        res = {"none": [], "basic": []}
        for rep in range(a.reps):
            for mode in ("none", "basic"):
                cmd = [sys.executable, os.path.join(ROOT, "main.py"), "train", "--data-dir", root, "--epochs", str(a.epochs), "--batch-size", str(a.n),
                       "--img-size", str(a.size), "--encoder", a.encoder, "--model", "Unet", "--workers", str(a.workers), "--augment", mode,
                       "--no-early-stopping", "--model-save-path", os.path.join(tmp, f"{mode}{rep}.pth"),
                       "--checkpoint-dir", os.path.join(tmp, f"ck_{mode}{rep}")]
                r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.e2e_timeout)
                if r.returncode != 0:
                    raise SystemExit(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout[-3000:]}")
                recs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{") and "images_per_sec" in l]
                res[mode].append([rec["images_per_sec"] for rec in recs])
        for mode, label in (("none", "host path: PIL decode + resize + normalise in the workers, fp32 upload, no augmentation"),
                            ("basic", "device path: PIL decode in the workers, uint8 upload, resize + augment + normalise on the device")):
            later = [v for run in res[mode] for v in run[1:]]
            print(f"main.py train --augment {mode:5s} ({label}): {np.mean(later):7.1f} img/s over epochs 2.. of {a.reps} runs "
                  f"(per epoch: {'; '.join(', '.join(f'{v:.1f}' for v in run) for run in res[mode])})")
        print(f"    ({a.images} PNGs of 300..899 pixels a side, {int(a.images * 0.8)} of them trained on per epoch, batch {a.n}, {a.size}x{a.size}, "
              f"{a.encoder} Unet, {a.workers} workers)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16); ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--images", type=int, default=320); ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--workers", type=int, default=8); ap.add_argument("--encoder", default="resnet34")
    ap.add_argument("--reps", type=int, default=2); ap.add_argument("--step-ms", type=float, default=13.6)
    ap.add_argument("--e2e-timeout", type=int, default=240); ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_augment.py measures on a HIP device"
    kernel_times(a)
    if not a.skip_e2e:
        end_to_end(a)


if __name__ == "__main__":
    main()
