#!/usr/bin/env python3
"""Device time of the ragged mask post-processing (uwm_optimize_masks_ragged) beside the routes it replaces or is bounded by, on
seeded blob + stroke + 1 % noise masks (tests/maskpost_ref.synth), per mask type:

  (a) one ragged call on 64 masks of 720 x 1280
  (b) 64 calls of uwm_optimize_mask at N = 1 on the same masks         (what predict_images did per batch before)
  (c) one uwm_optimize_mask call at N = 64                             (the floor for equal sizes)
  (d) (a) and (b) again on a mixed batch: 1 mask of 1440 x 2560 and 63 of 180 x 320
  (e) predict_images(mask_type='watermark') on 64 photographs of 720 x 1280 against predict_images(mask_type=None) followed by
      optimize_mask image by image                                    (whole calls, host clock around a device synchronise)

2 warm-ups of every route, then 7 windows in which the routes alternate; (a)-(d) are timed with HIP events around the window's calls
(100 calls of a one-call route, 10 turns of a 64-call route, 5 calls of (e): about 0.1 s of work per window).
A route's figure is the median of its 7 windows, with the least and the greatest beside it.

  python scripts/time_maskpost_ragged.py [--out profiles/maskpost_ragged_mi355x.txt] [--images 64] [--windows 7]"""
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


def host_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def windows(routes, n_windows, timer):
    """routes: {name: (fn, reps)} -> {name: [ms per call, one per window]}; 2 warm-ups each, then the routes alternate"""
    for fn, _ in routes.values():
        fn(); fn()
    torch.cuda.synchronize()
    out = {k: [] for k in routes}
    for _ in range(n_windows):
        for k, (fn, reps) in routes.items():
            out[k].append(timer(fn, reps))
    return out


def fmt(v):
    return f"median {np.median(v):8.3f} ms  (min {min(v):8.3f}, max {max(v):8.3f}, spread {max(v) - min(v):6.3f})"


def clears(fast, slow):
    """the acceptance rule: the medians differ by more than the min-to-max spread of either route's windows"""
    return np.median(slow) - np.median(fast) > max(max(fast) - min(fast), max(slow) - min(slow))


def ragged_batch(masks, dev):
    from unet_watermark_amd.data import DESC_DTYPE, descs_tensor
    descs = np.zeros(len(masks), DESC_DTYPE)
    off = 0
    for i, m in enumerate(masks):
        descs[i] = (off, m.shape[0], m.shape[1])
        off += m.size
    buf = torch.from_numpy(np.concatenate([m.reshape(-1) for m in masks])).to(dev)
    views = [buf[int(d["offset"]): int(d["offset"]) + int(d["h"]) * int(d["w"])].view(int(d["h"]), int(d["w"])) for d in descs]
    caps = dict(n=len(masks), max_pixels=max(m.size for m in masks), rows=sum(m.shape[0] for m in masks))
    return buf, descs_tensor(descs, dev), views, caps


def photographs(n, h, w, seed):
    """smooth seeded images with a bright rectangle each, as the tests use"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        base = rng.integers(0, 256, size=(h // 40 + 2, w // 40 + 2, 3), dtype=np.uint8)
        a = np.asarray(Image.fromarray(base).resize((w, h), Image.BILINEAR)).copy()
        a[h // 4: h // 4 + h // (2 + i % 3), w // 5: w // 5 + w // 2] = 255 - 40 * (i % 4)
        out.append(a)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "maskpost_ragged_mi355x.txt"))
    ap.add_argument("--images", type=int, default=64); ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--skip-predict", action="store_true", help="leave route (e) out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_maskpost_ragged needs a HIP device (a timing without one says nothing)")
    import maskpost_ref as R
    import unet_watermark_amd as U
    from unet_watermark_amd.postprocess import optimize_masks_ragged
    dev = torch.device("cuda:0")
    n = a.images
    say(f"scripts/time_maskpost_ragged.py : {torch.cuda.get_device_name(0)}, {n} masks, {a.windows} windows after 2 warm-ups of every route, routes alternating")
    equal = [R.synth(720, 1280, 2000 + i).astype(np.uint8) * 255 for i in range(n)]
    mixed = [R.synth(1440, 2560, 3000).astype(np.uint8) * 255] + [R.synth(180, 320, 3001 + i).astype(np.uint8) * 255 for i in range(n - 1)]
    say(f"equal batch: {n} x 720 x 1280, foreground {100 * float(np.mean([(m > 127).mean() for m in equal])):.1f} %;  mixed batch: 1 x 1440 x 2560 + {n - 1} x 180 x 320")
    ebuf, edesc, eviews, ecaps = ragged_batch(equal, dev)
    mbuf, mdesc, mviews, mcaps = ragged_batch(mixed, dev)
    block = ebuf.view(n, 720, 1280)
    eout, mout, bout = torch.empty_like(ebuf), torch.empty_like(mbuf), torch.empty_like(block)
    eone = [torch.empty_like(v) for v in eviews]
    mone = [torch.empty_like(v) for v in mviews]
    verdict = {}
    for t in R.MASK_TYPES:
        routes = {
            "a": (lambda: optimize_masks_ragged(ebuf, edesc, t, out=eout, **ecaps), 100),
            "b": (lambda: [U.optimize_mask(v, t, out=o) for v, o in zip(eviews, eone)], 10),
            "c": (lambda: U.optimize_mask(block, t, out=bout), 100),
            "d_ragged": (lambda: optimize_masks_ragged(mbuf, mdesc, t, out=mout, **mcaps), 100),
            "d_single": (lambda: [U.optimize_mask(v, t, out=o) for v, o in zip(mviews, mone)], 10),
        }
        r = windows(routes, a.windows, event_ms)
        same = torch.equal(eout, torch.cat([o.reshape(-1) for o in eone])) and torch.equal(eout, bout.reshape(-1)) \
            and torch.equal(mout, torch.cat([o.reshape(-1) for o in mone]))
        say(f"--- {t}")
        say(f"(a) one ragged call, equal batch          {fmt(r['a'])}")
        say(f"(b) {n} calls at N = 1, equal batch        {fmt(r['b'])}")
        say(f"(c) one call at N = {n}, equal batch       {fmt(r['c'])}")
        say(f"(d) one ragged call, mixed batch          {fmt(r['d_ragged'])}")
        say(f"(d) {n} calls at N = 1, mixed batch        {fmt(r['d_single'])}")
        say(f"    (a)/(b) = {np.median(r['a']) / np.median(r['b']):.3f}   (a)/(c) = {np.median(r['a']) / np.median(r['c']):.3f}   "
            f"(d ragged)/(d single) = {np.median(r['d_ragged']) / np.median(r['d_single']):.3f}")
        say(f"    the masks of (a) equal those of (b) and (c), and the masks of the two (d) routes are equal: {same}")
        verdict[t] = bool(clears(r["a"], r["b"])) and same
        say(f"    (a) below (b) by more than the spread of the windows: {verdict[t]}")
    if not a.skip_predict:
        from unet_watermark_amd.config import get_cfg_defaults
        from unet_watermark_amd.constants import IMAGENET_MEAN, IMAGENET_STD
        from unet_watermark_amd.predict import WatermarkPredictor
        torch.manual_seed(7)
        cfg = get_cfg_defaults(); cfg.MODEL.NAME = "Unet"; cfg.MODEL.ENCODER_NAME = "resnet18"
        pred = WatermarkPredictor(model=U.Unet("resnet18"), config=cfg, device=dev)
        photos = photographs(n, 720, 1280, 9)
        s = int(cfg.DATA.IMG_SIZE)
        packed, descs, _ = U.pack_images(photos[:8])
        _, lg = pred.model.predict_u8(U.device_resize(packed, descs, s, 3), IMAGENET_MEAN, IMAGENET_STD, 0.0, return_logits=True)
        pred.threshold = float(lg.median())
        res = {}

        def new():
            res["new"] = pred.predict_images(photos, mask_type="watermark")

        def old():
            res["old"] = [U.optimize_mask(m, "watermark") for m in pred.predict_images(photos, mask_type=None)]
        r = windows({"new": (new, 5), "old": (old, 5)}, a.windows, host_ms)
        same = all(torch.equal(x, y) for x, y in zip(res["new"], res["old"]))
        fg = float(np.mean([float((m > 0).float().mean()) for m in res["new"]]))
        say(f"--- (e) predict_images on {n} photographs of 720 x 1280, Unet resnet18 at IMG_SIZE {s}, seeded weights, threshold = median logit "
            f"(foreground of the results {100 * fg:.1f} %); whole calls incl. host packing and upload")
        say(f"(e) mask_type='watermark' inside the graph     {fmt(r['new'])}")
        say(f"(e) mask_type=None, then 64 x optimize_mask    {fmt(r['old'])}")
        say(f"    new/old = {np.median(r['new']) / np.median(r['old']):.3f}; the masks are equal: {same}")
        verdict["e"] = bool(clears(r["new"], r["old"])) and same
        say(f"    new below old by more than the spread of the windows: {verdict['e']}")
    say(f"acceptance: {verdict}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
