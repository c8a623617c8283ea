#!/usr/bin/env python3
"""Device time of prediction with test-time augmentation (WatermarkPredictor.predict_images / predict_images_tiled with tta=...,
uwm_predict_images_tta_u8 / uwm_predict_tiled_tta_u8, csrc/tta.hip), Unet-resnet34 (fp16x3, frozen) at 512:

  resized   64 seeded photographs of 720 x 1280, forward batch 64: the plain call is predict_images as it was (one forward of 64)
  tiled     16 seeded images of 2160 x 3840, tile 512, overlap 64, forward batch 48: the plain call is predict_images_tiled

Reported per case, all in the same run with HIP events, 2 warm-ups of every item and then --windows windows in which the items
alternate (a figure is the median of its windows, with the least and the greatest beside it):

  the plain call      one replay of the captured call without views
  d4 / flips / hflip  one replay of the captured call with that view set, beside k times the plain call
  the views           the input side of d4 alone, launched once per chunk as the call launches it (base planes into the staging buffer,
                      then the permuting kernel), and the base planes alone (the existing resize / gather kernel on the same images)
  the merges          uwm_op_view_merge of d4 alone, once per chunk, on a logit buffer of the forward's shape

beside the bytes views and merges must move and the time those bytes take at the measured copy rate of the device (6.29 TB/s).

  python scripts/time_tta.py [--out profiles/tta_mi355x.txt] [--windows 7] [--skip-tiled]"""
import argparse, ctypes as C, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

COPY_RATE = 6.29e12                      # bytes / s: the device's measured float4 copy
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def fmt(v):
    return f"median {np.median(v):9.3f} ms  (min {min(v):9.3f}, max {max(v):9.3f})"


def run_case(title, pred, imgs, tiled, overlap, windows):
    from unet_watermark_amd import _lib as L, tiling, tta
    from unet_watermark_amd.predict import IMAGENET_MEAN, IMAGENET_STD
    dev = pred.device
    T, N, n = int(pred.cfg.DATA.IMG_SIZE), int(pred.cfg.PREDICT.BATCH_SIZE), len(imgs)
    call = (lambda **kw: pred.predict_images_tiled(imgs, overlap, **kw)) if tiled else (lambda **kw: pred.predict_images(imgs, **kw))
    group = "tiled" if tiled else "tta"
    table = lambda: {e.key: e.graph for e in pred._graphs.values() if e.group == group}      # (looked up anew: a grown buffer drops entries)
    items, k_of = {}, {}
    call()
    plain_graph = [g for key, g in table().items() if "tta" not in key][-1] if tiled else pred._graphs["images"].graph
    items["plain"] = plain_graph.replay
    for name in ("d4", "flips", "hflip"):
        before = set(table())
        call(tta=name)
        key = [key for key in table() if key not in before]
        assert len(key) == 1
        items[name] = table()[key[0]].replay
        k_of[name] = len(tta.view_codes(name))
    if tiled:
        sizes = [tuple(im.shape[:2]) for im in imgs]
        tiles, _ = tiling.plan_batch(sizes, T, T, overlap, N)
        num = len(tiles)
    else:
        num = n
    # the two kernels alone, for d4, on buffers of the call's shapes
    lib = L.lib()
    st = C.c_void_p(L.stream_ptr(dev))
    P = lambda t: C.c_void_p(t.data_ptr())
    mc, sc = (C.c_float * 3)(*IMAGENET_MEAN[:3]), (C.c_float * 3)(*IMAGENET_STD[:3])
    views, k = 0xFF, 8
    chunks = -(-num * k // N)
    cp = int(lib.uwm_logits_channels(pred.model._h))
    x4 = torch.empty((N, T, T, 4), device=dev)
    stage_bytes = lib.uwm_view_stage_bytes(views, N, T, T)
    stage = torch.empty(stage_bytes // 4, device=dev)
    logits = torch.randn((N, T, T, cp), device=dev)
    store = torch.empty((num, T, T), device=dev)
    src_bytes = pred._ibuf.numel()

    def view_launches():
        for c in range(chunks):
            if tiled:
                L.check(lib.uwm_op_tile_norm_view_u8_nhwc4(P(pred._ibuf), src_bytes, P(pred._idesc), n, P(pred._xtiles), num, 3, T, T, mc, sc, views,
                                                           c * N, N, P(stage), stage_bytes, P(x4), st))
            else:
                L.check(lib.uwm_op_resize_norm_view_u8_nhwc4(P(pred._ibuf), src_bytes, P(pred._idesc), n, 3, T, T, mc, sc, views, c * N, N, P(stage),
                                                             stage_bytes, P(x4), st))

    def base_launches():
        for c in range(chunks):
            i0 = c * N // k
            cnt = min((c * N + N - 1) // k, num - 1) - i0 + 1
            if tiled:
                L.check(lib.uwm_op_tile_norm_u8_nhwc4(P(pred._ibuf), src_bytes, P(pred._idesc), n, C.c_void_p(pred._xtiles.data_ptr() + 16 * i0), cnt, 3,
                                                      T, T, mc, sc, P(stage), st))
            else:
                L.check(lib.uwm_op_resize_norm_u8_nhwc4(P(pred._ibuf), src_bytes, C.c_void_p(pred._idesc.data_ptr() + 16 * i0), cnt, 3, T, T, mc, sc,
                                                        P(stage), st))

    def merge_launches():
        for c in range(chunks):
            L.check(lib.uwm_op_view_merge(P(logits), cp, T, T, views, c * N, N, num, P(store), st))
    items.update(views=view_launches, base=base_launches, merges=merge_launches)
    ms = {name: [] for name in items}
    for _ in range(2):
        for fn in items.values():
            event_ms(fn)
    for _ in range(windows):
        for name, fn in items.items():
            ms[name].append(event_ms(fn))
    med = {name: float(np.median(v)) for name, v in ms.items()}
    say(title)
    say(f"  the plain call, one replay            {fmt(ms['plain'])}   = {1e3 * n / med['plain']:.1f} images/s")
    for name in ("d4", "flips", "hflip"):
        kk = k_of[name]
        say(f"  {name:5s} (k = {kk}), one replay            {fmt(ms[name])}   = {1e3 * n / med[name]:.1f} images/s; {med[name] / med['plain']:.3f} x the plain call, "
            f"{med[name] / (kk * med['plain']):.4f} x (k x the plain call = {kk * med['plain']:.3f} ms)")
    slots = chunks * N
    v_bytes = slots * T * T * 32                         # the permuting kernel: a staged float4 in, a float4 out, per pixel and slot
    m_bytes = num * k * T * T * 4 * cp + num * T * T * 4      # every logit line of the forward's padded output once in, the store once out
    say(f"  d4's views alone, {chunks} x 2 launches       {fmt(ms['views'])}   of which the base planes {med['base']:.3f} ms; the views move {v_bytes / 1e6:.0f} MB: "
        f"at 6.29 TB/s {1e3 * v_bytes / COPY_RATE:.3f} ms")
    say(f"  d4's merges alone, {chunks} launches          {fmt(ms['merges'])}   at least {m_bytes / 1e6:.0f} MB of logit lines and store: at 6.29 TB/s {1e3 * m_bytes / COPY_RATE:.3f} ms")
    say(f"      views + merges: {med['views'] + med['merges']:.3f} ms = {100 * (med['views'] + med['merges']) / med['d4']:.2f} % of the d4 call "
        f"(the permuting kernel and the merge alone, without the base planes: {med['views'] - med['base'] + med['merges']:.3f} ms = "
        f"{100 * (med['views'] - med['base'] + med['merges']) / med['d4']:.2f} %)")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "tta_mi355x.txt"))
    ap.add_argument("--windows", type=int, default=7); ap.add_argument("--encoder", default="resnet34")
    ap.add_argument("--images", type=int, default=64); ap.add_argument("--tiled-images", type=int, default=16)
    ap.add_argument("--skip-tiled", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_tta needs a HIP device (a timing without one says nothing)")
    from unet_watermark_amd.config import get_cfg_defaults
    from unet_watermark_amd.predict import WatermarkPredictor
    say(f"scripts/time_tta.py : {torch.cuda.get_device_name(0)}, {a.windows} windows after 2 warm-ups of every item, items alternating; "
        f"Unet-{a.encoder} (fp16x3, frozen), IMG_SIZE 512")
    say()
    rng = np.random.default_rng(7)
    for tiled in (False, True):
        if tiled and a.skip_tiled:
            continue
        cfg = get_cfg_defaults(); cfg.MODEL.NAME = "Unet"; cfg.MODEL.ENCODER_NAME = a.encoder; cfg.DATA.IMG_SIZE = 512
        cfg.PREDICT.BATCH_SIZE = 48 if tiled else a.images
        torch.manual_seed(42)
        pred = WatermarkPredictor(config=cfg, device="cuda", precision="f16x3", freeze=True)
        if tiled:
            imgs = [rng.integers(0, 256, size=(2160, 3840, 3), dtype=np.uint8) for _ in range(a.tiled_images)]
            title = f"tiled: {a.tiled_images} images of 2160 x 3840, tile 512, overlap 64, forward batch 48 (720 tiles per 16 images; d4: 8 slots per tile)"
        else:
            imgs = [rng.integers(0, 256, size=(720, 1280, 3), dtype=np.uint8) for _ in range(a.images)]
            title = f"resized: {a.images} photographs of 720 x 1280, forward batch {a.images} (the plain call: one forward of {a.images})"
        run_case(title, pred, imgs, tiled, 64, a.windows)
        del pred
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
