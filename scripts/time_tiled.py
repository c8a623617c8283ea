#!/usr/bin/env python3
"""Device time of prediction at native resolution (WatermarkPredictor.predict_images_tiled -> uwm_predict_tiled_u8, csrc/tile_u8.hip):

  16 seeded images of 2160 x 3840, Unet-resnet34 (fp16x3, frozen), tile 512, overlap 64, forward batch 48
  -> 5 x 9 = 45 tiles per image, 720 tiles, 15 forward chunks

Reported, all in the same run with HIP events, 2 warm-ups of every item and then 7 windows in which the items alternate (a figure is
the median of its 7 windows, with the least and the greatest beside it):

  the call         one replay of the captured uwm_predict_tiled_u8 (gather, forward, store copy per chunk; one blend)
  its forwards     the plain batch forward at the same N (WatermarkPredictor.logits, captured), replayed once per chunk
  the gathers      uwm_op_tile_norm_u8_nhwc4 launched once per chunk as the call launches it
  the blend        uwm_tile_blend_threshold_ragged on the call's tile-logit store
  (the per-chunk copy of the logit planes into the store has no entry of its own and is timed only inside the call; its bytes are listed)

beside the bytes gather and blend must move and the time those bytes take at the measured copy rate of the device (6.29 TB/s, float4
copy: DESIGN.md).  The number to judge is the call over its own forwards.  The masks of the first --check images are compared
with the numpy restatement (tests/tiled_ref.py) applied to the device's own tile logits.

  python scripts/time_tiled.py [--out profiles/tiled_mi355x.txt] [--images 16] [--size 2160 3840] [--batch 48] [--windows 7] [--check 1]"""
import argparse, ctypes as C, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "tiled_mi355x.txt"))
    ap.add_argument("--images", type=int, default=16); ap.add_argument("--size", type=int, nargs=2, default=(2160, 3840))
    ap.add_argument("--tile", type=int, default=512); ap.add_argument("--overlap", type=int, default=64)
    ap.add_argument("--batch", type=int, default=48); ap.add_argument("--encoder", default="resnet34")
    ap.add_argument("--windows", type=int, default=7); ap.add_argument("--check", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_tiled needs a HIP device (a timing without one says nothing)")
    import tiled_ref as R
    from unet_watermark_amd import _lib as L, tiling
    from unet_watermark_amd.config import get_cfg_defaults
    from unet_watermark_amd.predict import WatermarkPredictor, IMAGENET_MEAN, IMAGENET_STD
    dev = torch.device("cuda:0")
    h, w = a.size
    T, N = a.tile, a.batch
    cfg = get_cfg_defaults(); cfg.MODEL.NAME = "Unet"; cfg.MODEL.ENCODER_NAME = a.encoder; cfg.DATA.IMG_SIZE = T; cfg.PREDICT.BATCH_SIZE = N
    torch.manual_seed(42)
    pred = WatermarkPredictor(config=cfg, device="cuda", precision="f16x3", freeze=True)
    rng = np.random.default_rng(7)
    imgs = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for _ in range(a.images)]
    tiles, plans = tiling.plan_batch([(h, w)] * a.images, T, T, a.overlap, N)
    K, chunks = len(tiles), len(tiles) // N
    real = int((tiles["image"] >= 0).sum())
    say(f"scripts/time_tiled.py : {torch.cuda.get_device_name(0)}, {a.windows} windows after 2 warm-ups of every item, items alternating")
    say(f"{a.images} images of {h} x {w}, Unet-{a.encoder} (fp16x3, frozen), tile {T}, overlap {a.overlap}, forward batch {N}: "
        f"{plans[0]['ny']} x {plans[0]['nx']} tiles per image, {real} tiles in {K} entries, {chunks} chunks")
    # the call: captured by the predictor; its replay is what is timed
    masks = pred.predict_images_tiled(imgs, a.overlap)
    entry = [e for e in pred._graphs.values() if e.group == "tiled" and e.key[:3] == (a.images, chunks, N)]
    assert len(entry) == 1
    graph = entry[0].graph
    store = pred.model._tile_store                      # the store of the call (a view of the graph's workspace)
    # its forwards alone: the plain batch forward at the same N
    x = torch.randn(N, 3, T, T, device=dev)
    pred.logits(x)
    fgraph = pred._graphs["logits"].graph
    # gather and blend alone, on the call's own buffers
    lib = L.lib()
    st = C.c_void_p(L.stream_ptr(dev))
    mc, sc = (C.c_float * 3)(*IMAGENET_MEAN[:3]), (C.c_float * 3)(*IMAGENET_STD[:3])
    x4 = torch.empty((N, T, T, 4), device=dev)
    P = lambda t: C.c_void_p(t.data_ptr())
    src_bytes, mask_bytes = pred._ibuf.numel(), pred._mbuf.numel()

    def gathers():
        for c in range(chunks):
            L.check(lib.uwm_op_tile_norm_u8_nhwc4(P(pred._ibuf), src_bytes, P(pred._idesc), a.images, C.c_void_p(pred._xtiles.data_ptr() + 16 * c * N),
                                                  N, 3, T, T, mc, sc, P(x4), st))
    mask2 = torch.empty_like(pred._mbuf)

    def blend():
        L.check(lib.uwm_tile_blend_threshold_ragged(P(store), K, P(pred._xplans), a.images, T, T, a.overlap, P(pred._idesc), src_bytes, 3,
                                                    P(pred._mdesc), float(pred.threshold), 0, P(mask2), mask_bytes, None, st))

    def forwards():
        for _ in range(chunks):
            fgraph.replay()
    items = {"call": graph.replay, "forwards": forwards, "gathers": gathers, "blend": blend}
    ms = {k: [] for k in items}
    for _ in range(2):
        for fn in items.values():
            event_ms(fn)
    for _ in range(a.windows):
        for k, fn in items.items():
            ms[k].append(event_ms(fn))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    # the blend alone wrote what the call wrote
    graph.replay(); blend(); torch.cuda.synchronize()
    same_blend = bool(torch.equal(mask2[:a.images * h * w], pred._mbuf[:a.images * h * w]))
    # the first --check masks against the restatement on the device's own tile logits
    same_ref = True
    per = int(plans[0]["ny"]) * int(plans[0]["nx"])
    for i in range(min(a.check, a.images)):
        v = R.blend(store[i * per: (i + 1) * per].cpu().numpy(), h, w, T, T, a.overlap)
        same_ref = same_ref and bool(np.array_equal(masks[i].cpu().numpy(), R.predict_mask(v, pred.threshold, False)))
    pix_t, pix_o = K * T * T, a.images * h * w
    cover = real * T * T / pix_o                        # tile pixels per image pixel (the blend reads about this many logits per pixel)
    g_bytes = real * T * T * 3 + pix_t * 16             # image bytes of the real tiles in, the forward's NHWC4 input out
    c_bytes = pix_t * 16 + pix_t * 4                    # the forward's padded logits in (whole lines), the store out
    b_bytes = real * T * T * 4 + pix_o                  # every tile logit once in, one mask byte out
    say(f"the call, one replay                         {fmt(ms['call'])}   = {1e3 * a.images / med['call']:.2f} images/s, {1e3 * real / med['call']:.0f} tiles/s")
    say(f"its forwards alone, {chunks} x bs{N}                {fmt(ms['forwards'])}   = {1e3 * chunks * N / med['forwards']:.0f} tiles/s")
    say(f"    the call over its own forwards: {med['call'] / med['forwards']:.4f}  (tiling adds {med['call'] - med['forwards']:.3f} ms, "
        f"{100 * (med['call'] - med['forwards']) / med['call']:.2f} % of the call)")
    say(f"the gathers alone, {chunks} launches              {fmt(ms['gathers'])}   {g_bytes / 1e6:.0f} MB; at 6.29 TB/s {1e3 * g_bytes / COPY_RATE:.3f} ms; "
        f"{med['gathers'] / (1e3 * g_bytes / COPY_RATE):.1f} x that ({g_bytes / med['gathers'] / 1e6:.0f} GB/s)")
    say(f"the blend alone, 1 launch                    {fmt(ms['blend'])}   {b_bytes / 1e6:.0f} MB; at 6.29 TB/s {1e3 * b_bytes / COPY_RATE:.3f} ms; "
        f"{med['blend'] / (1e3 * b_bytes / COPY_RATE):.1f} x that ({b_bytes / med['blend'] / 1e6:.0f} GB/s); {cover:.2f} tile pixels per image pixel")
    say(f"    gather + blend: {med['gathers'] + med['blend']:.3f} ms = {100 * (med['gathers'] + med['blend']) / med['call']:.2f} % of the call")
    say(f"the store copies, {chunks} launches (inside the call only): {c_bytes / 1e6:.0f} MB; at 6.29 TB/s {1e3 * c_bytes / COPY_RATE:.3f} ms (not timed alone)")
    say(f"the blend alone writes the call's masks: {same_blend}; the first {min(a.check, a.images)} mask(s) equal the restatement on the device's tile logits: {same_ref}; "
        f"foreground {100 * float((pred._mbuf[:a.images * h * w] > 0).float().mean()):.1f} %")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
