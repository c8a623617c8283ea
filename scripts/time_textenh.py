#!/usr/bin/env python3
"""Device time of the text-feature enhancement (uwm_text_enhance_ragged) on 64 images of 720 x 1280, alone and inside predict_images,
beside the numpy restatement (tests/textenh_ref.py) on 16 processes of the same box.

The images: the seeded photographs of scripts/time_maskpost_ragged.py with the marks that script times (tests/maskpost_ref.synth:
blobs, strokes, 1 % noise) stamped on, each mark pixel moved by 40 grey levels — soft gradients, text-like strokes and speckle.

  (a) the call alone, 11 launches
  (b) predict_images(mask_type='text'), whole calls with host packing and upload, host clock: without and with text_enhance
  (c) the two captured graphs of (b) replayed alone, HIP events: what the device spends on resize + forward + resize back + threshold
      + _optimize_mask, and on the same with the enhancement in front
  (d) the restatement, 16 worker processes, host clock

2 warm-ups, then 7 windows of 20 calls (a) / 5 calls (b, c) each; the figure is the median of the windows with the least and the
greatest beside it.  The library is called with buffers made once, so no allocation or fill is inside a window.  (d) runs first,
before the device is touched, so its workers never hold it.  --profile: 3 calls of (a) and nothing else, for a run under
`rocprofv3 --kernel-trace --stats`, which gives the share of each kernel.

  python scripts/time_textenh.py [--out profiles/textenh_mi355x.txt] [--images 64] [--windows 7] [--no-cpu] [--profile]"""
import argparse, ctypes as C, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def make_images(n, h, w):
    import maskpost_ref
    from time_maskpost_ragged import photographs
    out = []
    for i, c in enumerate(photographs(n, h, w, 9)):
        m = maskpost_ref.synth(h, w, 2000 + i)
        c[m] = np.where(c[m] < 128, c[m] + 40, c[m] - 40)
        out.append(c)
    return out


def cpu_one(img):
    """one image through the restatement -> the number of dilated-edge pixels"""
    import textenh_ref as T
    return int((T.text_enhance(img)[1] > 0).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "textenh_mi355x.txt"))
    ap.add_argument("--images", type=int, default=64); ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--no-cpu", action="store_true"); ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    n, h, w = a.images, 720, 1280
    images = make_images(n, h, w)
    cpu_s = cpu_edges = None
    if not a.no_cpu and not a.profile:
        import multiprocessing as mp
        with mp.get_context("spawn").Pool(16) as pool:
            pool.map(cpu_one, [im[:64, :64] for im in images[:16]])              # the workers' imports
            t0 = time.perf_counter()
            cpu_edges = pool.map(cpu_one, images, chunksize=1)
            cpu_s = time.perf_counter() - t0
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_textenh needs a HIP device (a timing without one says nothing)")
    import unet_watermark_amd as U
    from unet_watermark_amd import _lib as L
    from unet_watermark_amd.data import descs_tensor
    from unet_watermark_amd.textenh import text_enhance_ragged
    from time_maskpost_ragged import event_ms, fmt, host_ms, windows
    dev = torch.device("cuda:0")
    packed, descs, mdescs = U.pack_images(images)
    src = packed.to(dev)
    total = n * h * w
    edges = torch.zeros(total, dtype=torch.uint8, device=dev)
    out, status = text_enhance_ragged(src, descs, edges=edges, edge_descs=mdescs, return_status=True)
    assert int(status.abs().sum()) == 0
    dev_edges = [int(v) for v in (edges.view(n, h * w) > 0).sum(dim=1).tolist()]
    say(f"scripts/time_textenh.py : {torch.cuda.get_device_name(0)}, {n} images of {h} x {w}")
    say(f"dilated-edge pixels {100 * sum(dev_edges) / total:.2f} % of the pixels; bytes changed by the enhancement "
        f"{100 * float((out != src).float().mean()):.1f} %")
    lib = L.lib()
    dd = descs_tensor(np.concatenate([descs, mdescs]), dev)
    ws = torch.empty(lib.uwm_text_enhance_workspace_bytes(total, n), dtype=torch.uint8, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t, o=0: C.c_void_p(t.data_ptr() + o)

    def call():
        L.check(lib.uwm_text_enhance_ragged(p(src), p(out), src.numel(), p(dd), n, 3, h * w, total, p(edges), edges.numel(), p(dd, 16 * n),
                                            p(ws), ws.numel(), st))
    if a.profile:
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        return
    ref = (out.clone(), edges.clone())
    r = windows({"call": (call, 20)}, a.windows, event_ms)
    same = all(torch.equal(x, y) for x, y in zip(ref, (out, edges)))
    med = float(np.median(r["call"]))
    say(f"(a) uwm_text_enhance_ragged, 11 launches                 {fmt(r['call'])}")
    say(f"    = {1e3 * med / n:.1f} us per image; {total * 3 / 1e6:.0f} MB of pixels in and out: {total * 3 / 1e6 / med:.1f} GB/s of input; "
        f"workspace {ws.numel() / 2 ** 20:.0f} MiB")
    say(f"    results after {2 + 20 * a.windows} more calls equal the first call's bit for bit: {same}")

    from unet_watermark_amd.config import get_cfg_defaults
    from unet_watermark_amd.constants import IMAGENET_MEAN, IMAGENET_STD
    from unet_watermark_amd.predict import WatermarkPredictor
    torch.manual_seed(7)
    cfg = get_cfg_defaults(); cfg.MODEL.NAME = "Unet"; cfg.MODEL.ENCODER_NAME = "resnet18"
    pred = WatermarkPredictor(model=U.Unet("resnet18"), config=cfg, device=dev)
    s = int(cfg.DATA.IMG_SIZE)
    pk, ds, _ = U.pack_images(images[:8])
    _, lg = pred.model.predict_u8(U.device_resize(pk, ds, s, 3), IMAGENET_MEAN, IMAGENET_STD, 0.0, return_logits=True)
    pred.threshold = float(lg.median())
    res = {}

    def plain():
        res["plain"] = pred.predict_images(images, mask_type="text")

    def enhanced():
        res["enhanced"] = pred.predict_images(images, mask_type="text", text_enhance=True)
    r = windows({"plain": (plain, 5), "enhanced": (enhanced, 5)}, a.windows, host_ms)
    say(f"--- predict_images(mask_type='text') on the same images, Unet resnet18 at IMG_SIZE {s}, seeded weights, threshold = median logit")
    say(f"(b) whole call, text_enhance=False                       {fmt(r['plain'])}")
    say(f"(b) whole call, text_enhance=True                        {fmt(r['enhanced'])}")
    say(f"    the flag adds {np.median(r['enhanced']) - np.median(r['plain']):.3f} ms to a call of {np.median(r['plain']):.3f} ms "
        f"(host packing, upload, graph replay, clone of the masks)")
    g = windows({"plain": (pred._graphs["images_post"].graph.replay, 5), "enhanced": (pred._graphs["text_images_post"].graph.replay, 5)}, a.windows, event_ms)
    say(f"(c) graph replay alone, text_enhance=False               {fmt(g['plain'])}")
    say(f"(c) graph replay alone, text_enhance=True                {fmt(g['enhanced'])}")
    say(f"    the enhancement is {np.median(g['enhanced']) - np.median(g['plain']):.3f} ms beside {np.median(g['plain']):.3f} ms of resize, forward, "
        f"resize back, threshold and _optimize_mask")
    if cpu_s is not None:
        say(f"(d) numpy restatement (literal Canny loop), 16 processes {1e3 * cpu_s:10.1f} ms for the {n} images, host clock, one run; "
            f"its edge counts equal the device's: {cpu_edges == dev_edges}")
        say(f"    (d) / (a) = {1e3 * cpu_s / med:.0f}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
