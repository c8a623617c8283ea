#!/usr/bin/env python3
"""Time of the dataset filter on a batch of equal-sized images, three figures:

  (a) WatermarkPredictor.watermark_counts: host images -> (N, 2) host counts through ONE captured call (uwm_filter_images_u8);
  (b) the unfused sequence that the library offered before it: predict_images(apply_sigmoid=True) -> every full-size mask in device
      memory -> postprocess.morphology erode, dilate, dilate, erode per image -> a count per image on the device -> one copy of the
      counts.  It interpolates the LOGITS (the other order of sigmoid and resize), so its masks are not the filter's: a timing
      yardstick only;
  (c) the fused kernel alone (uwm_prob_mask_count_ragged on the logits of (a)), with and without storing the masks.

(a) and (b) are host-clock times around work that ends in a device synchronise and include what both share: packing the images into
the pinned buffer, the upload and the forward (its time is printed too, so that the tail of each route can be read off).  (c) is HIP
events around `calls` launches.  Warm-ups first, the routes alternating, the figure of a route is the median over `reps` windows.

  python scripts/time_filter.py [--n 64] [--size 720 1280] [--img-size 256] [--encoder resnet34] [--reps 7] [--calls 20] [--out FILE]"""
import argparse, ctypes as C, math, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch


def host_window(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3           # ms per batch


def event_window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls                 # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64); ap.add_argument("--size", type=int, nargs=2, default=(720, 1280))
    ap.add_argument("--img-size", type=int, default=256); ap.add_argument("--encoder", type=str, default="resnet34")
    ap.add_argument("--reps", type=int, default=7); ap.add_argument("--calls", type=int, default=20); ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import unet_watermark_amd as U
    from unet_watermark_amd import _lib as L
    from unet_watermark_amd.config import get_cfg_defaults
    from unet_watermark_amd.data import descs_tensor, pack_images
    from unet_watermark_amd.postprocess import morphology
    from unet_watermark_amd.predict import IMAGENET_MEAN, IMAGENET_STD, WatermarkPredictor
    assert torch.cuda.is_available(), "time_filter.py measures on a HIP device"
    dev = torch.device("cuda:0")
    (h, w), n, s = a.size, a.n, a.img_size
    torch.manual_seed(0)
    model = U.Unet(a.encoder).to(dev)
    model.train()
    with torch.no_grad():                              # running statistics that fit the untrained weights, so that the logits are moderate
        for k in range(3):
            model(torch.randn(4, 3, s, s, device=dev) * (1.0 + 0.1 * k))
    model.eval()
    cfg = get_cfg_defaults(); cfg.MODEL.NAME = "Unet"; cfg.MODEL.ENCODER_NAME = a.encoder; cfg.DATA.IMG_SIZE = s
    pred = WatermarkPredictor(model=model, config=cfg, device=dev, precision="f32")
    # images with structure, every one different: smooth colour fields with a bright rectangle
    g = torch.Generator(device=dev).manual_seed(0)
    base = torch.rand(n, 3, h // 16 + 1, w // 16 + 1, device=dev, generator=g)
    imgs = (torch.nn.functional.interpolate(base, size=(h, w), mode="bilinear", align_corners=False) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    imgs[:, h // 4: h // 4 + h // 3, w // 5: w // 5 + w // 2] = 230
    images = list(imgs.cpu().numpy())

    def batch_logits(ims):
        packed, descs, mdescs = pack_images(ims)
        counts = torch.zeros((len(ims), 2), dtype=torch.int64, device=dev)
        _, lg = pred.model.filter_images_u8(packed.to(dev), descs_tensor(descs, dev), descs_tensor(mdescs, dev), counts, len(ims), (s, s),
                                            IMAGENET_MEAN, IMAGENET_STD, pred.threshold, True, None, return_logits=True)
        return lg.contiguous(), mdescs

    # a threshold at the median probability of the (untrained) model, so that the masks are neither empty nor full
    pred.threshold = 1.0 / (1.0 + math.exp(-min(8.0, max(-8.0, float(batch_logits(images[:4])[0].median())))))

    def fused():
        return pred.watermark_counts(images)

    def unfused():
        masks = pred.predict_images(images, apply_sigmoid=True)
        counts = []
        for m in masks:
            for op in ("erode", "dilate", "dilate", "erode"):
                m = morphology(m, op, "ellipse", 3)
            counts.append((m > 0).sum())
        return torch.stack(counts).cpu().numpy()

    def forward_only():
        return pred.predict_images(images, apply_sigmoid=True)

    for _ in range(2):
        cf = fused(); cu = unfused(); forward_only()
    t = {"fused": [], "unfused": [], "shared": []}
    for _ in range(a.reps):
        t["fused"].append(host_window(fused, dev)); t["unfused"].append(host_window(unfused, dev)); t["shared"].append(host_window(forward_only, dev))
    # (c) the kernel alone, on the logits of this batch
    lg, mdescs = batch_logits(images)
    lib, st = L.lib(), C.c_void_p(L.stream_ptr(dev))
    ptr = lambda t_: C.c_void_p(t_.data_ptr() if t_ is not None else 0)      # noqa: E731
    dm = descs_tensor(mdescs, dev)
    ws = torch.empty(int(lib.uwm_filter_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    mask = torch.empty(n * h * w, dtype=torch.uint8, device=dev)
    kc = torch.zeros((n, 2), dtype=torch.int64, device=dev)

    def kernel(m, post=1):
        L.check(lib.uwm_prob_mask_count_ragged(ptr(lg), 1, n, s, s, ptr(dm), float(pred.threshold), post, ptr(m), m.numel() if m is not None else 0,
                                               ptr(kc), ptr(ws), ws.numel(), st))

    for _ in range(3):
        kernel(None, 0); kernel(None); kernel(mask)
    torch.cuda.synchronize()
    same = kc.cpu().numpy().tolist() == cf.tolist()
    k = {"count only": [], "count + masks": [], "count only, no morphology": []}
    for _ in range(a.reps):
        k["count only"].append(event_window(lambda: kernel(None), a.calls)); k["count + masks"].append(event_window(lambda: kernel(mask), a.calls))
        k["count only, no morphology"].append(event_window(lambda: kernel(None, 0), a.calls))
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    lines = [f"dataset filter, {n} images of {h}x{w}x3, Unet/{a.encoder} at IMG_SIZE {s} (fp32, untrained weights), threshold {pred.threshold:.4f}: "
             f"{cf[:, 0].sum() / cf[:, 1].sum() * 100:.1f} % watermark pixels (fused rule), {cu.sum() / cf[:, 1].sum() * 100:.1f} % (unfused route, "
             f"the other sigmoid order) | the kernel alone gives watermark_counts' numbers: {same}"]
    for name, label in (("fused", "(a) watermark_counts (one captured call, 16 N bytes back)"),
                        ("unfused", "(b) predict_images(sigmoid) -> 4 x morphology per image -> count"),
                        ("shared", "    predict_images(sigmoid) alone (staging + forward + resize + threshold)")):
        v = sorted(t[name])
        lines.append(f"{label:76s} {med(v):8.2f} ms/batch, host clock to synchronise, median of {a.reps} (min {v[0]:.2f}, max {v[-1]:.2f}) = "
                     f"{n / med(v) * 1e3:7.0f} images/s")
    npx = n * h * w
    for name, v in k.items():
        v = sorted(v)
        lines.append(f"(c) uwm_prob_mask_count_ragged alone, {name:26s} {med(v):8.3f} ms/batch, HIP events, median of {a.reps} x {a.calls} calls "
                     f"(min {v[0]:.3f}, max {v[-1]:.3f}) = {npx / med(v) / 1e6:7.1f} Gpixel/s")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# python scripts/time_filter.py   (MI355X; {a.reps} windows, routes alternating, 2 warm-ups of every route)\n" + text + "\n")


if __name__ == "__main__":
    main()
