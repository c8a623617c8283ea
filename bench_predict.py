#!/usr/bin/env python3
"""BASELINE config 5: batch inference, 4096 synthetic 512x512 images in 64 batches of 64 on one GPU, eval-mode
forward (BatchNorm from running statistics) captured once in a hipGraph and replayed; masks by the
reference's raw-logit threshold.  Prints one JSON line.  (The driver's headline bench is bench.py.)"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64); ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--size", type=int, default=512); ap.add_argument("--encoder", default="resnet34")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--precision", default="f16x3", choices=["f32", "f16x3"],
                    help="f16x3 (default): fp16x3 split products on the 3x3 convolutions, fp32-class accuracy; f32: exact-fp32 matrix instruction")
    ap.add_argument("--freeze", action="store_true", help="freeze the weights (WatermarkPredictor(freeze=True)): BatchNorm scale / shift and filter banks made once")
    ap.add_argument("--u8", action="store_true", help="time uint8 images -> masks through uwm_predict_u8 (predict_mask_u8) instead of fp32 NCHW input -> masks")
    ap.add_argument("--mask-type", choices=["watermark", "text", "mixed"], default=None,
                    help="with --u8: post-process the masks on the device (predict_mask_u8(mask_type=...)); adds mask_type / out_size to the line")
    ap.add_argument("--out-size", type=int, nargs=2, metavar=("H", "W"), default=None, help="with --u8: resize the masks to H x W (default: the input size)")
    a = ap.parse_args()
    if (a.mask_type or a.out_size) and not a.u8:
        ap.error("--mask-type / --out-size need --u8")
    from unet_watermark_amd.predict import WatermarkPredictor, IMAGENET_MEAN, IMAGENET_STD
    from unet_watermark_amd.config import get_cfg_defaults
    cfg = get_cfg_defaults(); cfg.MODEL.NAME = "Unet"; cfg.MODEL.ENCODER_NAME = a.encoder      # BASELINE configs[4] names Unet
    torch.manual_seed(42)
    pred = WatermarkPredictor(config=cfg, device="cuda", precision=a.precision, **({"freeze": True} if a.freeze else {}))
    if a.u8:
        xu = torch.randint(0, 256, (a.batch, a.size, a.size, 3), dtype=torch.uint8, device="cuda")
        x = pred.preprocess(xu)
        post = {k: v for k, v in (("mask_type", a.mask_type), ("out_size", tuple(a.out_size) if a.out_size else None)) if v}
        step = lambda: pred.predict_mask_u8(xu, use_graph=not a.no_graph, **post)
    else:
        x = torch.randn(a.batch, 3, a.size, a.size, device="cuda")
        step = lambda: pred.predict_mask(x, use_graph=not a.no_graph)
    for _ in range(2):
        m = step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.batches):
        m = step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    fwd, _ = pred.model.conv_flops(a.size, a.size)
    n = a.batch * a.batches
    # per-image equality of the batched, graph-replayed path with the batch-1 eager path
    # (--u8: the logits uwm_predict_u8 itself computes from the bytes, against the batch-1 preprocess -> forward path)
    lb = pred.model.predict_u8(xu, IMAGENET_MEAN, IMAGENET_STD, pred.threshold, return_logits=True)[1].clone() if a.u8 else pred.logits(x, use_graph=not a.no_graph).clone()
    eq = True
    for i in (0, a.batch // 2, a.batch - 1):
        eq = eq and bool(torch.equal(pred.logits(x[i:i + 1], use_graph=False)[0], lb[i]))
    extra = {}
    if a.freeze or a.u8:
        # weight-preparation launches one forward of this batch enqueues (a replayed graph holds the same kernels): 0 when frozen
        p0 = pred.model.prep_launches()
        pred.logits(x, use_graph=False)
        extra = {"frozen": bool(pred.model.frozen), "prep_launches_per_batch": pred.model.prep_launches() - p0, "input": "u8" if a.u8 else "f32"}
    if a.mask_type:
        extra["mask_type"] = a.mask_type
    if a.out_size:
        extra["out_size"] = list(a.out_size)
    print(json.dumps({"metric": "predict_images_per_sec", "value": round(n / dt, 2), "unit": "images/s", "n_gpus": 1,
                      "images": n, "batch": a.batch, "ms_per_batch": round(1e3 * dt / a.batches, 3),
                      "dtype": "f32" if a.precision == "f32" else "f32 storage / accumulation, 3x3 conv products as fp16x3 splits (22-bit operands) on v_mfma_f32_16x16x32_f16",
                      "precision_mode": a.precision,
                      "data": "synthetic", "hipgraph": not a.no_graph,
                      "config": {"workload": f"Unet-{a.encoder} {a.size}x{a.size} eval forward + logit threshold, bs{a.batch} (BASELINE configs[4])"},
                      "model_tflops": round(n * fwd / dt / 1e12, 2), "mask_positive_frac": round(float((m > 0).float().mean()), 4),
                      "bitwise_equal_to_batch1_path": eq, **extra}))


if __name__ == "__main__":
    main()
