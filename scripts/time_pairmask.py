#!/usr/bin/env python3
"""Device time of the fused pair-mask kernel (uwm_pair_mask_u8) on a batch of equal-sized pairs, in ms per batch and in GB/s of its
floor traffic (7 bytes per pixel: 3 + 3 read, 1 written; the halo rows and columns a tile re-reads are not counted), beside the
unfused route on the same pairs: the thresholded plane (uwm_pair_mask_u8 with open = 0) followed by uwm_op_morph erode + dilate with
the 3 x 3 ellipse, which works on a uniform-size batch [N][H][W] and writes the plane twice more.  HIP events around `calls` launches,
after warm-ups, the two routes alternating; the figure of a route is the median over `reps` such windows.

  python scripts/time_pairmask.py [--n 64] [--size 720 1280] [--threshold 15] [--reps 7] [--calls 20]"""
import argparse, ctypes as C, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls                 # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64); ap.add_argument("--size", type=int, nargs=2, default=(720, 1280))
    ap.add_argument("--threshold", type=int, default=15); ap.add_argument("--reps", type=int, default=7); ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    import pairmask_ref as P
    from unet_watermark_amd import _lib as L
    from unet_watermark_amd.data import DESC_DTYPE, descs_tensor, mask_descs_for
    assert torch.cuda.is_available(), "time_pairmask.py measures on a HIP device"
    dev = torch.device("cuda:0")
    (h, w), n, thr = a.size, a.n, a.threshold
    # pairs with structure: a smooth clean image, a blended rectangle and sparse specks (the opening has something to remove); every
    # image differs, generated on the device
    g = torch.Generator(device=dev).manual_seed(0)
    base = torch.rand(n, 3, h // 16 + 1, w // 16 + 1, device=dev, generator=g)
    clean = (torch.nn.functional.interpolate(base, size=(h, w), mode="bilinear", align_corners=False) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    wm = clean.clone()
    wm[:, h // 4: h // 4 + h // 3, w // 5: w // 5 + w // 2] = (wm[:, h // 4: h // 4 + h // 3, w // 5: w // 5 + w // 2].to(torch.int32) * 5 // 10 + 120).to(torch.uint8)
    specks = torch.rand(n, h, w, device=dev, generator=g) < 0.01
    wm[specks] = 255 - wm[specks]
    descs = np.zeros(n, DESC_DTYPE)
    descs["offset"], descs["h"], descs["w"] = np.arange(n, dtype=np.int64) * h * w * 3, h, w
    md = mask_descs_for(descs)
    wm_f, cl_f = wm.view(-1), clean.view(-1)
    dd, dm = descs_tensor(descs, dev), descs_tensor(md, dev)
    lib, st = L.lib(), C.c_void_p(L.stream_ptr(dev))
    ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    fused_out = torch.empty(n * h * w, dtype=torch.uint8, device=dev)
    plane, unfused_out = torch.empty(n * h * w, dtype=torch.uint8, device=dev), torch.empty(n * h * w, dtype=torch.uint8, device=dev)
    ws = torch.empty(int(lib.uwm_mask_workspace_bytes(n, h, w)), dtype=torch.uint8, device=dev)

    def pair(open_, out):
        L.check(lib.uwm_pair_mask_u8(ptr(wm_f), wm_f.numel(), ptr(dd), ptr(cl_f), cl_f.numel(), ptr(dd), n, 3, thr, open_, ptr(out), out.numel(), ptr(dm), st))

    def fused():
        pair(1, fused_out)

    def unfused():
        pair(0, plane)
        L.check(lib.uwm_op_morph(ptr(plane), ptr(unfused_out), n, h, w, 0, 2, 3, 3, 1, ptr(ws), ws.numel(), st))
        L.check(lib.uwm_op_morph(ptr(unfused_out), ptr(unfused_out), n, h, w, 1, 2, 3, 3, 1, ptr(ws), ws.numel(), st))

    for _ in range(3):
        fused(); unfused()
    torch.cuda.synchronize()
    same = torch.equal(fused_out, unfused_out)
    k = 0
    ref = P.pair_mask(wm[k].cpu().numpy(), clean[k].cpu().numpy(), thr)
    exact = np.array_equal(fused_out[k * h * w:(k + 1) * h * w].view(h, w).cpu().numpy(), ref)
    t = {"fused": [], "unfused": []}
    for _ in range(a.reps):
        t["fused"].append(window(fused, a.calls)); t["unfused"].append(window(unfused, a.calls))
    floor_b = 7 * n * h * w
    print(f"pair masks, {n} pairs of {h}x{w}x3, threshold {thr}: {float((fused_out > 0).float().mean()) * 100:.1f} % foreground | fused equals the "
          f"unfused route: {same} | image 0 equals the numpy restatement: {exact}")
    for name, label in (("fused", "uwm_pair_mask_u8 (one kernel)"), ("unfused", "threshold plane -> uwm_op_morph erode -> dilate")):
        v = sorted(t[name]); med = v[len(v) // 2]
        print(f"{label:52s} {med:7.3f} ms/batch median of {a.reps} x {a.calls} calls (min {v[0]:.3f}, max {v[-1]:.3f}) = "
              f"{floor_b / med / 1e6:7.1f} GB/s against the {floor_b / 1e6:.1f} MB floor of 7 B/pixel")


if __name__ == "__main__":
    main()
