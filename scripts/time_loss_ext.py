#!/usr/bin/env python3
"""uwm_loss_ext beside the parent's uwm_loss, on a HIP device (profiles/loss_ext_mi355x.txt):

 1. e0: the gradient error max|g - g_ref| / max|g_ref| of uwm_loss (0.5 Dice + 0.5 BCE) against the fp64 reference of
    tests/loss_ext_ref.py on the inputs of tests/test_loss_ext_gpu.py — the measurement that test's gradient bound (4 e0) rests on;
 2. the same ratio, and the worst loss-term error, of uwm_loss_ext for every parameter set and input of that test;
 3. device time of the launch pair (memset + sums + finalize + gradient) at 16 x 512 x 512 logits, ld = ldd = 4, uint8 targets:
    uwm_loss with Dice, uwm_loss_ext with Jaccard (focal compiled out), with Jaccard + Focal and with Focal alone; HIP events
    around `calls` calls after warm-ups, the variants alternating, `reps` windows each.

  python scripts/time_loss_ext.py [--reps 5] [--calls 200]"""
import argparse, ctypes as C, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5); ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    import loss_ext_ref as R
    import test_loss_ext_gpu as T
    from unet_watermark_amd.losses import make_loss_spec
    assert torch.cuda.is_available(), "time_loss_ext.py measures on a HIP device"
    dev = torch.device("cuda:0")
    D = T.Device(dev)
    L = D.L
    inputs = {}
    for k, (name, shape) in enumerate(T.SMALL.items()):
        x, xf, t = T.make_inputs(shape, seed=11 + k)
        inputs[f"{name} plain"] = (x, t); inputs[f"{name} forced"] = (xf, t)
    x, xf, t = T.make_inputs(T.BIG, seed=5)
    inputs["840x840 forced"] = (xf, t)

    print("== e0: uwm_loss (0.5 Dice + 0.5 BCE, smooth 1e-5) against the fp64 reference")
    e0max = 0.0
    for what, (lg, t) in inputs.items():
        rterms, rgrad = R.loss_and_grad(lg, t, T.DICE_BCE)
        terms, dl = D.parent(lg, t, 0.5, 0.5, 1e-5)
        e0 = float((dl[:, 0] - rgrad.reshape(-1)).abs().max()) / float(rgrad.abs().max())
        e0max = max(e0max, e0)
        print(f"uwm_loss {what}: e0 {e0:.4e}  loss err {abs(float(terms[0]) - rterms['total']):.3e}")
    print(f"E0 = {e0max:.4e}   4 * E0 = {4 * e0max:.4e}")

    print("== uwm_loss_ext: gradient error ratio and worst loss-term error per parameter set and input")
    worst = 0.0
    for name, spec in {**T.SPECS, "dice-bce": T.DICE_BCE}.items():
        for what, (lg, t) in inputs.items():
            if what.startswith("840") and name not in ("jaccard-smooth1e-5", "all-five", "dice-bce"):
                continue
            rterms, rgrad = R.loss_and_grad(lg, t, spec)
            for nhwc in (False, True):
                terms, dl = D.ext(lg, t, spec, nhwc=nhwc)
                ratio = float((dl[:, 0] - rgrad.reshape(-1)).abs().max()) / float(rgrad.abs().max())
                terr = max(abs(float(terms[k]) - (rterms[n] if (n != "focal" or spec["w_focal"]) else 0.0)) for k, n in enumerate(R.TERMS))
                worst = max(worst, ratio)
                print(f"uwm_loss_ext {name} {what} nhwc={int(nhwc)}: grad ratio {ratio:.4e} ({ratio / e0max:.2f} E0)  worst term err {terr:.3e}  "
                      f"finite {bool(torch.isfinite(dl).all())}")
    print(f"worst uwm_loss_ext ratio {worst:.4e} = {worst / e0max:.2f} E0")

    print(f"== time: 16 x 512 x 512 logits, ld = ldd = 4, uint8 targets, {a.reps} alternating windows of {a.calls} calls, us per call")
    n = 16 * 512 * 512
    g = torch.Generator().manual_seed(0)
    logits = (4.0 * torch.randn(n, 4, generator=g)).to(dev)
    target = (torch.rand(n, generator=g) < 0.2).to(torch.uint8).to(dev)
    dl = torch.empty(n, 4, device=dev)
    scratch = torch.zeros(8, dtype=torch.float64, device=dev)
    out = torch.zeros(8, device=dev)
    st = C.c_void_p(L.stream_ptr(dev))
    lp, tp, dp, sp, op = (C.c_void_p(v.data_ptr()) for v in (logits, target, dl, scratch, out))
    jac = make_loss_spec(w_jaccard=1.0, jaccard_smooth=1e-5)
    foc = make_loss_spec(w_jaccard=0.5, w_focal=0.5, jaccard_smooth=1e-5, focal_alpha=0.25, focal_gamma=2.5)
    foc2 = make_loss_spec(w_focal=1.0, focal_gamma=2.0)
    lib = L.lib()
    variants = {
        "uwm_loss Dice": lambda: lib.uwm_loss(lp, 4, tp, 2, n, 1.0, 0.0, 1e-5, 1e-7, sp, op, dp, 4, 1.0, st),
        "uwm_loss_ext Jaccard (focal off)": lambda: lib.uwm_loss_ext(lp, 4, tp, 2, n, C.byref(jac), sp, op, dp, 4, 1.0, st),
        "uwm_loss_ext Jaccard + Focal(0.25, 2.5)": lambda: lib.uwm_loss_ext(lp, 4, tp, 2, n, C.byref(foc), sp, op, dp, 4, 1.0, st),
        "uwm_loss_ext Focal(none, 2)": lambda: lib.uwm_loss_ext(lp, 4, tp, 2, n, C.byref(foc2), sp, op, dp, 4, 1.0, st),
    }
    for f in variants.values():
        for _ in range(20):
            assert f() == 0
    torch.cuda.synchronize()
    res = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                f()
            e1.record(); torch.cuda.synchronize()
            res[k].append(e0.elapsed_time(e1) * 1000.0 / a.calls)
    for k, v in res.items():
        print(f"{k}: " + " ".join(f"{x:.1f}" for x in v) + f"   median {sorted(v)[len(v) // 2]:.1f}  spread {max(v) - min(v):.1f}")
    print(f"bytes per pair: read 2 x ({n} x 4 B logits at a 16 B stride + {n} B targets), written {n} x 16 B")


if __name__ == "__main__":
    main()
