#!/usr/bin/env python3
"""Routing equality of two builds of libuwm.so: every configuration below runs one training step (or one frozen eval forward) with the
routing record on, in a fresh process per library, and the two records ("<pass> <layer> <kernel>" per launch) must be the same line for
line.  The baseline library comes from scripts/build_baseline_lib.sh <rev>.
usage: scripts/routing_check.py --base unet-watermark_amd/abl/libuwm_base.so --out profiles/<name>.txt      (needs a GPU)
       scripts/routing_check.py --one '<json config>'      (what the driver starts per configuration: prints the record)"""
import argparse
import concurrent.futures as cf
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = ["f32", "bf16x3", "bf16x3_all", "f16x3", "f16x3_all", "f16x3_bwd2", "f16x1"]


def configs():
    r34 = dict(arch="Unet", enc="resnet34", size=512)
    out = [dict(r34, bs=16, prec=p) for p in PRECS]                                   # default fill rule
    out += [dict(r34, bs=2, prec=p, route=16) for p in PRECS]                         # a parity sample on the bs16 kernels
    out += [dict(r34, bs=2, prec=p, fill=1) for p in PRECS]                           # every eligible layer on fp16x3
    out += [dict(r34, bs=16, prec=p, wino=w) for w in (0, 2) for p in ("f32", "f16x3_all")]
    for p in ("f32", "f16x3_all"):
        out += [dict(arch="Unet", enc="resnet50", size=512, bs=8, prec=p), dict(arch="UnetPlusPlus", enc="resnet34", size=512, bs=8, prec=p),
                dict(arch="Unet", enc="efficientnet-b4", size=1024, bs=4, prec=p), dict(arch="UnetPlusPlus", enc="efficientnet-b3", size=512, bs=6, prec=p)]
    out += [dict(r34, bs=8, prec=p, frozen=1) for p in ("f32", "f16x3")]
    return out


def run_one(c):
    sys.path.insert(0, ROOT)
    import torch
    import unet_watermark_amd as U
    from unet_watermark_amd import _lib as L
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = getattr(U, c["arch"])(c["enc"]).to(dev)
    m.set_precision(c["prec"], min_workgroups=c.get("fill"), routing_batch=c.get("route"))
    if "wino" in c:
        L.check(L.lib().uwm_set_winograd_mode(m._h, c["wino"]))
    x = torch.randn(c["bs"], 3, c["size"], c["size"], device=dev)
    t = (torch.rand(c["bs"], 1, c["size"], c["size"], device=dev) > 0.5).float()
    if c.get("frozen"):
        m.eval(); m.freeze(); m.routing(enable=True)
        with torch.no_grad():
            m(x)
    else:
        m.train(); m.routing(enable=True)
        U.DiceLoss(mode="binary", smooth=1e-5)(m(x), t).backward()
    torch.cuda.synchronize()
    for rec in m.routing():
        print("ROUTE", *rec)


def record(c, lib):
    env = dict(os.environ)
    env.pop("UWM_LIB", None)
    if lib:
        env["UWM_LIB"] = os.path.abspath(lib)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", json.dumps(c)], env=env, cwd=ROOT, timeout=240,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0:
        raise RuntimeError(f"{c} lib={lib or 'working tree'}: exit {r.returncode}\n{r.stderr.decode(errors='replace')[-2000:]}")
    return [l for l in r.stdout.decode().splitlines() if l.startswith("ROUTE ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one"); ap.add_argument("--base"); ap.add_argument("--out"); ap.add_argument("--jobs", type=int, default=4)
    a = ap.parse_args()
    if a.one:
        return run_one(json.loads(a.one))
    lines, launches, differing = [], 0, 0
    with cf.ThreadPoolExecutor(a.jobs) as ex:       # (at most 2 x jobs processes hold the GPU; the first failure ends the run)
        futs = [(c, ex.submit(record, c, None), ex.submit(record, c, a.base)) for c in configs()]
        try:
            for c, fn, fb in futs:
                new, base = fn.result(), fb.result()
                diff = sum(1 for x, y in zip(new, base) if x != y) + abs(len(new) - len(base))
                launches += len(new); differing += diff
                lines.append(f"{json.dumps(c, sort_keys=True)}: launches compared {len(new)} (baseline {len(base)}), lines differing {diff}, "
                             f"kernels {len({l.split()[3].split('<')[0] for l in new})}")
        except Exception:
            for _, fn, fb in futs:
                fn.cancel(); fb.cancel()
            raise
    lines.append(f"TOTAL: {len(lines)} configurations, launches compared {launches}, lines differing {differing}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(os.path.join(ROOT, a.out), "w") as f:
            f.write(f"routing records of the working tree's libuwm.so against {a.base} (scripts/routing_check.py)\n" + text)
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
