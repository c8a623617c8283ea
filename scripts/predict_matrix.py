#!/usr/bin/env python3
"""bench_predict.py over batch sizes x variants, alternating, repeated: the table of DESIGN.md 8a.

  python scripts/predict_matrix.py --out profiles/frozen_predict_matrix.jsonl [--parent DIR] [--reps 3]

Variants: default flags, --freeze, --freeze --u8, --u8 of THIS tree, and (with --parent: a checkout of the commit to compare
against, its libuwm.so built) that tree's default flags.  One process per measurement, each under its own time limit; the first
failure ends the run.  One JSON line per measurement goes to --out; the summary (mean and min-max of ms per batch) to stdout."""
import argparse, collections, json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = {1: 1500, 8: 500, 64: 90}          # timed batches per batch size: a window of a second or more


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True); ap.add_argument("--parent", default=None); ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precisions", default="f16x3,f32")
    a = ap.parse_args()
    variants = [("this tree", ROOT, []), ("--freeze", ROOT, ["--freeze"]), ("--freeze --u8", ROOT, ["--freeze", "--u8"]), ("--u8", ROOT, ["--u8"])]
    if a.parent:
        variants.insert(0, ("parent", os.path.abspath(a.parent), []))
    rows = []
    with open(a.out, "w") as f:
        for rep in range(a.reps):
            for prec in a.precisions.split(","):
                for bs, k in BATCHES.items():
                    for name, cwd, flags in variants:
                        cmd = ["timeout", "-k", "10", "120", sys.executable, "bench_predict.py", "--batch", str(bs), "--batches", str(k), "--precision", prec] + flags
                        r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
                        if r.returncode != 0:
                            sys.exit(f"FAILED {name} {prec} bs{bs}: rc {r.returncode}\n{r.stderr[-2000:]}")
                        d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
                        rec = {"rep": rep, "variant": name, "precision": prec, "batch": bs, "ms_per_batch": d["ms_per_batch"], "images_per_s": d["value"],
                               "bitwise_equal_to_batch1_path": d["bitwise_equal_to_batch1_path"], "frozen": d.get("frozen"),
                               "prep_launches_per_batch": d.get("prep_launches_per_batch")}
                        rows.append(rec)
                        f.write(json.dumps(rec) + "\n"); f.flush()
                        print(json.dumps(rec), flush=True)
    g = collections.defaultdict(list)
    for r in rows:
        g[(r["precision"], r["variant"], r["batch"])].append(r["ms_per_batch"])
    print("\nms per batch: mean (min - max) over %d runs; all bitwise_equal_to_batch1_path: %s" % (a.reps, all(r["bitwise_equal_to_batch1_path"] for r in rows)))
    for prec in a.precisions.split(","):
        print(f"\n| {prec} | " + " | ".join(f"bs{b}" for b in BATCHES) + " |\n|---|" + "---|" * len(BATCHES))
        for name, _, _ in variants:
            print(f"| {name} | " + " | ".join(f"{statistics.mean(g[(prec, name, b)]):.3f} ({min(g[(prec, name, b)]):.3f} - {max(g[(prec, name, b)]):.3f})" for b in BATCHES) + " |")


if __name__ == "__main__":
    main()
