#!/usr/bin/env python3
"""bench_predict.py --freeze --u8 --out-size H W with and without each --mask-type, alternating, repeated: the table of DESIGN.md 8b.

  python scripts/maskpost_matrix.py --out profiles/maskpost_predict_matrix.jsonl [--reps 3] [--out-size 768 1024]

One process per measurement, each under its own time limit; the first failure ends the run.  One JSON line per measurement goes
to --out; the summary (mean and min-max of ms per batch, the post-processing as added ms and as a share of the forward) to stdout."""
import argparse, collections, json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = {8: 500, 64: 90}          # timed batches per batch size: a window of a second or more
VARIANTS = (None, "watermark", "text", "mixed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True); ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out-size", type=int, nargs=2, default=(768, 1024))
    a = ap.parse_args()
    rows = []
    with open(a.out, "w") as f:
        for rep in range(a.reps):
            for bs, k in BATCHES.items():
                for t in VARIANTS:
                    cmd = ["timeout", "-k", "10", "120", sys.executable, "bench_predict.py", "--freeze", "--u8", "--batch", str(bs), "--batches", str(k),
                           "--out-size", str(a.out_size[0]), str(a.out_size[1])] + (["--mask-type", t] if t else [])
                    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
                    if r.returncode != 0:
                        sys.exit(f"FAILED {t} bs{bs}: rc {r.returncode}\n{r.stderr[-2000:]}")
                    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
                    rec = {"rep": rep, "mask_type": t, "batch": bs, "out_size": list(a.out_size), "ms_per_batch": d["ms_per_batch"],
                           "images_per_s": d["value"], "mask_positive_frac": d["mask_positive_frac"]}
                    rows.append(rec)
                    f.write(json.dumps(rec) + "\n"); f.flush()
                    print(json.dumps(rec), flush=True)
    g = collections.defaultdict(list)
    for r in rows:
        g[(r["mask_type"], r["batch"])].append(r["ms_per_batch"])
    print(f"\nms per batch: mean (min - max) over {a.reps} runs; masks at {a.out_size[0]} x {a.out_size[1]}; [added ms, share of the run without post-processing]")
    print("| --mask-type | " + " | ".join(f"bs{b}" for b in BATCHES) + " |\n|---|" + "---|" * len(BATCHES))
    for t in VARIANTS:
        cells = []
        for b in BATCHES:
            v, base = g[(t, b)], statistics.mean(g[(None, b)])
            cell = f"{statistics.mean(v):.3f} ({min(v):.3f} - {max(v):.3f})"
            if t:
                cell += f" [+{statistics.mean(v) - base:.3f}, {100 * (statistics.mean(v) - base) / base:.1f} %]"
            cells.append(cell)
        print(f"| {t or 'absent'} | " + " | ".join(cells) + " |")


if __name__ == "__main__":
    main()
