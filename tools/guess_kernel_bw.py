"""Achieved bandwidth of the three-column guess kernels (csrc/ox_guess.hip) from a rocprofv3 kernel trace of

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/guess_bench.py --only tg --legs u110 ...

    python tools/guess_kernel_bw.py DIR [--rows 16974593] [--size 10] [--out profiles/r09_guess_kernel_bw.csv]

Bytes are counted from the shapes (n_rows x 3 doubles per vector; the run's velocity update is warm-started with the
caller's A x_w, model 1): dots of a guess (k slots, b, A x_w) k + 2 vectors, of an update (k + 1 slots, A d) k + 2;
combine 2k + 5 (2k + 4 with a full basis: no copy of x0); orth 2k + 4; sub 3 (2 for d = x).  The velocity update's k runs
0, 1, ..., size - 1, size, 1, ... from the first step on (a restart at k = size), which assigns k to every dispatch in
trace order.  Prints and writes one row per (kernel, k): bytes, mean duration and the fraction of 8 TB/s."""
from __future__ import annotations

import argparse
import collections
import csv
import glob
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--rows", type=int, default=16974593)
    ap.add_argument("--size", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    trace = glob.glob(f"{a.dir}/**/*_kernel_trace.csv", recursive=True)
    if not trace:
        sys.exit(f"no kernel trace under {a.dir}")
    rows = []
    for r in csv.DictReader(open(trace[0])):
        name = r["Kernel_Name"].split("(")[0].replace("void ", "")
        if name.startswith("k_guess_") and name.endswith("<3>"):
            rows.append((int(r["Start_Timestamp"]), name, int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    vec = a.rows * 3 * 8
    acc = collections.defaultdict(list)
    k, i = 0, 0
    while i < len(rows):
        # one velocity update: the guess (k > 0), then the basis update
        if k > 0:
            assert rows[i][1] == "k_guess_dots<3>" and rows[i + 1][1] == "k_guess_combine<3>", rows[i:i + 2]
            acc[("k_guess_dots<3> (guess)", k)].append((rows[i][2], (k + 2) * vec))
            acc[("k_guess_combine<3>", k)].append((rows[i + 1][2], (2 * k + (5 if k < a.size else 4)) * vec))
            i += 2
        kk = 0 if k == a.size else k
        assert rows[i][1] == "k_guess_sub<3>" and rows[i + 1][1] == "k_guess_dots<3>", rows[i:i + 2]
        acc[("k_guess_sub<3>", kk)].append((rows[i][2], (3 if kk > 0 else 2) * vec))
        acc[("k_guess_dots<3> (update)", kk)].append((rows[i + 1][2], (kk + 2) * vec))
        i += 2
        if kk > 0:
            assert rows[i][1] == "k_guess_orth<3>", rows[i]
            acc[("k_guess_orth<3>", kk)].append((rows[i][2], (2 * kk + 4) * vec))
            i += 1
        k = kk + 1
    out = [["kernel", "k", "dispatches", "bytes_MB", "avg_us", "frac_8TBps"]]
    for (name, kk), v in sorted(acc.items()):
        ns = sum(t for t, _ in v) / len(v)
        b = v[0][1]
        out.append([name, kk, len(v), f"{b / 1e6:.1f}", f"{ns / 1e3:.1f}", f"{b / ns / 8e3:.3f}"])
    for r in out:
        print(",".join(str(c) for c in r))
    if a.out:
        with open(a.out, "w") as f:
            csv.writer(f).writerows(out)


if __name__ == "__main__":
    main()
