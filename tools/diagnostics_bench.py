"""Flow diagnostics and running statistics at the bench size (Taylor-Green 128^3, P2-P1, Smagorinsky so that ``nut``
exists): HIP events, warm, medians, the variants alternating inside the timed loops.  The set-up is that of
tools/viscosity_bench.py.

    python tools/diagnostics_bench.py [-N 128] [--steps 12] [--warmup 4] [--reps 20] [--out FILE]
                                      [--bench-trees this=DIR parent=DIR] [--bench-runs 2]

Part 1, the kernels, launch after launch, alternating:
  * ``ox_flow_cells`` with and without ``fields`` beside ``ox_cell_viscosity`` (the same streams -- dof list, geometry
    record, u once per dof -- plus the quadrature loop; bytes from the stored sizes) and ``ox_flow_reduce``;
  * ``ox_stats_accumulate`` for ``u`` with the bytes it moves, ``(gdim + 2 (gdim + gdim (gdim + 1) / 2)) 8 B`` per dof, and
    for ``p``, beside ``ox_axpby`` (two reads, one write) on blocks of the same total bytes.
Part 2, whole steps, alternating: without and with both objects sampling after every step.
Part 3 (``--bench-trees``): ``bench.py --gpus 1 --steps 20 --warmup 5`` as child processes in the given source trees (this
commit, the parent commit), alternating: the default step makes none of the new calls."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.viscosity_bench import HBM_PEAK, bench_trees, build, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-N", type=int, default=128)
    ap.add_argument("--steps", type=int, default=12, help="timed steps per variant")
    ap.add_argument("--warmup", type=int, default=4, help="warm-up steps")
    ap.add_argument("--reps", type=int, default=20, help="timed launches per kernel variant")
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-trees", nargs="*", default=[], metavar="LABEL=DIR",
                    help="source trees to run bench.py's default line in, e.g. this=. parent=../parent")
    ap.add_argument("--bench-runs", type=int, default=2)
    a = ap.parse_args()
    import ctypes as C

    import torch

    import oasisx_amd as ox
    from oasisx_amd import _lib
    from oasisx_amd.viscosity import _cell_viscosity

    # part 3 first: the children have the device to themselves (this process has not touched it yet)
    bench = bench_trees(a.bench_trees, a.bench_runs) if a.bench_trees else None
    S, W, clk = build(a.N, ox.Smagorinsky())
    dt, nu = W["dt"], W["nu"]
    for _ in range(a.warmup):
        clk["t"] += dt
        S.solve(dt, nu, max_iter=1)
    torch.cuda.synchronize()
    lib, st = _lib.load(), _lib.current_stream()
    Vi = S._Vi[0][0]
    d = S._gdim
    ncells, nd, gs = int(S._geom.shape[0]), int(Vi.cell_dofs.shape[1]), int(S._geom.shape[1])
    n_u, n_q = int(S._n_u), int(S._n_q)
    Dall = ox.FlowDiagnostics(S, fields=("q_criterion",), cell_integrals=False)
    Dsum = ox.FlowDiagnostics(S)
    T = ox.FlowStatistics(S)
    T.sample(dt)  # (the timed launches take the general branch, not the first-sample copy)
    nut_scratch = torch.zeros_like(S._nut)

    def cells(D):
        _lib.check(lib.ox_flow_cells(Vi.degree, C.byref(S._cells), _lib.ptr(Vi.cell_dofs), S._U.rptr(), _lib.ptr(S._nut), dt, nu,
                                     _lib.ptr(D._fields), None, _lib.ptr(D._partials), st), "ox_flow_cells")

    def eddy():
        _cell_viscosity(S, nut_scratch, model=0, coefficient=0.1677)

    def reduce_():
        _lib.check(lib.ox_flow_reduce(Dsum.n_blocks, _lib.ptr(Dsum._partials), _lib.ptr(Dsum._ring), Dsum.capacity, 0, st),
                   "ox_flow_reduce")

    def stats(name):
        m = T._m[name]
        src = m.storage.rdev()
        _lib.check(lib.ox_stats_accumulate(m.ncomp, m.n, _lib.ptr(src), int(src.shape[1]), dt, 1.0, m.mean._storage.ptr(),
                                           _lib.ptr(m.cov), st), "ox_stats_accumulate")

    ncov = d * (d + 1) // 2
    stats_u_bytes = n_u * (d + 2 * (d + ncov)) * 8
    n_ax = stats_u_bytes // 24
    ax = [torch.zeros(n_ax, dtype=torch.float64, device="cuda") for _ in range(3)]

    def axpby():
        _lib.check(lib.ox_axpby(n_ax, 0.5, _lib.ptr(ax[0]), 0.25, _lib.ptr(ax[1]), _lib.ptr(ax[2]), st), "ox_axpby")

    variants = {"flow_cells_with_fields": lambda: cells(Dall), "flow_cells_sums_only": lambda: cells(Dsum),
                "eddy_viscosity": eddy, "flow_reduce": reduce_, "stats_u": lambda: stats("u"), "stats_p": lambda: stats("p"),
                "axpby_same_bytes": axpby}
    ev = {k: [] for k in variants}
    for _ in range(a.reps + 3):
        for k, fn in variants.items():
            ev[k].append(timed(torch, fn))
    torch.cuda.synchronize()
    cell_stream = ncells * (nd * 4 + gs * 8) + n_u * d * 8
    nbytes = {"flow_cells_with_fields": cell_stream + ncells * (8 + Dall._nf * 8) + Dall.n_blocks * 64,
              "flow_cells_sums_only": cell_stream + ncells * 8 + Dall.n_blocks * 64, "eddy_viscosity": cell_stream + ncells * 8,
              "flow_reduce": Dsum.n_blocks * 64, "stats_u": stats_u_bytes, "stats_p": n_q * 5 * 8, "axpby_same_bytes": n_ax * 24}
    kern = {}
    for k, pairs in ev.items():
        ms = statistics.median(x.elapsed_time(y) for x, y in pairs[3:])
        kern[k] = {"ms": round(ms, 4), "bytes": nbytes[k], "bytes_per_s": round(nbytes[k] / (ms * 1e-3), 1),
                   "fraction_of_hbm_peak": round(nbytes[k] / (ms * 1e-3) / HBM_PEAK, 3)}
    kern["stats_u"]["bytes_per_s_over_axpby"] = round(kern["stats_u"]["bytes_per_s"] / kern["axpby_same_bytes"]["bytes_per_s"], 3)

    # ---- part 2: whole steps, alternating ---------------------------------------------------------------------------------
    D = ox.FlowDiagnostics(S, fields=("q_criterion",))
    T.reset()
    rec = {"plain": [], "sampling": []}
    for i in range(a.steps + 1):
        for key in rec:
            clk["t"] += dt

            def step():
                S.solve(dt, nu, max_iter=1)
                if key == "sampling":
                    D.sample(clk["t"], dt, nu)
                    T.sample(dt)

            e = timed(torch, step)
            torch.cuda.synchronize()
            if i:
                rec[key].append(e[0].elapsed_time(e[1]))
    steps = {k: {"ms_per_step": round(statistics.median(v), 3)} for k, v in rec.items()}
    h = D.history()
    out = {"N": a.N, "cells": ncells, "rows_u": n_u, "rows_p": n_q, "partial_rows": Dsum.n_blocks, "nu": nu, "dt": dt,
           "kernel": kern, "steps": steps,
           "last_sample": {k: float(v[-1]) for k, v in h.items()}}
    if bench is not None:
        out["bench_default_steps_per_s"] = bench
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
