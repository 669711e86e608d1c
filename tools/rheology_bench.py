"""Generalised-Newtonian laws and the full stress form at the bench size (Taylor-Green 128^3, P2-P1, rtol 1e-8, warm
start): three solvers in one process (no model, Carreau-Yasuda, Smagorinsky), HIP events, medians, the variants
alternating inside the timed loops.  The set-up is that of tools/viscosity_bench.py.

    python tools/rheology_bench.py [-N 128] [--steps 12] [--warmup 4] [--reps 20] [--out FILE]
                                   [--bench-trees this=DIR parent=DIR] [--bench-runs 2]

Part 1, the kernels, launch after launch, alternating:
  * ``ox_cell_viscosity`` for the three laws beside its Smagorinsky model: the same streams, so the same
    bytes per launch from the stored sizes (dof list, geometry record, nut written, u_ab once per dof);
  * ``ox_assemble_stress_transpose`` beside one ``ox_assemble_grad_vector`` kind-0 launch (the same walk over the rows'
    cells) and one ``ox_assemble_matrix(STIFF)`` pass.  Bytes from the stored sizes: the adjacency table (cell and local
    index per slot), per cell the dof list, the geometry record and nut, u_ab once per dof, b read and written.
Part 2, whole steps, alternating: no model, Carreau-Yasuda, Smagorinsky with ``stress_form`` "laplacian" and "full" (one
solver, the option switched between steps), the ``stress_transpose_assemble`` phase split out.
Part 3 (``--bench-trees``): ``bench.py --gpus 1 --steps 20 --warmup 5`` as child processes in the given source trees
(this commit, the parent commit), alternating: the default step must not change."""
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
    ap.add_argument("--warmup", type=int, default=4, help="warm-up steps per solver")
    ap.add_argument("--reps", type=int, default=20, help="timed launches per kernel variant")
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-trees", nargs="*", default=[], metavar="LABEL=DIR",
                    help="source trees to run bench.py's default line in, e.g. this=. parent=../parent")
    ap.add_argument("--bench-runs", type=int, default=2)
    a = ap.parse_args()
    import ctypes as C

    import numpy as np
    import torch

    import oasisx_amd as ox
    from bench import make_workload
    from oasisx_amd import _lib
    from oasisx_amd.viscosity import _cell_viscosity
    from oasisx_amd.la import SellMatrix

    # part 3 first: the children have the device to themselves (this process has not touched it yet)
    bench = bench_trees(a.bench_trees, a.bench_runs) if a.bench_trees else None
    nu = make_workload("tg", a.N, np, torch)["nu"]
    cy = ox.CarreauYasuda(nu0=16.0 * nu, nu_inf=nu, lam=3.313, n=0.3568)  # (base_viscosity = the bench's nu)
    S0, W, clk0 = build(a.N, None)
    S1, _, clk1 = build(a.N, cy)
    S2, _, clk2 = build(a.N, ox.Smagorinsky())
    dt = W["dt"]
    for S, clk in ((S0, clk0), (S1, clk1), (S2, clk2)):
        for _ in range(a.warmup):
            clk["t"] += dt
            S.solve(dt, nu, max_iter=1)
    torch.cuda.synchronize()

    # ---- part 1: the kernels ------------------------------------------------------------------------------------------
    lib, st = _lib.load(), _lib.current_stream()
    Vi, Q = S2._Vi[0][0], S2._Q
    P = S2._A.pattern
    ncells, nd = int(S2._geom.shape[0]), int(Vi.cell_dofs.shape[1])
    gs = int(S2._geom.shape[1])

    def law_kernel(model):
        _cell_viscosity(S2, nut_scratch, model=model.model_id, params=model.params)

    def smagorinsky_kernel():
        _cell_viscosity(S2, nut_scratch, model=0, coefficient=0.1677)

    def transpose_kernel():
        _lib.check(lib.ox_assemble_stress_transpose(Vi.degree, C.byref(S2._cells), _lib.ptr(Vi.cell_dofs), C.byref(S2._adj_u),
                                                    Vi.n_owned, S2._UAB.rptr(), _lib.ptr(S2._nut), -1.0, _lib.ptr(b_scratch),
                                                    st), "ox_assemble_stress_transpose")

    def grad_kernel():
        _lib.check(lib.ox_assemble_grad_vector(0, Vi.degree, Q.degree, C.byref(S2._cells), _lib.ptr(Q.cell_dofs),
                                               C.byref(S2._adj_u), Vi.n_owned, S2._PS.ptr(), _lib.ptr(b_scratch), 1.0,
                                               _lib.ptr(b_scratch2), st), "ox_assemble_grad_vector")

    nut_scratch = torch.zeros_like(S2._nut)
    b_scratch = torch.zeros_like(S2._BFIRST.rdev())
    b_scratch2 = torch.zeros_like(b_scratch)
    k_scratch = SellMatrix(Vi.pattern, symmetric=True, name="K_bench")
    variants = {
        "nut_smagorinsky": smagorinsky_kernel,
        "nut_carreau_yasuda": lambda: law_kernel(cy),
        "nut_cross": lambda: law_kernel(ox.Cross(nu0=16.0 * nu, nu_inf=nu, lam=1.007, m=1.028)),
        "nut_power_law": lambda: law_kernel(ox.PowerLaw(k=5.0 * nu, n=0.6, nu_min=nu, nu_max=50.0 * nu)),
        "stress_transpose": transpose_kernel,
        "grad_vector_kind0": grad_kernel,
        "stiffness_pass": lambda: S2._assemble_matrix(1, Vi, k_scratch),
    }
    ev = {k: [] for k in variants}
    for r in range(a.reps + 3):
        for k, fn in variants.items():
            ev[k].append(timed(torch, fn))
    torch.cuda.synchronize()
    nut_bytes = ncells * (nd * 4 + gs * 8 + 8) + int(Vi.n_local) * 3 * 8
    adj = Vi.adj
    adj_bytes = sum(int(t.numel()) * int(t.element_size()) for t in (adj.adj_ptr, adj.adj_cell, adj.adj_loc))
    st_bytes = adj_bytes + ncells * (nd * 4 + gs * 8 + 8) + int(Vi.n_local) * 3 * 8 + 2 * int(Vi.n_owned) * 3 * 8
    kern = {}
    for k, pairs in ev.items():
        ms = statistics.median(x.elapsed_time(y) for x, y in pairs[3:])
        kern[k] = {"ms": round(ms, 4)}
        nbytes = nut_bytes if k.startswith("nut_") else (st_bytes if k == "stress_transpose" else None)
        if nbytes is not None:
            kern[k]["bytes"] = nbytes
            kern[k]["fraction_of_hbm_peak"] = round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)

    # ---- part 2: whole steps, alternating -----------------------------------------------------------------------------
    phase = []
    inner = S2.stress_transpose_assemble

    def wrapped():
        phase.append(timed(torch, inner))

    S2.stress_transpose_assemble = wrapped
    runs = (("constant_nu", S0, clk0, None), ("carreau_yasuda", S1, clk1, None),
            ("smagorinsky_laplacian", S2, clk2, "laplacian"), ("smagorinsky_full", S2, clk2, "full"))
    rec = {key: {"step": [], "transpose": []} for key, *_ in runs}
    for i in range(a.steps + 1):
        for key, S, clk, form in runs:
            if form is not None:
                S._stress_form = form
            phase.clear()
            clk["t"] += dt
            e = timed(torch, lambda: S.solve(dt, nu, max_iter=1))
            torch.cuda.synchronize()
            if i == 0:
                continue
            rec[key]["step"].append(e[0].elapsed_time(e[1]))
            if form == "full":
                rec[key]["transpose"].append(sum(x.elapsed_time(y) for x, y in phase))
    steps = {k: {"ms_per_step": round(statistics.median(v["step"]), 3)} for k, v in rec.items()}
    steps["smagorinsky_full"]["stress_transpose_assemble_ms"] = round(statistics.median(rec["smagorinsky_full"]["transpose"]), 4)
    for key, S in (("constant_nu", S0), ("carreau_yasuda", S1), ("smagorinsky", S2)):
        steps.setdefault(key, {})["iterations"] = {k: [int(i) for i in v] for k, v in S.iteration_counts().items()}
    eff = S1.effective_viscosity()
    out = {"N": a.N, "rows_u": int(P.n_rows), "entry_slots": int(P.size), "cells": ncells, "adjacency_bytes": adj_bytes,
           "nu": nu, "dt": dt, "carreau_yasuda_nu_min_mean_max": [float(eff.min()), float(eff.mean()), float(eff.max())],
           "kernel": kern, "steps": steps}
    if bench is not None:
        out["bench_default_steps_per_s"] = bench
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
