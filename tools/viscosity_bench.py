"""Eddy-viscosity models at the bench size (Taylor-Green 128^3, P2-P1, rtol 1e-8, warm start): two solvers in one
process (with and without ``viscosity_model=Smagorinsky()``), HIP events, medians, the variants alternating inside the
timed loops.

    python tools/viscosity_bench.py [-N 128] [--steps 12] [--warmup 4] [--reps 20] [--out FILE]
                                    [--bench-trees this=DIR parent=DIR] [--bench-runs 2]

Part 1, the kernels, launch after launch, alternating:
  * ``ox_cell_viscosity`` (Smagorinsky, WALE).  Bytes moved per launch from the stored sizes: per cell the dof list
    (nd x 4 B), the geometry record (10 x 8 B in 3-D) and 8 B of nut written; the u_ab gathers are served by the caches
    and count once per dof (gdim x 8 B);
  * ``assemble_first`` of the solver without a model (the constant-viscosity instantiation: the code of the parent
    commit), of the solver with a model without its nut kernel (the fused NUT instantiation alone) and as the step calls
    it (nut kernel + fused kernel);
  * one ``ox_assemble_matrix(STIFF)`` pass over the same pattern: what a separate weighted-stiffness assembly would cost
    at least, beside ``assemble_first``.
Part 2, whole steps with and without the model, alternating, the nut kernel's phase split out.
Part 3 (``--bench-trees``): ``bench.py --gpus 1 --steps 20 --warmup 5`` as child processes in the given source trees
(this commit, the parent commit), alternating, ``--bench-runs`` each: the default step must not change."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s


def build(N, model):
    import numpy as np
    import torch

    import oasisx_amd as ox
    from bench import make_workload
    from oasisx_amd import mesh as M

    W = make_workload("tg", N, np, torch)
    q0, q1 = W["box"]
    clk = {"t": 0.0}

    def on_bnd(x):
        on = np.zeros(x.shape[1], dtype=bool)
        for k in range(3):
            on |= np.isclose(x[k], q0[k]) | np.isclose(x[k], q1[k])
        return on

    def at(f, t):
        def g(x):
            return f(x, clk["t"] if t is None else t)
        g.supports_torch = True
        return g

    mesh = M.create_box(None, [q0, q1], [N, N, N])
    ksp = {"pc_type": "jacobi", "ksp_rtol": 1e-8, "ksp_atol": 1e-14, "ksp_max_it": 10000, "ksp_initial_guess_nonzero": True}
    G = ox.LocatorMethod.GEOMETRICAL
    kw = {} if model is None else {"viscosity_model": model}
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1),
                                bcs_u=[[ox.DirichletBC(at(f, None), G, on_bnd)] for f in W["fns"]], bcs_p=[],
                                solver_options={"tentative": dict(ksp, ksp_type="bcgs"), "pressure": dict(ksp, ksp_type="cg"),
                                                "scalar": dict(ksp, ksp_type="cg")}, options={}, **kw)
    for i, f in enumerate(W["fns"]):
        S._u2[i].interpolate(at(f, -W["dt"]))
        S._u1[i].interpolate(at(f, 0.0))
    S._p.interpolate(lambda x: W["p"](x, -W["dt"] / 2.0))
    return S, W, clk


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def bench_trees(trees, runs):
    """bench.py's default command line as a fresh child process per run, the trees (``label=directory``) alternating in
    the order given."""
    trees = [t.split("=", 1) if "=" in t else (t, t) for t in trees]
    out = {label: [] for label, _ in trees}
    for _ in range(runs):
        for t, where in trees:
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"],
                               cwd=os.path.abspath(where), capture_output=True, text=True)
            line = next((ln for ln in reversed(r.stdout.splitlines()) if ln.startswith("{")), None)
            if r.returncode != 0 or line is None:
                raise RuntimeError(f"bench.py in {t} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            out[t].append(round(float(json.loads(line)["value"]), 4))
            print(f"bench.py in {t}: {out[t][-1]} steps/s", flush=True)
    return out


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
    import torch

    import oasisx_amd as ox
    from oasisx_amd.la import SellMatrix
    from oasisx_amd.viscosity import _cell_viscosity

    # part 3 first: the children have the device to themselves (this process has not touched it yet)
    bench = bench_trees(a.bench_trees, a.bench_runs) if a.bench_trees else None
    S0, W, clk0 = build(a.N, None)
    S1, _, clk1 = build(a.N, ox.Smagorinsky())
    dt, nu = W["dt"], W["nu"]
    for S, clk in ((S0, clk0), (S1, clk1)):
        for _ in range(a.warmup):
            clk["t"] += dt
            S.solve(dt, nu, max_iter=1)
    torch.cuda.synchronize()

    # ---- part 1: the kernels ------------------------------------------------------------------------------------------
    Vi = S1._Vi[0][0]
    P = S1._A.pattern
    ncells, nd = int(S1._geom.shape[0]), int(Vi.cell_dofs.shape[1])
    want_au = True

    def nut_kernel(model_id, coef):
        _cell_viscosity(S1, S1._nut, model=model_id, coefficient=coef)

    scratch = SellMatrix(Vi.pattern, symmetric=True, name="K_bench")
    variants = {
        "assemble_first_constant_nu": lambda: S0.assemble_first(dt, nu),
        "assemble_first_with_model": lambda: S1.assemble_first(dt, nu),
        "fused_nut_kernel_alone": lambda: S1._assemble_first_rows(dt, nu, want_au),
        "stiffness_pass": lambda: S1._assemble_matrix(1, Vi, scratch),
        "nut_wale": lambda: nut_kernel(1, 0.325),
        "nut_smagorinsky": lambda: nut_kernel(0, 0.1677),
    }
    ev = {k: [] for k in variants}
    for r in range(a.reps + 3):
        for k, fn in variants.items():
            ev[k].append(timed(torch, fn))
    torch.cuda.synchronize()
    nut_bytes = ncells * (nd * 4 + int(S1._geom.shape[1]) * 8 + 8) + int(Vi.n_local) * 3 * 8
    kern = {}
    for k, pairs in ev.items():
        ms = statistics.median(x.elapsed_time(y) for x, y in pairs[3:])
        kern[k] = {"ms": round(ms, 4)}
        if k.startswith("nut_"):
            kern[k]["bytes"] = nut_bytes
            kern[k]["fraction_of_hbm_peak"] = round(nut_bytes / (ms * 1e-3) / HBM_PEAK, 3)
    kern["sum_constant_nu_plus_stiffness_pass"] = {
        "ms": round(kern["assemble_first_constant_nu"]["ms"] + kern["stiffness_pass"]["ms"], 4)}

    # ---- part 2: whole steps, alternating -----------------------------------------------------------------------------
    phase = []
    inner = S1.viscosity_assemble

    def wrapped(*args):
        phase.append(timed(torch, lambda: inner(*args)))

    S1.viscosity_assemble = wrapped
    rec = {"constant_nu": {"step": []}, "smagorinsky": {"step": [], "nut": []}}
    for i in range(a.steps + 1):
        for key, S, clk in (("constant_nu", S0, clk0), ("smagorinsky", S1, clk1)):
            phase.clear()
            clk["t"] += dt
            e = timed(torch, lambda: S.solve(dt, nu, max_iter=1))
            torch.cuda.synchronize()
            if i == 0:
                continue
            rec[key]["step"].append(e[0].elapsed_time(e[1]))
            if key == "smagorinsky":
                rec[key]["nut"].append(sum(x.elapsed_time(y) for x, y in phase))
    nut = S1.eddy_viscosity()
    steps = {k: {"ms_per_step": round(statistics.median(v["step"]), 3)} for k, v in rec.items()}
    steps["smagorinsky"]["viscosity_assemble_ms"] = round(statistics.median(rec["smagorinsky"]["nut"]), 4)
    for key, S in (("constant_nu", S0), ("smagorinsky", S1)):
        steps[key]["iterations"] = {k: [int(i) for i in v] for k, v in S.iteration_counts().items()}
    out = {"N": a.N, "rows_u": int(P.n_rows), "entry_slots": int(P.size), "cells": ncells,
           "value_dictionary": S1._M.vcode is not None and S1._K.vcode is not None, "row_blocks": bool(S1._row_blocks),
           "nu": nu, "dt": dt, "nut_min_mean_max": [float(nut.min()), float(nut.mean()), float(nut.max())],
           "kernel": kern, "steps": steps}
    if bench is not None:
        out["bench_default_steps_per_s"] = bench
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
