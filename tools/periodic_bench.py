"""Taylor-Green P2-P1 on the box periodic in all three axes beside the Dirichlet set-up of bench.py (exact data on all six
faces), both in ONE process at the bench's Krylov settings (rtol 1e-8, warm start), HIP events, medians, the two set-ups
alternating inside every timed loop.

    python tools/periodic_bench.py [-N 128] [--steps 12] [--warmup 4] [--reps 20] [--out profiles/periodic_bench_128.json]

Reported per set-up: set-up time (mesh + spaces + operators, wall clock), ms per step and Krylov iterations, the three
mat-vec kernels of a step (M with gdim columns, A with gdim columns, Ap with one), ``assemble_first``, and for both patterns
(velocity, pressure) rows, entries, padding (storage slots per entry - 1) and the share of the slots the 16-bit column
stream covers; after the timed steps the distance of u to the analytic field, and whether the products of M, A and Ap
through all storage forms equal the plain 32-bit / f64 stream bit for bit at this size.

What a seam can cost: the rows next to an identified face have columns at the far end of the numbering, so their gathers
leave the tile their neighbours share, and a slot whose column lies further than 2^16 from its block's base falls back to
the 32-bit stream."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(N, periodic):
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

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mesh = M.create_box(None, [q0, q1], [N, N, N])
    t_per = 0.0
    if periodic:
        t1 = time.perf_counter()
        mesh = M.make_periodic(mesh, (0, 1, 2))
        t_per = time.perf_counter() - t1
        bcs_u = [[], [], []]
    else:
        bcs_u = [[ox.DirichletBC(at(f, None), ox.LocatorMethod.GEOMETRICAL, on_bnd)] for f in W["fns"]]
    ksp = {"pc_type": "jacobi", "ksp_rtol": 1e-8, "ksp_atol": 1e-14, "ksp_max_it": 10000, "ksp_initial_guess_nonzero": True}
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_u=bcs_u, bcs_p=[],
                                solver_options={"tentative": dict(ksp, ksp_type="bcgs"), "pressure": dict(ksp, ksp_type="cg"),
                                                "scalar": dict(ksp, ksp_type="cg")},
                                options={"low_memory_version": False, "value_dictionary": True})
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0
    for i, f in enumerate(W["fns"]):
        S._u2[i].interpolate(at(f, -W["dt"]))
        S._u1[i].interpolate(at(f, 0.0))
    S._p.interpolate(lambda x: W["p"](x, -W["dt"] / 2.0))
    return S, W, clk, {"setup_s": round(setup_s, 3), "make_periodic_s": round(t_per, 3)}


def pattern_report(P):
    return {"rows": int(P.n_rows), "entries": int(P.nnz), "slots": int(P.size),
            "padding": round(int(P.size) / max(int(P.nnz), 1) - 1.0, 5),
            "cols16_share": None if getattr(P, "cols16", None) is None else round(float(P.frac16), 6),
            "row_len_max": int(P.row_len.max().item())}


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-N", type=int, default=128)
    ap.add_argument("--steps", type=int, default=12, help="timed steps per set-up")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20, help="timed launches per kernel")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    runs, report = {}, {"N": a.N, "steps": a.steps, "warmup": a.warmup, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    for name, periodic in (("dirichlet", False), ("periodic", True)):
        S, W, clk, info = build(a.N, periodic)
        runs[name] = (S, W, clk)
        Vi, Q = S._Vi[0][0], S._Q
        info.update({"velocity_dofs": int(Vi.num_dofs), "pressure_dofs": int(Q.num_dofs),
                     "velocity_pattern": pattern_report(Vi.pattern), "pressure_pattern": pattern_report(Q.pattern),
                     "M_value_codes": S._M.vcode is not None, "K_value_codes": S._K.vcode is not None,
                     "Ap_value_codes": S._Ap.vcode is not None, "Ap_pair_slots": S._Ap.ps_code is not None})
        report[name] = info
    dt, nu = runs["dirichlet"][1]["dt"], runs["dirichlet"][1]["nu"]

    def step(name):
        S, _, clk = runs[name]
        clk["t"] += dt
        S.solve(dt, nu, max_iter=1)

    for _ in range(a.warmup):
        for name in runs:
            step(name)
    torch.cuda.synchronize()
    ev = {name: [] for name in runs}
    its = {name: [] for name in runs}
    for _ in range(a.steps):
        for name in runs:
            ev[name].append(timed(torch, lambda n=name: step(n)))
            torch.cuda.synchronize()
            c = runs[name][0].iteration_counts()
            its[name].append([max(c["tentative"]), c["pressure"][0], max(c["update"])])
    for name in runs:
        ms = [x.elapsed_time(y) for x, y in ev[name]]
        report[name]["ms_per_step"] = round(statistics.median(ms), 3)
        report[name]["ms_per_step_min_max"] = [round(min(ms), 3), round(max(ms), 3)]
        report[name]["iterations_tentative_pressure_update"] = [round(statistics.mean(col), 2) for col in zip(*its[name])]
    # after the timed steps: the distance to the analytic field at the dofs, and -- the wrap-around rows at full size, where
    # the columns of one row lie up to the whole numbering apart -- the products of M, A and Ap through all the storage
    # forms the matrix carries against the plain 32-bit column / f64 value stream (level 1): equal bits
    for name, (S, W, clk) in runs.items():
        x = S._Vi[0][0].x
        X = torch.zeros((3, x.shape[0]), dtype=torch.float64, device=x.device)
        X[:3] = x.T
        exact = torch.stack([f(X, clk["t"]) for f in W["fns"]], dim=1)
        report[name]["t_end"] = clk["t"]
        report[name]["max_abs_u_minus_analytic"] = float((S._U.rdev()[: x.shape[0]] - exact).abs().max())
        g = torch.Generator(device=x.device).manual_seed(1)
        same = {}
        for label, A, nc in (("M", S._M, 3), ("A", S._A, 3), ("Ap", S._Ap, 1)):
            v = torch.randn((A.pattern.n_cols, nc), dtype=torch.float64, device=x.device, generator=g)
            ys = []
            for levels in (None, 1):
                A.set_levels(levels)
                y = torch.zeros_like(v)
                A.mult(v, y, nc)
                ys.append(y)
            A.set_levels(None)
            same[label] = bool(torch.equal(ys[0], ys[1])) and bool(torch.isfinite(ys[0]).all())
        report[name]["storage_levels_bit_identical"] = same
    # the kernels, launch after launch, the two set-ups alternating
    kern = {name: {} for name in runs}
    jobs = {}
    for name, (S, _, _) in runs.items():
        g = S._gdim
        xu, yu = torch.ones_like(S._U.rdev()), torch.zeros_like(S._U.rdev())
        xq, yq = torch.ones_like(S._P.rdev()), torch.zeros_like(S._P.rdev())
        jobs[name] = {"spmv_M_3col": lambda S=S, x=xu, y=yu, g=g: S._M.mult(x, y, g),
                      "spmv_A_3col": lambda S=S, x=xu, y=yu, g=g: S._A.mult(x, y, g),
                      "spmv_Ap_1col": lambda S=S, x=xq, y=yq: S._Ap.mult(x, y, 1),
                      "assemble_first": lambda S=S: S.assemble_first(dt, nu)}
    pairs = {(n, k): [] for n in jobs for k in jobs[n]}
    for _ in range(a.reps + 3):
        for k in jobs["dirichlet"]:
            for n in jobs:
                pairs[(n, k)].append(timed(torch, jobs[n][k]))
    torch.cuda.synchronize()
    for (n, k), p in pairs.items():
        ms = [x.elapsed_time(y) for x, y in p[3:]]
        kern[n][k] = {"ms": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}
    for n in runs:
        report[n]["kernels"] = kern[n]
    report["periodic_over_dirichlet"] = {
        "ms_per_step": round(report["periodic"]["ms_per_step"] / report["dirichlet"]["ms_per_step"], 4),
        **{k: round(kern["periodic"][k]["ms"] / kern["dirichlet"][k]["ms"], 4) for k in kern["periodic"]}}
    line = json.dumps(report)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(report, indent=1) + "\n")


if __name__ == "__main__":
    main()
