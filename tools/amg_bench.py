"""pc_type gamg against jacobi on the pressure solve of FractionalStep_AB_CN: per problem, the pressure solve's device
time per step and its iterations, the hierarchy's set-up seconds and the launches per iteration.

    python tools/amg_bench.py [--steps 5] [--warmup 3] [--only tg,tg0,beltrami,delaunay] [--out FILE]

Problems (bench.py's workloads, P2-P1, rtol 1e-8): Taylor-Green 128^3 with the warm start (the headline's setting) and
with a zero initial guess, Beltrami 128^3, and the Beltrami field on the Delaunay mesh (32, refined twice).  One JSON
line per problem and solver on stdout (and in --out)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROBLEMS = {"tg": ("tg", 128, None, False), "tg0": ("tg", 128, None, True), "beltrami": ("beltrami", 128, None, False),
            "delaunay": ("beltrami", 128, (32, 2), False)}


def run(name, pc, steps, warmup):
    import numpy as np
    import torch

    import oasisx_amd as ox
    from bench import make_workload
    from oasisx_amd import mesh as M

    wname, N, delaunay, zero = PROBLEMS[name]
    W = make_workload(wname, N, np, torch)
    q0, q1 = W["box"]
    clk = {"t": 0.0}

    def on_bnd(x):
        on = np.zeros(x.shape[1], dtype=bool)
        for k in range(3):
            on |= np.isclose(x[k], q0[k]) | np.isclose(x[k], q1[k])
        return on

    def bcv(f):
        def g(x):
            return f(x, clk["t"])
        g.supports_torch = True
        return g

    def at(f, t):
        def g(x):
            return f(x, t)
        g.supports_torch = True
        return g

    mesh = (M.create_box(None, [q0, q1], [N, N, N]) if delaunay is None
            else M.create_delaunay_box(None, [q0, q1], delaunay[0], refine=delaunay[1]))
    ksp = {"pc_type": "jacobi", "ksp_rtol": 1e-8, "ksp_atol": 1e-14, "ksp_max_it": 10000, "ksp_initial_guess_nonzero": not zero}
    pres = dict(ksp, ksp_type="cg", pc_type=pc)
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1),
                                bcs_u=[[ox.DirichletBC(bcv(f), ox.LocatorMethod.GEOMETRICAL, on_bnd)] for f in W["fns"]],
                                bcs_p=[], solver_options={"tentative": dict(ksp, ksp_type="bcgs"), "pressure": pres,
                                                          "scalar": dict(ksp, ksp_type="cg")}, options={})
    for i, f in enumerate(W["fns"]):
        S._u2[i].interpolate(at(f, -W["dt"]))
        S._u1[i].interpolate(at(f, 0.0))
    S._p.interpolate(lambda x: W["p"](x, -W["dt"] / 2.0))
    ev = []
    inner = S.pressure_solve

    def timed(*a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = inner(*a, **k)
        e1.record()
        ev.append((e0, e1))
        return r

    S.pressure_solve = timed
    its = []
    for i in range(warmup + steps):
        clk["t"] += W["dt"]
        S.solve(W["dt"], W["nu"], max_iter=1)
        its.append(int(S.iteration_counts()["pressure"][0]))
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev[warmup:]]
    sp = S._solver_p
    out = {"problem": name, "pc_type": pc, "rows": int(S._Ap.pattern.n_rows), "steps": steps,
           "pressure_ms_per_step": sum(ms) / len(ms), "pressure_iterations": its[warmup:],
           "kernels_per_iteration": int(sp._cg_kernels_per_iteration())}
    if pc == "gamg":
        mg = sp._hierarchy()
        out.update({"setup_s": round(mg.setup_s, 3), "setup_host_s": round(mg.setup_host_s, 3), "levels": mg.rows,
                    "cycle_kernels": mg.kernels_per_cycle()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=",".join(PROBLEMS))
    ap.add_argument("--pc", default="jacobi,gamg")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for name in a.only.split(","):
        for pc in a.pc.split(","):
            t0 = time.perf_counter()
            r = run(name, pc, a.steps, a.warmup)
            r["wall_s"] = round(time.perf_counter() - t0, 1)
            print(json.dumps(r), flush=True)
            rows.append(r)
            import torch

            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
