"""ksp_guess_type fischer on FractionalStep_AB_CN: per leg, the pressure solve's and the velocity update's device time per
step (the guess and the basis update included), their iterations per step and the device bytes of each basis.

    python tools/guess_bench.py [--steps 20] [--warmup 5] [--only tg,beltrami,delaunay] [--legs a,b,...] [--out FILE]

Problems as tools/amg_bench.py (P2-P1, rtol 1e-8, warm start): Taylor-Green 128^3, Beltrami 128^3 and the Beltrami field
on the Delaunay mesh (32, refined twice).  A leg sets the guess of the velocity update (the "scalar" solver) or of the pressure
solve; both phases are timed separately in every leg.  One JSON line per problem and leg on stdout (and --out)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# leg -> (scalar fischer "model,size" or None, pressure pc_type, pressure fischer or None): every leg changes ONE solver
# against "none" / "gamg" (a guess on the velocity update changes the next steps' pressure right-hand sides too)
LEGS = {
    "none": (None, "jacobi", None),
    "u12": ("1,2", "jacobi", None),
    "u14": ("1,4", "jacobi", None),
    "u110": ("1,10", "jacobi", None),
    "u24": ("2,4", "jacobi", None),
    "p14": (None, "jacobi", "1,4"),
    "p110": (None, "jacobi", "1,10"),
    "p120": (None, "jacobi", "1,20"),
    "gamg": (None, "gamg", None),
    "gamg_p110": (None, "gamg", "1,10"),
}
PROBLEMS = {"tg": ("tg", 128, None), "beltrami": ("beltrami", 128, None), "delaunay": ("beltrami", 128, (32, 2))}


def run(name, leg, steps, warmup):
    import numpy as np
    import torch

    import oasisx_amd as ox
    from bench import make_workload
    from oasisx_amd import _lib
    from oasisx_amd import mesh as M

    wname, N, delaunay = PROBLEMS[name]
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

    ug, pc, pg = LEGS[leg]
    mesh = (M.create_box(None, [q0, q1], [N, N, N]) if delaunay is None
            else M.create_delaunay_box(None, [q0, q1], delaunay[0], refine=delaunay[1]))
    ksp = {"pc_type": "jacobi", "ksp_rtol": 1e-8, "ksp_atol": 1e-14, "ksp_max_it": 10000, "ksp_initial_guess_nonzero": True}
    pres = dict(ksp, ksp_type="cg", pc_type=pc)
    upd = dict(ksp, ksp_type="cg")
    if pg:
        pres.update(ksp_guess_type="fischer", ksp_guess_fischer_model=pg)
    if ug:
        upd.update(ksp_guess_type="fischer", ksp_guess_fischer_model=ug)
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1),
                                bcs_u=[[ox.DirichletBC(bcv(f), ox.LocatorMethod.GEOMETRICAL, on_bnd)] for f in W["fns"]],
                                bcs_p=[], solver_options={"tentative": dict(ksp, ksp_type="bcgs"), "pressure": pres,
                                                          "scalar": upd}, options={})
    for i, f in enumerate(W["fns"]):
        S._u2[i].interpolate(at(f, -W["dt"]))
        S._u1[i].interpolate(at(f, 0.0))
    S._p.interpolate(lambda x: W["p"](x, -W["dt"] / 2.0))
    ev = {"pressure_solve": [], "velocity_update": []}
    for ph in ev:
        inner = getattr(S, ph)

        def timed(*a, _inner=inner, _ev=ev[ph], **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = _inner(*a, **k)
            e1.record()
            _ev.append((e0, e1))
            return r

        setattr(S, ph, timed)
    itp, itu = [], []
    for i in range(warmup + steps):
        clk["t"] += W["dt"]
        S.solve(W["dt"], W["nu"], max_iter=1)
        c = S.iteration_counts()
        itp.append(int(c["pressure"][0]))
        itu.append([int(v) for v in c["update"]])
    torch.cuda.synchronize()
    ms = {ph: [a.elapsed_time(b) for a, b in e[warmup:]] for ph, e in ev.items()}
    lib = _lib.load()

    def basis_bytes(ksp_):
        g = ksp_._guess
        return 0 if g is None else int(lib.ox_guess_bytes(g.handle))

    return {"problem": name, "leg": leg, "update_guess": ug, "pressure_pc": pc, "pressure_guess": pg,
            "rows_p": int(S._Ap.pattern.n_rows), "rows_u": int(S._M.pattern.n_rows), "steps": steps,
            "pressure_ms_per_step": sum(ms["pressure_solve"]) / steps, "pressure_iterations": itp[warmup:],
            "update_ms_per_step": sum(ms["velocity_update"]) / steps,
            "update_iterations": [max(v) for v in itu[warmup:]],
            "pressure_basis_bytes": basis_bytes(S._solver_p), "update_basis_bytes": basis_bytes(S._solver_c)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="tg")
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for name in a.only.split(","):
        for leg in a.legs.split(","):
            t0 = time.perf_counter()
            r = run(name, leg, a.steps, a.warmup)
            r["wall_s"] = round(time.perf_counter() - t0, 1)
            print(json.dumps(r), flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(json.dumps(r) + "\n")
            import torch

            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
