"""Passive scalar transport at the bench size (Taylor-Green 128^3, P2-P1, rtol 1e-8, warm start): ONE solver, one process,
HIP events, medians, the versions alternating inside the timed loop.

    python tools/scalar_bench.py [-N 128] [--steps 12] [--warmup 4] [--reps 20] [--out FILE]

Part 1, the kernel: ``ox_scalar_rows`` (1 and 3 columns, with and without the A_c c_1 output) timed beside the yardstick
it replaces -- ``assemble_first`` of the solver without scalars, i.e. what running the element loop again with kappa would
cost -- launch after launch, alternating.  Bytes moved per launch from the stored sizes: per entry slot 8 B of A read,
8 B of A_c written, 4 B of columns, 1 + 1 B of value codes of M and K (8 + 8 B without dictionaries); per row 8 B per
column of b0 read and of b (and a_c1) written; the c_1 gathers are served by the caches and count once per row.

Part 2, the step: ms per step with 0, 1, 3 scalars in three groups and 3 scalars in one group (the group list of the one
solver is switched from step to step, so the variants alternate), scalar_assemble and scalar_solve split out."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s


def build(N):
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

    def left(x):
        return np.isclose(x[0], q0[0])

    def at(f, t):
        def g(x):
            return f(x, clk["t"] if t is None else t)
        g.supports_torch = True
        return g

    mesh = M.create_box(None, [q0, q1], [N, N, N])
    ksp = {"pc_type": "jacobi", "ksp_rtol": 1e-8, "ksp_atol": 1e-14, "ksp_max_it": 10000, "ksp_initial_guess_nonzero": True}
    ini = lambda x: np.cos(np.pi * x[0]) * np.cos(np.pi * x[1])  # noqa: E731
    G = ox.LocatorMethod.GEOMETRICAL
    # three groups of one (different Schmidt numbers) and one group of three (same kappa, same rows)
    scalars = [ox.ScalarTransport(f"s{i}", schmidt=sc, initial=ini, bcs=[ox.DirichletBC(1.0, G, left)])
               for i, sc in enumerate((1.0, 2.0, 4.0))]
    scalars += [ox.ScalarTransport(f"g{i}", schmidt=0.5, initial=ini, source=float(i), bcs=[ox.DirichletBC(float(i), G, left)])
                for i in range(3)]
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1),
                                bcs_u=[[ox.DirichletBC(at(f, None), G, on_bnd)] for f in W["fns"]], bcs_p=[],
                                solver_options={"tentative": dict(ksp, ksp_type="bcgs"), "pressure": dict(ksp, ksp_type="cg"),
                                                "scalar": dict(ksp, ksp_type="cg")}, options={}, scalars=scalars)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-N", type=int, default=128)
    ap.add_argument("--steps", type=int, default=12, help="timed steps per variant")
    ap.add_argument("--warmup", type=int, default=4, help="warm-up steps (all scalars on)")
    ap.add_argument("--reps", type=int, default=20, help="timed launches per kernel variant")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from oasisx_amd import _lib

    S, W, clk = build(a.N)
    dt, nu = W["dt"], W["nu"]
    groups = list(S._scalar_groups)
    singles, triple = [g for g in groups if g.nc == 1], [g for g in groups if g.nc == 3]
    assert len(singles) == 3 and len(triple) == 1
    for _ in range(a.warmup):
        clk["t"] += dt
        S.solve(dt, nu, max_iter=1)
    torch.cuda.synchronize()

    # ---- part 1: the kernel beside assemble_first ----------------------------------------------------------------
    lib, st = _lib.load(), _lib.current_stream()
    P = S._A.pattern
    dictionary = S._M.vcode is not None and S._K.vcode is not None

    def kernel(g, au):
        _lib.check(lib.ox_scalar_rows(S._A.ref(), S._M.ref(), S._K.ref(), g.Ac.ref(), 0.5 * (g.members[0].kappa(nu) - nu), dt,
                                      g.nc, g.C1.rptr(), g.B0.rptr(), g.B.ptr(), g.AC1.ptr() if au else None, st),
                   "ox_scalar_rows")

    def bytes_moved(nc, au):
        per_slot = 8 + 8 + 4 + (2 if dictionary else 16)
        per_row = 8 * nc * (3 + (1 if au else 0))  # c_1 (once per row), b0, b, a_c1
        return int(P.size) * per_slot + int(P.n_rows) * per_row

    S._scalar_groups = []  # assemble_first as the solver without scalars runs it (leaves A before its boundary rows + them)
    variants = {"assemble_first": lambda: S.assemble_first(dt, nu),
                "rows_1": lambda: kernel(singles[0], False), "rows_1_au": lambda: kernel(singles[0], True),
                "rows_3": lambda: kernel(triple[0], False), "rows_3_au": lambda: kernel(triple[0], True)}
    ev = {k: [] for k in variants}
    for r in range(a.reps + 3):
        for k, fn in variants.items():
            ev[k].append(timed(torch, fn))
    torch.cuda.synchronize()
    kern = {}
    for k, pairs in ev.items():
        ms = statistics.median(x.elapsed_time(y) for x, y in pairs[3:])
        kern[k] = {"ms": round(ms, 4)}
        if k != "assemble_first":
            nc, au = (3 if "3" in k else 1), k.endswith("au")
            kern[k]["bytes"] = bytes_moved(nc, au)
            kern[k]["fraction_of_hbm_peak"] = round(bytes_moved(nc, au) / (ms * 1e-3) / HBM_PEAK, 3)
    S._scalar_groups = groups

    # ---- part 2: whole steps, the variants alternating -------------------------------------------------------------
    phases = {"scalar_assemble": [], "scalar_solve": []}
    for ph, store in phases.items():
        inner = getattr(S, ph)

        def wrapped(*args, _inner=inner, _store=store, **kw):
            out = {}
            _store.append(timed(torch, lambda: out.setdefault("r", _inner(*args, **kw))))
            return out["r"]

        setattr(S, ph, wrapped)
    sets = {"0": [], "1": singles[:1], "3_groups": singles, "3_lockstep": triple}
    rec = {k: {"step": [], "assemble": [], "solve": [], "its": []} for k in sets}
    for i in range(a.steps + 1):  # (the first round settles the scalars that were idle during the others' steps)
        for k, gs in sets.items():
            S._scalar_groups = gs
            for store in phases.values():
                store.clear()
            clk["t"] += dt
            e = timed(torch, lambda: S.solve(dt, nu, max_iter=1))
            torch.cuda.synchronize()
            if i == 0:
                continue
            rec[k]["step"].append(e[0].elapsed_time(e[1]))
            rec[k]["assemble"].append(sum(x.elapsed_time(y) for x, y in phases["scalar_assemble"]))
            rec[k]["solve"].append(sum(x.elapsed_time(y) for x, y in phases["scalar_solve"]))
            if gs:
                rec[k]["its"].append(max(v for g in gs for v in g.ksp.iterations[: g.nc]))
    steps = {k: {"ms_per_step": round(statistics.median(v["step"]), 3),
                 "scalar_assemble_ms": round(statistics.median(v["assemble"]), 3),
                 "scalar_solve_ms": round(statistics.median(v["solve"]), 3),
                 "scalar_iterations": v["its"]} for k, v in rec.items()}
    out = {"N": a.N, "rows_u": int(P.n_rows), "entry_slots": int(P.size), "value_dictionary": dictionary,
           "value_array_bytes": int(P.size) * 8, "kernel": kern, "steps": steps,
           "steps_per_s_without_scalars": round(1e3 / steps["0"]["ms_per_step"], 3)}
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
