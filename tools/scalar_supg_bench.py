"""SUPG-stabilised scalars at the bench size (Taylor-Green 128^3, P2-P1, Smagorinsky): ONE solver, one process, HIP events,
medians, the variants alternating inside the timed loop.

    python tools/scalar_supg_bench.py [-N 128] [--warmup 2] [--reps 20] [--step-reps 5] [--out FILE]

Timed, launch after launch:
  supg_cells           ``ox_supg_cells``: w_c and tau_c per cell
  supg_1 / supg_3      ``ox_scalar_rows_supg`` with one and three columns
  cellvisc_1 / _3      ``ox_scalar_rows_cellvisc`` on the same matrices (the sibling without the stabilising terms)
  rows_1 / rows_3      ``ox_scalar_rows`` on the same matrices (no pair loop at all)
  assemble_first_nut   ``ox_assemble_first`` with ``nut``: the pair loop WITH the convection turns and the u_ab gathers
Then (``--step-reps`` > 0) whole steps of a solver with ONE scalar, with and without ``stabilization=``, alternating.
Bytes moved per launch from the stored sizes: the streams of ``ox_scalar_rows`` (tools/scalar_les_bench.py), for the pair
loop per (row, cell) slot 4 B of cell index, 1 B of local index and ``pw`` position bytes, per cell (once: the rest is served
by the caches) the geometry record, 8 B of ``nut`` and -- SUPG -- the (gdim + 1) x 8 B record and the nd x 4 B of cell dofs,
per row once the 2 x 8 B per column of c_1 and f_h the right-hand-side term gathers."""
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


def build(N, scalars_of):
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
    G = ox.LocatorMethod.GEOMETRICAL
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1),
                                bcs_u=[[ox.DirichletBC(at(f, None), G, on_bnd)] for f in W["fns"]], bcs_p=[],
                                solver_options={"tentative": dict(ksp, ksp_type="bcgs"), "pressure": dict(ksp, ksp_type="cg"),
                                                "scalar": dict(ksp, ksp_type="cg"),
                                                "scalar_transport": dict(ksp, ksp_type="bcgs")}, options={},
                                scalars=scalars_of(ox, G, left), viscosity_model=ox.Smagorinsky())
    for i, f in enumerate(W["fns"]):
        S._u2[i].interpolate(at(f, -W["dt"]))
        S._u1[i].interpolate(at(f, 0.0))
    S._p.interpolate(lambda x: W["p"](x, -W["dt"] / 2.0))
    return S, W, clk


def _ini(x):
    import numpy as np

    return np.cos(np.pi * x[0]) * np.cos(np.pi * x[1])


def kernel_scalars(ox, G, left):
    s = [ox.ScalarTransport("s", schmidt=1000.0, initial=_ini, bcs=[ox.DirichletBC(1.0, G, left)], turbulent_schmidt=0.7,
                            stabilization=ox.SUPG())]
    s += [ox.ScalarTransport(f"g{i}", schmidt=500.0, initial=_ini, source=float(i), bcs=[ox.DirichletBC(float(i), G, left)],
                             turbulent_schmidt=0.9, stabilization=ox.SUPG()) for i in range(3)]
    return s


def one_scalar(stabilize):
    def f(ox, G, left):
        return [ox.ScalarTransport("s", schmidt=1000.0, initial=_ini, bcs=[ox.DirichletBC(1.0, G, left)],
                                   turbulent_schmidt=0.7, stabilization=ox.SUPG() if stabilize else None)]
    return f


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-N", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=2, help="warm-up steps")
    ap.add_argument("--reps", type=int, default=20, help="timed launches per variant")
    ap.add_argument("--step-reps", type=int, default=5, help="timed whole steps per variant (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from oasisx_amd import _lib
    from oasisx_amd import scalar as _sc

    S, W, clk = build(a.N, kernel_scalars)
    dt, nu = W["dt"], W["nu"]
    single, triple = [g for g in S._scalar_groups if g.nc == 1][0], [g for g in S._scalar_groups if g.nc == 3][0]
    for _ in range(a.warmup):
        clk["t"] += dt
        S.solve(dt, nu, max_iter=1)
    torch.cuda.synchronize()
    lib, st = _lib.load(), _lib.current_stream()
    Vi = S._Vi[0][0]
    P = S._A.pattern
    dictionary = S._M.vcode is not None and S._K.vcode is not None
    row_blocks = int(S._row_blocks and P.n_row_blocks > 0)

    def s_of(g):
        return 0.5 * (g.members[0].kappa(nu) - nu)

    def supg(g):
        _lib.check(lib.ox_scalar_rows_supg(C.byref(S._cells), C.byref(Vi.assembly_info()), S._A.ref(), S._M.ref(), S._K.ref(),
                                           g.Ac.ref(), _lib.ptr(S._nut), _lib.ptr(g.supg_rec), s_of(g),
                                           _sc.turbulent_factor(S, g.members[0]), dt, g.nc, g.C1.rptr(), g.B0.rptr(),
                                           g.FH.rptr(), g.B.ptr(), g.AC1.ptr(), row_blocks, st), "ox_scalar_rows_supg")

    def cellvisc(g):
        _lib.check(lib.ox_scalar_rows_cellvisc(C.byref(S._cells), C.byref(Vi.assembly_info()), S._A.ref(), S._M.ref(),
                                               S._K.ref(), g.Ac.ref(), _lib.ptr(S._nut), s_of(g),
                                               _sc.turbulent_factor(S, g.members[0]), dt, g.nc, g.C1.rptr(), g.B0.rptr(),
                                               g.B.ptr(), g.AC1.ptr(), row_blocks, st), "ox_scalar_rows_cellvisc")

    def rows(g):
        _lib.check(lib.ox_scalar_rows(S._A.ref(), S._M.ref(), S._K.ref(), g.Ac.ref(), s_of(g), dt, g.nc, g.C1.rptr(),
                                      g.B0.rptr(), g.B.ptr(), g.AC1.ptr(), st), "ox_scalar_rows")

    n_pairs, n_cells = int(Vi.adj.adj_cell.shape[0]), int(S._nut.shape[0])
    gs = int(S._geom.shape[1]) if S._geom.dim() == 2 else int(S._geom.numel() // n_cells)
    nd, gdim = int(Vi.cell_dofs.shape[1]), int(S._gdim)

    def stream_bytes(nc):
        per_slot = 8 + 8 + 4 + (2 if dictionary else 16)
        return int(P.size) * per_slot + int(P.n_rows) * 8 * nc * 4  # c_1 (once per row), b0, b, a_c1

    def pair_bytes(with_supg):
        b = n_pairs * (4 + 1 + int(Vi.adj.pw)) + n_cells * (gs * 8 + 8)
        return b + (n_cells * ((gdim + 1) * 8 + nd * 4) if with_supg else 0)

    variants = {"supg_cells": lambda: _sc.stabilization_cells(S, single, dt, nu), "supg_1": lambda: supg(single),
                "cellvisc_1": lambda: cellvisc(single), "rows_1": lambda: rows(single), "supg_3": lambda: supg(triple),
                "cellvisc_3": lambda: cellvisc(triple), "rows_3": lambda: rows(triple),
                "assemble_first_nut": lambda: S._assemble_first_rows(dt, nu, True)}
    # (every variant leaves A, M, K, nut and the records as they were or rewrites them with the same values)
    S._assemble_first_rows(dt, nu, True)
    for g in (single, triple):
        _sc.stabilization_cells(S, g, dt, nu)
    ev = {k: [] for k in variants}
    for r in range(a.reps + 3):
        for k, fn in variants.items():
            ev[k].append(timed(torch, fn))
    torch.cuda.synchronize()
    kern = {}
    for k, pairs in ev.items():
        t = sorted(x.elapsed_time(y) for x, y in pairs[3:])
        kern[k] = {"ms": round(statistics.median(t), 4), "ms_min": round(t[0], 4), "ms_max": round(t[-1], 4)}
    for k in variants:
        if k == "assemble_first_nut":
            continue
        if k == "supg_cells":  # dofs, geometry, nut in; the record out; u_ab gathered (once per dof)
            b = n_cells * (nd * 4 + gs * 8 + 8 + (gdim + 1) * 8) + int(P.n_rows) * gdim * 8
        else:
            nc = int(k[-1])
            b = stream_bytes(nc)
            if not k.startswith("rows"):
                b += pair_bytes(k.startswith("supg"))
            if k.startswith("supg"):
                b += int(P.n_rows) * 8 * nc * 2  # c_1 and f_h of the right-hand-side term (once per row)
        kern[k]["bytes"] = b
        kern[k]["fraction_of_hbm_peak"] = round(b / (kern[k]["ms"] * 1e-3) / HBM_PEAK, 3)
    out = {"N": a.N, "rows_u": int(P.n_rows), "entry_slots": int(P.size), "pair_slots": n_pairs, "cells": n_cells,
           "value_dictionary": dictionary, "row_blocks": bool(row_blocks), "reps": a.reps, "nut_max": float(S._nut.max()),
           "tau_max": float(single.supg_rec[-1].max()), "kernel": kern,
           "supg_over_cellvisc": {f"{nc}": round(kern[f"supg_{nc}"]["ms"] / kern[f"cellvisc_{nc}"]["ms"], 3) for nc in (1, 3)},
           "supg_over_assemble_first": {f"{nc}": round(kern[f"supg_{nc}"]["ms"] / kern["assemble_first_nut"]["ms"], 3)
                                        for nc in (1, 3)}}
    if a.step_reps > 0:  # whole steps with one scalar, with and without stabilisation: two solvers, alternating
        runs = {}
        for key, stab in (("galerkin", False), ("supg", True)):
            runs[key] = build(a.N, one_scalar(stab))
        for key, (Sx, Wx, cx) in runs.items():
            for _ in range(a.warmup):
                cx["t"] += dt
                Sx.solve(dt, nu, max_iter=1)
        torch.cuda.synchronize()
        evs = {k: [] for k in runs}
        its = {k: [] for k in runs}
        for r in range(a.step_reps):
            for key, (Sx, Wx, cx) in runs.items():
                cx["t"] += dt
                evs[key].append(timed(torch, lambda Sx=Sx: Sx.solve(dt, nu, max_iter=1)))
                its[key].append(Sx.iteration_counts()["scalar_transport"]["s"])
        torch.cuda.synchronize()
        out["step_one_scalar"] = {}
        for key, pairs in evs.items():
            t = sorted(x.elapsed_time(y) for x, y in pairs)
            out["step_one_scalar"][key] = {"ms": round(statistics.median(t), 3), "ms_min": round(t[0], 3),
                                           "ms_max": round(t[-1], 3), "scalar_iterations": its[key]}
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
