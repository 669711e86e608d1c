"""Scalars under a viscosity model at the bench size (Taylor-Green 128^3, P2-P1, Smagorinsky): ONE solver, one process, HIP
events, medians, the variants alternating inside the timed loop.

    python tools/scalar_les_bench.py [-N 128] [--warmup 2] [--reps 20] [--out FILE]

Timed, launch after launch:
  new_1 / new_3        ``ox_scalar_rows_cellvisc`` with one and three columns (A_c = A + s K + t K_t, b_c and A_c c_1)
  rows_1 / rows_3      (a) ``ox_scalar_rows`` on the same matrices (A_c = A + s K: what Sc_t = 1 costs)
  assemble_first_nut   (b) ``ox_assemble_first`` with ``nut``: the pair loop WITH the convection turns and gathers
  stiff_pass           one ``ox_assemble_matrix(OX_KIND_STIFF)`` pass into a value array of the velocity pattern
  composed_1 / _3      (c) the composed alternative priced from what exists: stiff_pass + rows_1 / rows_3 (a sum, not a run:
                       a weighted-stiffness kernel would cost at least the unweighted pass, and the three-matrix stream more
                       than rows_*)
Bytes moved per launch from the stored sizes.  Streams per entry slot: 8 B of A read, 8 B of A_c written, 4 B of columns,
1 + 1 B of value codes of M and K (8 + 8 B without dictionaries); per row 8 B per column of c_1 (gathers: once per row),
b0, b and a_c1.  The pair loop of the new launch adds per (row, cell) slot 4 B of cell index, 1 B of local index and the
``pw`` bytes of accumulator positions, and per cell (once: the rest is served by the caches) the geometry record and 8 B
of ``nut``."""
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
    scalars = [ox.ScalarTransport("s", schmidt=2.0, initial=ini, bcs=[ox.DirichletBC(1.0, G, left)], turbulent_schmidt=0.7)]
    scalars += [ox.ScalarTransport(f"g{i}", schmidt=0.5, initial=ini, source=float(i), bcs=[ox.DirichletBC(float(i), G, left)],
                                   turbulent_schmidt=0.9) for i in range(3)]
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1),
                                bcs_u=[[ox.DirichletBC(at(f, None), G, on_bnd)] for f in W["fns"]], bcs_p=[],
                                solver_options={"tentative": dict(ksp, ksp_type="bcgs"), "pressure": dict(ksp, ksp_type="cg"),
                                                "scalar": dict(ksp, ksp_type="cg"),
                                                "scalar_transport": dict(ksp, ksp_type="bcgs")}, options={}, scalars=scalars,
                                viscosity_model=ox.Smagorinsky())
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
    ap.add_argument("--warmup", type=int, default=2, help="warm-up steps")
    ap.add_argument("--reps", type=int, default=20, help="timed launches per variant")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from oasisx_amd import _lib
    from oasisx_amd import scalar as _sc
    from oasisx_amd.la import assemble_matrix

    S, W, clk = build(a.N)
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

    def new(g):
        _lib.check(lib.ox_scalar_rows_cellvisc(C.byref(S._cells), C.byref(Vi.assembly_info()), S._A.ref(), S._M.ref(),
                                               S._K.ref(), g.Ac.ref(), _lib.ptr(S._nut), 0.5 * (g.members[0].kappa(nu) - nu),
                                               _sc.turbulent_factor(S, g.members[0]), dt, g.nc, g.C1.rptr(), g.B0.rptr(),
                                               g.B.ptr(), g.AC1.ptr(), row_blocks, st), "ox_scalar_rows_cellvisc")

    def rows(g):
        _lib.check(lib.ox_scalar_rows(S._A.ref(), S._M.ref(), S._K.ref(), g.Ac.ref(), 0.5 * (g.members[0].kappa(nu) - nu), dt,
                                      g.nc, g.C1.rptr(), g.B0.rptr(), g.B.ptr(), g.AC1.ptr(), st), "ox_scalar_rows")

    n_pairs, n_cells = int(Vi.adj.adj_cell.shape[0]), int(S._nut.shape[0])
    gs = int(S._geom.shape[1]) if S._geom.dim() == 2 else int(S._geom.numel() // n_cells)

    def stream_bytes(nc):
        per_slot = 8 + 8 + 4 + (2 if dictionary else 16)
        return int(P.size) * per_slot + int(P.n_rows) * 8 * nc * 4  # c_1 (once per row), b0, b, a_c1

    def pair_bytes():
        return n_pairs * (4 + 1 + int(Vi.adj.pw)) + n_cells * (gs * 8 + 8)

    variants = {"new_1": lambda: new(single), "rows_1": lambda: rows(single), "new_3": lambda: new(triple),
                "rows_3": lambda: rows(triple), "assemble_first_nut": lambda: S._assemble_first_rows(dt, nu, True),
                "stiff_pass": lambda: assemble_matrix(1, Vi, S._cells, single.Ac, row_blocks=bool(row_blocks))}
    # (every variant leaves A, M, K, nut as they were or rewrites A with the same values: the order does not matter)
    S._assemble_first_rows(dt, nu, True)
    ev = {k: [] for k in variants}
    for r in range(a.reps + 3):
        for k, fn in variants.items():
            ev[k].append(timed(torch, fn))
    torch.cuda.synchronize()
    kern = {}
    for k, pairs in ev.items():
        t = sorted(x.elapsed_time(y) for x, y in pairs[3:])
        kern[k] = {"ms": round(statistics.median(t), 4), "ms_min": round(t[0], 4), "ms_max": round(t[-1], 4)}
    for k, nc in (("new_1", 1), ("new_3", 3), ("rows_1", 1), ("rows_3", 3)):
        b = stream_bytes(nc) + (pair_bytes() if k.startswith("new") else 0)
        kern[k]["bytes"] = b
        kern[k]["fraction_of_hbm_peak"] = round(b / (kern[k]["ms"] * 1e-3) / HBM_PEAK, 3)
    kern["stiff_pass"]["bytes"] = int(P.size) * 8 + pair_bytes()
    kern["stiff_pass"]["fraction_of_hbm_peak"] = round(kern["stiff_pass"]["bytes"] / (kern["stiff_pass"]["ms"] * 1e-3) / HBM_PEAK, 3)
    for nc in (1, 3):  # (c): a sum of measured launches; its traffic: the K_t array written, then read by the stream
        kern[f"composed_{nc}"] = {"ms": round(kern["stiff_pass"]["ms"] + kern[f"rows_{nc}"]["ms"], 4),
                                  "bytes": kern["stiff_pass"]["bytes"] + kern[f"rows_{nc}"]["bytes"] + int(P.size) * 8}
    out = {"N": a.N, "rows_u": int(P.n_rows), "entry_slots": int(P.size), "pair_slots": n_pairs, "cells": n_cells,
           "value_dictionary": dictionary, "row_blocks": bool(row_blocks), "value_array_bytes": int(P.size) * 8,
           "reps": a.reps, "nut_max": float(S._nut.max()), "kernel": kern,
           "new_over_assemble_first": {f"{nc}": round(kern[f"new_{nc}"]["ms"] / kern["assemble_first_nut"]["ms"], 3) for nc in (1, 3)},
           "new_over_composed": {f"{nc}": round(kern[f"new_{nc}"]["ms"] / kern[f"composed_{nc}"]["ms"], 3) for nc in (1, 3)}}
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
