"""Boussinesq forces and wall scalar fluxes at the bench size (Taylor-Green 128^3, P2-P1, rtol 1e-8, warm start): ONE
solver, one process, HIP events, medians, the versions alternating inside the timed loop.

    python tools/buoyancy_bench.py [-N 128] [--steps 12] [--warmup 4] [--reps 20] [--out FILE]

Part 1, the kernels, launch after launch, alternating:
  ``ox_buoyancy_rows`` with 1 term (a group of one scalar, force on z) and with 3 terms (a group of three, forces on all
  components) and with 1 term without a second level (``extrapolate=False``: one gather per entry instead of two), each
  beside the COMPOSED path it replaces -- ``ox_axpby`` for c* = 1.5 c_1 - 0.5 c_2 into a temporary, the
  mass-matrix product into a second temporary, then one strided add per live (term, component) pair into the interleaved
  block (the reference value 0, which spares the composed path a pass) -- and beside the yardstick, the one-column
  product ``M x``;  ``ox_scalar_flux`` on all six faces of the box, without and with the time average.
  Bytes moved per launch from the stored sizes: per entry slot 4 B of columns and 1 B of value code (8 B without a
  dictionary); per row the rows of c_1 and c_2 of the terms' groups once (the gathers are served by the caches) and 16 B
  per live component of b (read and written).  The product: the same per slot, 16 B per row.  The flux: per facet 8 B of
  record, 24 B of results (40 B with the average) and the gathered dof list, geometry record and nodal values.
Part 2, the step: ms per step with the coupling switched on and off from step to step (a force 1e-6 times the scalar, so
  both variants follow the same flow), ``buoyancy_assemble`` split out."""
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
    eps = 1e-6
    scalars = [ox.ScalarTransport("T", schmidt=1.0, initial=ini, bcs=[ox.DirichletBC(1.0, G, left)], buoyancy=(0.0, 0.0, eps))]
    scalars += [ox.ScalarTransport(f"g{i}", schmidt=0.5, initial=ini, bcs=[ox.DirichletBC(float(i), G, left)],
                                   buoyancy=(eps * (i + 1), -eps, eps)) for i in range(3)]
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
    ap.add_argument("--warmup", type=int, default=4, help="warm-up steps (coupling on)")
    ap.add_argument("--reps", type=int, default=20, help="timed launches per kernel variant")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import oasisx_amd as ox
    from oasisx_amd import _lib
    from oasisx_amd import scalar as _sc

    S, W, clk = build(a.N)
    dt, nu = W["dt"], W["nu"]
    one = next(g for g in S._scalar_groups if g.nc == 1)
    three = next(g for g in S._scalar_groups if g.nc == 3)
    for _ in range(a.warmup):
        clk["t"] += dt
        S.solve(dt, nu, max_iter=1)
    torch.cuda.synchronize()

    # ---- part 1: the kernels ---------------------------------------------------------------------------------------
    lib, st = _lib.load(), _lib.current_stream()
    P = S._M.pattern
    n, gdim = S._n_u, S._gdim
    dictionary = S._M.vcode is not None
    launches = {1: _sc.buoyancy_terms([one]), 3: _sc.buoyancy_terms([three])}
    assert [len(L) for L in launches.values()] == [1, 1] and len(launches[3][0][0]) == 3
    coefs = {nt: [[L[0][0][t].coef[i] for i in range(gdim)] for t in range(nt)] for nt, L in launches.items()}
    b = torch.zeros_like(S._BFIRST.rdev())
    tmp = {g.nc: (torch.zeros_like(g.C1.rdev()), torch.zeros_like(g.C1.rdev())) for g in (one, three)}
    x1, y1 = torch.ones(n, 1, dtype=torch.float64, device=b.device), torch.zeros(n, 1, dtype=torch.float64, device=b.device)

    first_order = (_lib.ox_buoy_term * 1)(launches[1][0][0][0])
    first_order[0].c2 = None

    def fused(nt, arr=None):
        arr = launches[nt][0][0] if arr is None else arr
        _lib.check(lib.ox_buoyancy_rows(S._M.ref(), gdim, len(arr), arr, _lib.ptr(b), st), "ox_buoyancy_rows")

    def composed(nt):
        g = one if nt == 1 else three
        cs, y = tmp[g.nc]
        _lib.check(lib.ox_axpby(n * g.nc, 1.5, g.C1.rptr(), -0.5, g.C2.rptr(), _lib.ptr(cs), st), "ox_axpby")
        S._M.mult(cs, y, g.nc)
        for t in range(nt):
            for i in range(gdim):
                if coefs[nt][t][i] != 0.0:
                    b[:, i].add_(y[:, t], alpha=coefs[nt][t][i])

    def rows_bytes(nt):
        live = sum(1 for i in range(gdim) if any(coefs[nt][t][i] != 0.0 for t in range(nt)))
        nc = 1 if nt == 1 else 3
        return int(P.size) * (4 + (1 if dictionary else 8)) + int(P.n_rows) * (2 * 8 * nc + 16 * live)

    flux = ox.ScalarFlux(S, "T")
    Vi = S._Vi[0][0]
    nd, gs = 10, 10  # P2 tetrahedron: dofs per cell, doubles of a geometry record

    def flux_kernel(weight):
        _lib.check(lib.ox_scalar_flux(Vi.degree, C.byref(S._cells), _lib.ptr(Vi.cell_dofs), flux.n_facets, _lib.ptr(flux._rec),
                                      one.C.rptr(), one.nc, 0, 0.01, weight, _lib.ptr(flux._q), _lib.ptr(flux._fq),
                                      _lib.ptr(flux._cbar), _lib.ptr(flux._acc), st), "ox_scalar_flux")

    variants = {"buoyancy_rows_1": lambda: fused(1), "composed_1": lambda: composed(1),
                "buoyancy_rows_1_first_order": lambda: fused(1, first_order),
                "buoyancy_rows_3": lambda: fused(3), "composed_3": lambda: composed(3),
                "mass_product_1": lambda: S._M.mult(x1, y1, 1),
                "scalar_flux": lambda: flux_kernel(0.0), "scalar_flux_average": lambda: flux_kernel(dt),
                "flux_sample": lambda: flux.sample(0.0, nu)}
    ev = {k: [] for k in variants}
    for r in range(a.reps + 3):
        for k, fn in variants.items():
            ev[k].append(timed(torch, fn))
        flux._times.clear()  # (the ring is not what is timed)
    torch.cuda.synchronize()
    nbytes = {"buoyancy_rows_1": rows_bytes(1), "buoyancy_rows_3": rows_bytes(3),
              "buoyancy_rows_1_first_order": rows_bytes(1) - int(P.n_rows) * 8,
              "mass_product_1": int(P.size) * (4 + (1 if dictionary else 8)) + int(P.n_rows) * 16,
              "scalar_flux": flux.n_facets * (8 + 24 + nd * 4 + gs * 8 + nd * 8),
              "scalar_flux_average": flux.n_facets * (8 + 40 + nd * 4 + gs * 8 + nd * 8)}
    kern = {}
    for k, pairs in ev.items():
        ms = statistics.median(x.elapsed_time(y) for x, y in pairs[3:])
        kern[k] = {"ms": round(ms, 4)}
        if k in nbytes:
            kern[k]["bytes"] = nbytes[k]
            kern[k]["fraction_of_hbm_peak"] = round(nbytes[k] / (ms * 1e-3) / HBM_PEAK, 4)
    for nt in (1, 3):
        kern[f"composed_over_fused_{nt}"] = round(kern[f"composed_{nt}"]["ms"] / kern[f"buoyancy_rows_{nt}"]["ms"], 3)

    # ---- part 2: whole steps, coupling on and off alternating ------------------------------------------------------
    phase = []
    inner = S.buoyancy_assemble

    def wrapped():
        phase.append(timed(torch, inner))

    S.buoyancy_assemble = wrapped
    coupled = S._buoyancy
    assert len(coupled) == 2  # four coupled scalars: launches of 3 + 1 terms
    sets = {"uncoupled": [], "coupled": coupled}
    rec = {k: {"step": [], "buoyancy": []} for k in sets}
    for i in range(a.steps + 1):
        for k, launches_ in sets.items():
            S._buoyancy = launches_
            phase.clear()
            clk["t"] += dt
            e = timed(torch, lambda: S.solve(dt, nu, max_iter=1))
            torch.cuda.synchronize()
            if i == 0:
                continue
            rec[k]["step"].append(e[0].elapsed_time(e[1]))
            rec[k]["buoyancy"].append(sum(x.elapsed_time(y) for x, y in phase))
    steps = {k: {"ms_per_step": round(statistics.median(v["step"]), 3),
                 "min_ms": round(min(v["step"]), 3), "max_ms": round(max(v["step"]), 3),
                 "buoyancy_assemble_ms": round(statistics.median(v["buoyancy"]), 4)} for k, v in rec.items()}
    out = {"N": a.N, "rows_u": int(P.n_rows), "entry_slots": int(P.size), "value_dictionary": dictionary,
           "facets": int(flux.n_facets), "scalars": 4, "coupled_terms_per_step": 4, "kernel": kern, "steps": steps}
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
