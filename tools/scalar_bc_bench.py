"""Flux and Robin conditions of a scalar at the bench size (Taylor-Green 128^3, P2-P1, rtol 1e-8, warm start, one scalar
with Sc = 1 beside the bench's velocity): HIP events, medians of ``--reps`` launches, the variants alternating.

    python tools/scalar_bc_bench.py [-N 128] [--steps 8] [--warmup 3] [--reps 20] [--out FILE]
                                    [--bench-trees this=DIR parent=DIR] [--bench-runs 2]

Part 1, the kernels, launch after launch, alternating, on one face (x = max, 2 N^2 facets) and on all six faces:
``ox_scalar_boundary`` in its three instances (FluxBC only; RobinBC; RobinBC with an advective part) beside
``ox_outlet_backflow`` on the same facets and beside ``ox_scalar_rows`` of the same group.  Bytes moved per launch of
the boundary pass from the stored sizes: per row its list entry and pointers (12 B) and nc values of b_c read and
written; per (row, facet) pair the pair's two indices (8 B), the facet's record (8 B) and geometry record, the nodal q
(nfd x nc x 8 B); a Robin pass adds per pair nfd slots
(8 B each), nfd values of A_c read and written, the facet's dofs (nfd x 4 B), h and c_inf, and c_1 once per distinct dof;
the advective instance adds beta and u_ab once per distinct dof.
Part 2, whole steps of two solvers, alternating: the scalar without conditions, and with a RobinBC(advective=1) on all
six faces.
Part 3 (``--bench-trees``): ``bench.py --gpus 1 --steps 20 --warmup 5`` as child processes in the given source trees
(this commit, the parent commit), alternating: the default step makes no new call and must not change."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_PEAK = 8.0e12  # B/s


def build(N, conditions):
    """The bench workload with one scalar; ``conditions(mesh) -> flux_bcs``."""
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
    sc = ox.ScalarTransport("c", schmidt=1.0, initial=1.0, flux_bcs=conditions(mesh))
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1),
                                bcs_u=[[ox.DirichletBC(at(f, None), G, on_bnd)] for f in W["fns"]], bcs_p=[],
                                solver_options={"tentative": dict(ksp, ksp_type="bcgs"), "pressure": dict(ksp, ksp_type="cg"),
                                                "scalar": dict(ksp, ksp_type="cg"), "scalar_transport": dict(ksp, ksp_type="bcgs")},
                                options={}, scalars=[sc])
    for i, f in enumerate(W["fns"]):
        S._u2[i].interpolate(at(f, -W["dt"]))
        S._u1[i].interpolate(at(f, 0.0))
    S._p.interpolate(lambda x: W["p"](x, -W["dt"] / 2.0))
    return S, W, clk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-N", type=int, default=128)
    ap.add_argument("--steps", type=int, default=8, help="timed steps per variant")
    ap.add_argument("--warmup", type=int, default=3, help="warm-up steps per solver")
    ap.add_argument("--reps", type=int, default=20, help="timed launches per kernel")
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-trees", nargs="*", default=[], metavar="LABEL=DIR",
                    help="source trees to run bench.py's default line in, e.g. this=. parent=../parent")
    ap.add_argument("--bench-runs", type=int, default=2)
    a = ap.parse_args()
    import numpy as np
    import torch
    from viscosity_bench import bench_trees, timed

    import oasisx_amd as ox
    from oasisx_amd import _lib
    from oasisx_amd import mesh as M
    from oasisx_amd import scalar as sc_mod
    from oasisx_amd.outlet import Backflow

    # part 3 first: the children have the device to themselves (this process has not touched it yet)
    bench = bench_trees(a.bench_trees, a.bench_runs) if a.bench_trees else None

    def six(mesh):
        return [ox.RobinBC(0.0, 0.0, None, advective=1.0)]

    solvers = {"plain": build(a.N, lambda mesh: []), "robin_six_faces": build(a.N, six)}
    dt, nu = solvers["plain"][1]["dt"], solvers["plain"][1]["nu"]

    def step(k):
        Sk, _, clk = solvers[k]
        clk["t"] += dt
        Sk.solve(dt, nu, max_iter=1)

    for k in solvers:
        for _ in range(a.warmup):
            step(k)
    torch.cuda.synchronize()

    # ---- part 1: the kernels, on the tables of the solver with conditions --------------------------------------------
    S, W, _ = solvers["robin_six_faces"]
    q1 = W["box"][1]
    mesh = S._mesh
    g = S._scalar_groups[0]
    Vi = S._Vi[0][0]
    d, gs, nc = S._gdim, int(S._geom.shape[1]), g.nc
    S.assemble_first(dt, nu)
    faces = {"one_face": np.sort(np.asarray(M.locate_entities_boundary(mesh, 2, lambda x: np.isclose(x[0], q1[0])), dtype=np.int64)),
             "six_faces": np.sort(np.asarray(mesh.exterior_facets(), dtype=np.int64))}
    lists = {"flux": lambda ids: [ox.FluxBC(1.0, ids)], "robin": lambda ids: [ox.RobinBC(1.0, 0.5, ids)],
             "robin_advective": lambda ids: [ox.RobinBC(1.0, 0.5, ids, advective=1.0)]}

    def scalar_rows():
        _lib.check(S._lib.ox_scalar_rows(S._A.ref(), S._M.ref(), S._K.ref(), g.Ac.ref(), 0.0, float(dt), nc, g.C1.rptr(),
                                         g.B0.rptr(), g.B.ptr(), None, _lib.current_stream()), "ox_scalar_rows")

    variants, nbytes, sizes = {"scalar_rows": scalar_rows}, {}, {}
    pat = Vi.pattern
    nbytes["scalar_rows"] = int(pat.size) * (8 + 8 + 4 + 2) + int(S._n_u) * nc * 8 * 3  # A, A_c, columns, codes; c_1, b0, b_c
    for fk, ids in faces.items():
        bf = Backflow(S, [types.SimpleNamespace(_facets=ids, backflow=0.5)])
        variants[f"outlet_backflow/{fk}"] = bf.add
        n_pairs, nfd = int(bf.pair_facet.shape[0]), bf.nfd
        sizes[fk] = {"facets": int(ids.shape[0]), "rows": bf.n_rows, "pairs": n_pairs}
        nbytes[f"outlet_backflow/{fk}"] = (bf.n_rows * (12 + 2 * d * 8) + n_pairs * (8 + nfd * 8 + 8 + 8 + gs * 8 + nfd * 4 + nfd * 16)
                                            + 2 * bf.n_rows * d * 8)
        for lk, make in lists.items():
            member = ox.ScalarTransport("c", schmidt=1.0, flux_bcs=make(ids))
            shim = types.SimpleNamespace(members=[member], C1=g.C1, Ac=g.Ac, B=g.B)
            bp = sc_mod.BoundaryPass(S, shim, [sc_mod.flux_key(member, mesh)[1]])
            variants[f"scalar_boundary_{lk}/{fk}"] = bp.add
            rows, pairs = bp.pairs.n_rows, bp.pairs.n_pairs
            b = rows * (12 + 2 * nc * 8) + pairs * (8 + 8 + gs * 8 + nfd * nc * 8)
            if bp.robin:
                b += pairs * (nfd * 8 + nfd * 16 + nfd * 4 + nfd * 8 + nfd * nc * 8) + rows * nc * 8
            if bp.adv:
                b += pairs * 8 + rows * d * 8
            nbytes[f"scalar_boundary_{lk}/{fk}"] = b
    ev = {k: [] for k in variants}
    for r in range(a.reps + 3):
        for k, fn in variants.items():
            ev[k].append(timed(torch, fn))
    torch.cuda.synchronize()
    kern = {}
    for k, pairs in ev.items():
        ms = statistics.median(x.elapsed_time(y) for x, y in pairs[3:])
        kern[k] = {"ms": round(ms, 4), "bytes": int(nbytes[k]), "fraction_of_hbm_peak": round(nbytes[k] / (ms * 1e-3) / HBM_PEAK, 5)}

    # ---- part 2: whole steps, alternating -----------------------------------------------------------------------------
    rec_t = {k: [] for k in solvers}
    for i in range(a.steps + 1):
        for k in solvers:
            e = timed(torch, lambda: step(k))
            torch.cuda.synchronize()
            if i > 0:
                rec_t[k].append(e[0].elapsed_time(e[1]))
    steps = {k: round(statistics.median(v), 4) for k, v in rec_t.items()}
    out = {"N": a.N, "nu": nu, "dt": dt, "reps": a.reps, "sizes": sizes, "kernel": kern, "step_ms": steps,
           "step_ms_all": {k: [round(x, 3) for x in v] for k, v in rec_t.items()},
           "iterations": {k: Sk.iteration_counts() for k, (Sk, _, _) in solvers.items()},
           "c_range": {k: [float(Sk._scalar_groups[0].C.rdev().min()), float(Sk._scalar_groups[0].C.rdev().max())]
                       for k, (Sk, _, _) in solvers.items()}}
    if bench is not None:
        out["bench_default_steps_per_s"] = bench
    print(json.dumps(out, default=str), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1, default=str) + "\n")


if __name__ == "__main__":
    main()
