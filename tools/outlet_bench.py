"""Outlet models at the bench size (Taylor-Green 128^3, P2-P1, rtol 1e-8, warm start; the side x = max of the box as
outlet: 32 768 facets, Dirichlet velocity on the other five sides; the Taylor-Green field plus a uniform through-flow
(THROUGH, 0, 0), so that the open side carries a net outflow while the flow still re-enters on half of it): HIP events,
medians, the variants alternating.

    python tools/outlet_bench.py [-N 128] [--steps 8] [--warmup 3] [--reps 20] [--out FILE]
                                 [--bench-trees this=DIR parent=DIR] [--bench-runs 2]

Part 1, the three kernels, launch after launch, alternating: ``ox_outlet_flux``, ``ox_outlet_update`` (one tag with a
Windkessel) and ``ox_outlet_backflow``.  Bytes moved per launch from the stored sizes: flux -- per facet the record (8 B),
the cell's dof list (nd x 4 B), the geometry record and the result (8 B), the gathered velocities once per distinct dof;
update -- the fluxes, the dof list and h on the outlet's pressure dofs; backflow -- per row its list entry and pointers
(12 B) and b_first read and written, per (row, facet) pair the pair's two indices and nfd slots (8 + nfd x 8 B), the
facet's record, beta, geometry and facet dofs, nfd values of A read and written, the gathered u_ab and u1 once per
distinct dof.
Part 2, whole steps of three solvers, alternating: a float outlet, a Windkessel, a Windkessel with backflow = 0.5.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_PEAK = 8.0e12  # B/s
OUTLET = 7
THROUGH = 0.5


def build(N, value, beta):
    """The bench workload with the side x = max open: (solver, workload, clock)."""
    import numpy as np
    import torch

    import oasisx_amd as ox
    from bench import make_workload
    from oasisx_amd import mesh as M

    W = make_workload("tg", N, np, torch)
    q0, q1 = W["box"]
    clk = {"t": 0.0}

    def on_five(x):
        on = np.isclose(x[0], q0[0])
        for k in (1, 2):
            on |= np.isclose(x[k], q0[k]) | np.isclose(x[k], q1[k])
        return on

    def at(f, t, shift=0.0):
        def g(x):
            return f(x, clk["t"] if t is None else t) + shift
        g.supports_torch = True
        return g

    mesh = M.create_box(None, [q0, q1], [N, N, N])
    right = M.locate_entities_boundary(mesh, 2, lambda x: np.isclose(x[0], q1[0]))
    tags = M.meshtags(mesh, 2, np.sort(right), np.full(right.shape, OUTLET, dtype=np.int32))
    ksp = {"pc_type": "jacobi", "ksp_rtol": 1e-8, "ksp_atol": 1e-14, "ksp_max_it": 10000, "ksp_initial_guess_nonzero": True}
    G = ox.LocatorMethod.GEOMETRICAL
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1),
                                bcs_u=[[ox.DirichletBC(at(f, None, THROUGH if i == 0 else 0.0), G, on_five)]
                                       for i, f in enumerate(W["fns"])],
                                bcs_p=[ox.PressureBC(value, (tags, OUTLET), backflow=beta)],
                                solver_options={"tentative": dict(ksp, ksp_type="bcgs"), "pressure": dict(ksp, ksp_type="cg"),
                                                "scalar": dict(ksp, ksp_type="cg")}, options={})
    for i, f in enumerate(W["fns"]):
        S._u2[i].interpolate(at(f, -W["dt"], THROUGH if i == 0 else 0.0))
        S._u1[i].interpolate(at(f, 0.0, THROUGH if i == 0 else 0.0))
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

    # part 3 first: the children have the device to themselves (this process has not touched it yet)
    bench = bench_trees(a.bench_trees, a.bench_runs) if a.bench_trees else None
    # small resistances: the model's pressure stays within 1e-2 of the zero pressure of the float run, whose initial
    # pressure on the outlet the step never corrects (dp = 0 there): the three runs solve nearly the same flow and differ
    # in the launches priced here.  (Rp = 0.5, Rd = 4 against that initial pressure diverged in the second step.)
    wk = dict(Rp=1e-3, C=1.0, Rd=1e-2)
    solvers = {"float": build(a.N, 0.0, 0.0), "windkessel": build(a.N, ox.Windkessel(**wk), 0.0),
               "windkessel_backflow": build(a.N, ox.Windkessel(**wk), 0.5)}
    dt, nu = solvers["float"][1]["dt"], solvers["float"][1]["nu"]
    failed = {}

    def step(k):
        """One step of solver k; a failed Krylov solve takes the variant out of the timed loops (and is reported)."""
        Sk, _, clk = solvers[k]
        clk["t"] += dt
        try:
            Sk.solve(dt, nu, max_iter=1)
        except AssertionError as e:
            failed[k] = f"t = {clk['t']:.4f}: {e}"
            print(f"{k}: {failed[k]}", file=sys.stderr, flush=True)

    for k in solvers:
        for _ in range(a.warmup):
            if k not in failed:
                step(k)
    torch.cuda.synchronize()

    # ---- part 1: the kernels (the solver with both) -------------------------------------------------------------------
    S = solvers["windkessel_backflow"][0]
    if "windkessel_backflow" in failed:  # (the kernels' cost does not depend on the field: time them on the initial one)
        S = build(a.N, ox.Windkessel(**wk), 0.5)[0]
    S.assemble_first(dt, nu)
    G, B = S._outlet_models, S._outlet_backflow
    Vi = S._Vi[0][0]
    d, nd, gs = S._gdim, int(Vi.cell_dofs.shape[1]), int(S._geom.shape[1])
    nf = G._set.n_facets

    def update():
        G._times.clear()  # slot 0 again: the timed launches do not grow the ring
        G.advance(dt)

    variants = {"outlet_flux": lambda: G._set.launch_flux(S, S._U1.rptr()), "outlet_update": update, "outlet_backflow": B.add}
    ev = {k: [] for k in variants}
    state = G._state.clone()
    for r in range(a.reps + 3):
        for k, fn in variants.items():
            ev[k].append(timed(torch, fn))
    torch.cuda.synchronize()
    G._state.copy_(state)
    cells = torch.from_numpy(np.unique(G._set.kpos)).to(Vi.cell_dofs.device).long()
    vdofs = int(torch.unique(Vi.cell_dofs[cells]).shape[0])
    n_pairs, nfd = int(B.pair_facet.shape[0]), B.nfd
    fdofs = int(B.n_rows)  # the distinct dofs on the facets are the touched rows
    nbytes = {"outlet_flux": nf * (8 + nd * 4 + gs * 8 + 8) + vdofs * d * 8,
              "outlet_update": nf * 8 + int(G._dofs.shape[0]) * (4 + 8) + 64,
              "outlet_backflow": B.n_rows * (12 + 2 * d * 8) + n_pairs * (8 + nfd * 8 + 8 + 8 + gs * 8 + nfd * 4 + nfd * 16)
              + 2 * fdofs * d * 8}
    kern = {}
    for k, pairs in ev.items():
        ms = statistics.median(x.elapsed_time(y) for x, y in pairs[3:])
        kern[k] = {"ms": round(ms, 4), "bytes": int(nbytes[k]), "fraction_of_hbm_peak": round(nbytes[k] / (ms * 1e-3) / HBM_PEAK, 5)}

    # ---- part 2: whole steps, alternating -----------------------------------------------------------------------------
    rec_t = {k: [] for k in solvers}
    for i in range(a.steps + 1):
        for k in solvers:
            if k in failed:
                continue
            e = timed(torch, lambda: step(k))
            torch.cuda.synchronize()
            if i > 0 and k not in failed:
                rec_t[k].append(e[0].elapsed_time(e[1]))
    steps = {k: (round(statistics.median(v), 4) if v else None) for k, v in rec_t.items()}
    H = S._bcs_p[0]._model.history()
    out = {"N": a.N, "facets": nf, "outlet_pressure_dofs": int(G._dofs.shape[0]), "backflow_rows": B.n_rows,
           "backflow_pairs": n_pairs, "nu": nu, "dt": dt, "kernel": kern, "step_ms": steps, "failed": failed,
           "umax": {k: float(Sk._U.rdev().abs().max()) for k, (Sk, _, _) in solvers.items()},
           "iterations": {k: Sk.iteration_counts() for k, (Sk, _, _) in solvers.items()},
           "last_Q_P_Pc": [float(H["Q"][-1]), float(H["P"][-1]), float(H["Pc"][-1])]}
    if bench is not None:
        out["bench_default_steps_per_s"] = bench
    print(json.dumps(out, default=str), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1, default=str) + "\n")


if __name__ == "__main__":
    main()
