"""Slab-averaged statistics at the bench size: Taylor-Green 128^3, P2-P1, periodic in all three axes (the periodic set-up
of tools/periodic_bench.py, plus one transported scalar), slabs along axis 1.  HIP events, warm, medians, the variants
alternating inside the timed loops.

    python tools/profile_bench.py [-N 128] [--steps 12] [--warmup 4] [--reps 20] [--out profiles/profile_bench_128.json]
                                  [--bench-trees this=DIR parent=DIR] [--bench-runs 2]

Part 1, the kernels, launch after launch, alternating: ``ox_profile_cells`` and ``ox_profile_update`` for ``u`` (NQ = 3),
for ``u`` + one scalar (NQ = 4) and for ``p`` (NQ = 1, the pressure space), beside ``ox_flow_cells`` (sums only) on the same
mesh: the same three streams -- dof list, geometry record, u once per dof -- plus a quadrature loop there, a permutation
and the second moments here.  Bytes from the stored sizes (the geometry record counted whole: the kernel reads 8 of its
80 bytes, the lines come in full), the share of the HBM peak as in tools/diagnostics_bench.py, and how many chunks hold
consecutive cells (the permutation is then the identity inside the chunk: its loads coalesce as those of ox_flow_cells).
Part 2, whole steps, alternating: without and with ``ProfileStatistics.sample`` (u + scalar, p) after every step.
Part 3 (``--bench-trees``): ``bench.py --gpus 1 --steps 20 --warmup 5`` as child processes in the given source trees (this
commit, the parent commit), alternating: the default step makes none of the new calls."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.viscosity_bench import HBM_PEAK, bench_trees, timed  # noqa: E402


def build(N):
    """tools/periodic_bench.py's periodic set-up with one scalar."""
    import numpy as np
    import torch

    import oasisx_amd as ox
    from bench import make_workload
    from oasisx_amd import mesh as M

    W = make_workload("tg", N, np, torch)
    q0, q1 = W["box"]
    clk = {"t": 0.0}

    def at(f, t):
        def g(x):
            return f(x, clk["t"] if t is None else t)
        g.supports_torch = True
        return g

    mesh = M.make_periodic(M.create_box(None, [q0, q1], [N, N, N]), (0, 1, 2))
    ksp = {"pc_type": "jacobi", "ksp_rtol": 1e-8, "ksp_atol": 1e-14, "ksp_max_it": 10000, "ksp_initial_guess_nonzero": True}
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_u=[[], [], []], bcs_p=[],
                                solver_options={"tentative": dict(ksp, ksp_type="bcgs"), "pressure": dict(ksp, ksp_type="cg"),
                                                "scalar": dict(ksp, ksp_type="cg")},
                                options={"low_memory_version": False, "value_dictionary": True},
                                scalars=[ox.ScalarTransport("T", diffusivity=W["nu"])])
    for i, f in enumerate(W["fns"]):
        S._u2[i].interpolate(at(f, -W["dt"]))
        S._u1[i].interpolate(at(f, 0.0))
    S._p.interpolate(lambda x: W["p"](x, -W["dt"] / 2.0))
    for level in (0, 1):
        S.scalar("T", level).interpolate(at(W["fns"][0], 0.0))
    return S, W, clk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-N", type=int, default=128)
    ap.add_argument("--steps", type=int, default=12, help="timed steps per variant")
    ap.add_argument("--warmup", type=int, default=4, help="warm-up steps")
    ap.add_argument("--reps", type=int, default=20, help="timed launches per kernel variant")
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-trees", nargs="*", default=[], metavar="LABEL=DIR",
                    help="source trees to run bench.py's default line in, e.g. this=. parent=../parent")
    ap.add_argument("--bench-runs", type=int, default=2)
    a = ap.parse_args()
    import ctypes as C

    import torch

    import oasisx_amd as ox
    from oasisx_amd import _lib

    # part 3 first: the children have the device to themselves (this process has not touched it yet)
    bench = bench_trees(a.bench_trees, a.bench_runs) if a.bench_trees else None
    S, W, clk = build(a.N)
    dt, nu = W["dt"], W["nu"]
    for _ in range(a.warmup):
        clk["t"] += dt
        S.solve(dt, nu, max_iter=1)
    torch.cuda.synchronize()
    Vi, Q, d = S._Vi[0][0], S._Q, S._gdim
    ncells, nd, ndq, gs = int(S._geom.shape[0]), int(Vi.cell_dofs.shape[1]), int(Q.cell_dofs.shape[1]), int(S._geom.shape[1])
    n_u, n_q = int(S._n_u), int(S._n_q)
    Pu = ox.ProfileStatistics(S, axis=1, fields=("u",))
    Put = ox.ProfileStatistics(S, axis=1, fields=("u", "p"), scalars=("T",))
    for P in (Pu, Put):
        P.sample(dt)  # (the timed launches run about a running mean)
    D = ox.FlowDiagnostics(S)
    gu, gut, gp = Pu._groups[0], Put._groups[0], Put._groups[1]
    assert (gu.nq, gut.nq, gp.nq) == (d, d + 1, 1)

    def pair(P, g):
        return (lambda: P._cells(g, g.sources, g.mean),
                lambda: P._update(g, g.mean, dt, P.total_weight, False, g.mean, g.m2, P._vol))

    lib, st = _lib.load(), _lib.current_stream()

    def flow_cells():
        _lib.check(lib.ox_flow_cells(Vi.degree, C.byref(S._cells), _lib.ptr(Vi.cell_dofs), S._U.rptr(), _lib.ptr(S._nut), dt, nu,
                                     None, None, _lib.ptr(D._partials), st), "ox_flow_cells")

    variants = {"flow_cells_sums_only": flow_cells}
    for label, P, g in (("u", Pu, gu), ("u_T", Put, gut), ("p", Put, gp)):
        variants[f"profile_cells_{label}"], variants[f"profile_update_{label}"] = pair(P, g)
    ev = {k: [] for k in variants}
    for _ in range(a.reps + 3):
        for k, fn in variants.items():
            ev[k].append(timed(torch, fn))
    torch.cuda.synchronize()
    nch, nb = Pu.n_chunks, Pu.n_bins

    def cell_bytes(nd_, n_rows, nq):
        nr = 1 + nq + nq * (nq + 1) // 2
        return ncells * (nd_ * 4 + gs * 8 + 4) + n_rows * nq * 8 + nch * (16 + nr * 8)

    def update_bytes(nq):
        nr = 1 + nq + nq * (nq + 1) // 2
        return nch * nr * 8 + nb * (4 + 8 + 8 * (3 * nq + 2 * (nr - 1 - nq)))

    nbytes = {"flow_cells_sums_only": ncells * (nd * 4 + gs * 8) + n_u * d * 8 + D.n_blocks * 64,
              "profile_cells_u": cell_bytes(nd, n_u, d), "profile_cells_u_T": cell_bytes(nd, n_u, d + 1),
              "profile_cells_p": cell_bytes(ndq, n_q, 1), "profile_update_u": update_bytes(d),
              "profile_update_u_T": update_bytes(d + 1), "profile_update_p": update_bytes(1)}
    kern = {}
    for k, pairs in ev.items():
        ms = [x.elapsed_time(y) for x, y in pairs[3:]]
        med = statistics.median(ms)
        kern[k] = {"ms": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4), "bytes": nbytes[k],
                   "bytes_per_s": round(nbytes[k] / (med * 1e-3), 1),
                   "fraction_of_hbm_peak": round(nbytes[k] / (med * 1e-3) / HBM_PEAK, 4)}
    kern["profile_cells_u"]["over_flow_cells"] = round(kern["profile_cells_u"]["ms"] / kern["flow_cells_sums_only"]["ms"], 3)

    # ---- part 2: whole steps, alternating ---------------------------------------------------------------------------------
    Put.reset()
    rec = {"plain": [], "sampling": []}
    for i in range(a.steps + 1):
        for key in rec:
            clk["t"] += dt

            def step():
                S.solve(dt, nu, max_iter=1)
                if key == "sampling":
                    Put.sample(dt)

            e = timed(torch, step)
            torch.cuda.synchronize()
            if i:
                rec[key].append(e[0].elapsed_time(e[1]))
    steps = {k: {"ms_per_step": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
             for k, v in rec.items()}
    ch = Pu._chunks
    out = {"N": a.N, "device": torch.cuda.get_device_name(0), "cells": ncells, "rows_u": n_u, "rows_p": n_q, "bins": nb,
           "chunks": nch, "chunks_of_consecutive_cells": int(ch[:, 3].sum()), "cells_per_chunk_mean": round(ncells / nch, 2),
           "order_is_identity": bool(torch.equal(Pu._order.to(torch.int64), torch.arange(ncells, device=ch.device))),
           "nu": nu, "dt": dt, "reps": a.reps, "kernel": kern, "steps": steps,
           "profile_after_timed_steps": {"tke_max": float(Put.tke().max()), "volume": float(Put.volume().sum()),
                                         "samples": Put.n_samples}}
    if bench is not None:
        out["bench_default_steps_per_s"] = bench
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
