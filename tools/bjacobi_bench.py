"""pc_type bjacobi + sub_pc_type gamg on the partitioned pressure solve of FractionalStep_AB_CN (TG 3-D P2-P1, rtol 1e-8,
warm start).

    python tools/bjacobi_bench.py [--sizes 32,64] [--steps 5] [--per-rank-n 128] [--ranks 8] [--out FILE]

(a) Pressure iterations per step on the 2 x 2 x 2 split, run as 8 rank threads on one GPU (tests/helpers.run_rank_threads):
    bjacobi + gamg and jacobi on the split, one-GPU gamg on the same mesh.
(b) Rank 0 of the 8-rank job at --per-rank-n alone on a self-loop plan (parallel.SelfLoopComm, as
    tools/selfloop_cg_trace.py): the time of one pressure-CG iteration (bjacobi + gamg and jacobi), of the rank's local
    V-cycle, and the local set-up time.
The last line is a PREDICTION, not a measurement: iterations (extrapolated from (a)) times the per-rank iteration time
of (b).  No multi-GPU node has run this code.  One JSON line per record on stdout (and in --out)."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KSP = {"ksp_rtol": 1e-8, "ksp_atol": 1e-14, "ksp_max_it": 10000, "ksp_initial_guess_nonzero": True}
PRESSURE = {"jacobi": dict(KSP, ksp_type="cg", pc_type="jacobi"), "gamg": dict(KSP, ksp_type="cg", pc_type="gamg"),
            "bjacobi": dict(KSP, ksp_type="cg", pc_type="bjacobi", sub_pc_type="gamg")}


def _solver(mesh, pc):
    import numpy as np

    import oasisx_amd as ox
    from oracle import ipcs_oracle as O

    nu, dt = 0.01, 0.005
    clock = {"t": 0.0}
    on = lambda x: np.isclose(np.abs(x[0]), 1.0) | np.isclose(np.abs(x[1]), 1.0) | np.isclose(np.abs(x[2]), 1.0)
    fns = [O.tg_u, O.tg_v, O.tg_w]
    bcs = [[ox.DirichletBC(lambda x, f=f: f(x, clock["t"], nu), ox.LocatorMethod.GEOMETRICAL, on)] for f in fns]
    so = {"tentative": dict(KSP, ksp_type="bcgs", pc_type="jacobi"), "pressure": PRESSURE[pc],
          "scalar": dict(KSP, ksp_type="cg", pc_type="jacobi")}
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_u=bcs, bcs_p=[], solver_options=so,
                                options={})
    for i, f in enumerate(fns):
        S._u2[i].interpolate(lambda x, f=f: f(x, -dt, nu))
        S._u1[i].interpolate(lambda x, f=f: f(x, 0.0, nu))
    S._p.interpolate(lambda x: O.tg_p(x, -dt / 2, nu))
    return S, clock, nu, dt


def _steps(comm, N, pc, steps):
    import torch

    from oasisx_amd import mesh as M

    mesh = M.create_box(comm, [[-1.0] * 3, [1.0] * 3], [N, N, N])
    S, clock, nu, dt = _solver(mesh, pc)
    its = []
    for _ in range(steps):
        clock["t"] += dt
        S.solve(dt, nu, max_iter=1)
        its.append(int(S.iteration_counts()["pressure"][0]))
    torch.cuda.synchronize()
    return its, S


def iterations(N, steps, ranks):
    from tests.helpers import run_rank_threads

    out = {"record": "iterations", "N": N, "ranks": ranks, "steps": steps}
    for pc in ("bjacobi", "jacobi"):
        t0 = time.perf_counter()
        res, _ = run_rank_threads(ranks, lambda comm, pc=pc: _steps(comm, N, pc, steps)[0], timeout_s=1200.0)
        assert all(r == res[0] for r in res), res
        out[f"{pc}_{ranks}ranks"] = res[0]
        out[f"{pc}_wall_s"] = round(time.perf_counter() - t0, 1)
    its, S = _steps(None, N, "gamg", steps)
    out["gamg_1gpu"] = its
    out["pressure_rows"] = int(S._Ap.pattern.n_rows)
    return out


def per_rank(N, ranks, reps=3, its=200):
    import numpy as np
    import torch

    from oasisx_amd import mesh as M
    from oasisx_amd.fem import FieldStorage
    from oasisx_amd.ksp import KSPSolver
    from oasisx_amd.parallel import SelfLoopComm

    comm = SelfLoopComm(0, ranks, "p2p")
    mesh = M.create_box(comm, [[-1.0] * 3, [1.0] * 3], [N, N, N])
    S, _, _, _ = _solver(mesh, "jacobi")
    Q, A = S._Q, S._Ap
    n = Q.n_local
    B, X = FieldStorage(n, 1, "cuda"), FieldStorage(n, 1, "cuda")
    B.dev()[:n, 0] = torch.from_numpy(np.random.default_rng(0).standard_normal(n)).cuda()
    out = {"record": "per_rank", "N": N, "ranks": ranks, "rank": 0, "transport": "p2p self-loop",
           "owned_rows": int(Q.n_owned), "ghost_rows": int(n - Q.n_owned)}
    for pc in ("bjacobi", "jacobi"):
        # (forced iterations: on the self-loop plan the operator is not the job's, so no divergence test either)
        ksp = KSPSolver(comm, dict(PRESSURE[pc], ksp_rtol=0.0, ksp_atol=0.0, ksp_max_it=its, ksp_divtol=1e300,
                                   ksp_initial_guess_nonzero=False))
        ksp.setOperators(A)
        if pc == "bjacobi":
            t0 = time.perf_counter()
            H = ksp._hierarchy()
            out["setup_s"] = round(time.perf_counter() - t0, 3)
            out["setup_host_s"] = round(H.setup_host_s, 3)
            out["levels"] = H.rows
            out["cycle_kernels"] = H.kernels_per_cycle()
            r = torch.randn(Q.n_owned, dtype=torch.float64, device="cuda")
            z = torch.empty_like(r)
            for _ in range(5):
                H.apply(r, z)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(100):
                H.apply(r, z)
            e1.record()
            torch.cuda.synchronize()
            out["vcycle_us"] = round(1e3 * e0.elapsed_time(e1) / 100, 1)
        best = None
        for _ in range(reps):
            X.dev().zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ksp.solve_block(B, X)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / max(1, ksp.iterations[0])
            best = dt if best is None else min(best, dt)
        out[f"{pc}_timed_iterations"] = int(ksp.iterations[0])
        out[f"{pc}_iteration_us"] = round(1e6 * best, 1)
        out[f"{pc}_kernels_per_iteration"] = int(ksp._cg_kernels_per_iteration())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32,64")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--per-rank-n", type=int, default=128)
    ap.add_argument("--skip", default="", help="iterations,per_rank")
    ap.add_argument("--its-from", default=None, help="take the (a) records from this file (with --skip iterations)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(r) + "\n")

    if a.out and os.path.exists(a.out):
        os.remove(a.out)
    its = {}
    if a.its_from:
        with open(a.its_from) as f:
            for line in f:
                r = json.loads(line)
                if r.get("record") == "iterations":
                    its[r["N"]] = r
                    emit(r)
    if "iterations" not in a.skip:
        for N in (int(v) for v in a.sizes.split(",")):
            r = iterations(N, a.steps, a.ranks)
            its[N] = r
            emit(r)
    if "per_rank" not in a.skip:
        pr = per_rank(a.per_rank_n, a.ranks)
        emit(pr)
        if len(its) >= 2:
            # PREDICTION: the iteration count at per_rank_n extrapolated from the two largest sizes of (a) (the ratio
            # per doubling of N kept), times the per-rank iteration time of (b); no exchange or all-reduce latency
            # between GPUs is in (b)
            n1, n2 = sorted(its)[-2:]
            pred = {"record": "PREDICTION (not a measurement)", "N": a.per_rank_n, "ranks": a.ranks,
                    "basis": f"iterations from N={n1},{n2} extrapolated by their ratio per doubling; "
                             f"time per iteration of rank 0 on its self-loop plan"}
            for pc in ("bjacobi", "jacobi"):
                k1 = sum(its[n1][f"{pc}_{a.ranks}ranks"]) / a.steps
                k2 = sum(its[n2][f"{pc}_{a.ranks}ranks"]) / a.steps
                k = k2 * (k2 / k1) ** (math.log2(a.per_rank_n / n2) / math.log2(n2 / n1))
                pred[f"{pc}_iterations"] = round(k, 1)
                pred[f"{pc}_pressure_ms_per_step"] = round(k * pr[f"{pc}_iteration_us"] / 1e3, 2)
            emit(pred)


if __name__ == "__main__":
    main()
