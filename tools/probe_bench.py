"""Point evaluation at sizes a user runs: Taylor-Green 128^3, P2-P1, one GPU.

    python tools/probe_bench.py [-N 128] [--probes 10000] [--steps 20] [--lattice 256] [--reps 5] [--out FILE]

(i)  ``--probes`` random points sampled by ``Probes`` (u and p: two launches) -- 2 x ``--steps`` time steps in one process,
     alternating a plain step and a step followed by ``sample``; reported: the mean of both kinds from device events, their
     difference (added ms per step), the spread (standard deviation) of the plain steps, and the sample calls timed alone.
(ii) the velocity resampled on a uniform ``--lattice``^3 lattice strictly inside the box: locate and evaluate times from
     device events, points/s, and bytes/s over the bytes the evaluation NEEDS, computed from the shapes (per point: cell
     position, barycentric coordinates and permutation in, nd indices and nd rows of 3 doubles read, 3 doubles out), as a
     share of the 8 TB/s peak -- a gather kernel's share, not a target.  The same evaluation written in plain torch (index
     ``cell_dofs``, gather the rows, ``einsum`` with the basis: what a user would write without the library) is timed in
     the same process, alternating, warm, on the same sorted inputs; it is given every advantage (no scatter back to the
     caller's order; timed with and without forming the basis).  ``hip_not_slower_than_torch`` is the one gate.
One JSON line per case on stdout (and appended to --out)."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES_PER_S = 8.0e12


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

    def at(f, t=None):
        def g(x):
            return f(x, clk["t"] if t is None else t)
        g.supports_torch = True
        return g

    mesh = M.create_box(None, [q0, q1], [N, N, N])
    ksp = {"pc_type": "jacobi", "ksp_rtol": 1e-8, "ksp_atol": 1e-14, "ksp_max_it": 10000, "ksp_initial_guess_nonzero": True}
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1),
                                bcs_u=[[ox.DirichletBC(at(f), ox.LocatorMethod.GEOMETRICAL, on_bnd)] for f in W["fns"]],
                                bcs_p=[], solver_options={"tentative": dict(ksp, ksp_type="bcgs"), "pressure": dict(ksp, ksp_type="cg"),
                                                          "scalar": dict(ksp, ksp_type="cg")}, options={})
    for i, f in enumerate(W["fns"]):
        S._u2[i].interpolate(at(f, -W["dt"]))
        S._u1[i].interpolate(at(f, 0.0))
    S._p.interpolate(lambda x: W["p"](x, -W["dt"] / 2.0))
    return S, W, clk, mesh


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    return (e0, e1), r


def case_probes(S, W, clk, mesh, n_probes, steps, warmup):
    import numpy as np
    import torch

    import oasisx_amd as ox

    q0, q1 = np.asarray(W["box"][0]), np.asarray(W["box"][1])
    rng = np.random.default_rng(0)
    x = q0 + (q1 - q0) * (0.001 + 0.998 * rng.random((n_probes, 3)))
    probes = ox.Probes(x, [S.u, S._p], capacity=steps)
    for _ in range(warmup):
        clk["t"] += W["dt"]
        S.solve(W["dt"], W["nu"], max_iter=1)
    plain, probed, alone = [], [], []
    for k in range(2 * steps):
        clk["t"] += W["dt"]
        if k % 2 == 0:
            plain.append(timed(torch, lambda: S.solve(W["dt"], W["nu"], max_iter=1))[0])
        else:
            def both():
                S.solve(W["dt"], W["nu"], max_iter=1)
                alone.append(timed(torch, lambda: probes.sample(clk["t"]))[0])
            probed.append(timed(torch, both)[0])
    torch.cuda.synchronize()
    ms = lambda evs: np.asarray([a.elapsed_time(b) for a, b in evs])  # noqa: E731
    p, q, a = ms(plain), ms(probed), ms(alone)
    vals = probes.array()
    return {"case": "probes", "n_probes": n_probes, "steps_each": steps,
            "values_per_probe": probes.n_values, "plain_step_ms_mean": float(p.mean()), "plain_step_ms_std": float(p.std()),
            "plain_step_ms_min": float(p.min()), "plain_step_ms_max": float(p.max()),
            "probed_step_ms_mean": float(q.mean()), "added_ms_per_step": float(q.mean() - p.mean()),
            "sample_alone_ms_mean": float(a.mean()), "sample_alone_ms_max": float(a.max()),
            "samples": int(vals.shape[0]), "nan": int(np.isnan(vals).sum())}


def case_lattice(S, W, mesh, L, reps):
    import numpy as np
    import torch

    from oasisx_amd import _lib, fem
    from oasisx_amd import geometry as G

    dev = mesh.device
    q0, q1 = W["box"]
    ax = [torch.linspace(q0[k] + 1e-3 * (q1[k] - q0[k]), q1[k] - 1e-3 * (q1[k] - q0[k]), L, dtype=torch.float64, device=dev)
          for k in range(3)]
    X = torch.stack(torch.meshgrid(*ax, indexing="ij"), dim=-1).reshape(-1, 3).contiguous()
    n = int(X.shape[0])
    Vs = G.scalar_space(S.u.function_space)
    import time

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fresh = G.BoundingBoxTree(mesh)  # (creation synchronises: wall clock; space_tree below may be cached by case (i))
    tree_build_ms = (time.perf_counter() - t0) * 1e3
    del fresh
    tree = G.space_tree(Vs)
    ev_find, (cells, bary) = timed(torch, lambda: tree.find(X))
    ev_find2, _ = timed(torch, lambda: tree.find(X))
    ev_plan, plan = timed(torch, lambda: G.PointPlan(Vs, cells, bary))
    missing = int((cells < 0).sum())
    ptr, nc, col, nv = G.field_args(S.u)
    out = torch.empty((n, nv), dtype=torch.float64, device=dev)
    lib, st = _lib.load(), _lib.current_stream()

    def hip():
        _lib.check(lib.ox_eval_points(*plan.args(), ptr, nc, col, _lib.ptr(out), nv, 0, st), "ox_eval_points")

    U = S._U.rdev()
    cd = Vs.cell_dofs
    edges = fem.local_edges(3)

    def basis(lam):  # fem.lagrange_basis, degree 2, in torch
        cols = [lam[:, a] * (2 * lam[:, a] - 1) for a in range(4)] + [4 * lam[:, a] * lam[:, b] for a, b in edges]
        return torch.stack(cols, dim=1)

    def torch_eval(phi=None, chunk=1 << 22):  # chunks: the gathered rows of all points at once are 4 GB
        res = torch.empty((n, nv), dtype=torch.float64, device=dev)
        for p0 in range(0, n, chunk):
            sl = slice(p0, min(n, p0 + chunk))
            ph = basis(plan.bary[sl]) if phi is None else phi[sl]
            rows = U[cd[plan.pos[sl]].to(torch.int64)]  # (m, nd, 3)
            res[sl] = torch.einsum("na,nak->nk", ph, rows)
        return res

    phi_all = basis(plan.bary)
    hip()
    ref = torch_eval()
    torch.cuda.synchronize()
    dev_max = float((out[plan.perm] - ref).abs().max()) if missing == 0 else float("nan")
    t_hip, t_torch, t_torch_nb = [], [], []
    for _ in range(reps):
        t_hip.append(timed(torch, hip)[0])
        t_torch.append(timed(torch, torch_eval)[0])
        t_torch_nb.append(timed(torch, lambda: torch_eval(phi_all))[0])
    torch.cuda.synchronize()
    ms = lambda evs: np.asarray([a.elapsed_time(b) for a, b in evs])  # noqa: E731
    h, t, tn = ms(t_hip), ms(t_torch), ms(t_torch_nb)
    nd = int(cd.shape[1])
    bytes_pt = 8 + 4 * 8 + 8 + nd * 4 + nd * nc * 8 + nv * 8  # position, lambda, permutation; indices; rows; out
    info = tree.info()
    bps = n * bytes_pt / (float(np.median(h)) * 1e-3)
    return {"case": "lattice", "lattice": L, "points": n, "values": nv, "missing": missing, "cells": mesh.num_cells,
            "locator_bins": info["bins"], "locator_list_entries": info["list"],
            "tree_build_ms": tree_build_ms, "locate_ms_first": ev_find[0].elapsed_time(ev_find[1]),
            "locate_ms": ev_find2[0].elapsed_time(ev_find2[1]), "sort_ms": ev_plan[0].elapsed_time(ev_plan[1]),
            "locate_points_per_s": n / (ev_find2[0].elapsed_time(ev_find2[1]) * 1e-3),
            "eval_hip_ms_median": float(np.median(h)), "eval_hip_ms_all": [round(float(v), 3) for v in h],
            "eval_points_per_s": n / (float(np.median(h)) * 1e-3), "bytes_needed_per_point": bytes_pt,
            "eval_bytes_per_s": bps, "share_of_8TBps_peak_gather_kernel": bps / PEAK_BYTES_PER_S,
            "eval_torch_ms_median": float(np.median(t)), "eval_torch_ms_all": [round(float(v), 3) for v in t],
            "eval_torch_basis_given_ms_median": float(np.median(tn)),
            "max_abs_hip_minus_torch": dev_max,
            "hip_not_slower_than_torch": bool(np.median(h) <= min(np.median(t), np.median(tn)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-N", type=int, default=128)
    ap.add_argument("--probes", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--lattice", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="probes,lattice")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    S, W, clk, mesh = build(a.N)
    recs = []
    if "probes" in a.only:
        recs.append(case_probes(S, W, clk, mesh, a.probes, a.steps, a.warmup))
    if "lattice" in a.only:
        recs.append(case_lattice(S, W, mesh, a.lattice, a.reps))
    for r in recs:
        r["mesh_N"] = a.N
        print(json.dumps(r), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(r) + "\n")
    return 0 if all(r.get("hip_not_slower_than_torch", True) for r in recs) else 1


if __name__ == "__main__":
    sys.exit(main())
