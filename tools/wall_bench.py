"""Wall-stress evaluation at the bench size (Taylor-Green 128^3, P2-P1, rtol 1e-8, warm start; all six faces of the box,
one tag per face: 196 608 facets): HIP events, medians, the variants alternating inside the timed loops.

    python tools/wall_bench.py [-N 128] [--steps 12] [--warmup 4] [--reps 20] [--out FILE]
                               [--bench-trees this=DIR parent=DIR] [--bench-runs 2]

Part 1, the two kernels, launch after launch, alternating: ``ox_wall_stress`` without and with the statistics
(``weight > 0``) and ``ox_wall_forces``.  Bytes moved per launch from the stored sizes: per facet the record (8 B), the
cell's two dof lists (nd x 4 B + ndq x 4 B) and geometry record (10 x 8 B in 3-D), t, wss and |f| t written (3 x gdim x
8 B) and, with the statistics, the accumulators read and written (2 x (2 gdim + 1) x 8 B); the gathers of u and p are
served by the caches and count once per distinct dof (gdim x 8 B, 8 B).  ``ox_wall_forces`` reads |f| t once.
Part 2, whole steps with and without ``sample`` after every step, alternating, on one solver.
Part 3 (``--bench-trees``): ``bench.py --gpus 1 --steps 20 --warmup 5`` as child processes in the given source trees
(this commit, the parent commit), alternating: the default step must not change."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_PEAK = 8.0e12  # B/s


def face_tags(mesh, np):
    """Meshtags of all exterior facets of a box, one tag per face."""
    from oasisx_amd import mesh as M

    d = mesh.gdim
    ext = np.asarray(mesh.exterior_facets(), dtype=np.int32)
    fv, _ = mesh._entities(d - 1)
    x = mesh.coords.cpu().numpy()
    mid = x[fv[ext]].mean(axis=1)
    lo, hi = x.min(axis=0), x.max(axis=0)
    val = np.full(ext.shape[0], -1, dtype=np.int32)
    for k in range(d):
        val[np.isclose(mid[:, k], lo[k])] = 2 * k
        val[np.isclose(mid[:, k], hi[k])] = 2 * k + 1
    assert (val >= 0).all()
    return M.meshtags(mesh, d - 1, ext, val), tuple(range(2 * d))


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
    import numpy as np
    import torch
    from viscosity_bench import bench_trees, build, timed

    import oasisx_amd as ox
    from oasisx_amd import _lib

    # part 3 first: the children have the device to themselves (this process has not touched it yet)
    bench = bench_trees(a.bench_trees, a.bench_runs) if a.bench_trees else None
    S, W, clk = build(a.N, None)
    dt, nu = W["dt"], W["nu"]
    tags, ids = face_tags(S._mesh, np)
    wall = ox.WallStress(S, facets=(tags, ids), capacity=4 * (a.steps + a.warmup + a.reps + 8))
    for _ in range(a.warmup):
        clk["t"] += dt
        S.solve(dt, nu, max_iter=1)
        wall.sample(clk["t"], nu, dt=dt)
    torch.cuda.synchronize()

    # ---- part 1: the kernels ------------------------------------------------------------------------------------------
    lib, st = _lib.load(), _lib.current_stream()
    Vi, Q = S._Vi[0][0], S._Q
    nf, d = wall.n_facets, wall.gdim

    def stress(weight):
        _lib.check(lib.ox_wall_stress(Vi.degree, Q.degree, C.byref(S._cells), _lib.ptr(Vi.cell_dofs), _lib.ptr(Q.cell_dofs), nf,
                                      _lib.ptr(wall._rec), S._U.rptr(), S._P.rptr(), None, nu, weight, _lib.ptr(wall._t),
                                      _lib.ptr(wall._wss), _lib.ptr(wall._ft), _lib.ptr(wall._acc_vec),
                                      _lib.ptr(wall._acc_mag), _lib.ptr(wall._acc_t), st), "ox_wall_stress")

    def forces():
        _lib.check(lib.ox_wall_forces(d, wall.n_tags, _lib.ptr(wall._tag_ptr), _lib.ptr(wall._ft), wall.rho,
                                      _lib.ptr(wall._ring), wall.capacity, 0, st), "ox_wall_forces")

    variants = {"wall_stress": lambda: stress(0.0), "wall_stress_with_statistics": lambda: stress(dt), "wall_forces": forces}
    ev = {k: [] for k in variants}
    for r in range(a.reps + 3):
        for k, fn in variants.items():
            ev[k].append(timed(torch, fn))
    torch.cuda.synchronize()
    rec = wall._rec.cpu().numpy()
    cells = np.unique(rec[:, 0])
    nd, ndq, gs = int(Vi.cell_dofs.shape[1]), int(Q.cell_dofs.shape[1]), int(S._geom.shape[1])
    vdofs = np.unique(Vi.cell_dofs[torch.from_numpy(cells).to(Vi.cell_dofs.device).long()].cpu().numpy()).shape[0]
    qdofs = np.unique(Q.cell_dofs[torch.from_numpy(cells).to(Q.cell_dofs.device).long()].cpu().numpy()).shape[0]
    base = nf * (8 + nd * 4 + ndq * 4 + gs * 8 + 3 * d * 8) + vdofs * d * 8 + qdofs * 8
    nbytes = {"wall_stress": base, "wall_stress_with_statistics": base + nf * 2 * (2 * d + 1) * 8,
              "wall_forces": nf * d * 8 + (wall.n_tags + 1) * 8 + wall.n_tags * d * 8}
    kern = {}
    for k, pairs in ev.items():
        ms = statistics.median(x.elapsed_time(y) for x, y in pairs[3:])
        kern[k] = {"ms": round(ms, 4), "bytes": int(nbytes[k]),
                   "fraction_of_hbm_peak": round(nbytes[k] / (ms * 1e-3) / HBM_PEAK, 4)}

    # ---- part 2: whole steps, alternating -----------------------------------------------------------------------------
    rec_t = {"plain": [], "with_sample": [], "sample_alone": []}
    for i in range(2 * (a.steps + 1)):
        sampled = i % 2 == 1
        clk["t"] += dt
        e = timed(torch, lambda: S.solve(dt, nu, max_iter=1))
        es = timed(torch, lambda: wall.sample(clk["t"], nu, dt=dt)) if sampled else None
        torch.cuda.synchronize()
        if i < 2:
            continue
        if sampled:
            rec_t["with_sample"].append(e[0].elapsed_time(es[1]))
            rec_t["sample_alone"].append(es[0].elapsed_time(es[1]))
        else:
            rec_t["plain"].append(e[0].elapsed_time(e[1]))
    steps = {k: round(statistics.median(v), 4) for k, v in rec_t.items()}
    F = wall.forces()
    out = {"N": a.N, "facets": nf, "tags": wall.n_tags, "boundary_cells": int(cells.shape[0]), "nu": nu, "dt": dt,
           "kernel": kern, "step_ms": steps, "samples": wall.n_samples, "ring_capacity": wall.capacity,
           "last_force_sum": [float(v) for v in F[-1].sum(axis=0)],
           "tawss_min_mean_max": [float(wall.tawss().min()), float(wall.tawss().mean()), float(wall.tawss().max())]}
    if bench is not None:
        out["bench_default_steps_per_s"] = bench
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
