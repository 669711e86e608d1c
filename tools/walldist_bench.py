"""Wall distance and van Driest damping at the bench size (Taylor-Green box 128^3, P2-P1): set-up and per-step cost, HIP
events, medians, the variants alternating inside the timed loops.

    python tools/walldist_bench.py [-N 128] [--walls two six] [--steps 8] [--warmup 3] [--reps 20] [--out FILE]
                                   [--bench-trees this=DIR parent=DIR] [--bench-runs 2]

Per wall set (``two``: the faces y = lo and y = hi; ``six``: all exterior facets):
  * set-up: ``ox_walldist_create`` (host-synchronous: wall clock) and the query of all cell centroids (HIP events); the
    mean number of rings a centroid visits, estimated from its distance and the bin widths (``ceil(d / min h) + 1``, capped
    by the grid);
  * kernels, alternating: the damped nut kernel plus its ``ox_wall_stress`` launch beside the undamped
    ``ox_cell_viscosity``; the bytes model is +12 B per cell (dist, nearest) on the undamped kernel's stream;
  * whole steps without a model, with Smagorinsky and with Smagorinsky + VanDriest, alternating.
``--bench-trees``: ``bench.py``'s default line as child processes in the given source trees, alternating (the default
path makes no new call)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def wall_facets(mesh, which):
    import numpy as np

    if which == "six":
        return None
    fv, _ = mesh._entities(mesh.gdim - 1)
    X = mesh.coords.cpu().numpy()
    ext = np.asarray(mesh.exterior_facets(), dtype=np.int64)
    y = X[fv[ext]][:, :, 1]
    return ext[np.isclose(y, X[:, 1].min()).all(axis=1) | np.isclose(y, X[:, 1].max()).all(axis=1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-N", type=int, default=128)
    ap.add_argument("--walls", nargs="*", default=["two", "six"], choices=["two", "six"])
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-trees", nargs="*", default=[], metavar="LABEL=DIR")
    ap.add_argument("--bench-runs", type=int, default=2)
    a = ap.parse_args()
    import numpy as np
    import torch
    from viscosity_bench import bench_trees, build, timed

    import oasisx_amd as ox
    from oasisx_amd.viscosity import _cell_viscosity

    bench = bench_trees(a.bench_trees, a.bench_runs) if a.bench_trees else None
    S0, W, clk0 = build(a.N, None)
    S1, _, clk1 = build(a.N, ox.Smagorinsky())
    dt, nu = W["dt"], W["nu"]
    mesh = S0._mesh
    out = {"N": a.N, "cells": int(mesh.num_cells), "nu": nu, "dt": dt, "walls": {}}
    for which in a.walls:
        ids = wall_facets(mesh, which)
        # ---- set-up ----------------------------------------------------------------------------------------------------
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wd = ox.WallDistance(mesh, ids)
        torch.cuda.synchronize()
        create_ms = (time.perf_counter() - t0) * 1e3  # (with the host's facet selection and the copy of the vertices)
        cen = mesh.coords[mesh.cells.to(torch.int64)].mean(dim=1).contiguous()
        wd.query(cen[:1024])
        e = timed(torch, lambda: wd.query(cen))
        torch.cuda.synchronize()
        query_ms = e[0].elapsed_time(e[1])
        dist, _ = wd.query(cen)
        info = wd.info()
        X = mesh.coords
        ext = (X.max(dim=0).values - X.min(dim=0).values).cpu().numpy()
        h = min(ext[k] / b for k, b in enumerate(info["bins_per_axis"]) if b > 1)
        rings = torch.clamp(torch.ceil(dist / h) + 1.0, max=float(max(info["bins_per_axis"])))
        rec = {"facets": wd.n_facets, "grid": info, "create_ms": round(create_ms, 2), "query_centroids_ms": round(query_ms, 2),
               "mean_rings_estimate": round(float(rings.mean()), 2), "max_distance": float(dist.max())}
        print(json.dumps({which: rec}), flush=True)
        # ---- kernels and steps -----------------------------------------------------------------------------------------
        model = ox.Smagorinsky(damping=ox.VanDriest(ids))
        S2, _, clk2 = build(a.N, model)
        for S, clk in ((S0, clk0), (S1, clk1), (S2, clk2)):
            for _ in range(a.warmup):
                clk["t"] += dt
                S.solve(dt, nu, max_iter=1)
        torch.cuda.synchronize()
        Vi = S1._Vi[0][0]

        def plain():
            _cell_viscosity(S1, S1._nut, model=0, coefficient=0.1677)

        variants = {"nut_smagorinsky": plain, "nut_damped_with_wall_stress": lambda: S2.viscosity_assemble(nu)}
        ev = {k: [] for k in variants}
        for _ in range(a.reps + 3):
            for k, fn in variants.items():
                ev[k].append(timed(torch, fn))
        torch.cuda.synchronize()
        ncells, nd = int(S1._geom.shape[0]), int(Vi.cell_dofs.shape[1])
        nut_bytes = ncells * (nd * 4 + int(S1._geom.shape[1]) * 8 + 8) + int(Vi.n_local) * 3 * 8
        kern = {}
        for k, pairs in ev.items():
            t = [x.elapsed_time(y) for x, y in pairs[3:]]
            half = len(t) // 2
            kern[k] = {"ms": round(statistics.median(t), 4),
                       "ms_median_of_halves": [round(statistics.median(t[:half]), 4), round(statistics.median(t[half:]), 4)]}
        kern["bytes_undamped"], kern["bytes_damped"] = nut_bytes, nut_bytes + 12 * ncells
        kern["bytes_ratio"] = round((nut_bytes + 12 * ncells) / nut_bytes, 4)
        kern["time_ratio"] = round(kern["nut_damped_with_wall_stress"]["ms"] / kern["nut_smagorinsky"]["ms"], 4)
        times = {"constant_nu": [], "smagorinsky": [], "van_driest": []}
        for i in range(a.steps + 1):
            for key, S, clk in (("constant_nu", S0, clk0), ("smagorinsky", S1, clk1), ("van_driest", S2, clk2)):
                clk["t"] += dt
                e = timed(torch, lambda: S.solve(dt, nu, max_iter=1))
                torch.cuda.synchronize()
                if i:
                    times[key].append(e[0].elapsed_time(e[1]))
        yp, damp = S2.wall_units()
        rec.update(kernel=kern, step_ms={k: round(statistics.median(v), 3) for k, v in times.items()},
                   y_plus_max=float(yp.max()), damping_min_max=[float(damp.min()), float(damp.max())])
        out["walls"][which] = rec
        print(json.dumps({which: rec}), flush=True)
        del S2, wd
    if bench is not None:
        out["bench_default_steps_per_s"] = bench
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
