"""Drag zones at the bench size (Taylor-Green 128^3, P2-P1): ONE solver, one process, HIP events, medians, the variants
alternating inside the timed loop.

    python tools/drag_bench.py [-N 128] [--warmup 3] [--reps 20] [--out FILE] [--bench-trees this=DIR parent=DIR] [--bench-runs 2]

Part 1, the launches, alternating: ``ox_drag_sigma``, ``ox_drag_rows`` (theta = 1 without a target: the matrix alone; and
theta = 0.5 with a target: the matrix and both terms of the right-hand side) and ``DragZone.sample`` (``ox_drag_force_cells``
+ ``ox_wall_forces``) for two zones -- a slab of one eighth of the domain and the whole domain -- beside
``ox_assemble_first`` and one ``ox_assemble_matrix`` mass pass on the same pattern (the composed alternative, which would
also need a value array of its own and an add).
Bytes per launch from the stored sizes (every table entry once: what has to come from HBM if the caches serve the
re-reads): rows -- per pair of the touched slices 4 B of cell, 1 B of local index and ``pw`` position bytes, per entry
slot of the touched slices 16 B of ``A`` (read and written), per zone cell 8 B of sigma and 8 B of |det J|, with a
right-hand side 4 nd B of dofs per zone cell and per touched row gdim x (16 B of b_first + 8 B of w), and with theta < 1 the
pass that forms w = u_t - (1 - theta) u_1; sigma
-- per zone cell 4 B of list, 16 B of coefficients, 8 B of result, 4 nd B of dofs and per row of the zone gdim x 8 B of
u_ab; the mass pass -- per pair the same 5 + pw B, per slot 8 B written, per cell 8 gs B of geometry.
Part 2 (``--bench-trees``): ``bench.py --gpus 1 --steps 20 --warmup 5`` as child processes in the given source trees (this
commit, the parent commit), alternating: the default step makes no new call and must not change."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from viscosity_bench import HBM_PEAK, bench_trees, build, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-N", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=3, help="warm-up steps")
    ap.add_argument("--reps", type=int, default=20, help="timed launches per variant")
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-trees", nargs="*", default=[], metavar="LABEL=DIR")
    ap.add_argument("--bench-runs", type=int, default=2)
    a = ap.parse_args()
    import numpy as np
    import torch

    import oasisx_amd as ox
    from oasisx_amd.drag import DragGroup, check_zones
    from oasisx_amd.la import SellMatrix

    # the children first: they have the device to themselves (this process has not touched it yet)
    bench = bench_trees(a.bench_trees, a.bench_runs) if a.bench_trees else None
    S, W, clk = build(a.N, None)
    dt, nu = W["dt"], W["nu"]
    for _ in range(a.warmup):
        clk["t"] += dt
        S.solve(dt, nu, max_iter=1)
    torch.cuda.synchronize()
    q0, q1 = W["box"]
    cut = q0[2] + (q1[2] - q0[2]) / 8.0  # (the numbering runs slowest along the last axis: the slab is compact in the rows)
    target = lambda x: np.stack([0.1 + 0.0 * x[0], 0.0 * x[0], 0.0 * x[0]])  # noqa: E731
    specs = {"slab": (lambda x: x[2] < cut, 1.0, None), "whole": (lambda x: x[0] > q0[0] - 1.0, 1.0, None),
             "whole_rhs": (lambda x: x[0] > q0[0] - 1.0, 0.5, target)}
    groups = {}
    for k, (marker, theta, tgt) in specs.items():
        z = ox.DragZone(marker, darcy=2.0, forchheimer=0.5, target=tgt)
        groups[k] = DragGroup(S, z, theta, check_zones(z, S._mesh, False, theta))
    Vi = S._Vi[0][0]
    P = S._M.pattern
    Mtmp = SellMatrix(Vi.pattern, symmetric=True, name="Mtmp")
    S.assemble_first(dt, nu)  # u_ab of the last step in place

    variants = {"assemble_first": lambda: S._assemble_first_rows(dt, nu, False),
                "mass_pass": lambda: S._assemble_matrix(0, Vi, Mtmp)}
    for k, G in groups.items():
        variants[f"sigma_{k}"] = G.launch_sigma
        variants[f"rows_{k}"] = G.launch_rows
        variants[f"sample_{k}"] = lambda G=G: G.zones[0].sample(0.0)
    ev = {k: [] for k in variants}
    for r in range(a.reps + 3):
        for k, fn in variants.items():
            ev[k].append(timed(torch, fn))
        for G in groups.values():
            G.zones[0]._times.clear()  # (the ring is not what is timed)
    torch.cuda.synchronize()

    adj = Vi.adj
    ap_h = adj.adj_ptr.cpu().numpy()
    sp_h = P.slice_ptr.cpu().numpy()
    nd, gs, gdim, pw = int(adj.nd), 10, 3, int(adj.pw)
    n_pairs_all, n_slots_all = int(ap_h[-1]), int(sp_h[-1])
    nc = int(S._geom.shape[0])
    nbytes = {"mass_pass": n_pairs_all * (5 + pw) + n_slots_all * 8 + nc * 8 * gs}
    sizes = {}
    for k, G in groups.items():
        sl = G._slices.cpu().numpy().astype(np.int64)
        pairs = int((ap_h[sl + 1] - ap_h[sl]).sum())
        slots = int((sp_h[sl + 1] - sp_h[sl]).sum())
        rows = int(sl.shape[0]) * 64
        zc = G.n_zone_cells
        rhs = G._ut is not None or G.theta != 1.0
        nbytes[f"rows_{k}"] = pairs * (5 + pw) + slots * 16 + zc * 16 + (zc * 4 * nd + rows * gdim * 24 if rhs else 0)
        if G.theta != 1.0:  # the pass that forms w = u_t - (1 - theta) u_1
            nbytes[f"rows_{k}"] += int(S._n_u) * gdim * 8 * (3 if G._ut is not None else 2)
        zrows = int(torch.unique(Vi.cell_dofs[G._zc64].reshape(-1)).shape[0])
        nbytes[f"sigma_{k}"] = zc * (28 + 4 * nd) + zrows * gdim * 8 * (2 if G._ut is not None else 1)
        nbytes[f"sample_{k}"] = zc * (4 + 8 + 8 + 4 * nd + 2 * gdim * 8) + zrows * gdim * 8 * (2 if G._ut is not None else 1)
        sizes[k] = {"zone_cells": zc, "touched_slices": int(sl.shape[0]), "pairs": pairs, "entry_slots": slots}
    kern = {}
    for k, pairs_ in ev.items():
        ms = statistics.median(x.elapsed_time(y) for x, y in pairs_[3:])
        kern[k] = {"ms": round(ms, 4)}
        if k in nbytes:
            kern[k]["bytes"] = nbytes[k]
            kern[k]["fraction_of_hbm_peak"] = round(nbytes[k] / (ms * 1e-3) / HBM_PEAK, 4)
    kern["rows_whole_over_mass_pass"] = round(kern["rows_whole"]["ms"] / kern["mass_pass"]["ms"], 3)
    kern["rows_whole_over_assemble_first"] = round(kern["rows_whole"]["ms"] / kern["assemble_first"]["ms"], 3)
    out = {"N": a.N, "cells": nc, "rows_u": int(P.n_rows), "entry_slots": n_slots_all, "pairs": n_pairs_all,
           "slices": int(adj.n_slices), "zones": sizes, "kernel": kern, "bench": bench}
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
