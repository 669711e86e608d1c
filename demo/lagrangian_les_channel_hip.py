#!/usr/bin/env python3
"""The Lagrangian average of the dynamic Smagorinsky model beside the local one, on the periodic channel, HIP path.

The channel and the perturbed Poiseuille state are those of demo/dynamic_les_channel_hip.py.  Neither
``DynamicSmagorinsky(average="local")`` nor ``average="lagrangian"`` needs a homogeneous direction: both find a ``Cs2``
per cell.  The local average has no memory -- where the Germano-Lilly ratio of a cell's neighbourhood is negative the
coefficient is clipped to 0, and it changes from step to step as the field does.  The Lagrangian average carries
``F_LM`` and ``F_MM`` along the path lines with a fading memory (Meneveau, Lund & Cabot 1996), starts from
``cs2_initial`` and relaxes towards the sources over the time ``T``.  Printed after ``--steps`` steps, per slab across the
channel: the mean ``Cs2`` of both; then, for each, the share of cells whose coefficient is clipped to 0 and the mean
change of ``Cs2`` per cell from one step to the next.

    python demo/lagrangian_les_channel_hip.py [-N 8] [--dim 2] [--steps 4] [--nu 0.01] [-G 0.02] [--amplitude 0.3]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dynamic_les_channel_hip import perturbed_poiseuille  # noqa: E402
from les_channel_hip import H, build_channel  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-N", type=int, default=8, help="cells (and slabs) across the channel")
    ap.add_argument("--dim", type=int, default=2, choices=[2, 3])
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--nu", type=float, default=0.01)
    ap.add_argument("-G", type=float, default=0.02, help="body force along x")
    ap.add_argument("--amplitude", type=float, default=0.3, help="perturbation over the centre-line velocity")
    ap.add_argument("--dt", type=float, default=0.05)
    a = ap.parse_args(argv)
    if a.steps < 2:
        ap.error("--steps: at least 2 (the step-to-step change needs two)")
    import torch

    import oasisx_amd as ox

    fns = perturbed_poiseuille(a.G, a.nu, a.amplitude, a.dim)
    res = {}
    for key in ("local", "lagrangian"):
        model = ox.DynamicSmagorinsky(average=key)
        mesh, S = build_channel(a.N, a.dim, a.G, model)
        for i, f in enumerate(fns):
            S._u1[i].interpolate(f)
            S._u2[i].interpolate(f)
        history = []
        for _ in range(a.steps):
            S.solve(a.dt, a.nu, max_iter=1)
            history.append(S.smagorinsky_coefficient().cpu().numpy())
        cs2 = history[-1]
        change = float(np.mean([np.abs(history[k + 1] - history[k]).mean() for k in range(a.steps - 1)]))
        res[key] = {"cs2": cs2, "clipped": float((cs2 == 0.0).mean()), "change": change,
                    "nut": S.eddy_viscosity().cpu().numpy()}
        if key == "lagrangian":
            status = model.backtrace_status().cpu().numpy()
            res[key]["left"] = float((status == 1).mean())
    bins = ox.slab_bins(mesh, 1)[0]
    y = mesh.coords[mesh.cells.to(torch.int64)].cpu().numpy().mean(axis=1)[:, 1]
    print(f"dynamic LES channel, {a.dim}-D: {mesh.num_cells} cells, perturbation {a.amplitude} of the centre-line velocity "
          f"{a.G * H * H / (8.0 * a.nu):.4f}, after {a.steps} steps of dt = {a.dt}")
    print(f"{'slab':>5} {'y':>8} {'Cs2 local':>12} {'Cs2 lagrangian':>15} {'nut local':>14} {'nut lagrangian':>15}")
    for key in res:
        res[key]["rows"] = []
    for k in range(int(bins.max()) + 1):
        m = bins == k
        for key in res:
            res[key]["rows"].append({"slab": k, "y": float(y[m].mean()), "cs2": float(res[key]["cs2"][m].mean()),
                                     "nut": float(res[key]["nut"][m].mean())})
        lo, la = res["local"]["rows"][-1], res["lagrangian"]["rows"][-1]
        print(f"{k:>5} {lo['y']:>8.4f} {lo['cs2']:>12.5f} {la['cs2']:>15.5f} {lo['nut']:>14.6e} {la['nut']:>15.6e}")
    for key in res:
        print(f"{key:>11}: cells clipped to 0: {100.0 * res[key]['clipped']:5.1f} %, mean |Cs2(n+1) - Cs2(n)| per cell: "
              f"{res[key]['change']:.3e}")
    print(f"lagrangian: {100.0 * res['lagrangian']['left']:.1f} % of the vertex classes traced back out of the mesh in the "
          "last step (walls: they keep their own old value)")
    return res


if __name__ == "__main__":
    main()
