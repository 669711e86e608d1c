#!/usr/bin/env python3
"""The dynamic Smagorinsky model on the periodic channel at a perturbed Poiseuille state, HIP path.

The channel of demo/les_channel_hip.py ([0, L] x [0, H] (x [0, W] with ``--dim 3``), periodic along the stream and the
span, no-slip walls) holds the profile u_x = G y (H - y) / (2 nu) plus a smooth perturbation of relative amplitude
``--amplitude`` that vanishes on the walls.  ``DynamicSmagorinsky(axis=1)`` averages the Germano-Lilly ratio over the
slabs of cells across the channel and finds one ``Cs2`` per slab from the resolved field: small in the wall slabs, where
the flow is a laminar shear (for which the ratio is zero), larger in the core -- without a wall distance, a friction
velocity or a constant chosen in advance.  Printed per slab: ``Cs2`` and the mean ``nut`` of the dynamic model beside
the constant-``Cs`` Smagorinsky model without and with van Driest damping.

    python demo/dynamic_les_channel_hip.py [-N 8] [--dim 2] [--nu 0.01] [-G 0.02] [--Cs 0.17] [--amplitude 0.3]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from les_channel_hip import H, build_channel  # noqa: E402


def perturbed_poiseuille(G, nu, amplitude, dim):
    """The velocity components as callables of x (3, n): Poiseuille plus a perturbation that vanishes on the walls, is
    periodic along x (period 2) and z (period 1) and whose cross-stream component changes sign at the centre line."""
    pi, Uc = np.pi, G * H * H / (8.0 * nu)
    a = amplitude * Uc
    env = lambda x: np.sin(pi * x[1] / H)  # noqa: E731
    u = lambda x: G * x[1] * (H - x[1]) / (2.0 * nu) + a * env(x) * np.sin(pi * x[0] + 0.3) * np.cos(2.0 * pi * x[2] + 0.2)  # noqa: E731
    v = lambda x: a * np.sin(2.0 * pi * x[1] / H) * np.cos(pi * x[0] + 0.3 + 2.0 * np.abs(x[1] - 0.5 * H))  # noqa: E731
    w = lambda x: a * env(x) * np.sin(2.0 * pi * x[2] + pi * x[0] + 1.0)  # noqa: E731
    return [u, v, w][:dim]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-N", type=int, default=8, help="cells (and slabs) across the channel")
    ap.add_argument("--dim", type=int, default=2, choices=[2, 3])
    ap.add_argument("--nu", type=float, default=0.01)
    ap.add_argument("-G", type=float, default=0.02, help="body force along x")
    ap.add_argument("--Cs", type=float, default=0.17, help="the constant of the two Smagorinsky runs beside")
    ap.add_argument("--A-plus", type=float, default=26.0)
    ap.add_argument("--amplitude", type=float, default=0.3, help="perturbation over the centre-line velocity")
    ap.add_argument("--dt", type=float, default=0.05)
    a = ap.parse_args(argv)
    import torch

    import oasisx_amd as ox

    fns = perturbed_poiseuille(a.G, a.nu, a.amplitude, a.dim)
    dyn = ox.DynamicSmagorinsky(axis=1)
    nut = {}
    for key, model in (("dynamic", dyn), ("plain", ox.Smagorinsky(a.Cs)),
                       ("damped", ox.Smagorinsky(a.Cs, damping=ox.VanDriest(None, A_plus=a.A_plus)))):
        mesh, S = build_channel(a.N, a.dim, a.G, model)
        for i, f in enumerate(fns):
            S._u1[i].interpolate(f)
            S._u2[i].interpolate(f)
        S.assemble_first(a.dt, a.nu)
        nut[key] = S.eddy_viscosity().cpu().numpy()
        if key == "dynamic":
            cs2 = dyn.bin_coefficients().cpu().numpy()
            raw = dyn.bin_coefficients(clipped=False).cpu().numpy()
            bins = ox.slab_bins(mesh, 1)[0]
    y = mesh.coords[mesh.cells.to(torch.int64)].cpu().numpy().mean(axis=1)[:, 1]
    print(f"dynamic LES channel, {a.dim}-D: {mesh.num_cells} cells in {cs2.shape[0]} slabs, perturbation {a.amplitude} of the "
          f"centre-line velocity {a.G * H * H / (8.0 * a.nu):.4f}; constant model: Cs = {a.Cs} (Cs2 = {a.Cs ** 2:.5f})")
    print(f"{'slab':>5} {'y':>8} {'Cs2 ratio':>12} {'Cs2':>10} {'nut dynamic':>14} {'nut Smagorinsky':>16} {'nut van Driest':>15}")
    rows = []
    for k in range(cs2.shape[0]):
        m = bins == k
        rows.append({"slab": k, "y": float(y[m].mean()), "cs2_raw": float(raw[k]), "cs2": float(cs2[k]),
                     "nut": float(nut["dynamic"][m].mean()), "nut_plain": float(nut["plain"][m].mean()),
                     "nut_damped": float(nut["damped"][m].mean())})
        r = rows[-1]
        print(f"{k:>5} {r['y']:>8.4f} {r['cs2_raw']:>12.5f} {r['cs2']:>10.5f} {r['nut']:>14.6e} {r['nut_plain']:>16.6e} "
              f"{r['nut_damped']:>15.6e}")
    return {"rows": rows, "cs2_constant": a.Cs ** 2}


if __name__ == "__main__":
    main()
