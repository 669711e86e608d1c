#!/usr/bin/env python3
"""Smagorinsky with van Driest wall damping on the periodic channel at its Poiseuille state, HIP path.

The channel [0, L] x [0, H] (x [0, W] with ``--dim 3``) of demo/periodic_channel_hip.py, periodic along the stream (and
the span), holds the steady profile u_x = G y (H - y) / (2 nu).  ``Smagorinsky(Cs, damping=VanDriest(walls))`` finds the
wall distance of every cell centroid once (``oasisx_amd.WallDistance``: the walls are the exterior facets, the identified
faces are no boundary) and, in every ``assemble_first``, the friction velocity of the nearest wall facet from ``u_ab``.
Here ``|wss| = G H / 2`` on both walls, so with ``y+ = d u_tau / nu`` and ``D = 1 - exp(-y+ / A+)``

    nut_c = Cs^2 Delta_c^2 D(y_c)^2 G |H - 2 y_c| / (2 nu),      Delta_c = |cell|^(1/dim)

which vanishes at the wall, where the undamped model peaks.  Printed: ``y+`` of the wall-adjacent cells, and per slab of
cells across the channel the mean ``nut`` with and without damping beside the closed form.

    python demo/les_channel_hip.py [-N 8] [--dim 2] [--nu 0.01] [-G 0.02] [--Cs 0.17] [--A-plus 26]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KRYLOV = {"tentative": {"ksp_type": "bcgs", "pc_type": "jacobi", "ksp_rtol": 1e-10, "ksp_atol": 1e-30},
          "pressure": {"ksp_type": "cg", "pc_type": "jacobi", "ksp_rtol": 1e-10, "ksp_atol": 1e-30}}
H = 1.0


def walls(x):
    return np.isclose(x[1], 0.0) | np.isclose(x[1], H)


def build_channel(N: int, dim: int, G: float, model, L: float = 2.0, W: float = 1.0):
    import oasisx_amd as ox
    from oasisx_amd import mesh as M

    if dim == 2:
        mesh = M.make_periodic(M.create_rectangle(None, [[0.0, 0.0], [L, H]], [max(3, N), N]), (0,))
    else:
        mesh = M.make_periodic(M.create_box(None, [[0.0, 0.0, 0.0], [L, H, W]], [max(3, N), N, max(3, N)]), (0, 2))
    noslip = [[ox.DirichletBC(0.0, ox.LocatorMethod.GEOMETRICAL, walls)] for _ in range(dim)]
    solver = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_u=noslip, bcs_p=[], solver_options=KRYLOV,
                                     body_force=(G,) + (0.0,) * (dim - 1), viscosity_model=model)
    return mesh, solver


def closed_form(Cs, delta2, y, G, nu, a_plus):
    """nut of the damped model at the Poiseuille state for cells of size Delta^2 = delta2 with centroids at height y."""
    d = np.minimum(y, H - y)
    damp = -np.expm1(-(d * np.sqrt(G * H / 2.0) / nu) / a_plus)
    return Cs ** 2 * delta2 * damp ** 2 * G * np.abs(H - 2.0 * y) / (2.0 * nu)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-N", type=int, default=8, help="cells across the channel")
    ap.add_argument("--dim", type=int, default=2, choices=[2, 3])
    ap.add_argument("--nu", type=float, default=0.01)
    ap.add_argument("-G", type=float, default=0.02, help="body force along x")
    ap.add_argument("--Cs", type=float, default=0.17)
    ap.add_argument("--A-plus", type=float, default=26.0)
    ap.add_argument("--dt", type=float, default=0.05)
    a = ap.parse_args(argv)
    import torch

    import oasisx_amd as ox

    out = {}
    for key, model in (("damped", ox.Smagorinsky(a.Cs, damping=ox.VanDriest(None, A_plus=a.A_plus))),
                       ("plain", ox.Smagorinsky(a.Cs))):
        mesh, S = build_channel(a.N, a.dim, a.G, model)
        for u in (S._u1[0], S._u2[0]):
            u.interpolate(lambda x: a.G * x[1] * (H - x[1]) / (2.0 * a.nu))
        S.assemble_first(a.dt, a.nu)
        out[key] = S.eddy_viscosity().cpu().numpy()
        if key == "damped":
            yp, damp = (t.cpu().numpy() for t in S.wall_units())
            vd = model.damping
            n_wall, info = vd.n_facets, vd.wall_distance.info()
            u_tau = vd.friction_velocity().cpu().numpy()
    cells = mesh.cells.to(torch.int64)
    X = mesh.coords[cells].cpu().numpy()  # (nc, d + 1, d)
    y = X.mean(axis=1)[:, 1]
    e = X[:, 1:] - X[:, :1]
    vol = np.abs(np.linalg.det(e)) / (2.0 if a.dim == 2 else 6.0)
    delta2 = vol ** (2.0 / a.dim)
    ref = closed_form(a.Cs, delta2, y, a.G, a.nu, a.A_plus)
    err = float(np.abs(out["damped"] - ref).max())
    slab = np.minimum((y / H * a.N).astype(int), a.N - 1)
    adjacent = (slab == 0) | (slab == a.N - 1)
    print(f"LES channel, {a.dim}-D: {mesh.num_cells} cells, {n_wall} wall facets in {info['bins']} bins "
          f"({info['bins_per_axis']} per axis), u_tau = {u_tau.min():.6f} .. {u_tau.max():.6f} "
          f"(sqrt(G H / 2) = {np.sqrt(a.G * H / 2.0):.6f})")
    print(f"y+ of the wall-adjacent cells: {yp[adjacent].min():.4f} .. {yp[adjacent].max():.4f}; of all cells up to {yp.max():.4f}")
    print(f"{'slab':>5} {'y':>8} {'y+':>10} {'D':>10} {'nut damped':>14} {'closed form':>14} {'nut plain':>14}")
    rows = []
    for k in range(a.N):
        m = slab == k
        rows.append({"slab": k, "y": float(y[m].mean()), "y_plus": float(yp[m].mean()), "damping": float(damp[m].mean()),
                     "nut": float(out["damped"][m].mean()), "closed_form": float(ref[m].mean()),
                     "nut_plain": float(out["plain"][m].mean())})
        r = rows[-1]
        print(f"{k:>5} {r['y']:>8.4f} {r['y_plus']:>10.4f} {r['damping']:>10.6f} {r['nut']:>14.6e} {r['closed_form']:>14.6e} "
              f"{r['nut_plain']:>14.6e}")
    print(f"max |nut - closed form| = {err:.3e} (max nut {ref.max():.3e})")
    return {"rows": rows, "error": err, "nut_max": float(ref.max()), "y_plus_wall": float(yp[adjacent].max())}


if __name__ == "__main__":
    main()
