#!/usr/bin/env python3
"""Start-up of plane Poiseuille flow in a channel that is periodic along the stream, HIP path.

The channel [0, L] x [-1, 1] (x [0, W] with ``--dim 3``) has no inlet and no outlet: ``oasisx_amd.mesh.make_periodic``
identifies x = L with x = 0 (and z = W with z = 0), the walls y = +-1 carry no-slip, and a constant body force
(G, 0[, 0]) drives the flow from rest towards U(y) = G (1 - y^2) / (2 nu).  Per step the centre-line velocity, the bulk
velocity and the drag on the walls (``WallStress`` on the exterior facets -- the walls: the identified faces are no
boundary) are printed beside the series solution of the start-up problem

    u(y, t) = G/(2 nu) (1 - y^2) - sum_k 16 G (-1)^k / (nu pi^3 (2k+1)^3) cos((2k+1) pi y / 2) exp(-nu (2k+1)^2 pi^2 t / 4);

at the steady state the drag balances G |Omega|.

    python demo/periodic_channel_hip.py [-N 8] [--dim 2] [--steps 20] [--dt 0.05] [--nu 0.5] [-G 1.0]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KRYLOV = {"tentative": {"ksp_type": "bcgs", "pc_type": "jacobi", "ksp_rtol": 1e-10, "ksp_atol": 1e-30},
          "pressure": {"ksp_type": "cg", "pc_type": "jacobi", "ksp_rtol": 1e-10, "ksp_atol": 1e-30},
          "scalar": {"ksp_type": "cg", "pc_type": "jacobi", "ksp_rtol": 1e-10, "ksp_atol": 1e-30}}


def walls(x):
    return np.isclose(np.abs(x[1]), 1.0)


def startup_profile(y, t, nu, G, terms=60):
    k = np.arange(terms)[:, None]
    m = 2 * k + 1
    series = (16.0 * G * (-1.0) ** k / (nu * np.pi ** 3 * m ** 3) * np.cos(m * np.pi * y[None, :] / 2.0)
              * np.exp(-nu * m ** 2 * np.pi ** 2 * t / 4.0)).sum(axis=0)
    return G / (2.0 * nu) * (1.0 - y ** 2) - series


def build_channel(N: int, dim: int, nu: float, G: float, L: float = 3.0, W: float = 2.0):
    import oasisx_amd as ox
    from oasisx_amd import mesh as M

    if dim == 2:
        mesh = M.make_periodic(M.create_rectangle(None, [[0.0, -1.0], [L, 1.0]], [max(3, N), N]), (0,))
    else:
        mesh = M.make_periodic(M.create_box(None, [[0.0, -1.0, 0.0], [L, 1.0, W]], [max(3, N), N, max(3, N)]), (0, 2))
    noslip = [[ox.DirichletBC(0.0, ox.LocatorMethod.GEOMETRICAL, walls)] for _ in range(dim)]
    force = (G,) + (0.0,) * (dim - 1)
    solver = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_u=noslip, bcs_p=[], solver_options=KRYLOV,
                                     body_force=force)
    return mesh, solver


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-N", type=int, default=8, help="cells across the channel")
    ap.add_argument("--dim", type=int, default=2, choices=[2, 3])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--dt", type=float, default=0.05)
    ap.add_argument("--nu", type=float, default=0.5)
    ap.add_argument("-G", type=float, default=1.0, help="body force along x")
    a = ap.parse_args(argv)
    import oasisx_amd as ox

    mesh, S = build_channel(a.N, a.dim, a.nu, a.G)
    per = mesh.periodic
    vol = float(np.prod(per.hi - per.lo))
    Ws = ox.WallStress(S)
    x = S._Vi[0][0].x.cpu().numpy()
    centre = np.nonzero(np.isclose(x[:, 1], 0.0))[0]
    print(f"periodic channel, {a.dim}-D: {mesh.num_cells} cells, {S._Vi[0][0].num_dofs} velocity dofs per component "
          f"({mesh.num_vertices - per.n_free_vertices} identified vertices), {Ws.n_facets} wall facets, "
          f"{mesh.periodic_facets().shape[0]} identified facets")
    print(f"{'step':>5} {'t':>8} {'u centre':>14} {'series':>14} {'max |u - series|':>18} {'drag':>14} {'G |Omega|':>12}")
    rows = []
    for n in range(1, a.steps + 1):
        t = n * a.dt
        S.solve(a.dt, a.nu, max_iter=1)
        Ws.sample(t, a.nu)
        u = S._U.rhost()
        ref = startup_profile(x[:, 1], t, a.nu, a.G)
        drag = float(Ws.forces()[-1].sum(axis=0)[0])
        rows.append({"step": n, "t": t, "u_centre": float(u[centre, 0].mean()), "series": float(ref[centre].mean()),
                     "error": float(np.abs(u[:, 0] - ref).max()), "drag": drag, "balance": a.G * vol})
        r = rows[-1]
        print(f"{n:>5} {t:>8.3f} {r['u_centre']:>14.8f} {r['series']:>14.8f} {r['error']:>18.3e} {drag:>14.8f} {r['balance']:>12.6f}")
    return rows


if __name__ == "__main__":
    main()
