#!/usr/bin/env python3
"""Wall shear stress and drag of plane Poiseuille flow, HIP path.

A 2-D channel [0, L] x [0, 1] driven by a constant body force (G, 0), open at both ends: ``PressureBC`` p = 0 at the
inlet and at the outlet, no-slip walls, the natural condition for the velocity at the open ends.  The steady solution
is U(y) = G y (1 - y) / (2 nu), p = 0: the wall shear stress is nu |dU/dy| = G / 2 on both walls and the drag on the two
walls G L (rho = 1, unit depth) -- the body force on the fluid.
``oasisx_amd.WallStress`` evaluates traction, shear and the force per tag on the device after every step (one launch
over the wall facets, one per-tag reduction; nothing is read back until the end).  The run starts 5 % below the exact
profile (which the P2 velocity space holds) and relaxes towards it; per step this prints the largest and smallest wall
|wss| against G / 2 and the drag against G L.

    python demo/wall_shear_hip.py [-N 16] [--steps 10] [--dt 0.01] [--nu 0.1] [--out wall.vtu]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KRYLOV = {"tentative": {"ksp_type": "bcgs", "pc_type": "jacobi", "ksp_rtol": 1e-10, "ksp_atol": 1e-30},
          "pressure": {"ksp_type": "cg", "pc_type": "jacobi", "ksp_rtol": 1e-10, "ksp_atol": 1e-30},
          "scalar": {"ksp_type": "cg", "pc_type": "jacobi", "ksp_rtol": 1e-10, "ksp_atol": 1e-30}}
INLET, WALLS, OUTLET = 1, 2, 3


def build_channel(N: int, nu: float, G: float = 1.0, L: float = 2.0):
    """(mesh, facet tags, solver) of the channel, the velocity levels and the pressure set to the exact solution."""
    import oasisx_amd as ox
    from oasisx_amd import mesh as M

    mesh = M.create_rectangle(None, [[0.0, 0.0], [L, 1.0]], [int(round(L)) * N, N])
    left = M.locate_entities_boundary(mesh, 1, lambda x: np.isclose(x[0], 0.0))
    walls = M.locate_entities_boundary(mesh, 1, lambda x: np.isclose(x[1], 0.0) | np.isclose(x[1], 1.0))
    right = M.locate_entities_boundary(mesh, 1, lambda x: np.isclose(x[0], L))
    facets = np.hstack([left, walls, right])
    values = np.hstack([np.full_like(left, INLET), np.full_like(walls, WALLS), np.full_like(right, OUTLET)]).astype(np.int32)
    srt = np.argsort(facets)
    tags = M.meshtags(mesh, 1, facets[srt], values[srt])
    noslip = ox.DirichletBC(0.0, ox.LocatorMethod.TOPOLOGICAL, (tags, WALLS))
    # (the velocity components share one matrix: both carry the same Dirichlet rows, the walls; the open ends keep the
    # natural condition nu du/dn - p n = 0, which the Poiseuille solution with p = 0 satisfies)
    solver = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_u=[[noslip], [noslip]],
                                     bcs_p=[ox.PressureBC(0.0, (tags, INLET)), ox.PressureBC(0.0, (tags, OUTLET))],
                                     solver_options=KRYLOV, body_force=(G, 0.0), options={"sell_window": 256})
    set_poiseuille(solver, nu, G, L)
    return mesh, tags, solver


def set_poiseuille(solver, nu: float, G: float, L: float, scale: float = 1.0, cross: float = 0.0) -> None:
    """u, u_1, u_2 = (scale G y (1 - y) / (2 nu), cross sin(2 pi x / L) sin(pi y)) and p = 0: the exact steady
    solution for scale = 1, cross = 0."""
    U = lambda x: scale * G * x[1] * (1.0 - x[1]) / (2.0 * nu)  # noqa: E731
    V = lambda x: cross * np.sin(2.0 * np.pi * x[0] / L) * np.sin(np.pi * x[1])  # noqa: E731
    for level in (solver._u, solver._u1, solver._u2):
        level[0].interpolate(U)
        level[1].interpolate(V)
    solver._p.interpolate(lambda x: 0.0 * x[0])


def run(N: int = 16, steps: int = 10, dt: float = 0.01, nu: float = 0.1, G: float = 1.0, L: float = 2.0, out: str | None = None):
    """Returns (wall, rows) with rows = [dict(t, wss_min, wss_max, drag)] per step."""
    import oasisx_amd as ox

    mesh, tags, solver = build_channel(N, nu, G, L)
    # start 5 % below the steady profile, with a small cross-flow: the run relaxes towards it (time scale 1 / (nu pi^2))
    set_poiseuille(solver, nu, G, L, scale=0.95, cross=0.01)
    wall = ox.WallStress(solver, facets=(tags, WALLS), rho=1.0, capacity=8)
    mags = []
    for n in range(1, steps + 1):
        solver.solve(dt, nu, max_iter=1)
        wall.sample(n * dt, nu, dt=dt)
        w = wall.wss()
        mags.append(_wss_range(w))  # (device scalars: read after the loop)
    forces = wall.forces()  # (steps, 1, 2): the only transfer of the forces
    rows = [dict(t=float(t), wss_min=float(lo), wss_max=float(hi), drag=float(forces[k, 0, 0]))
            for k, (t, (lo, hi)) in enumerate(zip(wall.times, mags))]
    if out:
        ox.io.write_facet_vtu(out, mesh, wall.facets, {"wss": wall.wss(), "tawss": wall.tawss(), "osi": wall.osi()},
                              time=float(wall.times[-1]))
    return wall, rows


def _wss_range(w):
    import torch

    m = torch.sqrt((w * w).sum(dim=1))
    return m.min(), m.max()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-N", type=int, default=16, help="cells across the channel")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--nu", type=float, default=0.1)
    ap.add_argument("--out", default=None, help="write the wall surface with wss, tawss and osi to this .vtu")
    a = ap.parse_args(argv)
    G, L = 1.0, 2.0
    wall, rows = run(a.N, a.steps, a.dt, a.nu, G, L, a.out)
    print(f"{wall.n_facets} wall facets; exact: |wss| = nu |dU/dy| = {G / 2:.6f}, drag = {G * L:.6f}")
    for r in rows:
        print(f"t = {r['t']:.4f}  |wss| in [{r['wss_min']:.6f}, {r['wss_max']:.6f}]  drag = {r['drag']:.6f}")
    print(f"TAWSS in [{float(wall.tawss().min()):.6f}, {float(wall.tawss().max()):.6f}], max OSI = {float(wall.osi().max()):.3e}")
    return rows


if __name__ == "__main__":
    main()
