#!/usr/bin/env python3
"""Brinkman channel: flow through a porous medium between two walls, HIP path.

The square [-1, 1]^2, P2-P1, filled with a porous medium of Darcy coefficient sigma (``oasisx_amd.DragZone`` over every
cell, ``drag_theta = 1``: backward Euler), driven by a constant body force (f, 0) between no-slip walls at y = +-1.  With
p = 0 the steady solution of ``-nu u'' + sigma u = f`` is

    u(y) = (f / sigma) (1 - cosh(m y) / cosh(m)),   m = sqrt(sigma / nu),        v = 0

(the Poiseuille parabola for sigma -> 0, a plug with wall layers of width 1 / m for large sigma), which is also the
Dirichlet datum at x = +-1.  The run starts from the parabola with the same centre-line velocity and is stepped to a steady
state; it prints the maximum error against the closed form relative to the centre-line value, and the force on the medium
(``DragZone.sample``) beside ``f |Omega|`` minus the friction on the boundary (``WallStress``): at a steady state the body
force is carried by the medium and the walls.

With nu = 0.5, sigma = 2, f = 1, N = 8: the direct solve of ``nu K + sigma M`` on the same forms is 7.5e-5 off the closed form
(tests/test_drag_host.py); the numpy model of the time-stepped scheme (tests/drag_model.py) is 8.76e-5 off after 100 steps
of dt = 0.1 and 8.69e-5 after 60: the splitting leaves a pressure of 2e-4 that the direct solve does not have.
tests/test_gpu_drag_demo.py holds this demo's printed error to that model's value, step for step.

    python demo/porous_channel_hip.py [-N 8] [--steps 100] [--dt 0.1] [--nu 0.5] [--sigma 2] [-f 1]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KRYLOV = {"tentative": {"ksp_type": "bcgs", "pc_type": "jacobi", "ksp_rtol": 1e-11, "ksp_atol": 1e-30},
          "pressure": {"ksp_type": "cg", "pc_type": "jacobi", "ksp_rtol": 1e-11, "ksp_atol": 1e-30},
          "scalar": {"ksp_type": "cg", "pc_type": "jacobi", "ksp_rtol": 1e-11, "ksp_atol": 1e-30}}


def brinkman_profile(y, nu: float, sigma: float, f: float):
    """u(y) = (f / sigma) (1 - cosh(m y) / cosh(m)), m = sqrt(sigma / nu)."""
    m = np.sqrt(sigma / nu)
    return (f / sigma) * (1.0 - np.cosh(m * np.asarray(y)) / np.cosh(m))


def parabola(y, nu: float, sigma: float, f: float):
    """The parabola with the centre-line velocity of the Brinkman profile: where the run starts."""
    return brinkman_profile(0.0, nu, sigma, f) * (1.0 - np.asarray(y) ** 2)


def build_channel(N: int, nu: float, sigma: float, f: float, degree: int = 2):
    """(mesh, solver, zone): Dirichlet data on the whole boundary -- no slip on the walls, the closed form at the two ends --,
    every velocity level on the parabola, p = 0."""
    import oasisx_amd as ox
    from oasisx_amd import mesh as M

    mesh = M.create_rectangle(None, [[-1.0, -1.0], [1.0, 1.0]], [N, N])
    edge = lambda x: np.isclose(np.abs(x[0]), 1.0) | np.isclose(np.abs(x[1]), 1.0)  # noqa: E731
    bc_u = ox.DirichletBC(lambda x: brinkman_profile(x[1], nu, sigma, f), ox.LocatorMethod.GEOMETRICAL, edge)
    bc_v = ox.DirichletBC(lambda x: 0.0 * x[0], ox.LocatorMethod.GEOMETRICAL, edge)
    zone = ox.DragZone(lambda x: x[0] > -2.0, darcy=sigma)
    solver = ox.FractionalStep_AB_CN(mesh, ("Lagrange", degree), ("Lagrange", 2 if degree == 3 else 1), bcs_u=[[bc_u], [bc_v]],
                                     bcs_p=[], solver_options=KRYLOV, body_force=(f, 0.0), options={"sell_window": 256},
                                     drag=zone, drag_theta=1.0)
    for level in (solver._u, solver._u1, solver._u2):
        level[0].interpolate(lambda x: parabola(x[1], nu, sigma, f))
        level[1].interpolate(lambda x: 0.0 * x[0])
    solver._p.interpolate(lambda x: 0.0 * x[0])
    return mesh, solver, zone


def profile_error(solver, nu: float, sigma: float, f: float) -> float:
    """max |u_h - u| over the dofs of the first component, relative to the centre-line value."""
    y = solver._Vi[0][0].x[:, 1].cpu().numpy()
    return float(np.abs(solver._U.rhost()[:, 0] - brinkman_profile(y, nu, sigma, f)).max() / brinkman_profile(0.0, nu, sigma, f))


def run(N: int = 8, steps: int = 100, dt: float = 0.1, nu: float = 0.5, sigma: float = 2.0, f: float = 1.0, degree: int = 2):
    """One run to a steady state.  Returns dict(N, error, errors, force, balance, wall, volume, change, solver): the error
    against the closed form (after every step: ``errors``), the force on the medium, ``f |Omega|`` minus the friction on
    the boundary, that friction, the zone's volume and the last change of the velocity per step."""
    import oasisx_amd as ox

    mesh, solver, zone = build_channel(N, nu, sigma, f, degree)
    wall = ox.WallStress(solver, capacity=1)
    change, errors = 0.0, []
    for _ in range(steps):
        change = solver.solve(dt, nu, max_iter=1)
        errors.append(profile_error(solver, nu, sigma, f))
    zone.sample(steps * dt)
    wall.sample(steps * dt, nu)
    force = zone.forces()[-1, 0]
    friction = wall.forces()[-1, 0]
    vol = float(zone.volume()[0])
    return dict(N=N, error=errors[-1], errors=errors, force=force, balance=f * vol - friction[0], wall=friction, volume=vol,
                change=float(change), solver=solver)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-N", type=int, nargs="+", default=[8], help="cells per direction (one run each)")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--dt", type=float, default=0.1)
    ap.add_argument("--nu", type=float, default=0.5)
    ap.add_argument("--sigma", type=float, default=2.0, help="Darcy coefficient of the medium")
    ap.add_argument("-f", type=float, default=1.0, help="body force")
    ap.add_argument("--degree", type=int, default=2, choices=[1, 2, 3])
    a = ap.parse_args(argv)
    print(f"Brinkman channel: nu = {a.nu}, sigma = {a.sigma}, f = {a.f}; centre-line velocity "
          f"{brinkman_profile(0.0, a.nu, a.sigma, a.f):.6f}, wall layer 1/m = {np.sqrt(a.nu / a.sigma):.3f}")
    rows = []
    for N in a.N:
        r = run(N, a.steps, a.dt, a.nu, a.sigma, a.f, a.degree)
        rows.append(r)
        print(f"N = {N:3d}  max error / u(0) = {r['error']:.6e}  force on the medium = {r['force'][0]:.6f}  "
              f"f |Omega| - wall friction = {r['balance']:.6f} (friction {r['wall'][0]:.6f}, |Omega| = {r['volume']:.4f})  "
              f"last change per step {r['change']:.2e}")
    return rows


if __name__ == "__main__":
    main()
