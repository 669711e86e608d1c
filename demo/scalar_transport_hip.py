#!/usr/bin/env python3
"""A passive scalar in the 2-D Taylor-Green vortex, HIP path.

``c(x, t) = cos(pi x) cos(pi y) exp(-2 kappa pi^2 t)`` is a function of the vortex's stream function, so
``u . grad c = 0`` and c solves the advection-diffusion equation exactly for ANY diffusivity kappa.  The scalar rides on
``FractionalStep_AB_CN(..., scalars=[ScalarTransport(...)])``: advected by the extrapolated velocity of every step,
Crank-Nicolson diffusion, exact Dirichlet data; its operator is formed from the velocity matrix in one pass over the
values (``ox_scalar_rows``), not by a second element loop.  Prints the L2 error at the end time per mesh and the observed
order (P2: about 3).

    python demo/scalar_transport_hip.py [-N 8 -N 16 -N 32] [--dt 0.005] [-T 0.05] [--kappa 0.05] [--schmidt SC]
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run_scalar(N: int, dt: float = 0.005, T: float = 0.05, nu: float = 0.01, kappa: float | None = 0.05,
               schmidt: float | None = None, degree_u: int = 2):
    """Returns (L2 error of c at T, L2 error of u at T, scalar iterations of the last step)."""
    import oasisx_amd as ox
    from oasisx_amd import fem
    from oasisx_amd import mesh as M
    from taylor_green_hip import KRYLOV, TaylorGreen2D

    field = TaylorGreen2D(nu)
    kap = kappa if schmidt is None else nu / schmidt

    def exact(t=None):
        return lambda x: np.cos(np.pi * x[0]) * np.cos(np.pi * x[1]) * math.exp(
            -2.0 * kap * math.pi ** 2 * (field.now if t is None else t))

    def on_boundary(x):
        return np.isclose(np.abs(x[0]), 1.0) | np.isclose(np.abs(x[1]), 1.0)

    mesh = M.create_rectangle(None, [[-1.0, -1.0], [1.0, 1.0]], [N, N])
    G = ox.LocatorMethod.GEOMETRICAL
    spec = {"diffusivity": kappa} if schmidt is None else {"schmidt": schmidt}
    scalar = ox.ScalarTransport("c", initial=exact(0.0), bcs=[ox.DirichletBC(exact(), G, on_boundary)], **spec)
    options = dict(KRYLOV, scalar_transport=dict(KRYLOV["tentative"]))
    solver = ox.FractionalStep_AB_CN(mesh, ("Lagrange", degree_u), ("Lagrange", degree_u - 1), bcs_p=[],
                                     bcs_u=[[ox.DirichletBC(field.velocity(c), G, on_boundary)] for c in range(2)],
                                     solver_options=options, scalars=[scalar])
    for c in range(2):
        solver._u2[c].interpolate(field.velocity(c, -dt))
        solver._u1[c].interpolate(field.velocity(c, 0.0))
    solver._p.interpolate(field.pressure(-dt / 2.0))
    steps = int(round(T / dt))
    for n in range(1, steps + 1):
        field.now = n * dt
        solver.solve(dt, nu, max_iter=1)
    err_c = math.sqrt(fem.assemble_l2_error_sq(solver.scalar("c"), exact()))
    err_u = math.sqrt(sum(fem.assemble_l2_error_sq(solver._u[c], field.velocity(c)) for c in range(2)))
    return err_c, err_u, solver.iteration_counts()["scalar_transport"]["c"]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-N", type=int, action="append", default=None)
    ap.add_argument("--dt", type=float, default=0.005)
    ap.add_argument("-T", type=float, default=0.05)
    ap.add_argument("--nu", type=float, default=0.01)
    ap.add_argument("--kappa", type=float, default=0.05)
    ap.add_argument("--schmidt", type=float, default=None, help="kappa = nu / Sc instead of --kappa")
    ap.add_argument("-u", "--degree-u", type=int, default=2)
    a = ap.parse_args(argv)
    rows, prev = [], None
    print(f"{'N':>5} {'L2 error c':>14} {'order':>7} {'L2 error u':>14} {'its':>5}")
    for N in a.N or [8, 16, 32]:
        ec, eu, its = run_scalar(N, a.dt, a.T, a.nu, a.kappa, a.schmidt, a.degree_u)
        order = "" if prev is None else f"{math.log(prev[1] / ec) / math.log(N / prev[0]):.2f}"
        print(f"{N:>5} {ec:>14.6e} {order:>7} {eu:>14.6e} {its:>5}")
        rows.append((N, ec, eu, its))
        prev = (N, ec)
    return rows


if __name__ == "__main__":
    main()
