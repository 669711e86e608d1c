#!/usr/bin/env python3
"""Convective cooling of a slab in a fluid at rest, HIP path: ``RobinBC`` on both faces, no Dirichlet condition.

The slab ``-L <= x <= L`` (2-D and thin: a strip of cells, insulated on its long sides) starts from the series solution
at ``t0 > 0`` and exchanges heat with surroundings at ``c_inf`` through a film coefficient ``h`` on ``x = +-L``::

    dc/dt = kappa c_xx,      -kappa dc/dn = h (c - c_inf)  on x = +-L              Bi = h L / kappa
    (c - c_inf) / (c_0 - c_inf) = sum_n C_n cos(zeta_n x / L) exp(-zeta_n^2 kappa t / L^2)
    zeta_n tan zeta_n = Bi,      C_n = 4 sin zeta_n / (2 zeta_n + sin 2 zeta_n)

The roots ``zeta_n`` in ``(n pi, n pi + pi/2)`` are found by bisection.  The scalar rides on
``FractionalStep_AB_CN(..., scalars=[ScalarTransport(..., flux_bcs=[RobinBC(h, c_inf, faces)])])``; the film term is added
to the scalar's operator and right-hand side by ``ox_scalar_boundary``, Crank-Nicolson in ``c``.  Prints the L2 error at
the end time per mesh with the observed order (P2: about 3, until the time step's error shows), and the wall flux that
``ScalarFlux`` measures (leaving the domain) beside the film law ``h (c_wall - c_inf)``.

    python demo/robin_slab_hip.py [-N 4 -N 8 -N 16] [--dt 0.002] [-T 0.1] [--kappa 1.0] [--film 2.0] [--c-inf 0.0]
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

L = 1.0
T0 = 0.05  # the series at t0 is smooth: the start is compatible with the film condition


def roots(biot: float, n: int = 40, sweeps: int = 80) -> np.ndarray:
    """The first n roots of zeta tan zeta = Bi by bisection: one in every (k pi, k pi + pi/2), where the left side rises
    from 0 to infinity."""
    lo = np.arange(n) * math.pi
    hi = lo + 0.5 * math.pi
    for _ in range(sweeps):
        mid = 0.5 * (lo + hi)
        above = mid * np.tan(mid) > biot
        hi = np.where(above, mid, hi)
        lo = np.where(above, lo, mid)
    return 0.5 * (lo + hi)


def series(kappa: float, film: float, c_inf: float, c0: float = 1.0):
    """``f(t) -> (lambda x: c(x, t))`` of the series solution."""
    z = roots(film * L / kappa)
    coef = 4.0 * np.sin(z) / (2.0 * z + np.sin(2.0 * z))

    def at(t):
        decay = coef * np.exp(-z ** 2 * kappa * t / L ** 2)
        return lambda x: c_inf + (c0 - c_inf) * (np.cos(np.multiply.outer(x[0] / L, z)) @ decay)

    return at


def run_slab(N: int, dt: float = 0.002, T: float = 0.1, kappa: float = 1.0, film: float = 2.0, c_inf: float = 0.0,
             nu: float = 0.01, degree: int = 2):
    """Returns (L2 error of c at T0 + T, wall flux of ScalarFlux per unit area, h (c_wall - c_inf), scalar iterations)."""
    import oasisx_amd as ox
    from oasisx_amd import fem
    from oasisx_amd import mesh as M

    height = 4.0 * L / N  # two rows of cells of the aspect ratio of the square's
    mesh = M.create_rectangle(None, [[-L, 0.0], [L, height]], [N, 2])
    faces = M.locate_entities_boundary(mesh, 1, lambda x: np.isclose(np.abs(x[0]), L))
    exact = series(kappa, film, c_inf)

    def on_boundary(x):
        return np.isclose(np.abs(x[0]), L) | np.isclose(x[1], 0.0) | np.isclose(x[1], height)

    G = ox.LocatorMethod.GEOMETRICAL
    scalar = ox.ScalarTransport("c", diffusivity=kappa, initial=exact(T0), flux_bcs=[ox.RobinBC(film, c_inf, faces)])
    tight = {"ksp_type": "bcgs", "pc_type": "jacobi", "ksp_rtol": 1e-12, "ksp_atol": 1e-30}
    options = {"tentative": dict(tight), "pressure": dict(tight, ksp_type="cg"), "scalar": dict(tight, ksp_type="cg"),
               "scalar_transport": dict(tight)}
    solver = ox.FractionalStep_AB_CN(mesh, ("Lagrange", degree), ("Lagrange", 1), bcs_p=[],
                                     bcs_u=[[ox.DirichletBC(0.0, G, on_boundary)] for _ in range(2)],
                                     solver_options=options, scalars=[scalar])
    flux = ox.ScalarFlux(solver, "c", facets=faces, capacity=1)
    steps = int(round(T / dt))
    for _ in range(steps):
        solver.solve(dt, nu, max_iter=1)
    err = math.sqrt(fem.assemble_l2_error_sq(solver.scalar("c"), exact(T0 + steps * dt)))
    flux.sample(T0 + steps * dt, nu)
    area = float(flux.areas.sum())
    measured = float(flux.totals()[0]) / area
    wall = float((flux.facet_mean().cpu().numpy() * flux.areas).sum()) / area
    return err, measured, film * (wall - c_inf), solver.iteration_counts()["scalar_transport"]["c"]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-N", type=int, action="append", default=None)
    ap.add_argument("--dt", type=float, default=0.002)
    ap.add_argument("-T", type=float, default=0.1)
    ap.add_argument("--kappa", type=float, default=1.0)
    ap.add_argument("--film", type=float, default=2.0, help="h; the Biot number is h L / kappa with L = 1")
    ap.add_argument("--c-inf", type=float, default=0.0)
    ap.add_argument("-u", "--degree", type=int, default=2)
    a = ap.parse_args(argv)
    rows, prev = [], None
    print(f"Bi = {a.film * L / a.kappa:g}, first roots of zeta tan zeta = Bi: "
          + ", ".join(f"{z:.6f}" for z in roots(a.film * L / a.kappa, 3)))
    print(f"{'N':>5} {'L2 error c':>14} {'order':>7} {'ScalarFlux':>14} {'h (c_wall - c_inf)':>20} {'its':>5}")
    for N in a.N or [4, 8, 16]:
        err, measured, film_law, its = run_slab(N, a.dt, a.T, a.kappa, a.film, a.c_inf, degree=a.degree)
        order = "" if prev is None else f"{math.log(prev[1] / err) / math.log(N / prev[0]):.2f}"
        print(f"{N:>5} {err:>14.6e} {order:>7} {measured:>14.6e} {film_law:>20.6e} {its:>5}")
        rows.append((N, err, measured, film_law))
        prev = (N, err)
    return rows


if __name__ == "__main__":
    main()
