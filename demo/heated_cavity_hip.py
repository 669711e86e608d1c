#!/usr/bin/env python3
"""Natural convection in the de Vahl Davis differentially heated square, HIP path.

The unit square with no-slip walls, T = 1 on the wall x = 0, T = 0 on x = 1, adiabatic top and bottom, in diffusion
units: nu = Pr = 0.71, kappa = 1 and the Boussinesq force (0, Ra Pr (T - 1/2)).  The temperature is a
``ScalarTransport(..., buoyancy=(0, Ra Pr), reference=0.5)``: every step adds ``b M (T* - 1/2)`` to the momentum
right-hand side in one pass over the mass matrix (``ox_buoyancy_rows``), with ``T*`` the temperature extrapolated to
the step's midpoint.  ``oasisx_amd.ScalarFlux`` evaluates the heat flux through the hot and the cold wall on the device
after every step; nothing is read back until the end.  The run starts from rest and the conduction profile and is
marched to the steady state; it prints the wall Nusselt numbers, max |u| and max |v| beside the benchmark's values at
Ra = 1e3 (de Vahl Davis 1983: 1.118, 3.649, 3.697).

    python demo/heated_cavity_hip.py [-N 16] [--steps 60] [--dt 0.01] [--Ra 1e3] [--out walls.vtu]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KRYLOV = {"tentative": {"ksp_type": "bcgs", "pc_type": "jacobi", "ksp_rtol": 1e-10, "ksp_atol": 1e-30},
          "pressure": {"ksp_type": "cg", "pc_type": "jacobi", "ksp_rtol": 1e-10, "ksp_atol": 1e-30},
          "scalar": {"ksp_type": "cg", "pc_type": "jacobi", "ksp_rtol": 1e-10, "ksp_atol": 1e-30},
          "scalar_transport": {"ksp_type": "bcgs", "pc_type": "jacobi", "ksp_rtol": 1e-10, "ksp_atol": 1e-30}}
HOT, COLD, ADIABATIC = 1, 2, 3
BENCHMARK = {1e3: (1.118, 3.649, 3.697)}  # Ra: (Nu, max u on x = 1/2, max v on y = 1/2)


def build_cavity(N: int, Ra: float = 1e3, Pr: float = 0.71, solver_options=None, extrapolate: bool = True):
    """(mesh, facet tags, solver, flux): the cavity at rest with the conduction profile T = 1 - x; ``flux`` samples the
    hot and the cold wall (tags HOT, COLD)."""
    import oasisx_amd as ox
    from oasisx_amd import mesh as M

    mesh = M.create_rectangle(None, [[0.0, 0.0], [1.0, 1.0]], [N, N])
    hot = M.locate_entities_boundary(mesh, 1, lambda x: np.isclose(x[0], 0.0))
    cold = M.locate_entities_boundary(mesh, 1, lambda x: np.isclose(x[0], 1.0))
    rest = M.locate_entities_boundary(mesh, 1, lambda x: np.isclose(x[1], 0.0) | np.isclose(x[1], 1.0))
    facets = np.hstack([hot, cold, rest])
    values = np.hstack([np.full_like(hot, HOT), np.full_like(cold, COLD), np.full_like(rest, ADIABATIC)]).astype(np.int32)
    srt = np.argsort(facets)
    tags = M.meshtags(mesh, 1, facets[srt], values[srt])
    G = ox.LocatorMethod.GEOMETRICAL

    def walls(x):
        return np.isclose(x[0], 0.0) | np.isclose(x[0], 1.0) | np.isclose(x[1], 0.0) | np.isclose(x[1], 1.0)

    def heated(x):
        return np.isclose(x[0], 0.0) | np.isclose(x[0], 1.0)

    conduction = lambda x: 1.0 - x[0]  # noqa: E731
    T = ox.ScalarTransport("T", diffusivity=1.0, initial=conduction, bcs=[ox.DirichletBC(conduction, G, heated)],
                           buoyancy=(0.0, Ra * Pr), reference=0.5, extrapolate=extrapolate)
    solver = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_p=[],
                                     bcs_u=[[ox.DirichletBC(0.0, G, walls)] for _ in range(2)],
                                     solver_options=solver_options or KRYLOV, scalars=[T], options={"sell_window": 256})
    flux = ox.ScalarFlux(solver, "T", facets=(tags, (HOT, COLD)))
    return mesh, tags, solver, flux


def nusselt(flux):
    """(hot, cold) wall Nusselt numbers of the latest sample: heat enters through the hot wall (a negative outward flux)
    and leaves through the cold one; wall length, kappa and the temperature difference are 1."""
    hot, cold = flux.totals()
    return -float(hot), float(cold)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-N", type=int, default=16)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--Ra", type=float, default=1e3)
    ap.add_argument("--Pr", type=float, default=0.71)
    ap.add_argument("--out", default=None, help="write the walls' flux as .vtu (and .npz beside it)")
    a = ap.parse_args(argv)
    mesh, tags, solver, flux = build_cavity(a.N, a.Ra, a.Pr)
    for n in range(1, a.steps + 1):
        solver.solve(a.dt, a.Pr, max_iter=1)
        flux.sample(n * a.dt, a.Pr, dt=a.dt)
    nu_hot, nu_cold = nusselt(flux)
    u = solver._U.rhost()
    umax, vmax = float(np.abs(u[:, 0]).max()), float(np.abs(u[:, 1]).max())
    ref = BENCHMARK.get(a.Ra, (float("nan"),) * 3)
    print(f"heated cavity, Ra = {a.Ra:g}, Pr = {a.Pr:g}, N = {a.N}, {a.steps} steps of dt = {a.dt:g}")
    print(f"{'quantity':<22} {'computed':>10} {'benchmark':>10}")
    for name, v, r in (("Nusselt, hot wall", nu_hot, ref[0]), ("Nusselt, cold wall", nu_cold, ref[0]),
                       ("max |u|", umax, ref[1]), ("max |v|", vmax, ref[2])):
        print(f"{name:<22} {v:>10.4f} {r:>10.3f}")
    if a.out:
        flux.save(os.path.splitext(a.out)[0] + ".npz", vtu=a.out, time=a.steps * a.dt)
    return {"nu_hot": nu_hot, "nu_cold": nu_cold, "umax": umax, "vmax": vmax, "history": flux.history()}


if __name__ == "__main__":
    main()
