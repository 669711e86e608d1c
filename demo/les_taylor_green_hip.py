#!/usr/bin/env python3
"""3-D Taylor-Green with and without a Smagorinsky eddy viscosity, HIP path.

The z-extruded Taylor-Green vortex on [-1, 1]^3 (exact Dirichlet velocity, no pressure condition) is marched twice from
the same initial data: with the constant viscosity alone, and with ``viscosity_model=oasisx_amd.Smagorinsky(Cs)``, whose
``nut`` per cell is evaluated from the extrapolated velocity of every step (``ox_cell_viscosity``) and added by the fused
assembly kernel.  Per step the kinetic energy (1/2) u^T M u and the minimum / mean / maximum of ``nut`` are printed: the
model takes energy out of the resolved field, so its run ends below the other.

    python demo/les_taylor_green_hip.py [-N 16] [--steps 10] [--dt 0.005] [--nu 0.01] [--Cs 0.1677] [--wale] [--periodic]

``--periodic``: the box periodic in all three axes (``oasisx_amd.mesh.make_periodic``) instead of the exact velocity pinned
on its six faces -- the set-up the Taylor-Green vortex is usually run in; no Dirichlet condition at all.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def on_boundary(x):
    return np.isclose(np.abs(x[0]), 1.0) | np.isclose(np.abs(x[1]), 1.0) | np.isclose(np.abs(x[2]), 1.0)


def kinetic_energy(solver) -> float:
    """(1/2) sum_d u_d^T M u_d with the assembled mass matrix, on the device."""
    import torch

    u = solver._U.rdev()
    Mu = torch.zeros_like(u)
    solver._M.mult(u, Mu, u.shape[1])
    n = solver._no_u
    return 0.5 * float((u[:n] * Mu[:n]).sum())


def run(N: int, model, steps: int, dt: float, nu: float, degree_u: int = 2, periodic: bool = False):
    """``steps`` steps on the N^3 box; returns one record per step: energy and, with a model, min / mean / max of nut."""
    import oasisx_amd as ox
    from oasisx_amd import mesh as M
    from taylor_green_hip import KRYLOV, TaylorGreen2D

    field = TaylorGreen2D(nu)
    zero = lambda x: np.zeros_like(x[0])  # noqa: E731

    def velocity(c, t=None):
        return field.velocity(c, t) if c < 2 else zero

    mesh = M.create_box(None, [[-1.0] * 3, [1.0] * 3], [N, N, N])
    G = ox.LocatorMethod.GEOMETRICAL
    kw = {} if model is None else {"viscosity_model": model}
    if periodic:
        mesh = M.make_periodic(mesh, (0, 1, 2))
        bcs_u = [[], [], []]
    else:
        bcs_u = [[ox.DirichletBC(velocity(c), G, on_boundary)] for c in range(3)]
    solver = ox.FractionalStep_AB_CN(mesh, ("Lagrange", degree_u), ("Lagrange", degree_u - 1), bcs_p=[], bcs_u=bcs_u,
                                     solver_options=KRYLOV, **kw)
    for c in range(3):
        solver._u2[c].interpolate(velocity(c, -dt))
        solver._u1[c].interpolate(velocity(c, 0.0))
    solver._p.interpolate(field.pressure(-dt / 2.0))
    rows = []
    for n in range(1, steps + 1):
        field.now = n * dt
        solver.solve(dt, nu, max_iter=1)
        rec = {"step": n, "energy": kinetic_energy(solver)}
        if model is not None:
            nut = solver.eddy_viscosity()
            rec.update(nut_min=float(nut.min()), nut_mean=float(nut.mean()), nut_max=float(nut.max()))
        rows.append(rec)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-N", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--dt", type=float, default=0.005)
    ap.add_argument("--nu", type=float, default=0.01)
    ap.add_argument("--Cs", type=float, default=0.1677)
    ap.add_argument("--wale", action="store_true", help="also run WALE (Cw = 0.325)")
    ap.add_argument("--periodic", action="store_true", help="periodic in x, y and z instead of exact Dirichlet data")
    a = ap.parse_args(argv)
    import oasisx_amd as ox

    models = {"none": None, "smagorinsky": ox.Smagorinsky(Cs=a.Cs)}
    if a.wale:
        models["wale"] = ox.Wale()
    out = {}
    for name, model in models.items():
        print(f"--- {name}: N = {a.N}, dt = {a.dt}, nu = {a.nu}" + ("" if model is None else f", {model!r}")
              + (", periodic" if a.periodic else ""))
        print(f"{'step':>5} {'kinetic energy':>20} {'nut min':>12} {'nut mean':>12} {'nut max':>12}")
        out[name] = run(a.N, model, a.steps, a.dt, a.nu, periodic=a.periodic)
        for r in out[name]:
            nut = "" if model is None else f" {r['nut_min']:>12.4e} {r['nut_mean']:>12.4e} {r['nut_max']:>12.4e}"
            print(f"{r['step']:>5} {r['energy']:>20.12e}{nut}")
    return out


if __name__ == "__main__":
    main()
