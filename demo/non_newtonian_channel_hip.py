#!/usr/bin/env python3
"""Plane channel flow of a power-law fluid, HIP path.

The channel [0, 4] x [-1, 1], P2-P1, driven by a constant body force (G, 0) between no-slip walls.  The viscosity is
``oasisx_amd.PowerLaw(k, n, nu_min, nu_max)``: nu(gd) = k gd^(n - 1) of the shear rate gd = sqrt(2 S:S), evaluated per cell
from the extrapolated velocity of every step (``ox_cell_viscosity``) and added by the fused assembly kernel; the solver
runs at nu = ``base_viscosity`` = nu_min.  With p = 0 the steady solution is

    u(y) = n / (n + 1) (G / k)^(1 / n) (1 - |y|^((n + 1) / n)),        v = 0

(the Newtonian parabola for n = 1; blunter for a shear-thinning fluid, n < 1), which is also the Dirichlet datum at the
inlet and at the outlet.  The run starts from the Newtonian parabola with the same centre-line velocity and is stepped
to a steady state; per N this prints the L2 error of the velocity against the analytic profile and, on a line of probes
across the channel at x = 2, the distance to the power-law profile and to the parabola it started from.  The viscosity
is constant per cell (its value at the centroid) and clipped at nu_max around the centre line, where gd -> 0: the error
falls with N, no rate is claimed.

The flow is unidirectional, so the transposed term of the full stress form vanishes in the continuum and the default
here is ``stress_form="laplacian"``.  ``--stress-form full`` is there to look at the explicit treatment of that term: it
is conditionally stable, and with nut up to 250 nu as in this channel it is not stable at this time step (DESIGN.md
section 16).

    python demo/non_newtonian_channel_hip.py [-N 8 16] [--steps 120] [--dt 0.05] [-n 0.5] [-k 0.5] [--stress-form laplacian]
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
LENGTH = 4.0


def power_law_profile(y, G: float, k: float, n: float):
    """u(y) = n / (n + 1) (G / k)^(1 / n) (1 - |y|^((n + 1) / n))."""
    return n / (n + 1.0) * (G / k) ** (1.0 / n) * (1.0 - np.abs(y) ** ((n + 1.0) / n))


def parabola(y, G: float, k: float, n: float):
    """The Newtonian parabola with the centre-line velocity of the power-law profile."""
    return power_law_profile(0.0, G, k, n) * (1.0 - np.asarray(y) ** 2)


def build_channel(N: int, G: float, k: float, n: float, nu_min: float, nu_max: float, stress_form: str = "laplacian"):
    """(mesh, solver, law): Dirichlet data on the whole boundary -- no slip on the walls, the analytic profile at the two
    ends --, every velocity level on the Newtonian parabola, p = 0."""
    import oasisx_amd as ox
    from oasisx_amd import mesh as M

    mesh = M.create_rectangle(None, [[0.0, -1.0], [LENGTH, 1.0]], [2 * N, N])
    law = ox.PowerLaw(k, n, nu_min, nu_max)
    edge = lambda x: np.isclose(np.abs(x[1]), 1.0) | np.isclose(x[0], 0.0) | np.isclose(x[0], LENGTH)  # noqa: E731
    bc_u = ox.DirichletBC(lambda x: power_law_profile(x[1], G, k, n), ox.LocatorMethod.GEOMETRICAL, edge)
    bc_v = ox.DirichletBC(lambda x: 0.0 * x[0], ox.LocatorMethod.GEOMETRICAL, edge)
    solver = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_u=[[bc_u], [bc_v]], bcs_p=[],
                                     solver_options=KRYLOV, body_force=(G, 0.0), options={"sell_window": 256},
                                     viscosity_model=law, stress_form=stress_form)
    for level in (solver._u, solver._u1, solver._u2):
        level[0].interpolate(lambda x: parabola(x[1], G, k, n))
        level[1].interpolate(lambda x: 0.0 * x[0])
    solver._p.interpolate(lambda x: 0.0 * x[0])
    return mesh, solver, law


def l2_error(solver, G: float, k: float, n: float) -> float:
    """sqrt(sum_i e_i^T M e_i), e = u_h - I_h u: the L2 norm of the error against the interpolated analytic profile."""
    import torch

    Vi = solver._Vi[0][0]
    e = solver._U.rdev().clone()
    y = Vi.x[:, 1].cpu().numpy()
    e[:, 0] -= torch.from_numpy(power_law_profile(y, G, k, n)).to(e.device)
    Me = torch.zeros_like(e)
    solver._M.mult(e, Me, 2)
    return float(torch.sqrt((e[: Vi.n_owned] * Me[: Vi.n_owned]).sum()))


def run(N: int = 8, steps: int = 120, dt: float = 0.05, G: float = 1.0, k: float = 0.5, n: float = 0.5,
        nu_min: float = 0.01, nu_max: float = 5.0, stress_form: str = "laplacian", n_probes: int = 41):
    """One run to a steady state.  Returns dict(N, l2, y, u, to_power_law, to_parabola, nu_min, nu_max, change): the L2
    error, the probed profile u(y) at x = 2 and its root-mean-square distance over the probes to the two profiles, the
    range of the effective viscosity and the last change of the velocity per step."""
    import oasisx_amd as ox

    mesh, solver, law = build_channel(N, G, k, n, nu_min, nu_max, stress_form)
    change = 0.0
    for _ in range(steps):
        change = solver.solve(dt, law.base_viscosity, max_iter=1)
    y = np.linspace(-1.0, 1.0, n_probes)
    pts = np.stack([np.full_like(y, 0.5 * LENGTH), y, np.zeros_like(y)], axis=1)
    probes = ox.Probes(pts, [solver.u], capacity=1)
    probes.sample(steps * dt)
    u = probes.array()[0, :, 0]
    nu_eff = solver.effective_viscosity()
    rms = lambda d: float(np.sqrt(np.mean(d * d)))  # noqa: E731
    return dict(N=N, l2=l2_error(solver, G, k, n), y=y, u=u, to_power_law=rms(u - power_law_profile(y, G, k, n)),
                to_parabola=rms(u - parabola(y, G, k, n)), nu_min=float(nu_eff.min()), nu_max=float(nu_eff.max()),
                change=float(change))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-N", type=int, nargs="+", default=[8, 16], help="cells across the channel (one run each)")
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--dt", type=float, default=0.05)
    ap.add_argument("-G", type=float, default=1.0, help="body force")
    ap.add_argument("-k", type=float, default=0.5, help="consistency")
    ap.add_argument("-n", type=float, default=0.5, help="power-law index")
    ap.add_argument("--nu-min", type=float, default=0.01)
    ap.add_argument("--nu-max", type=float, default=5.0)
    ap.add_argument("--stress-form", default="laplacian", choices=["laplacian", "full"])
    a = ap.parse_args(argv)
    print(f"power-law channel: n = {a.n}, k = {a.k}, G = {a.G}; centre-line velocity "
          f"{power_law_profile(0.0, a.G, a.k, a.n):.6f}; stress_form = {a.stress_form}")
    rows = []
    for N in a.N:
        r = run(N, a.steps, a.dt, a.G, a.k, a.n, a.nu_min, a.nu_max, a.stress_form)
        rows.append(r)
        print(f"N = {N:3d}  L2 error = {r['l2']:.4e}  probes at x = 2: rms to the power-law profile {r['to_power_law']:.4e}, "
              f"to the Newtonian parabola {r['to_parabola']:.4e}  nu in [{r['nu_min']:.4f}, {r['nu_max']:.4f}]  "
              f"last change per step {r['change']:.2e}")
    return rows


if __name__ == "__main__":
    main()
