#!/usr/bin/env python3
"""A scalar under Smagorinsky with van Driest damping: turbulent Schmidt number on the periodic channel, HIP path.

The channel of demo/les_channel_hip.py at its Poiseuille state u_x = G y (H - y) / (2 nu), with a scalar held at 0 on the
wall y = 0 and at 1 on the wall y = H (initially the conduction profile c = y / H) and
``ScalarTransport(..., turbulent_schmidt=Sc_t)``: the scalar's diffusivity is ``kappa + nut_c / Sc_t`` per cell, with the
``nut`` of the damped model, whose closed form at this state is (demo/les_channel_hip.py)

    nut_c = Cs^2 Delta_c^2 D(y_c)^2 G |H - 2 y_c| / (2 nu),      D = 1 - exp(-y+ / A+),  y+ = d sqrt(G H / 2) / nu.

``assemble_first`` forms the scalar's operator ``A_c = A + s K + t K_t`` in one launch (``ox_scalar_rows_cellvisc``: the rows of
``K_t = sum_c nut_c K_c`` once more, in LDS).  Printed: per slab of cells across the channel the mean of
``solver.scalar_diffusivity("c", nu)`` beside the closed form ``kappa + nut(y) / Sc_t``, and the two wall fluxes from
``oasisx_amd.ScalarFlux`` -- ``-(kappa + nut_c / Sc_t) n . grad c`` with the ``nut`` of the wall's cells -- before and after
the steps.

    python demo/les_scalar_channel_hip.py [-N 8] [--dim 2] [--nu 0.01] [-G 0.02] [--Cs 0.17] [--A-plus 26] [--kappa 0.005]
                                          [--Sct 0.7] [--steps 2]
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
LOWER, UPPER = 1, 2


def walls(x):
    return np.isclose(x[1], 0.0) | np.isclose(x[1], H)


def build_channel(N: int, dim: int, G: float, model, kappa: float, sct: float, L: float = 2.0, W: float = 1.0):
    """(mesh, solver, flux): the periodic channel with the scalar ``c`` and its flux through the two walls."""
    import oasisx_amd as ox
    from oasisx_amd import mesh as M

    if dim == 2:
        mesh = M.make_periodic(M.create_rectangle(None, [[0.0, 0.0], [L, H]], [max(3, N), N]), (0,))
    else:
        mesh = M.make_periodic(M.create_box(None, [[0.0, 0.0, 0.0], [L, H, W]], [max(3, N), N, max(3, N)]), (0, 2))
    lower = M.locate_entities_boundary(mesh, dim - 1, lambda x: np.isclose(x[1], 0.0))
    upper = M.locate_entities_boundary(mesh, dim - 1, lambda x: np.isclose(x[1], H))
    facets = np.hstack([lower, upper])
    values = np.hstack([np.full_like(lower, LOWER), np.full_like(upper, UPPER)]).astype(np.int32)
    srt = np.argsort(facets)
    tags = M.meshtags(mesh, dim - 1, facets[srt], values[srt])
    geo = ox.LocatorMethod.GEOMETRICAL
    profile = lambda x: x[1] / H  # noqa: E731
    c = ox.ScalarTransport("c", diffusivity=kappa, initial=profile, bcs=[ox.DirichletBC(profile, geo, walls)],
                           turbulent_schmidt=sct)
    noslip = [[ox.DirichletBC(0.0, geo, walls)] for _ in range(dim)]
    solver = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_u=noslip, bcs_p=[], solver_options=KRYLOV,
                                     body_force=(G,) + (0.0,) * (dim - 1), viscosity_model=model, scalars=[c])
    flux = ox.ScalarFlux(solver, "c", facets=(tags, (LOWER, UPPER)))
    return mesh, solver, flux


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-N", type=int, default=8, help="cells across the channel")
    ap.add_argument("--dim", type=int, default=2, choices=[2, 3])
    ap.add_argument("--nu", type=float, default=0.01)
    ap.add_argument("-G", type=float, default=0.02, help="body force along x")
    ap.add_argument("--Cs", type=float, default=0.17)
    ap.add_argument("--A-plus", type=float, default=26.0)
    ap.add_argument("--kappa", type=float, default=0.005)
    ap.add_argument("--Sct", type=float, default=0.7)
    ap.add_argument("--dt", type=float, default=0.05)
    ap.add_argument("--steps", type=int, default=2)
    a = ap.parse_args(argv)
    import torch

    import oasisx_amd as ox
    from les_channel_hip import closed_form

    model = ox.Smagorinsky(a.Cs, damping=ox.VanDriest(None, A_plus=a.A_plus))
    mesh, S, flux = build_channel(a.N, a.dim, a.G, model, a.kappa, a.Sct)
    for u in (S._u[0], S._u1[0], S._u2[0]):
        u.interpolate(lambda x: a.G * x[1] * (H - x[1]) / (2.0 * a.nu))
    S.assemble_first(a.dt, a.nu)
    kap = S.scalar_diffusivity("c", a.nu).cpu().numpy()
    flux.sample(0.0, a.nu)
    first = flux.totals().copy()
    cells = mesh.cells.to(torch.int64)
    X = mesh.coords[cells].cpu().numpy()  # (nc, d + 1, d)
    y = X.mean(axis=1)[:, 1]
    e = X[:, 1:] - X[:, :1]
    vol = np.abs(np.linalg.det(e)) / (2.0 if a.dim == 2 else 6.0)
    turb = closed_form(a.Cs, vol ** (2.0 / a.dim), y, a.G, a.nu, a.A_plus) / a.Sct
    ref = a.kappa + turb
    err = float(np.abs(kap - ref).max())
    err_turb = float(np.abs((kap - a.kappa) - turb).max())  # the turbulent part alone, beside its own size
    slab = np.minimum((y / H * a.N).astype(int), a.N - 1)
    print(f"LES channel with a scalar, {a.dim}-D: {mesh.num_cells} cells, kappa = {a.kappa}, Sc_t = {a.Sct}, "
          f"{flux.n_facets} wall facets")
    print(f"{'slab':>5} {'y':>8} {'kappa + nut/Sc_t':>18} {'closed form':>14}")
    rows = []
    for k in range(a.N):
        m = slab == k
        rows.append({"slab": k, "y": float(y[m].mean()), "diffusivity": float(kap[m].mean()), "closed_form": float(ref[m].mean())})
        r = rows[-1]
        print(f"{k:>5} {r['y']:>8.4f} {r['diffusivity']:>18.6e} {r['closed_form']:>14.6e}")
    print(f"max |scalar_diffusivity - closed form| = {err:.3e} (max {ref.max():.3e}, kappa {a.kappa:.3e}); turbulent part alone "
          f"{err_turb:.3e} of max nut / Sc_t = {turb.max():.3e}")
    t = 0.0
    for _ in range(a.steps):
        S.solve(a.dt, a.nu, max_iter=1)
        t += a.dt
        flux.sample(t, a.nu, dt=a.dt)
    last = flux.totals()
    area = 2.0  # L = 2 (x W = 1 in 3-D)
    print(f"wall fluxes (sum |f| q; conduction alone: {a.kappa * area / H:.6e}): lower {first[0]:+.6e}, upper {first[1]:+.6e} "
          f"at t = 0; lower {last[0]:+.6e}, upper {last[1]:+.6e} after {a.steps} steps")
    return {"rows": rows, "error": err, "diffusivity_max": float(ref.max()), "kappa": a.kappa,
            "error_turbulent": err_turb, "turbulent_max": float(turb.max()),
            "flux_first": (float(first[0]), float(first[1])), "flux_last": (float(last[0]), float(last[1]))}


if __name__ == "__main__":
    main()
