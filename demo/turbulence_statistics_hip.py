#!/usr/bin/env python3
"""LES Taylor-Green with flow diagnostics and running statistics on the device, HIP path.

The set-up of demo/les_taylor_green_hip.py (Smagorinsky on [-1, 1]^3) with a ``FlowDiagnostics`` and a ``FlowStatistics``
object sampling every step: nothing is read back while the run goes on.  Afterwards the ring is read once and printed per
step -- kinetic energy, its rate dE/dt (backward difference) against -dissipation (resolved + modelled: (nu + nut) 2 S:S;
the boundary is driven, so the two agree only roughly), enstrophy, ||div u||, max CFL -- and the time means, the turbulent
kinetic energy and the Q-criterion of the last step are written for ParaView.

    python demo/turbulence_statistics_hip.py [-N 16] [--steps 10] [--dt 0.005] [--nu 0.01] [--Cs 0.1677] [--out results_stats]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-N", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--dt", type=float, default=0.005)
    ap.add_argument("--nu", type=float, default=0.01)
    ap.add_argument("--Cs", type=float, default=0.1677)
    ap.add_argument("--out", default="results_stats")
    a = ap.parse_args(argv)
    import oasisx_amd as ox
    from les_taylor_green_hip import on_boundary
    from oasisx_amd import mesh as M
    from taylor_green_hip import KRYLOV, TaylorGreen2D

    field = TaylorGreen2D(a.nu)
    zero = lambda x: np.zeros_like(x[0])  # noqa: E731

    def velocity(c, t=None):
        return field.velocity(c, t) if c < 2 else zero

    mesh = M.create_box(None, [[-1.0] * 3, [1.0] * 3], [a.N] * 3)
    G = ox.LocatorMethod.GEOMETRICAL
    solver = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_p=[],
                                     bcs_u=[[ox.DirichletBC(velocity(c), G, on_boundary)] for c in range(3)],
                                     solver_options=KRYLOV, viscosity_model=ox.Smagorinsky(Cs=a.Cs))
    for c in range(3):
        solver._u2[c].interpolate(velocity(c, -a.dt))
        solver._u1[c].interpolate(velocity(c, 0.0))
    solver._p.interpolate(field.pressure(-a.dt / 2.0))
    diag = ox.FlowDiagnostics(solver, fields=("q_criterion", "vorticity", "cfl"))
    stats = ox.FlowStatistics(solver, fields=("u", "p"))
    for n in range(1, a.steps + 1):
        field.now = n * a.dt
        solver.solve(a.dt, a.nu, max_iter=1)
        diag.sample(n * a.dt, a.dt, a.nu)  # two launches, no synchronisation
        stats.sample(a.dt)  # one launch per field
    h = diag.history()  # the one read-back
    print(f"--- Smagorinsky(Cs={a.Cs}): N = {a.N}, dt = {a.dt}, nu = {a.nu}; volume {h['volume'][-1]:.12f}")
    print(f"{'step':>5} {'kinetic energy':>20} {'dE/dt':>13} {'-dissipation':>13} {'enstrophy':>13} {'||div u||':>11} {'max CFL':>9}")
    rows = []
    for k in range(a.steps):
        dedt = (h["kinetic_energy"][k] - h["kinetic_energy"][k - 1]) / a.dt if k else float("nan")
        rows.append(dict(step=k + 1, energy=float(h["kinetic_energy"][k]), dedt=float(dedt), dissipation=float(h["dissipation"][k]),
                         enstrophy=float(h["enstrophy"][k]), div_l2=float(h["div_l2"][k]), cfl_max=float(h["cfl_max"][k])))
        print(f"{k + 1:>5} {h['kinetic_energy'][k]:>20.12e} {dedt:>13.5e} {-h['dissipation'][k]:>13.5e} {h['enstrophy'][k]:>13.5e} "
              f"{h['div_l2'][k]:>11.3e} {h['cfl_max'][k]:>9.4f}")
    os.makedirs(a.out, exist_ok=True)
    with ox.io.VTXWriter(None, os.path.join(a.out, "mean_u.bp"), [stats.mean("u"), stats.tke()]) as w:
        w.write(a.steps * a.dt)
    with ox.io.VTXWriter(None, os.path.join(a.out, "mean_p.bp"), [stats.mean("p")]) as w:
        w.write(a.steps * a.dt)
    ox.io.write_cell_vtu(os.path.join(a.out, "q_criterion.vtu"), mesh,
                         {"q_criterion": diag.cell_field("q_criterion"), "vorticity": diag.cell_field("vorticity"),
                          "cfl": diag.cell_field("cfl"), "nut": solver.eddy_viscosity()}, time=a.steps * a.dt)
    diag.save(os.path.join(a.out, "diagnostics.npz"))
    stats.save(os.path.join(a.out, "statistics.npz"))
    tke = stats.tke()._storage.rhost()
    print(f"mean over T = {stats.total_weight:g}: max TKE = {float(tke.max()):.4e}; files in {a.out}/")
    return dict(rows=rows, out=a.out, tke_max=float(tke.max()), total_weight=stats.total_weight)


if __name__ == "__main__":
    main()
