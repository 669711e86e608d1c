#!/usr/bin/env python3
"""Pulsatile channel flow into a three-element Windkessel, HIP path.

A 2-D channel [0, L] x [0, 1]: a parabolic inlet profile whose flow rate pulsates, q(t) = q0 + q1 sin(2 pi t / T), no-slip
walls, and at the outlet a ``PressureBC`` whose value is an RCR ``Windkessel`` with ``backflow=0.5``.  Every step the
solver takes the flow rate of the last finished step through the outlet facets, advances the capacitor pressure Pc by
backward Euler and writes h = (Pc + Rp Q) / rho on the outlet's pressure dofs -- two small launches, nothing is read
back; the backflow term keeps the step stable should the flow re-enter through the outlet.  ``oasisx_amd.FlowRate``
samples the rates through inlet and outlet after every step.  Per step this prints the outlet's Q, P and Pc and the rates
of the sampled velocity; the history is read once, after the loop.

    python demo/windkessel_channel_hip.py [-N 16] [--steps 20] [--dt 0.01] [--nu 0.1]
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


def run(N: int = 16, steps: int = 20, dt: float = 0.01, nu: float = 0.1, L: float = 2.0, period: float = 0.5,
        q0: float = 0.6, q1: float = 0.5, Rp: float = 0.01, C: float = 1.0, Rd: float = 0.1, backflow: float = 0.5):
    """Returns (model, flow, rows) with rows = [dict(t, Q, P, Pc, Q_in, Q_out, umax)] per step.  Pressures are gauged to
    the mean flow (p_distal = -Rd q0, so P = Rp q0 at the mean rate) and the resistances are small: h enters the step
    through the outlet term it has from the reference, int h n_i dv/dx_i ds, under which a pressure of order one drives the
    outlet's flow away from the inlet's within a few steps (DESIGN.md section 17 has the figures); max |u| is printed so
    that this shows."""
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
    clock = {"t": 0.0}
    rate = lambda t: q0 + q1 * np.sin(2.0 * np.pi * t / period)  # noqa: E731
    profile = lambda x: 6.0 * rate(clock["t"]) * x[1] * (1.0 - x[1])  # noqa: E731  (int_0^1 6 y (1 - y) dy = 1)
    noslip = ox.DirichletBC(0.0, ox.LocatorMethod.TOPOLOGICAL, (tags, WALLS))
    inlet_x = ox.DirichletBC(profile, ox.LocatorMethod.TOPOLOGICAL, (tags, INLET))
    inlet_y = ox.DirichletBC(0.0, ox.LocatorMethod.TOPOLOGICAL, (tags, INLET))
    # gauge: the capacitor rests at 0 under the mean flow
    model = ox.Windkessel(Rp, C, Rd, p_distal=-Rd * q0, p0=0.0, rho=1.0)
    solver = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_u=[[inlet_x, noslip], [inlet_y, noslip]],
                                     bcs_p=[ox.PressureBC(model, (tags, OUTLET), backflow=backflow)],
                                     solver_options=KRYLOV, options={"sell_window": 256})
    for level in (solver._u, solver._u1, solver._u2):  # the developed profile of the mean flow everywhere
        level[0].interpolate(profile)
        level[1].interpolate(lambda x: 0.0 * x[0])
    solver._p.interpolate(lambda x: Rp * q0 + 0.0 * x[0])
    flow = ox.FlowRate(solver, facets=(tags, (INLET, OUTLET)), capacity=8)
    umax = []
    for n in range(1, steps + 1):
        clock["t"] = n * dt
        solver.solve(dt, nu, max_iter=1)
        flow.sample(clock["t"])
        umax.append(solver._U.rdev().abs().max())  # (a device scalar: read after the loop)
    H, Qs = model.history(), flow.rates()  # the only transfers
    rows = [dict(t=float(H["times"][k]), Q=float(H["Q"][k]), P=float(H["P"][k]), Pc=float(H["Pc"][k]),
                 Q_in=float(Qs[k, 0]), Q_out=float(Qs[k, 1]), umax=float(umax[k])) for k in range(steps)]
    return model, flow, rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-N", type=int, default=16, help="cells across the channel")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--nu", type=float, default=0.1)
    a = ap.parse_args(argv)
    model, flow, rows = run(a.N, a.steps, a.dt, a.nu)
    print(f"{flow.n_facets} facets on inlet and outlet; Windkessel Rp = {model.Rp}, C = {model.C}, Rd = {model.Rd}; "
          "Q, P, Pc: the model's step (Q of the last finished step); Q_in, Q_out: the rates of the step's velocity")
    for r in rows:
        print(f"t = {r['t']:.4f}  Q = {r['Q']:+.6f}  P = {r['P']:.6f}  Pc = {r['Pc']:.6f}  "
              f"Q_in = {r['Q_in']:+.6f}  Q_out = {r['Q_out']:+.6f}  max |u| = {r['umax']:.4f}")
    return rows


if __name__ == "__main__":
    main()
