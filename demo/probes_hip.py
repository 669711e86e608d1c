#!/usr/bin/env python3
"""Probes on the 2-D Taylor-Green vortex, HIP path: a line of points through the vortex sampled every time step.

``oasisx_amd.Probes`` locates the points once (``oasisx_amd.geometry``: the lowest cell id containing each point), keeps
cells, barycentric coordinates and the sort permutation on the device, and ``sample(t)`` enqueues one launch per function
into a device-resident ring -- no host synchronisation, no copy of the dof arrays, and the velocity is read through its
read-only pointer, so the solver's ``A u1`` shortcut survives.  Per step this prints the largest deviation of the sampled
velocity and pressure from the analytic fields on the line.

    python demo/probes_hip.py [-N 32] [--steps 20] [--dt 0.005] [--points 101] [--out probes.npz]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run_probes(N: int = 32, steps: int = 20, dt: float = 0.005, nu: float = 0.01, n_points: int = 101, out: str | None = None):
    """Returns (probes, rows) with rows = [(t, max |u_h - u|, max |p_h - p|)] per step."""
    import oasisx_amd as ox
    from taylor_green_hip import KRYLOV, TaylorGreen2D, build_solver

    field = TaylorGreen2D(nu)
    mesh, solver = build_solver(N, field, 2, KRYLOV, False, False)
    for c in range(2):
        solver._u2[c].interpolate(field.velocity(c, -dt))
        solver._u1[c].interpolate(field.velocity(c, 0.0))
    solver._p.interpolate(field.pressure(-dt / 2.0))
    # a line through the domain that is no mesh line: y = 0.3 x + 0.1
    s = np.linspace(-1.0, 1.0, n_points)
    x = np.stack([s, 0.3 * s + 0.1, np.zeros_like(s)], axis=1)
    probes = ox.Probes(x, [solver.u, solver._p], capacity=8)
    for n in range(1, steps + 1):
        field.now = n * dt
        solver.solve(dt, nu, max_iter=1)
        probes.sample(field.now)
    values = probes.array()  # (steps, n_points, 3): the only transfer to the host
    X = x.T
    rows = []
    for n, t in enumerate(probes.times):
        eu = max(float(np.abs(values[n, :, c] - field.velocity(c, t)(X)).max()) for c in range(2))
        ep = float(np.abs(values[n, :, 2] - field.pressure(t - dt / 2.0)(X)).max())
        rows.append((float(t), eu, ep))
    if out:
        probes.save(out)
    return probes, rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-N", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--dt", type=float, default=0.005)
    ap.add_argument("--nu", type=float, default=0.01)
    ap.add_argument("--points", type=int, default=101)
    ap.add_argument("--out", default=None, help="write the samples to this .npz")
    a = ap.parse_args(argv)
    probes, rows = run_probes(a.N, a.steps, a.dt, a.nu, a.points, a.out)
    for t, eu, ep in rows:
        print(f"t = {t:.4f}  max |u_h - u| = {eu:.3e}  max |p_h - p| = {ep:.3e}")
    print(f"{probes.n_samples} samples of {probes.n_points} points x {probes.n_values} values, ring capacity {probes.capacity}")
    return rows


if __name__ == "__main__":
    main()
