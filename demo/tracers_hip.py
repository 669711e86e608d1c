#!/usr/bin/env python3
"""Residence times in a 2-D channel from Lagrangian tracers, HIP path.

A channel [0, L] x [0, 1]: a parabolic inlet profile of unit flow rate, no-slip walls and p = 0 at the outlet.  Particles
are seeded on a line just behind the inlet and re-injected every ``--every`` steps; after every ``solve`` one
``Tracers.advance(dt)`` carries them through the step's velocity (u^n -> u^{n+1}, RK4) in one kernel, without a host
synchronisation and without touching u.  A particle that crosses the outlet -- or touches a wall -- is frozen with its
exit time; its age then is its residence time.  The summary line prints the fraction that exited and the mean and maximum
residence time of the exited ones; the recorded trajectories go to ``--out`` (npz).

    python demo/tracers_hip.py [-N 16] [--steps 200] [--dt 0.02] [--nu 0.1] [--every 20] [--seeds 64] [--out tracers.npz]
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


def run_tracers(N: int = 16, steps: int = 200, dt: float = 0.02, nu: float = 0.1, L: float = 2.0, every: int = 20,
                seeds: int = 64, out: str | None = None, record_every: int = 5):
    """Returns (tracers, summary) with summary = dict(n, exited, fraction, mean, max)."""
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
    profile = lambda x: 6.0 * x[1] * (1.0 - x[1])  # noqa: E731  (unit flow rate)
    noslip = ox.DirichletBC(0.0, ox.LocatorMethod.TOPOLOGICAL, (tags, WALLS))
    inlet_x = ox.DirichletBC(profile, ox.LocatorMethod.TOPOLOGICAL, (tags, INLET))
    inlet_y = ox.DirichletBC(0.0, ox.LocatorMethod.TOPOLOGICAL, (tags, INLET))
    solver = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_u=[[inlet_x, noslip], [inlet_y, noslip]],
                                     bcs_p=[ox.PressureBC(0.0, (tags, OUTLET))], solver_options=KRYLOV,
                                     options={"sell_window": 256})
    for level in (solver._u, solver._u1, solver._u2):  # the developed profile everywhere
        level[0].interpolate(profile)
        level[1].interpolate(lambda x: 0.0 * x[0])
    line = np.stack([np.full(seeds, 0.05 * L / 2.0), (np.arange(seeds) + 0.5) / seeds], axis=1)
    tracers = ox.Tracers(solver, line, scheme="rk4")
    tracers.record()
    for n in range(1, steps + 1):
        solver.solve(dt, nu, max_iter=1)
        tracers.advance(dt)
        if n % record_every == 0:
            tracers.record()
        if every and n % every == 0 and n < steps:
            tracers.inject(line)
    status, age = tracers.status(), tracers.age()  # the only transfers
    gone = status == 1
    summary = dict(n=int(status.shape[0]), exited=int(gone.sum()), fraction=float(gone.mean()),
                   mean=float(age[gone].mean()) if gone.any() else float("nan"),
                   max=float(age[gone].max()) if gone.any() else float("nan"), invalid=int((status == 2).sum()))
    if out:
        tracers.save(out)
    return tracers, summary


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-N", type=int, default=16, help="cells across the channel")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--dt", type=float, default=0.02)
    ap.add_argument("--nu", type=float, default=0.1)
    ap.add_argument("--every", type=int, default=20, help="re-inject the seed line every so many steps (0: never)")
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--out", default="tracers.npz")
    a = ap.parse_args(argv)
    tracers, s = run_tracers(a.N, a.steps, a.dt, a.nu, every=a.every, seeds=a.seeds, out=a.out)
    print(f"{s['n']} particles, {s['exited']} exited ({100.0 * s['fraction']:.1f} %), residence time of the exited: mean "
          f"{s['mean']:.4f}, max {s['max']:.4f}; {tracers.n_records} records in {a.out}")
    return s


if __name__ == "__main__":
    main()
