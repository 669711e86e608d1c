#!/usr/bin/env python3
"""Sedimentation of inertial particles in plane Poiseuille flow along a channel that is periodic along the stream, HIP path.

The channel [0, L] x [-1, 1] is periodic in x (``oasisx_amd.mesh.make_periodic``); the fluid moves with
U(y) = U0 (1 - y^2), which a P2 field holds exactly, and gravity (0, -g) points at the lower wall.  The particles
(``oasisx_amd.InertialParticles``, Stokes drag) start at rest across the stream.  Because u_y = 0, the wall-normal motion
decouples from the streamwise one,

    y(t) = y0 - w_s (t - tau (1 - e^{-t / tau})),      w_s = tau (1 - rho_f / rho_p) g,

so every particle's deposition time -- y(t_d) = -1 -- is known in closed form, and the exponential integrator follows y(t)
exactly whatever the step: a particle is caught at the start of the first substep whose end lies below the wall.  The run
prints the deposited fraction against time beside the closed form, checks every exit time against its t_d to within one
substep, and reports the mean streamwise distance travelled (through ``unfolded_positions``: the particles wrap).

    python demo/particle_deposition_hip.py [-N 8] [--steps 40] [--dt 0.05] [--substeps 2] [--seeds 256] [--out FILE.vtu]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def lower_wall(x):
    return np.isclose(x[1], -1.0)


def build_channel(N: int, U0: float = 1.0, L: float = 3.0):
    """(mesh, the Poiseuille field, meshtags with the lower wall as 1)."""
    from oasisx_amd import fem
    from oasisx_amd import mesh as M

    mesh = M.make_periodic(M.create_rectangle(None, [[0.0, -1.0], [L, 1.0]], [max(3, N), N]), (0,))
    W = fem.VectorFunctionSpace(fem.FunctionSpace(mesh, 2, window=128), 2)
    u = fem.Function(W)
    u.interpolate(lambda x: np.stack([U0 * (1.0 - x[1] ** 2), 0.0 * x[0]]))
    facets = M.locate_entities_boundary(mesh, 1, lower_wall)
    tags = M.meshtags(mesh, 1, facets, np.full(facets.shape[0], 1, dtype=np.int32))
    return mesh, u, tags


def settled(t, tau, ws):
    """The distance a particle released at rest has fallen by t."""
    return ws * (t - tau * (-np.expm1(-t / tau))) if tau > 0.0 else ws * t


def deposition_time(drop, tau, ws):
    """t_d with settled(t_d) = drop, per particle (bisection on a monotone function; inf where ws = 0)."""
    drop = np.asarray(drop, dtype=np.float64)
    if not ws > 0.0:
        return np.full(drop.shape, np.inf)
    lo, hi = np.zeros_like(drop), drop / ws + tau + 1.0  # settled(hi) >= ws (hi - tau) > drop
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        below = settled(mid, tau, ws) < drop
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    return 0.5 * (lo + hi)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-N", type=int, default=8, help="cells across the channel")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--dt", type=float, default=0.05)
    ap.add_argument("--substeps", type=int, default=2)
    ap.add_argument("--seeds", type=int, default=256)
    ap.add_argument("--diameter", type=float, default=0.03)
    ap.add_argument("--density", type=float, default=1000.0)
    ap.add_argument("--nu", type=float, default=0.1)
    ap.add_argument("-g", type=float, default=2.0, help="gravity towards the lower wall")
    ap.add_argument("--out", default=None, help="write the deposition count per wall facet to this .vtu")
    a = ap.parse_args(argv)
    import oasisx_amd as ox
    from oasisx_amd import io

    mesh, u, tags = build_channel(a.N)
    rng = np.random.default_rng(0)
    x0 = np.stack([rng.uniform(0.0, 3.0, a.seeds), rng.uniform(-0.95, 0.95, a.seeds)], axis=1)
    P = ox.InertialParticles(u, x0, a.diameter, a.density, fluid_density=1.0, nu=a.nu, gravity=(0.0, -a.g),
                             velocities=np.zeros_like(x0), drag="stokes", scheme="exp2", substeps=a.substeps, walls=(tags, 1))
    tau = float(P.response_time()[0])
    ws = tau * (1.0 - 1.0 / a.density) * a.g
    t_d = deposition_time(x0[:, 1] + 1.0, tau, ws)
    h = a.dt / a.substeps
    print(f"particle deposition: {mesh.num_cells} cells, {a.seeds} particles, tau_p = {tau:.4g}, settling velocity {ws:.4g}, "
          f"h / tau_p = {h / tau:.3g}")
    print(f"{'step':>5} {'t':>8} {'deposited':>10} {'closed form':>12}")
    worst = 0
    for n in range(1, a.steps + 1):
        P.advance(a.dt)
        t = n * a.dt
        got = int((P.status() == ox.DEPOSITED).sum())
        # caught at the start of the substep in which y passes the wall: deposited by t <=> t_d < t (substep ends are the
        # multiples of h); a t_d within rounding of a multiple of h may fall on either side
        sure, maybe = int((t_d < t - 1e-9).sum()), int((t_d < t + 1e-9).sum())
        worst = max(worst, max(sure - got, got - maybe, 0))
        if n % max(1, a.steps // 10) == 0 or n == a.steps:
            print(f"{n:>5} {t:>8.3f} {got / a.seeds:>10.4f} {sure / a.seeds:>12.4f}")
    S, E, T = P.status(), P.exit_time(), a.steps * a.dt
    dep = S == ox.DEPOSITED
    late = np.abs(E[dep] - t_d[dep])
    lower = np.isin(P.facet()[dep], tags.find(1))
    ok = bool(worst == 0 and (late <= h + 1e-9).all() and (E[dep] <= t_d[dep] + 1e-9).all() and lower.all()
              and (t_d[~dep] >= T - 1e-9).all() and (S[~dep] == 0).all())
    travelled = P.unfolded_positions()[:, 0] - x0[:, 0]
    print(f"deposited {int(dep.sum())} of {a.seeds} by t = {T:.3f}; closed-form deposition times met to "
          f"{(late.max() if dep.any() else 0.0):.3e} (one substep = {h:.3e}): {'PASS' if ok else 'FAIL'}")
    print(f"mean streamwise distance travelled {travelled.mean():.4f} (deposited {travelled[dep].mean() if dep.any() else 0.0:.4f}), "
          f"up to {int(P.wraps()[:, 0].max())} passes through the periodic seam")
    if a.out:
        io.write_facet_vtu(a.out, mesh, P.exterior, {"deposition": P.deposition().astype(np.float64)}, time=T)
    return {"n": a.seeds, "deposited": int(dep.sum()), "ok": ok, "mean_distance": float(travelled.mean()), "tau": tau,
            "late": float(late.max()) if dep.any() else 0.0, "h": h, "deposition": P.deposition()}


if __name__ == "__main__":
    main()
