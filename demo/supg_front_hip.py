#!/usr/bin/env python3
"""SUPG stabilisation of a convection-dominated scalar, HIP path.

1. A step profile carried skew to a 2-D lattice at ``kappa = 1e-6`` (cell Peclet number ~ 1e5): c = 1 enters through the
   face x = -1 above y = -0.3, c = 0 below it and through y = -1; the uniform velocity makes ``--angle`` degrees with the
   x axis.  Plain Crank-Nicolson Galerkin answers with node-to-node oscillations; ``stabilization=SUPG()`` damps them along
   the streamlines (it has no discontinuity capturing: the layer ACROSS the streamlines keeps an overshoot).  Prints min / max
   of c with and without stabilisation.
2. A smooth cone (a Gaussian) in solid-body rotation with the exact solution as Dirichlet data: the L2 error at
   N = 8, 16, 32 (dt ~ 1/N) and the measured orders -- reported, not promised.

The velocity is prescribed, so only the scalar phases of the step run: ``assemble_first`` (which forms the velocity matrix
the scalar's operator is taken from) and ``scalar_solve``.

    python demo/supg_front_hip.py [-N 32] [--steps 20] [--dt 0.025] [--angle 30] [-u 1] [--cone-sizes 8 16 32]
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BCGS = {"ksp_type": "bcgs", "pc_type": "jacobi", "ksp_rtol": 1e-11, "ksp_atol": 1e-30}
STEP_Y0 = -0.3  # the step of the inflow profile on the face x = -1
NU = 1e-3  # the viscosity of the (prescribed) velocity's matrix; the scalar's diffusivity is absolute


def on_boundary(x):
    return np.isclose(np.abs(x[0]), 1.0) | np.isclose(np.abs(x[1]), 1.0)


def inflow(x):
    return np.isclose(x[0], -1.0) | np.isclose(x[1], -1.0)


def step_profile(x):
    """1 on the face x = -1 above y = STEP_Y0, 0 elsewhere: the inflow data and (inside: 0) the initial state."""
    return np.where(np.isclose(x[0], -1.0) & (x[1] > STEP_Y0), 1.0, 0.0)


def _solver(N, degree, velocity, scalar, krylov=None):
    """A solver on the N x N lattice of [-1, 1]^2 whose two velocity levels hold the callables ``velocity``."""
    import oasisx_amd as ox
    from oasisx_amd import mesh as M
    from taylor_green_hip import KRYLOV

    mesh = M.create_rectangle(None, [[-1.0, -1.0], [1.0, 1.0]], [N, N])
    G = ox.LocatorMethod.GEOMETRICAL
    options = dict(KRYLOV, scalar_transport=dict(krylov or BCGS))
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", degree), ("Lagrange", 2 if degree == 3 else 1), bcs_p=[],
                                bcs_u=[[ox.DirichletBC(f, G, on_boundary)] for f in velocity], solver_options=options,
                                scalars=[scalar])
    for i, f in enumerate(velocity):
        S._u2[i].interpolate(f)
        S._u1[i].interpolate(f)
    return S


def skew_solver(N, degree, kappa, angle_deg, stabilize, krylov=None, scale=1.0):
    """The skew step: a uniform velocity of modulus 1 at ``angle_deg`` to the x axis, ``step_profile`` on the inflow faces."""
    import oasisx_amd as ox

    a = math.radians(angle_deg)
    vel = [lambda x, v=v: np.full(x.shape[1], v) for v in (math.cos(a), math.sin(a))]
    sc = ox.ScalarTransport("c", diffusivity=kappa, initial=step_profile,
                            bcs=[ox.DirichletBC(step_profile, ox.LocatorMethod.GEOMETRICAL, inflow)],
                            stabilization=ox.SUPG(scale=scale) if stabilize else None)
    return _solver(N, degree, vel, sc, krylov)


def run_front(N, degree, kappa, angle_deg, dt, steps, stabilize):
    """(min c, max c) after ``steps`` steps."""
    S = skew_solver(N, degree, kappa, angle_deg, stabilize)
    for _ in range(steps):
        S.assemble_first(dt, NU)
        S.scalar_solve()
    c = S.scalar("c")._storage.rhost()[:, 0]
    return float(c.min()), float(c.max())


def run_cone(N, degree, kappa, angle, steps, stabilize, sigma=0.2, x0=0.4):
    """L2 error of a Gaussian of width ``sigma`` that starts at (x0, 0) after a solid-body rotation by ``angle`` radians
    in ``steps`` steps.  Exact: the centre turns, sigma^2 grows by 2 kappa t, the amplitude falls as sigma^2 / sigma(t)^2."""
    import oasisx_amd as ox
    from oasisx_amd import fem

    clock = {"t": 0.0}

    def exact(x):
        t = clock["t"]
        cx, cy = x0 * math.cos(t), x0 * math.sin(t)
        s2 = sigma * sigma + 2.0 * kappa * t
        return (sigma * sigma / s2) * np.exp(-((x[0] - cx) ** 2 + (x[1] - cy) ** 2) / (2.0 * s2))

    vel = [lambda x: -x[1].copy(), lambda x: x[0].copy()]
    bc = ox.DirichletBC(exact, ox.LocatorMethod.GEOMETRICAL, on_boundary)
    sc = ox.ScalarTransport("c", diffusivity=kappa, initial=exact, bcs=[bc],
                            stabilization=ox.SUPG() if stabilize else None)
    S = _solver(N, degree, vel, sc)
    dt = angle / steps
    for n in range(1, steps + 1):
        clock["t"] = n * dt  # (unit angular velocity: the angle is the time)
        bc.update_bc()
        S.assemble_first(dt, NU)
        S.scalar_solve()
    return math.sqrt(fem.assemble_l2_error_sq(S.scalar("c"), exact))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-N", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--dt", type=float, default=0.025)
    ap.add_argument("--angle", type=float, default=30.0)
    ap.add_argument("--kappa", type=float, default=1e-6)
    ap.add_argument("-u", "--degree-u", type=int, default=1)
    ap.add_argument("--cone-sizes", type=int, nargs="+", default=[8, 16, 32])
    ap.add_argument("--cone-steps", type=int, default=8, help="steps of the rotation at the first size (~ N after that)")
    ap.add_argument("--cone-angle", type=float, default=0.5)
    a = ap.parse_args(argv)
    res = {"front": {}, "cone": [], "orders": []}
    print(f"skew step, N = {a.N}, P{a.degree_u}, kappa = {a.kappa:g}, {a.steps} steps of dt = {a.dt:g}, {a.angle:g} degrees")
    for key, stab in (("galerkin", False), ("supg", True)):
        lo, hi = run_front(a.N, a.degree_u, a.kappa, a.angle, a.dt, a.steps, stab)
        res["front"][key] = (lo, hi)
        print(f"  {'SUPG    ' if stab else 'Galerkin'}: min c = {lo:+.6f}, max c = {hi:+.6f}   (undershoot {-lo:.4f}, "
              f"overshoot {hi - 1.0:.4f})")
    print(f"rotating cone, P2, kappa = {a.kappa:g}, rotation by {a.cone_angle:g} rad, SUPG")
    print(f"{'N':>5} {'steps':>6} {'L2 error SUPG':>15} {'order':>7} {'L2 error Galerkin':>19}")
    prev = None
    for N in a.cone_sizes:
        steps = max(1, a.cone_steps * N // a.cone_sizes[0])
        e = run_cone(N, 2, a.kappa, a.cone_angle, steps, True)
        eg = run_cone(N, 2, a.kappa, a.cone_angle, steps, False)
        order = ""
        if prev is not None:
            res["orders"].append(math.log(prev[1] / e) / math.log(N / prev[0]))
            order = f"{res['orders'][-1]:.2f}"
        print(f"{N:>5} {steps:>6} {e:>15.6e} {order:>7} {eg:>19.6e}")
        res["cone"].append({"N": N, "steps": steps, "error": e, "error_galerkin": eg})
        prev = (N, e)
    return res


if __name__ == "__main__":
    main()
