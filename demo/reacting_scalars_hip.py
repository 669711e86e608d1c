#!/usr/bin/env python3
"""Reacting scalars, HIP path: stiff mass-action kinetics split from the transport step.

1. A batch reactor: the fluid is at rest, the fields are uniform, ``A + B -> C`` at the rate ``k A B``.  Transport does
   nothing, so the step is the Strang pair of ROS2 half steps; the result at ``t = T`` is compared with the closed form of
   second-order kinetics (``A0 != B0``, ``d = A0 - B0``)::

       A(t) = A0 d / (A0 - B0 exp(-d k t)),    B = A - d,    C = C0 + A0 - A

   for a halving sequence of ``dt``; prints the errors and the measured order in ``dt``.
2. A plug-flow reactor: a uniform flow ``(U, 0)`` through [-1, 1]^2, ``A -> B`` at the rate ``k A``, ``A = 1``, ``B = 0`` on
   the inflow face.  At steady state, without diffusion, ``A = exp(-k (x + 1) / U)`` along the channel; prints the profile
   on the centre line and the largest difference (which holds the diffusion the formula leaves out and the splitting
   error).

The velocity is prescribed, so only the scalar phases of the step run, in the order ``solve`` runs them:
``scalar_react(dt/2)``, ``assemble_first`` (which forms the velocity matrix the scalars' operators are taken from),
``scalar_solve``, ``scalar_react(dt/2)``.

    python demo/reacting_scalars_hip.py [-N 8] [--batch-steps 4 8 16 32] [--pfr-steps 60] [--pfr-dt 0.05]
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TIGHT = {"ksp_type": "bcgs", "pc_type": "jacobi", "ksp_rtol": 1e-12, "ksp_atol": 1e-30}
NU = 1e-3  # the viscosity of the (prescribed) velocity's matrix; the scalars' diffusivities are absolute


def on_boundary(x):
    return np.isclose(np.abs(x[0]), 1.0) | np.isclose(np.abs(x[1]), 1.0)


def inflow(x):
    return np.isclose(x[0], -1.0)


def make_solver(N, degree, velocity, scalars, network, krylov=None):
    """A solver on the N x N lattice of [-1, 1]^2 whose two velocity levels hold the constants ``velocity``."""
    import oasisx_amd as ox
    from oasisx_amd import mesh as M
    from taylor_green_hip import KRYLOV

    mesh = M.create_rectangle(None, [[-1.0, -1.0], [1.0, 1.0]], [N, N])
    vel = [lambda x, v=float(v): np.full(x.shape[1], v) for v in velocity]
    options = dict(KRYLOV, scalar_transport=dict(krylov or TIGHT))
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", degree), ("Lagrange", 1), bcs_p=[],
                                bcs_u=[[ox.DirichletBC(f, ox.LocatorMethod.GEOMETRICAL, on_boundary)] for f in vel],
                                solver_options=options, scalars=scalars, reactions=network)
    for i, f in enumerate(vel):
        S._u2[i].interpolate(f)
        S._u1[i].interpolate(f)
    return S, mesh


def advance(S, dt, nu=NU):
    """One step of the scalar phases under the network's splitting."""
    net = S._reactions
    net.update()
    strang = net.splitting == "strang"
    if strang:
        S.scalar_react(0.5 * dt)
    S.assemble_first(dt, nu)
    S.scalar_solve()
    S.scalar_react(0.5 * dt if strang else dt)


def values(S, name):
    f = S.scalar(name)
    return f._storage.rhost()[:, f._comp]


# ---- 1. batch reactor -------------------------------------------------------------------------------------------------------
def batch_exact(t, k, A0, B0, C0=0.0):
    d = A0 - B0
    A = A0 * d / (A0 - B0 * math.exp(-d * k * t))
    return A, A - d, C0 + A0 - A


def run_batch(N, degree, steps, T=1.0, k=2.0, A0=1.0, B0=0.6, splitting="strang", substeps=1):
    """max over the species and the dofs of |c - closed form| at t = T after ``steps`` steps."""
    import oasisx_amd as ox

    sc = [ox.ScalarTransport(n, diffusivity=0.01, initial=v) for n, v in (("A", A0), ("B", B0), ("C", 0.0))]
    net = ox.ReactionNetwork([ox.Reaction(k, {"A": 1, "B": 1}, {"C": 1})], substeps=substeps, splitting=splitting)
    S, _ = make_solver(N, degree, (0.0, 0.0), sc, net)
    for _ in range(steps):
        advance(S, T / steps)
    return max(float(np.abs(values(S, n) - e).max()) for n, e in zip("ABC", batch_exact(T, k, A0, B0)))


# ---- 2. plug-flow reactor ---------------------------------------------------------------------------------------------------
def pfr_exact(x, k, U):
    return np.exp(-k * (x[0] + 1.0) / U)


def run_pfr(N, degree, steps, dt, k=2.0, U=1.0, kappa=0.01, substeps=1):
    """The plug-flow reactor after ``steps`` steps from an empty channel.  Returns (solver, mesh, max |A - exp(-k (x+1)/U)|)."""
    import oasisx_amd as ox

    G = ox.LocatorMethod.GEOMETRICAL
    sc = [ox.ScalarTransport("A", diffusivity=kappa, bcs=[ox.DirichletBC(1.0, G, inflow)]),
          ox.ScalarTransport("B", diffusivity=kappa, bcs=[ox.DirichletBC(0.0, G, inflow)])]
    net = ox.ReactionNetwork([ox.Reaction(k, {"A": 1}, {"B": 1})], substeps=substeps)
    S, mesh = make_solver(N, degree, (U, 0.0), sc, net)
    for _ in range(steps):
        advance(S, dt)
    x = S._Vi[0][0].x.cpu().numpy()
    X = np.zeros((3, x.shape[0]))
    X[:2] = x.T
    return S, mesh, float(np.abs(values(S, "A") - pfr_exact(X, k, U)).max())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-N", type=int, default=8)
    ap.add_argument("-u", "--degree-u", type=int, default=2)
    ap.add_argument("--batch-steps", type=int, nargs="+", default=[4, 8, 16, 32])
    ap.add_argument("--pfr-steps", type=int, default=60)
    ap.add_argument("--pfr-dt", type=float, default=0.05)
    ap.add_argument("-k", "--rate", type=float, default=2.0)
    a = ap.parse_args(argv)
    res = {"batch": [], "orders": []}
    print(f"batch reactor, A + B -> C, k = {a.rate:g}, A0 = 1, B0 = 0.6, T = 1, Strang splitting, N = {a.N}, P{a.degree_u}")
    print(f"{'steps':>6} {'dt':>10} {'max error':>14} {'order':>7}")
    prev = None
    for n in a.batch_steps:
        e = run_batch(a.N, a.degree_u, n, k=a.rate)
        order = ""
        if prev is not None:
            res["orders"].append(math.log(prev[1] / e) / math.log(n / prev[0]))
            order = f"{res['orders'][-1]:.2f}"
        print(f"{n:>6} {1.0 / n:>10.5f} {e:>14.6e} {order:>7}")
        res["batch"].append({"steps": n, "error": e})
        prev = (n, e)
    S, _, err = run_pfr(a.N, a.degree_u, a.pfr_steps, a.pfr_dt, k=a.rate)
    print(f"plug-flow reactor, A -> B, k = {a.rate:g}, U = 1, kappa = 0.01, {a.pfr_steps} steps of dt = {a.pfr_dt:g}")
    x = S._Vi[0][0].x.cpu().numpy()
    line = np.nonzero(np.isclose(x[:, 1], 0.0))[0]
    line = line[np.argsort(x[line, 0])]
    A, B = values(S, "A"), values(S, "B")
    print(f"{'x':>8} {'A':>12} {'exp(-k(x+1)/U)':>16} {'A + B':>12}")
    for i in line[:: max(1, line.size // 8)]:
        print(f"{x[i, 0]:>8.3f} {A[i]:>12.6f} {math.exp(-a.rate * (x[i, 0] + 1.0)):>16.6f} {A[i] + B[i]:>12.6f}")
    print(f"max |A - exp(-k (x + 1) / U)| = {err:.3e}")
    res["pfr_error"] = err
    return res


if __name__ == "__main__":
    main()
