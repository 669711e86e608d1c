"""Tracers in a constant velocity field on the meshes of tests/hard_meshes.py: seeds, the closed form and its bounds
(plain numpy: importable without a GPU).  A constant field is exact in P1, so a particle follows ``x0 + t v`` whatever
the scheme; what the device (k_tracer_advance, csrc/ox_probe.hip) may be off by is counted here, per completed substep
of length h and per axis k (u = 2^-53, D the dimension):

* the velocity at a located point is ``sum_a lambda_a v_k`` accumulated in D + 1 fmas: ``(D + 1) u |v_k| sum |lambda|``;
  the lambda_a sum to one up to the D rounded subtractions that formed lambda_0: ``D u (1 + sum |lambda|) |v_k|``; with
  ``sum |lambda| <= 1 + 2 (D + 1) tol`` at a located point: ``(3 D + 1) u |v_k|`` (both time levels are the same array:
  the blend ``fma(theta, u_b - u_a, u_a)`` adds nothing);
* the stage sum ``k_1 + 2 k_2 + 2 k_3 + k_4`` is four fmas on partial sums of at most ``6 |v_k|``, scaled by h / 6:
  ``4 u h |v_k|`` (Euler and the midpoint rule: fewer);
* the step length: ``dt / substeps`` and ``h / 6``, one rounding each: ``2 u h |v_k|``;
* the update ``fma(scale, ks, x)``: one rounding on ``|x_k| + h |v_k|``;

together ``E_k = u (max |x_k| + (3 D + 8) h |v_k|)`` per substep.  The field is constant, so the errors of n substeps add
and nothing amplifies them: ``|x_k - (x0 + n h v)_k| <= 1.01 n E_k``.  ``age`` adds h (a power of two here: exact) n times,
each sum rounded on at most T: ``1.01 (n + 1) u T``.  ``path`` adds ``sqrt(sum d_k^2)`` with ``d_k = x_new - x_old`` within
``E_k + u h |v_k|`` of ``h v_k``, D fmas and a square root ``(D + 3) u h |v|``, and the running sum rounded on at most
``T |v|``: ``1.01 n (|E + u h |v|| + (D + 3) u h |v| + u T |v|)``.

Decisions.  Per substep the device locates the stage points at the fractions 1/2 (midpoint rule, RK4) and 1 (RK4, and the
end point of every scheme) of the substep.  The closed-form points are held to ``locator_model.locate`` with the device's
possible distance from them (twice the position bound, which also covers the rounding of the closed form to float64)
added to the bound of every comparison; every one must be decided.  A particle freezes at the start of the first substep
one of whose points lies in no cell, with status 1 and that substep's start time ``t + (s / m) dt``."""
from __future__ import annotations

import numpy as np

from tests import hard_meshes as H
from tests import locator_model as LM
from tests.assembly_model import U, ext, to_f64

SCHEMES = ("euler", "rk2", "rk4")
FRACTIONS = {"euler": (1.0,), "rk2": (0.5, 1.0), "rk4": (0.5, 1.0)}
DT, ADVANCES, SUBSTEPS = 0.5, 2, (1, 4)  # h = 1/2 and 1/8: every time of the closed form is exact
CASES = [(2, "fan254"), (2, "stretched"), (2, "flipped"), (2, "tiny_far"),
         (3, "spindle254"), (3, "stretched"), (3, "flipped"), (3, "squashed"), (3, "tiny_far")]


def _linear(name, d, xi):
    """The linear part of the map that made the lattice-derived mesh ``name`` out of [-1, 1]^d (tests/hard_meshes.py)."""
    p = np.array(xi, dtype=np.float64)
    if name in ("stretched", "flipped"):
        p = p * (np.array([1e4, 1.0]) if d == 2 else np.array([1.0, 1e-2, 1e-4]))
        p[..., 0] += 0.37 * p[..., 1]
        if d == 3:
            p[..., 1] += 0.37 * p[..., 2]
    elif name == "squashed":
        p = p * np.array([1.0, 1.0, 1e-6])
    elif name == "tiny_far":
        p = p * 1e-3
    return p


def case(d, name, seed=0):
    """dict(points, cells, v (d,), seeds (n, d)): the velocity crosses many cells -- through the centre vertex of the fan
    and the axis of the spindle, across the slivers and the cells of both orientations of the stretched lattices, at 1e-3
    per unit time on tiny_far -- and some seeds leave the mesh within T = 1."""
    rng = np.random.default_rng(seed + 10 * d)
    pts, cells = H.zoo(d, 1)[name]
    if name == "fan254":
        v = np.array([0.75, 0.25])
        line = -np.arange(1, 16)[:, None] / 16.0 * v[None, :]  # through the centre: at the origin after k / 16
        rho, th = 0.5 * np.sqrt(rng.uniform(0, 1, 100)), rng.uniform(0, 2 * np.pi, 100)
        rho2, th2 = rng.uniform(0.8, 0.95, 60), rng.uniform(0, 2 * np.pi, 60)
        ring = lambda r, t: np.stack([3.0 * r * np.cos(t), r * np.sin(t)], axis=1)  # noqa: E731
        seeds = np.concatenate([line, ring(rho, th), ring(rho2, th2)])
    elif name == "spindle254":
        v = np.array([0.5, 0.25, 0.125])
        line = -np.arange(1, 16)[:, None] / 16.0 * v[None, :]  # through the axis
        ball = rng.standard_normal((100, 3))
        ball *= 0.1 * rng.uniform(0, 1, (100, 1)) ** (1 / 3) / np.linalg.norm(ball, axis=1, keepdims=True)
        ahead = rng.uniform(0.3, 1.2, (60, 1)) * v[None, :] + 0.02 * rng.uniform(-1, 1, (60, 3))
        seeds = np.concatenate([line, ball, ahead])
    else:
        v = _linear(name, d, np.array([0.75, 0.5, 0.25])[:d])
        stay = rng.uniform(-0.9, -0.1, (150, d))
        leave = rng.uniform(-0.9, -0.1, (60, d))
        leave[:, 0] = rng.uniform(0.3, 0.9, 60)  # through the face xi_0 = 1 after (1 - xi_0) / 0.75 < 1
        seeds = _linear(name, d, np.concatenate([stay, leave])) + (1e3 if name == "tiny_far" else 0.0)
    return {"points": pts, "cells": cells, "v": v, "seeds": seeds, "d": d, "name": name}


def position_bound(C, h, n):
    """(n_particles, d): the bound on |x - (x0 + n h v)| after n (per particle) completed substeps of length h."""
    d, v, x0 = C["d"], C["v"], C["seeds"]
    xmax = np.maximum(np.abs(x0), np.abs(x0 + DT * ADVANCES * v))
    return LM.SLACK * np.asarray(n, dtype=np.float64)[:, None] * U * (xmax + (3 * d + 8) * h * np.abs(v))


def age_bound(n):
    return LM.SLACK * (np.asarray(n, dtype=np.float64) + 1) * U * DT * ADVANCES


def path_bound(C, h, n):
    d, v = C["d"], C["v"]
    one = position_bound(C, h, np.ones(C["seeds"].shape[0])) / LM.SLACK + U * h * np.abs(v)
    speed, T = float(np.linalg.norm(v)), DT * ADVANCES
    return LM.SLACK * np.asarray(n, dtype=np.float64) * (np.linalg.norm(one, axis=1) + (d + 3) * U * h * speed + U * T * speed)


_EXPECT = {}


def expectation(C, m):
    """What the closed form says for ``m`` substeps per advance, per scheme: dict scheme -> dict(n (completed substeps),
    status, x (extended), age, path, t_exit, decided (all located points of the particle's life), cells_end (the model's
    cell of the end point; -1 for a frozen particle))."""
    key = (C["d"], C["name"], m)
    if key in _EXPECT:
        return _EXPECT[key]
    x0, v = C["seeds"], C["v"]
    npart, d = x0.shape
    N, h = ADVANCES * m, DT / m
    shift = 2.0 * position_bound(C, h, np.full(npart, N))
    loc = {}
    for f in (0.5, 1.0):
        t = (np.arange(N) + f) * h  # (N,)
        xe = ext(x0)[None] + ext(t)[:, None, None] * ext(v)[None, None, :]  # (N, npart, d)
        R = LM.locate(C["points"], C["cells"], to_f64(xe).reshape(-1, d), shift=np.broadcast_to(shift, (N, npart, d)).reshape(-1, d))
        loc[f] = (R["cell"].reshape(N, npart), R["decided"].reshape(N, npart))
    out = {}
    for scheme in SCHEMES:
        found = np.all([loc[f][0] >= 0 for f in FRACTIONS[scheme]], axis=0)  # (N, npart): the substep completes
        decided = np.all([loc[f][1] for f in FRACTIONS[scheme]], axis=0)
        gone = ~found.all(axis=0)
        n = np.where(gone, np.argmin(found, axis=0), N)  # the first substep that does not complete
        lived = np.arange(N)[:, None] <= np.minimum(n, N - 1)[None, :]  # the substeps the device works on
        adv, s = n // m, n % m
        t_exit = np.where(gone, adv * DT + (s / m) * DT, np.nan)
        out[scheme] = {"n": n, "status": gone.astype(np.int32), "x": ext(x0) + ext(n * h)[:, None] * ext(v)[None, :],
                       "age": n * h, "path": n * h * float(np.linalg.norm(v)), "t_exit": t_exit,
                       "decided": (decided | ~lived).all(axis=0),
                       "cells_end": np.where(gone, -1, loc[1.0][0][N - 1])}
    _EXPECT[key] = out
    return out
