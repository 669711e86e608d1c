"""Numpy model of the Lagrangian tracers (what ``ox_tracer_advance`` of csrc/ox_probe.hip computes), vectorised over the
particles and otherwise a line-by-line statement of the rules of DESIGN section 18:

* ``h = dt / substeps``; substep s starts at ``theta_s = s / substeps``; the stage at the fraction c evaluates
  ``v(x, theta) = theta * (u_b(x) - u_a(x)) + u_a(x)`` (the kernel's ``fma(theta, u_b - u_a, u_a)``: one rounding fewer) at
  ``theta = (s + c) / substeps``;
* Euler: ``x + h k1``.  Midpoint: ``k2`` at ``x + h/2 k1``, ``x + h k2``.  RK4: stage points ``x + a_j h k_{j-1}``,
  a = (0, 1/2, 1/2, 1), ``x + h/6 (k1 + 2 k2 + 2 k3 + k4)``;
* the substep's start lies in the particle's cell (no search); every later stage point AND the end point are located:
  with the hint the cached cell is kept when all its barycentric coordinates are >= 0, otherwise -- and without the hint
  -- the lowest containing cell with lambda >= -tol (``probe_model.locate``);
* a located point in no cell: status 1, the particle stays at the substep's start, ``exit_time = t + theta_s * dt`` (product
  and sum rounded separately), cell -1; a non-finite velocity or a cell out of range: status 2, frozen the same way;
* a completed substep adds h to the age and ``|x_new - x_old|`` to the path length.

Location goes through a *locator* ``(x, cell) -> cell`` and evaluation through a *field* ``(x, cell, theta) -> v``:
``MeshLocator`` + ``FEField`` are the finite-element statement (``probe_model.locate`` / ``probe_model.evaluate`` on
host copies of the two levels); ``AnalyticField`` takes ``v(x, theta)`` in closed form and ``BoxLocator`` an axis-aligned
box in any dimension (one "cell", id 0)."""
from __future__ import annotations

import numpy as np

from tests import probe_model as PM

ALIVE, EXITED, INVALID = 0, 1, 2
STAGES = {"euler": 1, "rk2": 2, "rk4": 4}


def blend(ua, ub, theta):
    return theta * (ub - ua) + ua


def cell_barycentric(coords, cells, cell, x):
    """(n, d + 1): barycentric coordinates of point i in cell[i]."""
    xc = coords[cells[cell]]  # (n, d+1, d)
    J = np.moveaxis(xc[:, 1:, :] - xc[:, :1, :], 1, 2)
    lam = np.einsum("nak,nk->na", np.linalg.inv(J), x - xc[:, 0, :])
    return np.concatenate([1.0 - lam.sum(axis=1, keepdims=True), lam], axis=1)


class MeshLocator:
    def __init__(self, mesh, tol=1e-10, hint=True):
        self.coords, self.cells = mesh.coords.cpu().numpy(), mesh.cells.cpu().numpy()
        self.n_cells, self.tol, self.hint = int(self.cells.shape[0]), float(tol), bool(hint)

    def __call__(self, x, cell):
        out = np.full(x.shape[0], -1, dtype=np.int64)
        todo = np.ones(x.shape[0], dtype=bool)
        if self.hint:
            cand = np.nonzero((cell >= 0) & (cell < self.n_cells))[0]
            if cand.size:
                keep = cell_barycentric(self.coords, self.cells, cell[cand], x[cand]).min(axis=1) >= 0.0
                out[cand[keep]] = cell[cand[keep]]
                todo[cand[keep]] = False
        if todo.any():
            out[todo] = PM.locate(self.coords, self.cells, x[todo], self.tol)[0]
        return out


class BoxLocator:
    def __init__(self, lo, hi):
        self.lo, self.hi, self.n_cells = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64), 1

    def __call__(self, x, cell):
        inside = ((x >= self.lo) & (x <= self.hi)).all(axis=1)  # (NaN: outside)
        return np.where(inside, 0, -1).astype(np.int64)


class FEField:
    """The two levels ``ua``, ``ub`` (n_local, >= gdim) of a blocked field on the scalar space ``Vs``."""

    def __init__(self, Vs, ua, ub=None):
        d = Vs.mesh.gdim
        self.Vs = Vs
        self.coords, self.cells = Vs.mesh.coords.cpu().numpy(), Vs.mesh.cells.cpu().numpy()
        self.ua = np.asarray(ua, dtype=np.float64)[:, :d]
        self.ub = self.ua if ub is None else np.asarray(ub, dtype=np.float64)[:, :d]

    def __call__(self, x, cell, theta):
        lam = cell_barycentric(self.coords, self.cells, cell, x)
        va = PM.evaluate(self.Vs, self.ua, x, cell, lam)
        vb = va if self.ub is self.ua else PM.evaluate(self.Vs, self.ub, x, cell, lam)
        return blend(va, vb, theta)


class AnalyticField:
    """``fn(x (n, d), theta) -> (n, d)``."""

    def __init__(self, fn):
        self.fn = fn

    def __call__(self, x, cell, theta):
        return np.asarray(self.fn(x, theta), dtype=np.float64).reshape(x.shape)


class Tracers:
    """The model's particle set; the same getters as ``oasisx_amd.Tracers`` as plain arrays (``x``, ``cell``, ``status``,
    ``age``, ``path``, ``t_exit``, ``t``).  ``watch``: called with every located point set (stage and end points)."""

    def __init__(self, field, locator, points, scheme="rk4", substeps=1, watch=None):
        self.field, self.locator, self.scheme, self.substeps, self.watch = field, locator, scheme, int(substeps), watch
        self.n_stages = STAGES[scheme]
        d = np.asarray(points).shape[1]
        self.x = np.zeros((0, d))
        self.cell = np.zeros(0, dtype=np.int64)
        self.status = np.zeros(0, dtype=np.int32)
        self.age, self.path, self.t_exit = np.zeros(0), np.zeros(0), np.zeros(0)
        self.t = 0.0
        self.inject(points)

    def inject(self, points):
        x = np.array(points, dtype=np.float64)
        cell = self.locator(x, np.full(x.shape[0], -1, dtype=np.int64)) if not isinstance(self.locator, MeshLocator) else \
            PM.locate(self.locator.coords, self.locator.cells, x, self.locator.tol)[0]
        n0 = self.x.shape[0]
        self.x = np.concatenate([self.x, x])
        self.cell = np.concatenate([self.cell, cell])
        self.status = np.concatenate([self.status, np.where(cell >= 0, ALIVE, EXITED).astype(np.int32)])
        self.age = np.concatenate([self.age, np.zeros(x.shape[0])])
        self.path = np.concatenate([self.path, np.zeros(x.shape[0])])
        self.t_exit = np.concatenate([self.t_exit, np.where(cell >= 0, np.nan, self.t)])
        return np.arange(n0, n0 + x.shape[0])

    def _weights(self, j):
        a = 0.0 if j == 0 else (1.0 if j == 3 else 0.5)
        if self.scheme == "euler":
            return a, 1.0
        if self.scheme == "rk2":
            return a, float(j)
        return a, (1.0 if j in (0, 3) else 2.0)

    def advance(self, dt, field=None):
        field = self.field if field is None else field
        m = float(self.substeps)
        h = dt / m
        scale = h / 6.0 if self.scheme == "rk4" else h
        for s in range(self.substeps):
            live = np.nonzero(self.status == ALIVE)[0]
            if live.size == 0:
                break
            x, cell = self.x[live].copy(), self.cell[live].copy()
            code = np.zeros(live.size, dtype=np.int32)
            ks, kj, xs = np.zeros_like(x), np.zeros_like(x), x.copy()
            for j in range(self.n_stages):
                a, w = self._weights(j)
                act = np.nonzero(code == 0)[0]
                if j == 0:
                    code[act[(cell[act] < 0) | (cell[act] >= self.locator.n_cells)]] = INVALID
                else:
                    xs[act] = x[act] + (a * h) * kj[act]
                    self._locate(xs, cell, code, act)
                act = np.nonzero(code == 0)[0]
                if act.size:
                    v = field(xs[act], cell[act], (float(s) + a) / m)
                    bad = ~np.isfinite(v).all(axis=1)
                    code[act[bad]] = INVALID
                    kj[act] = v
                    good = act[~bad]
                    ks[good] = ks[good] + w * kj[good]
            act = np.nonzero(code == 0)[0]
            xs[act] = x[act] + scale * ks[act]
            self._locate(xs, cell, code, act)
            done, froze = live[code == 0], live[code != 0]
            step = xs[code == 0] - x[code == 0]
            self.path[done] += np.sqrt((step * step).sum(axis=1))
            self.age[done] += h
            self.x[done] = xs[code == 0]
            self.cell[done] = cell[code == 0]
            self.status[froze] = code[code != 0]
            self.t_exit[froze] = self.t + (float(s) / m) * dt
            self.cell[froze] = -1
        self.t += dt

    def _locate(self, xs, cell, code, act):
        if act.size == 0:
            return
        if self.watch is not None:
            self.watch(xs[act])
        new = self.locator(xs[act], cell[act])
        cell[act[new >= 0]] = new[new >= 0]
        code[act[new < 0]] = EXITED
