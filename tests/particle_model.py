"""Numpy model of the inertial particles (what ``ox_particle_advance`` of csrc/ox_probe.hip computes), vectorised over the
particles and otherwise a line-by-line statement of the rules of DESIGN section 30:

* ``dx/dt = v``, ``dv/dt = (f / tau_p)(u - v) + beta g``; ``f = 1`` (Stokes) or ``1 + 0.15 Re_p^0.687``,
  ``Re_p = d |u - v| / nu`` (Schiller-Naumann);
* ``h = dt / substeps``; substep s starts at ``theta_s = s / substeps``; the field is the tracers' blend
  (``tracer_model.blend``);
* ``u0`` = the field at the substep's start (in the particle's cell, no search); ``f`` from ``(u0, v)``, frozen;
  ``tau_e = tau_p / f``; ``w = u0 + (tau_e beta) g``; ``tau_e == 0``: ``E = phi = 0``, else ``r = h / tau_e``,
  ``E = exp(-r)``, ``phi = tau_e (-expm1(-r))``; ``x_new = x + h w + phi (v - w)``, ``v_new = w + E (v - w)`` (exp1);
* exp2: the position of the same formulas with ``h / 2`` is folded and located, ``u_m`` = the field there at
  ``theta = (s + 1/2) / substeps``, ``w_m = u_m + (tau_e beta) g``, and the update above uses ``w_m``;
* every predictor and end point is folded into ``[lo, hi)`` on the periodic axes before it is located
  (``x -= period floor((x - lo) / period)``, then ``x -= period`` where ``x >= hi``); the images are added to ``wraps`` when
  the substep completes; the path length adds the UNFOLDED step;
* a located point in no cell: the particle stays at the substep's start with ``t_exit = t + theta_s dt`` and cell -1
  (the tracers' rule); the nearest exterior facet of the folded point (``walldist_model.nearest``: ties to the lower
  position) is its ``facet``; where ``action[facet] == 1`` the status is 3 and the velocity 0, else the status is 1.  A
  non-finite position or velocity, or a cell out of range: status 2, frozen the same way, no facet.

``margin`` is the smallest distance of any decisive test from its threshold over the run: ``|min lambda|`` of the hinted
cell, ``|max_c min lambda_c|`` and the same ``+ tol`` over all cells (is the point in the mesh?), the gap between the two
nearest facets of a classified point when they act differently or always (``gap_all``), and the distance of a folded
coordinate to ``lo`` and ``hi``.

Location and evaluation go through ``tracer_model``'s locators and fields, unchanged."""
from __future__ import annotations

import numpy as np

from tests import tracer_model as TM
from tests import walldist_model as WD

ALIVE, EXITED, INVALID, DEPOSITED = 0, 1, 2, 3
STAGES = {"exp1": 1, "exp2": 2}


# ---- the closed form of a uniform steady field with gravity (the exactness cases of the host and the GPU tests) --------
RATIOS = (1e-6, 1.0, 1e6, None)  # h / tau_p; None: tau_p = 0


def exact_case(ratio, d, h=0.02):
    """(tau_p, u, g, beta) of the exactness cases in d dimensions; gravity is scaled so that the settling velocity
    tau beta g stays of order one (tests/test_particle_model_host.py says why)."""
    tau = 0.0 if ratio is None else h / ratio
    u = np.array([0.11, -0.07, 0.05])[:d]
    g = np.array([0.3, -0.9, 0.2])[:d] * min(1.0, 1.0 / tau if tau > 0.0 else 1.0)
    return tau, u, g, 0.75


def closed_form(x0, v0, u, g, beta, tau, t):
    w = u + tau * beta * g
    if tau == 0.0:
        return x0 + w * t, np.broadcast_to(w, v0.shape).copy()
    e = np.exp(-t / tau)
    return x0 + w * t + tau * (v0 - w) * (-np.expm1(-t / tau)), w + (v0 - w) * e


def rel_err(a, b):
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())


def response_time(diameter, density, fluid_density, nu):
    return (np.asarray(density, dtype=np.float64) / fluid_density) * np.asarray(diameter, dtype=np.float64) ** 2 / (18.0 * nu)


def coefficients(h, tau_e):
    """(E, phi) per particle."""
    tau_e = np.asarray(tau_e, dtype=np.float64)
    zero = tau_e == 0.0
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        r = h / np.where(zero, 1.0, tau_e)
        E = np.where(zero, 0.0, np.exp(-r))
        phi = np.where(zero, 0.0, tau_e * (-np.expm1(-r)))
    return E, phi


def drag_factor(u, v, diameter, nu, drag):
    if drag == "stokes":
        return np.ones(u.shape[0])
    rel = u - v
    re = diameter * np.sqrt((rel * rel).sum(axis=1)) / nu
    return 1.0 + 0.15 * re ** 0.687


def fold(x, periodic):
    """(x folded, images (n, d) int64, the distance of the folded periodic coordinates to lo / hi (inf: none))."""
    x = np.array(x, dtype=np.float64)
    w = np.zeros(x.shape, dtype=np.int64)
    gap = np.inf
    if periodic is not None:
        axes, lo, hi, period = periodic
        for k in axes:
            with np.errstate(invalid="ignore"):
                q = np.floor((x[:, k] - lo[k]) / period[k])
                xk = x[:, k] - period[k] * q
                over = xk >= hi[k]
            xk = np.where(over, xk - period[k], xk)
            x[:, k] = xk
            w[:, k] = np.where(np.isfinite(q), q, 0).astype(np.int64) + over
            if xk.size:
                gap = min(gap, float(np.nanmin(np.minimum(np.abs(xk - lo[k]), np.abs(hi[k] - xk)))))
    return x, w, gap


def periodic_of(mesh):
    per = getattr(mesh, "periodic", None)
    if per is None:
        return None
    return (tuple(per.axes), np.asarray(per.lo, dtype=np.float64), np.asarray(per.hi, dtype=np.float64),
            np.asarray(per.period, dtype=np.float64))


def exterior_xyz(mesh):
    """(facet ids ascending, their vertices (nf, d, d)): the exterior facets, on a periodic mesh the non-identified ones."""
    ids = np.sort(np.asarray(mesh.exterior_facets(), dtype=np.int64))
    fv, _ = mesh._entities(mesh.gdim - 1)
    return ids, mesh.coords.cpu().numpy()[fv[ids]]


class Particles:
    """The model's particle set: plain arrays ``x``, ``v``, ``cell``, ``status``, ``age``, ``path``, ``t_exit``, ``wraps``,
    ``facet`` (position in ``facet_xyz``, -1: none), ``t`` and ``margin``.

    ``field`` / ``locator``: as ``tracer_model.Tracers``.  ``periodic``: ``(axes, lo, hi, period)`` or None.
    ``facet_xyz`` (nf, d, d) with ``action`` (nf,): the exterior facets and what they do (1: deposit); None: particles that
    leave keep ``facet = -1`` and status 1."""

    def __init__(self, field, locator, points, velocities, tau_p, diameter=0.0, beta=1.0, gravity=None, nu=1.0,
                 drag="stokes", scheme="exp2", substeps=1, periodic=None, facet_xyz=None, action=None,
                 gap_all=True):
        x = np.array(points, dtype=np.float64)
        n, d = x.shape
        self.field, self.locator, self.scheme, self.substeps = field, locator, scheme, int(substeps)
        self.n_stages, self.drag, self.nu, self.periodic = STAGES[scheme], drag, float(nu), periodic
        self.g = np.zeros(d) if gravity is None else np.asarray(gravity, dtype=np.float64)[:d]
        self.facet_xyz = None if facet_xyz is None else np.asarray(facet_xyz, dtype=np.float64)
        self.action = None if facet_xyz is None else (np.zeros(self.facet_xyz.shape[0], dtype=np.int32) if action is None
                                                      else np.asarray(action, dtype=np.int32))
        self.gap_all = gap_all
        full = lambda a: np.broadcast_to(np.asarray(a, dtype=np.float64), (n,)).copy()  # noqa: E731
        self.tau_p, self.diam, self.beta = full(tau_p), full(diameter), full(beta)
        self.margin = np.inf
        x, w, gap = fold(x, periodic)
        self.margin = min(self.margin, gap)
        self.x, self.wraps = x, w
        none = np.full(n, -1, dtype=np.int64)
        if isinstance(locator, TM.MeshLocator):
            from tests import probe_model as PM

            self.cell = PM.locate(locator.coords, locator.cells, x, locator.tol)[0]
        else:
            self.cell = locator(x, none)
        self.status = np.where(self.cell >= 0, ALIVE, EXITED).astype(np.int32)
        self.age, self.path = np.zeros(n), np.zeros(n)
        self.t = 0.0
        self.t_exit = np.where(self.cell >= 0, np.nan, self.t)
        self.facet = none.copy()
        if velocities is None:
            self.v = np.zeros((n, d))
            ok = self.cell >= 0
            if ok.any():
                self.v[ok] = field(x[ok], self.cell[ok], 1.0)
        else:
            self.v = np.array(velocities, dtype=np.float64).reshape(n, d)

    def unfolded(self):
        x = self.x.copy()
        if self.periodic is not None:
            x += self.wraps * self.periodic[3][None, : x.shape[1]]
        return x

    # ---- margins ---------------------------------------------------------------------------------------------------------
    def _locate(self, xs, cell, code, act):
        if act.size == 0:
            return
        loc = self.locator
        if isinstance(loc, TM.MeshLocator):
            if loc.hint:
                ok = (cell[act] >= 0) & (cell[act] < loc.n_cells)
                if ok.any():
                    lam = TM.cell_barycentric(loc.coords, loc.cells, cell[act][ok], xs[act][ok])
                    self.margin = min(self.margin, float(np.abs(lam.min(axis=1)).min()))
            from tests import probe_model as PM

            lam_all = PM.barycentric(loc.coords, loc.cells, np.arange(loc.n_cells), xs[act])  # (cells, points, d + 1)
            best = lam_all.min(axis=2).max(axis=0)
            self.margin = min(self.margin, float(np.minimum(np.abs(best), np.abs(best + loc.tol)).min()))
        elif isinstance(loc, TM.BoxLocator):
            self.margin = min(self.margin, float(np.minimum(np.abs(xs[act] - loc.lo), np.abs(xs[act] - loc.hi)).min()))
        new = loc(xs[act], cell[act])
        cell[act[new >= 0]] = new[new >= 0]
        code[act[new < 0]] = EXITED

    def _classify(self, idx, xq):
        """Status and facet of the particles ``idx`` that left at the (folded) points ``xq``."""
        if idx.size == 0:
            return
        if self.facet_xyz is None:
            self.status[idx] = EXITED
            return
        _, near, D = WD.nearest(self.facet_xyz, xq)
        Ds = np.sort(D, axis=1)
        if D.shape[1] > 1:
            second = np.where(np.arange(D.shape[1])[None, :] == near[:, None], np.inf, D)
            rival = second.argmin(axis=1)
            differs = (self.action[rival] != self.action[near]) | self.gap_all
            gap = (Ds[:, 1] - Ds[:, 0])[differs]
            if gap.size:
                self.margin = min(self.margin, float(gap.min()))
        self.facet[idx] = near
        dep = self.action[near] == 1
        self.status[idx] = np.where(dep, DEPOSITED, EXITED).astype(np.int32)
        self.v[idx[dep]] = 0.0

    # ---- the step --------------------------------------------------------------------------------------------------------
    def advance(self, dt, field=None):
        field = self.field if field is None else field
        m = float(self.substeps)
        h = dt / m
        for s in range(self.substeps):
            live = np.nonzero(self.status == ALIVE)[0]
            if live.size == 0:
                break
            x, v, cell = self.x[live].copy(), self.v[live].copy(), self.cell[live].copy()
            tau_p, diam, beta = self.tau_p[live], self.diam[live], self.beta[live]
            code = np.zeros(live.size, dtype=np.int32)
            code[(cell < 0) | (cell >= self.locator.n_cells)] = INVALID
            xs, xu, vn = x.copy(), x.copy(), v.copy()
            ws = np.zeros(x.shape, dtype=np.int64)
            w = np.zeros_like(x)
            tau_e, tg = np.zeros(live.size), np.zeros(live.size)
            for j in range(self.n_stages + 1):
                act = np.nonzero(code == 0)[0]
                if j > 0 and act.size:
                    hq = h if j == self.n_stages else 0.5 * h
                    E, phi = coefficients(hq, tau_e[act])
                    dv = v[act] - w[act]
                    with np.errstate(invalid="ignore", over="ignore"):
                        xu[act] = x[act] + hq * w[act] + phi[:, None] * dv
                        vn[act] = w[act] + E[:, None] * dv
                    bad = ~(np.isfinite(xu[act]).all(axis=1) & np.isfinite(vn[act]).all(axis=1))
                    code[act[bad]] = INVALID
                    act = act[~bad]
                    xs[act], ws[act], gap = fold(xu[act], self.periodic)
                    self.margin = min(self.margin, gap)
                    self._locate(xs, cell, code, act)
                    act = np.nonzero(code == 0)[0]
                if j < self.n_stages and act.size:
                    u = field(xs[act], cell[act], (float(s) + (0.0 if j == 0 else 0.5)) / m)
                    bad = ~np.isfinite(u).all(axis=1)
                    code[act[bad]] = INVALID
                    good = act[~bad]
                    u = u[~bad]
                    if j == 0:
                        f = drag_factor(u, v[good], diam[good], self.nu, self.drag)
                        tau_e[good] = tau_p[good] / f
                        tg[good] = tau_e[good] * beta[good]
                    w[good] = u + tg[good][:, None] * self.g[None, :]
            done, froze = code == 0, code != 0
            step = xu[done] - x[done]
            self.path[live[done]] += np.sqrt((step * step).sum(axis=1))
            self.age[live[done]] += h
            self.x[live[done]] = xs[done]
            self.v[live[done]] = vn[done]
            self.wraps[live[done]] += ws[done]
            self.cell[live[done]] = cell[done]
            self.status[live[froze]] = code[froze]
            self.t_exit[live[froze]] = self.t + (float(s) / m) * dt
            self.cell[live[froze]] = -1
            left = code == EXITED
            self._classify(live[left], xs[left])
        self.t += dt
