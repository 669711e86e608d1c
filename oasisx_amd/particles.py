"""Inertial particles: point particles with mass, one-way coupled to the velocity of a solver or of a blocked ``Function``.

    dx/dt = v,      dv/dt = (f / tau_p) (u(x, t) - v) + (1 - rho_f / rho_p) g

``tau_p = (rho_p / rho_f) d^2 / (18 nu)``; ``f = 1`` (``drag="stokes"``) or ``1 + 0.15 Re_p^0.687`` with
``Re_p = d |u - v| / nu`` (``drag="schiller_naumann"``).  Added mass, lift, the history force and collisions are left out:
the model holds for ``rho_p >> rho_f``.

``InertialParticles.advance(dt)`` enqueues ``ox_particle_advance`` (csrc/ox_probe.hip): one kernel that carries every
live particle through all substeps in registers, and behind it the classification of the particles that left the mesh in
this advance.  Nothing is read back; the fields are read through ``rptr()``.  There is no CPU path.

Semantics (tests/particle_model.py is the numpy statement of the same rules):

* the field across a step is the tracers': ``u(x, theta) = fma(theta, u_b(x) - u_a(x), u_a(x))``;
* a substep of ``h = dt / substeps`` from ``(x, v)`` at ``theta_s``: ``u0`` = the field at ``x``; ``f`` from ``(u0, v)``,
  frozen; ``tau_e = tau_p / f``; ``w = u0 + tau_e beta g``; ``E = exp(-h / tau_e)``, ``phi = tau_e (1 - E)`` (both 0 at
  ``tau_e = 0``); ``x_new = x + h w + phi (v - w)``, ``v_new = w + E (v - w)``: exact for a uniform steady field whatever
  ``h / tau_p`` (``scheme="exp1"``).  ``scheme="exp2"`` takes the fluid velocity of the update at the end point of the
  same formulas with ``h / 2``, at ``theta_s + 1 / (2 substeps)``.  At ``tau_p = 0`` these are the tracers' ``euler`` and
  ``rk2``;
* on a ``make_periodic`` mesh every predictor and end point is folded into ``[lo, hi)`` on the identified axes before it is
  located, and the images are counted: ``unfolded_positions() = x + wraps * period``;
* a point that lies in no cell ends the particle at the START of that substep, as a tracer (``exit_time``, cell -1); its
  nearest exterior facet (ties: the lower facet id) is the particle's ``facet``; on a facet of ``walls`` the particle is
  ``DEPOSITED`` (status 3, velocity 0), elsewhere ``EXITED`` (status 1).  A non-finite velocity or a bad index: status 2.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from . import geometry as G
from .fem import Function
from .tracers import EXITED, _blocked

__all__ = ["InertialParticles", "DEPOSITED"]

DEPOSITED = 3


def _per_particle(value, m: int, what: str, positive: bool = False) -> np.ndarray:
    """(m,) float64 of a float or a per-particle array; finite, >= 0 (> 0 with ``positive``)."""
    a = np.asarray(value, dtype=np.float64)
    if a.ndim == 0:
        a = np.full(m, float(a))
    a = np.ascontiguousarray(a.reshape(-1))
    if a.shape[0] != m:
        raise ValueError(f"InertialParticles: {what} has {a.shape[0]} entries for {m} particles")
    if not np.isfinite(a).all():
        raise ValueError(f"InertialParticles: {what} is not finite")
    if positive and not (a > 0.0).all():
        raise ValueError(f"InertialParticles: {what} <= 0 (a density is positive; response_time= sets tau_p directly)")
    if (a < 0.0).any():
        raise ValueError(f"InertialParticles: {what} is negative")
    return a


class InertialParticles:
    """``InertialParticles(velocity, points, diameter, density, fluid_density=1.0, nu=..., gravity=None, velocities=None,
    drag="stokes", scheme="exp2", substeps=1, walls=None, tol=1e-10, hint=True, sort_every=8, allow_missing=False,
    response_time=None)``.

    ``velocity``: a ``FractionalStep_AB_CN`` (call ``advance(dt)`` after ``solve``) or a blocked vector ``Function`` of
    degree 1 to 3, as for ``Tracers``.  ``diameter`` / ``density``: floats or per-particle arrays; ``response_time=`` gives
    ``tau_p`` directly in place of ``density`` (0 is allowed: a tracer); without a density the buoyancy factor
    ``beta = 1 - rho_f / rho_p`` is 1.  ``velocities=None`` starts the particles at the fluid velocity of level b.
    ``walls``: ``None`` (nothing deposits), ``(meshtags, id | ids)`` or an array of facet ids: the exterior facets on which
    a particle deposits.  ``hint`` / ``sort_every``: as for ``Tracers``; every getter returns id order and the results are
    bit-identical with and without sorting.  One GPU."""

    def __init__(self, velocity, points, diameter, density=None, fluid_density: float = 1.0, nu: float | None = None,
                 gravity=None, velocities=None, drag: str = "stokes", scheme: str = "exp2", substeps: int = 1, walls=None,
                 tol: float = G.DEFAULT_TOL, hint: bool = True, sort_every: int = 8, allow_missing: bool = False,
                 response_time=None):
        from .wall import select_facets

        if scheme not in _lib.PARTICLE_SCHEMES:
            raise ValueError(f"InertialParticles: scheme = {scheme!r}; one of {sorted(_lib.PARTICLE_SCHEMES)}")
        if drag not in _lib.PARTICLE_DRAG:
            raise ValueError(f"InertialParticles: drag = {drag!r}; one of {sorted(_lib.PARTICLE_DRAG)}")
        if int(substeps) != substeps or not 1 <= int(substeps) <= _lib.TRACER_MAX_SUBSTEPS:
            raise ValueError(f"InertialParticles: substeps = {substeps} (1..{_lib.TRACER_MAX_SUBSTEPS})")
        if not (0.0 <= float(tol) <= 1e-2):
            raise ValueError(f"InertialParticles: tol = {tol}: a tolerance on barycentric coordinates, 0 <= tol <= 1e-2")
        if int(sort_every) != sort_every or int(sort_every) < 0:
            raise ValueError(f"InertialParticles: sort_every = {sort_every}")
        if nu is None:
            raise ValueError("InertialParticles: nu (the kinematic viscosity of the fluid) is required")
        nu, rho_f = float(nu), float(fluid_density)
        if not math.isfinite(nu) or nu < 0.0:
            raise ValueError(f"InertialParticles: nu = {nu} is negative or not finite")
        if not math.isfinite(rho_f) or rho_f <= 0.0:
            raise ValueError(f"InertialParticles: fluid_density = {rho_f}")
        if density is None and response_time is None:
            raise ValueError("InertialParticles: density <= 0 is not a particle; give density= or response_time=")
        if nu == 0.0 and (response_time is None or drag != "stokes"):
            raise ValueError("InertialParticles: nu = 0 leaves tau_p and Re_p undefined (response_time= with Stokes drag only)")
        self._solver = None
        if isinstance(velocity, Function):
            Vs, storage = _blocked(velocity, "velocity")
            self._levels = (storage, storage)
        elif all(hasattr(velocity, a) for a in ("_U1", "_U2", "_V", "solve")):
            Vs = G.scalar_space(velocity._V)
            self._solver = velocity
            self._levels = (velocity._U2, velocity._U1)
        else:
            raise TypeError(f"InertialParticles: velocity is a FractionalStep_AB_CN or a blocked vector Function, not "
                            f"{type(velocity).__name__}")
        if Vs.part is not None:
            raise NotImplementedError("InertialParticles on a mesh partition run on one GPU: particles that cross ranks "
                                      "need migration")
        if not 1 <= int(Vs.degree) <= 3:
            raise NotImplementedError(f"InertialParticles: degree {Vs.degree}; the device path covers degree 1 to 3")
        mesh = Vs.mesh
        d = mesh.gdim
        if self._levels[0].nc < d or self._levels[0].nc > 3:
            raise ValueError(f"InertialParticles: a velocity block of {self._levels[0].nc} columns on a {d}-D mesh")
        g = np.zeros(3) if gravity is None else np.asarray(gravity, dtype=np.float64).reshape(-1)
        if g.shape[0] not in (d, 3) or not np.isfinite(g).all():
            raise ValueError(f"InertialParticles: gravity = {gravity!r}: {d} finite components")
        self.gravity = np.concatenate([g[:d], np.zeros(3 - d)])
        self.Vs, self.mesh = Vs, mesh
        self.nu, self.fluid_density, self.drag, self.scheme = nu, rho_f, drag, scheme
        self.substeps, self.tol = int(substeps), float(tol)
        self.hint, self.sort_every, self.allow_missing = bool(hint), int(sort_every), bool(allow_missing)
        self._tree = G.space_tree(Vs, self.tol)  # (a mesh on the CPU: OasisxHipError, as bb_tree)
        self._cell_inv = G.kernel_position_table(Vs)
        # the exterior facets (on a periodic mesh: the non-identified ones), ascending ids, and what each does to a particle
        self._walls = G.WallDistance(mesh)
        self.exterior = np.asarray(self._walls.facets, dtype=np.int64)
        action = np.zeros(self.exterior.shape[0], dtype=np.int32)
        if walls is not None:
            ids = select_facets(mesh, walls, "InertialParticles")[0]
            if not np.isin(ids, self.exterior).all():
                raise ValueError("InertialParticles: walls names facets that are not exterior facets of the mesh")
            action[np.isin(self.exterior, ids)] = 1
        dev = mesh.device
        self._action = torch.from_numpy(action).to(dev)
        self._ext_dev = torch.from_numpy(self.exterior).to(dev)
        per = getattr(mesh, "periodic", None)
        self._periodic, self._lo, self._hi, self._period = [0] * 3, [0.0] * 3, [0.0] * 3, [0.0] * 3
        if per is not None:
            for k in per.axes:
                self._periodic[k], self._lo[k], self._hi[k] = 1, float(per.lo[k]), float(per.hi[k])
                self._period[k] = float(per.period[k])
        self.period = np.asarray(self._period[:d], dtype=np.float64)
        f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)  # noqa: E731
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)  # noqa: E731
        self._x, self._v, self._xq = f64(0, d), f64(0, d), f64(0, d)
        self._cell = torch.empty(0, dtype=torch.int64, device=dev)
        self._status, self._facet, self._wraps = i32(0), i32(0), i32(0, d)
        self._age, self._path, self._t_exit = f64(0), f64(0), f64(0)
        self._tau, self._diam, self._beta = f64(0), f64(0), f64(0)
        self._ids = None  # id of storage slot i (None: i)
        self.t = 0.0
        self._n_advances = 0
        self._ring_x = self._ring_v = self._ring_s = None
        self._times = []
        self.inject(points, velocities, diameter=diameter, density=density, response_time=response_time)

    # ---- particles -------------------------------------------------------------------------------------------------------
    @property
    def n(self) -> int:
        return int(self._x.shape[0])

    _FIELDS = ("_x", "_v", "_cell", "_status", "_age", "_path", "_t_exit", "_wraps", "_facet", "_tau", "_diam", "_beta")

    def _fold(self, X: torch.Tensor):
        """(X folded into [lo, hi) on the periodic axes, the image counts): the kernel's fold."""
        X = X.clone()
        W = torch.zeros(X.shape, dtype=torch.int32, device=X.device)
        for k in range(self.mesh.gdim):
            if self._periodic[k]:
                q = torch.floor((X[:, k] - self._lo[k]) / self._period[k])
                xk = X[:, k] - self._period[k] * q
                over = xk >= self._hi[k]
                xk = torch.where(over, xk - self._period[k], xk)
                ok = torch.isfinite(q)
                X[:, k] = xk
                W[:, k] = (torch.where(ok, q, torch.zeros_like(q)) + over.to(q.dtype)).to(torch.int32)
        return X, W

    def _fluid_velocity(self, X, cells, bary) -> torch.Tensor:
        """The field of level b at located points (0 where there is no cell)."""
        d, sb = self.mesh.gdim, self._levels[1]
        plan = G.PointPlan(self.Vs, cells, bary)
        out = torch.empty((plan.n, sb.nc), dtype=torch.float64, device=X.device)
        if plan.n:
            _lib.check(_lib.load().ox_eval_points(*plan.args(), sb.rptr(), sb.nc, -1, _lib.ptr(out), sb.nc, 0,
                                                  _lib.current_stream()), "ox_eval_points")
        return torch.where((cells >= 0)[:, None], out[:, :d], torch.zeros_like(out[:, :d])).contiguous()

    def inject(self, points, velocities=None, diameter=None, density=None, response_time=None) -> np.ndarray:
        """Append particles of age 0 at ``points``; returns their ids (they continue the sequence)."""
        d, dev = self.mesh.gdim, self.mesh.device
        X = G.as_points(points, d, dev)
        m, n0 = int(X.shape[0]), self.n
        if diameter is None:
            raise ValueError("InertialParticles.inject: diameter is required")
        diam = _per_particle(diameter, m, "diameter")
        if response_time is not None:
            tau = _per_particle(response_time, m, "response_time")
            beta = np.ones(m)
            if density is not None:
                beta = 1.0 - self.fluid_density / _per_particle(density, m, "density", positive=True)
        else:
            if density is None:
                raise ValueError("InertialParticles.inject: density <= 0 is not a particle; give density= or response_time=")
            rho = _per_particle(density, m, "density", positive=True)
            tau = (rho / self.fluid_density) * diam * diam / (18.0 * self.nu)
            beta = 1.0 - self.fluid_density / rho
        X, W = self._fold(X)
        cells, bary = self._tree.find(X)
        found = cells >= 0
        if not self.allow_missing and not bool(found.all()):
            bad = torch.nonzero(~found).reshape(-1)
            raise ValueError(f"InertialParticles: {int(bad.shape[0])} point(s) lie in no cell of the mesh, the first at "
                             f"{X[bad[0]].tolist()} (allow_missing=True starts them as exited)")
        if velocities is None:
            V = self._fluid_velocity(X, cells, bary)
        else:
            V = G.as_points(velocities, d, dev)
            if int(V.shape[0]) != m:
                raise ValueError(f"InertialParticles: {int(V.shape[0])} velocities for {m} points")
        status = (~found).to(torch.int32) * EXITED  # (found: ALIVE)
        t_exit = torch.full((m,), self.t, dtype=torch.float64, device=dev)
        t_exit = torch.where(found, torch.full_like(t_exit, math.nan), t_exit)
        zeros = torch.zeros(m, dtype=torch.float64, device=dev)
        new = dict(_x=X, _v=V, _cell=cells, _status=status, _age=zeros, _path=zeros.clone(), _t_exit=t_exit, _wraps=W,
                   _facet=torch.full((m,), -1, dtype=torch.int32, device=dev), _tau=torch.from_numpy(tau).to(dev),
                   _diam=torch.from_numpy(diam).to(dev), _beta=torch.from_numpy(np.ascontiguousarray(beta)).to(dev))
        for name in self._FIELDS:
            setattr(self, name, torch.cat([getattr(self, name), new[name]]).contiguous())
        self._xq = torch.zeros((n0 + m, d), dtype=torch.float64, device=dev)
        if self._ids is not None:
            self._ids = torch.cat([self._ids, torch.arange(n0, n0 + m, dtype=torch.int64, device=dev)])
        if self._ring_x is not None and m:  # earlier records: NaN positions and velocities, status -1 (not injected yet)
            cap = int(self._ring_x.shape[0])
            nan = torch.full((cap, m, d), math.nan, dtype=torch.float64, device=dev)
            self._ring_x = torch.cat([self._ring_x, nan], dim=1)
            self._ring_v = torch.cat([self._ring_v, nan.clone()], dim=1)
            self._ring_s = torch.cat([self._ring_s, torch.full((cap, m), -1, dtype=torch.int32, device=dev)], dim=1)
        return np.arange(n0, n0 + m, dtype=np.int64)

    def _sort(self) -> None:
        """Storage order <- ascending kernel-cell position (frozen particles last); stable, so the same on every run."""
        far = int(self._cell_inv.shape[0])
        key = torch.where(self._cell >= 0, self._cell_inv[self._cell.clamp_min(0)], torch.full_like(self._cell, far))
        perm = torch.argsort(key, stable=True)
        self._ids = perm if self._ids is None else self._ids[perm]
        for name in self._FIELDS:
            setattr(self, name, getattr(self, name)[perm].contiguous())

    def _level(self, f, what: str):
        Vs, storage = _blocked(f, what)
        if Vs is not self.Vs or storage.nc != self._levels[0].nc:
            raise ValueError(f"InertialParticles: {what} must live on the velocity's space")
        return storage

    def advance(self, dt: float, level_a=None, level_b=None) -> None:
        """Move every live particle from ``t`` to ``t + dt`` (enqueue only).  ``level_a`` / ``level_b``: blocked Functions
        on the velocity's space for theta = 0 and 1 instead of the constructor's field."""
        dt = float(dt)
        if not math.isfinite(dt):
            raise ValueError(f"InertialParticles.advance: dt = {dt}")
        if (level_a is None) != (level_b is None):
            raise ValueError("InertialParticles.advance: level_a and level_b come together")
        if level_a is not None:
            sa, sb = self._level(level_a, "level_a"), self._level(level_b, "level_b")
        else:
            sa, sb = self._levels
        if self.sort_every and self._n_advances % self.sort_every == 0:
            self._sort()
        Vs, d3 = self.Vs, C.c_double * 3
        args = _lib.ox_particle_args(
            self._tree._h, self._walls._h, int(Vs.degree), self.mesh.gdim, sa.nc, _lib.ptr(Vs.cell_dofs),
            int(Vs.cell_dofs.shape[0]), int(Vs.n_local), _lib.ptr(self._cell_inv), int(self.mesh.num_cells), sa.rptr(),
            sb.rptr(), self.t, dt, self.substeps, _lib.PARTICLE_SCHEMES[self.scheme], _lib.PARTICLE_DRAG[self.drag],
            int(self.hint), self.tol, self.nu, d3(*self.gravity), (C.c_int * 3)(*self._periodic), d3(*self._lo),
            d3(*self._hi), d3(*self._period), _lib.ptr(self._action), int(self._action.shape[0]), self.n, _lib.ptr(self._x),
            _lib.ptr(self._v), _lib.ptr(self._cell), _lib.ptr(self._status), _lib.ptr(self._age), _lib.ptr(self._path),
            _lib.ptr(self._t_exit), _lib.ptr(self._wraps), _lib.ptr(self._facet), _lib.ptr(self._xq), _lib.ptr(self._tau),
            _lib.ptr(self._diam), _lib.ptr(self._beta))
        _lib.check(_lib.load().ox_particle_advance(C.byref(args), _lib.current_stream()), "ox_particle_advance")
        self.t += dt
        self._n_advances += 1

    # ---- getters: id order -----------------------------------------------------------------------------------------------
    def _by_id(self, a: torch.Tensor) -> torch.Tensor:
        if self._ids is None:
            return a
        out = torch.empty_like(a)
        out[self._ids] = a
        return out

    def positions(self) -> np.ndarray:
        return self._by_id(self._x).cpu().numpy()

    def wraps(self) -> np.ndarray:
        """(n, gdim) int32: the periodic images every particle went through."""
        return self._by_id(self._wraps).cpu().numpy()

    def unfolded_positions(self) -> np.ndarray:
        """``x + wraps * period``: the position without the periodic fold (for dispersion)."""
        return self.positions() + self.wraps().astype(np.float64) * self.period[None, :]

    def velocities(self) -> np.ndarray:
        return self._by_id(self._v).cpu().numpy()

    def status(self) -> np.ndarray:
        return self._by_id(self._status).cpu().numpy()

    def cells(self) -> np.ndarray:
        return self._by_id(self._cell).cpu().numpy()

    def age(self) -> np.ndarray:
        return self._by_id(self._age).cpu().numpy()

    def path_length(self) -> np.ndarray:
        return self._by_id(self._path).cpu().numpy()

    def exit_time(self) -> np.ndarray:
        return self._by_id(self._t_exit).cpu().numpy()

    def response_time(self) -> np.ndarray:
        return self._by_id(self._tau).cpu().numpy()

    def facet(self) -> np.ndarray:
        """The mesh facet id nearest to the point at which the particle left the mesh (-1: it has not left, it never was
        inside, or its status is 2)."""
        pos = self._by_id(self._facet).cpu().numpy().astype(np.int64)
        return np.where(pos >= 0, self.exterior[np.clip(pos, 0, self.exterior.shape[0] - 1)], -1)

    def deposition(self) -> np.ndarray:
        """Deposited particles per exterior facet, in ``mesh.exterior_facets()`` order (``io.write_facet_vtu`` writes it)."""
        pos = self._facet.cpu().numpy().astype(np.int64)
        hit = (self._status.cpu().numpy() == DEPOSITED) & (pos >= 0)
        return np.bincount(pos[hit], minlength=self.exterior.shape[0]).astype(np.int64)

    # ---- records ---------------------------------------------------------------------------------------------------------
    def record(self, capacity: int = 64) -> None:
        """Append positions, velocities and status (id order) to a device ring that doubles when full."""
        if int(capacity) < 1:
            raise ValueError(f"InertialParticles.record: capacity = {capacity}")
        dev, d = self._x.device, self.mesh.gdim
        if self._ring_x is None:
            self._ring_x = torch.full((int(capacity), self.n, d), math.nan, dtype=torch.float64, device=dev)
            self._ring_v = torch.full((int(capacity), self.n, d), math.nan, dtype=torch.float64, device=dev)
            self._ring_s = torch.full((int(capacity), self.n), -1, dtype=torch.int32, device=dev)
        k, cap = len(self._times), int(self._ring_x.shape[0])
        if k == cap:
            self._ring_x = torch.cat([self._ring_x, torch.full_like(self._ring_x, math.nan)])
            self._ring_v = torch.cat([self._ring_v, torch.full_like(self._ring_v, math.nan)])
            self._ring_s = torch.cat([self._ring_s, torch.full_like(self._ring_s, -1)])
        if self._ids is None:
            self._ring_x[k].copy_(self._x)
            self._ring_v[k].copy_(self._v)
            self._ring_s[k].copy_(self._status)
        else:
            self._ring_x[k].index_copy_(0, self._ids, self._x)
            self._ring_v[k].index_copy_(0, self._ids, self._v)
            self._ring_s[k].index_copy_(0, self._ids, self._status)
        self._times.append(self.t)

    @property
    def n_records(self) -> int:
        return len(self._times)

    def trajectories(self):
        """(positions (n_records, n, gdim), velocities (n_records, n, gdim), status (n_records, n), times (n_records,)) on
        the host; a particle injected after a record has NaN positions and velocities and status -1 there."""
        k, d = len(self._times), self.mesh.gdim
        if self._ring_x is None:
            return np.zeros((0, self.n, d)), np.zeros((0, self.n, d)), np.zeros((0, self.n), dtype=np.int32), np.zeros(0)
        return (self._ring_x[:k].cpu().numpy(), self._ring_v[:k].cpu().numpy(), self._ring_s[:k].cpu().numpy(),
                np.asarray(self._times, dtype=np.float64))

    # ---- restart ---------------------------------------------------------------------------------------------------------
    def save(self, path) -> None:
        """The whole particle state (id order) and the records: ``load`` continues the run bit for bit."""
        X, V, S, times = self.trajectories()
        np.savez(path, positions=self.positions(), velocities=self.velocities(), cells=self.cells(), status=self.status(),
                 age=self.age(), path_length=self.path_length(), exit_time=self.exit_time(), wraps=self.wraps(),
                 facet_position=self._by_id(self._facet).cpu().numpy(), facet=self.facet(), response_time=self.response_time(),
                 diameter=self._by_id(self._diam).cpu().numpy(), beta=self._by_id(self._beta).cpu().numpy(), t=self.t,
                 n_advances=self._n_advances, record_positions=X, record_velocities=V, record_status=S, record_times=times,
                 deposition=self.deposition(), exterior_facets=self.exterior)

    def load(self, path) -> None:
        """Replace the particles by the state ``save`` wrote (same mesh, field and settings): the run continues bit for bit."""
        z = np.load(path)
        dev, d = self.mesh.device, self.mesh.gdim
        if z["positions"].ndim != 2 or z["positions"].shape[1] != d or not np.array_equal(z["exterior_facets"], self.exterior):
            raise ValueError("InertialParticles.load: the file belongs to another mesh")
        names = dict(_x="positions", _v="velocities", _cell="cells", _status="status", _age="age", _path="path_length",
                     _t_exit="exit_time", _wraps="wraps", _facet="facet_position", _tau="response_time", _diam="diameter",
                     _beta="beta")
        for name in self._FIELDS:
            setattr(self, name, torch.from_numpy(np.ascontiguousarray(z[names[name]])).to(dev))
        self._xq = torch.zeros((self.n, d), dtype=torch.float64, device=dev)
        self._ids = None
        self.t, self._n_advances = float(z["t"]), int(z["n_advances"])
        self._times = [float(v) for v in z["record_times"]]
        self._ring_x = self._ring_v = self._ring_s = None
        if self._times:
            self._ring_x = torch.from_numpy(z["record_positions"]).to(dev)
            self._ring_v = torch.from_numpy(z["record_velocities"]).to(dev)
            self._ring_s = torch.from_numpy(z["record_status"]).to(dev)
