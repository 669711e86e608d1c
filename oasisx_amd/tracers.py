"""Lagrangian tracers: massless particles advected through the velocity of a solver or of a blocked ``Function``.

``Tracers.advance(dt)`` enqueues ONE kernel (``ox_tracer_advance``, csrc/ox_probe.hip) that carries every live particle
through the whole step in registers -- all substeps, all Runge-Kutta stages, each with its location, basis, gather of both
time levels and blend -- on the current stream, with no host synchronisation; the fields are read through ``rptr()``, so
advancing never counts as a write of ``u``.  There is no CPU path.

Semantics (tests/tracer_model.py is the numpy statement of the same rules):

* the field across a step is ``v(x, theta) = fma(theta, u_b(x) - u_a(x), u_a(x))``, theta in [0, 1]; for a
  ``FractionalStep_AB_CN`` u_a = u^n (``_U2``) and u_b = u^{n+1} (``_U1``) after ``solve``; a ``Function`` is steady;
* ``h = dt / substeps``; substep s starts at theta_s = s / substeps and a stage at the fraction c of the substep
  evaluates at theta = (s + c) / substeps;
* a particle one of whose stage points -- or whose end point, the next substep's first stage point -- lies in no cell
  stays at the start of that substep with status ``EXITED``, ``exit_time = t + theta_s dt`` and cell -1; a non-finite
  velocity or an index out of range does the same with status ``INVALID``.  Frozen particles are skipped from then on;
* a completed substep adds h to the age and ``|x_new - x_old|`` to the path length.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from . import geometry as G
from .fem import Function, VectorFunctionSpace

__all__ = ["Tracers", "ALIVE", "EXITED", "INVALID"]

ALIVE, EXITED, INVALID = 0, 1, 2


def _blocked(f, what: str):
    """(scalar space, storage) of a blocked vector Function; raises for anything else."""
    if not isinstance(f, Function):
        raise TypeError(f"Tracers: {what} is a FractionalStep_AB_CN or a blocked vector Function, not {type(f).__name__}")
    Vs = G.scalar_space(f.function_space)  # (DGSpace / HighOrderLagrangeSpace: NotImplementedError)
    if not isinstance(f.function_space, VectorFunctionSpace) or f._comp is not None:
        raise TypeError(f"Tracers: {what} must be a blocked Function on a VectorFunctionSpace (all components in one block)")
    return Vs, f._storage


class Tracers:
    """``Tracers(velocity, points, scheme="rk4", substeps=1, tol=1e-10, hint=True, sort_every=8, allow_missing=False)``.

    ``velocity``: a ``FractionalStep_AB_CN`` (call ``advance(dt)`` after ``solve(dt, ...)``) or a blocked vector
    ``Function`` of degree 1 to 3 (steady; ``advance(dt, level_a, level_b)`` takes two such Functions on the same space
    for theta = 0 and 1).  ``hint``: test the particle's last cell before the grid (rounding-level differences only: the
    field is continuous).  ``sort_every = k > 0``: every k advances the particle storage is re-sorted by kernel-cell
    position (a stable ``argsort`` and a gather on the current stream); every getter returns id order whatever the
    storage order, and the results are bit-identical with and without sorting; 0: never.  The defaults are the fastest
    of the measured combinations.  One GPU.

    On a periodic mesh (``mesh.make_periodic``) particles do NOT wrap: a particle that leaves through an identified face
    leaves the geometric mesh and freezes with status 1, as at any other boundary (``InertialParticles`` fold and count
    the images; with ``response_time=0`` they are tracers that wrap)."""

    def __init__(self, velocity, points, scheme: str = "rk4", substeps: int = 1, tol: float = G.DEFAULT_TOL,
                 hint: bool = True, sort_every: int = 8, allow_missing: bool = False):
        if scheme not in _lib.TRACER_SCHEMES:
            raise ValueError(f"Tracers: scheme = {scheme!r}; one of {sorted(_lib.TRACER_SCHEMES)}")
        if int(substeps) != substeps or not 1 <= int(substeps) <= _lib.TRACER_MAX_SUBSTEPS:
            raise ValueError(f"Tracers: substeps = {substeps} (1..{_lib.TRACER_MAX_SUBSTEPS})")
        if not (0.0 <= float(tol) <= 1e-2):
            raise ValueError(f"Tracers: tol = {tol}: a tolerance on barycentric coordinates, 0 <= tol <= 1e-2")
        if int(sort_every) != sort_every or int(sort_every) < 0:
            raise ValueError(f"Tracers: sort_every = {sort_every}")
        self._solver = None
        if isinstance(velocity, Function):
            Vs, storage = _blocked(velocity, "velocity")
            self._levels = (storage, storage)
        elif all(hasattr(velocity, a) for a in ("_U1", "_U2", "_V", "solve")):
            Vs = G.scalar_space(velocity._V)
            self._solver = velocity
            self._levels = (velocity._U2, velocity._U1)
        else:
            raise TypeError(f"Tracers: velocity is a FractionalStep_AB_CN or a blocked vector Function, not "
                            f"{type(velocity).__name__}")
        if Vs.part is not None:
            raise NotImplementedError("Tracers on a mesh partition run on one GPU: particles that cross ranks need migration")
        if not 1 <= int(Vs.degree) <= 3:
            raise NotImplementedError(f"Tracers: degree {Vs.degree}; the device path covers degree 1 to 3")
        mesh = Vs.mesh
        if self._levels[0].nc < mesh.gdim or self._levels[0].nc > 3:
            raise ValueError(f"Tracers: a velocity block of {self._levels[0].nc} columns on a {mesh.gdim}-D mesh")
        X = G.as_points(points, mesh.gdim, mesh.device)  # (the shape check)
        self.Vs, self.mesh = Vs, mesh
        self.scheme, self.substeps, self.tol = scheme, int(substeps), float(tol)
        self.hint, self.sort_every, self.allow_missing = bool(hint), int(sort_every), bool(allow_missing)
        self._tree = G.space_tree(Vs, self.tol)  # (a mesh on the CPU: OasisxHipError, as bb_tree)
        self._cell_inv = G.kernel_position_table(Vs)
        dev = mesh.device
        self._x = torch.empty((0, mesh.gdim), dtype=torch.float64, device=dev)
        self._cell = torch.empty(0, dtype=torch.int64, device=dev)
        self._status = torch.empty(0, dtype=torch.int32, device=dev)
        self._age = torch.empty(0, dtype=torch.float64, device=dev)
        self._path = torch.empty(0, dtype=torch.float64, device=dev)
        self._t_exit = torch.empty(0, dtype=torch.float64, device=dev)
        self._ids = None  # id of storage slot i (None: i)
        self.t = 0.0
        self._n_advances = 0
        self._ring_x = self._ring_s = None
        self._times = []
        self.inject(X)

    # ---- particles -------------------------------------------------------------------------------------------------------
    @property
    def n(self) -> int:
        return int(self._x.shape[0])

    def inject(self, points) -> np.ndarray:
        """Append particles of age 0 at ``points``; returns their ids (they continue the sequence)."""
        X = G.as_points(points, self.mesh.gdim, self.mesh.device)
        m, n0 = int(X.shape[0]), self.n
        cells, _ = self._tree.find(X)
        found = cells >= 0
        if not self.allow_missing and not bool(found.all()):
            bad = torch.nonzero(~found).reshape(-1)
            raise ValueError(f"Tracers: {int(bad.shape[0])} point(s) lie in no cell of the mesh, the first at "
                             f"{X[bad[0]].tolist()} (allow_missing=True starts them as exited)")
        dev = X.device
        status = (~found).to(torch.int32) * EXITED  # (found: ALIVE)
        t_exit = torch.full((m,), self.t, dtype=torch.float64, device=dev)
        t_exit = torch.where(found, torch.full_like(t_exit, math.nan), t_exit)
        self._x = torch.cat([self._x, X])
        self._cell = torch.cat([self._cell, cells])
        self._status = torch.cat([self._status, status])
        self._age = torch.cat([self._age, torch.zeros(m, dtype=torch.float64, device=dev)])
        self._path = torch.cat([self._path, torch.zeros(m, dtype=torch.float64, device=dev)])
        self._t_exit = torch.cat([self._t_exit, t_exit])
        if self._ids is not None:
            self._ids = torch.cat([self._ids, torch.arange(n0, n0 + m, dtype=torch.int64, device=dev)])
        if self._ring_x is not None and m:  # earlier records: NaN positions, status -1 (not injected yet)
            cap = int(self._ring_x.shape[0])
            self._ring_x = torch.cat([self._ring_x, torch.full((cap, m, self.mesh.gdim), math.nan, dtype=torch.float64, device=dev)], dim=1)
            self._ring_s = torch.cat([self._ring_s, torch.full((cap, m), -1, dtype=torch.int32, device=dev)], dim=1)
        return np.arange(n0, n0 + m, dtype=np.int64)

    def _sort(self) -> None:
        """Storage order <- ascending kernel-cell position (frozen particles last); stable, so the same on every run."""
        far = int(self._cell_inv.shape[0])
        key = torch.where(self._cell >= 0, self._cell_inv[self._cell.clamp_min(0)], torch.full_like(self._cell, far))
        perm = torch.argsort(key, stable=True)
        ids = perm if self._ids is None else self._ids[perm]
        self._x, self._cell, self._status = self._x[perm].contiguous(), self._cell[perm], self._status[perm]
        self._age, self._path, self._t_exit = self._age[perm], self._path[perm], self._t_exit[perm]
        self._ids = ids

    def _level(self, f, what: str):
        Vs, storage = _blocked(f, what)
        if Vs is not self.Vs or storage.nc != self._levels[0].nc:
            raise ValueError(f"Tracers: {what} must live on the velocity's space")
        return storage

    def advance(self, dt: float, level_a=None, level_b=None) -> None:
        """Move every live particle from ``t`` to ``t + dt`` (enqueue only).  ``level_a`` / ``level_b``: blocked Functions
        on the velocity's space for theta = 0 and 1 instead of the constructor's field."""
        dt = float(dt)
        if not math.isfinite(dt):
            raise ValueError(f"Tracers.advance: dt = {dt}")
        if (level_a is None) != (level_b is None):
            raise ValueError("Tracers.advance: level_a and level_b come together")
        if level_a is not None:
            sa, sb = self._level(level_a, "level_a"), self._level(level_b, "level_b")
        else:
            sa, sb = self._levels
        if self.sort_every and self._n_advances % self.sort_every == 0:
            self._sort()
        Vs = self.Vs
        args = _lib.ox_tracer_args(
            self._tree._h, int(Vs.degree), self.mesh.gdim, sa.nc, _lib.ptr(Vs.cell_dofs), int(Vs.cell_dofs.shape[0]),
            int(Vs.n_local), _lib.ptr(self._cell_inv), int(self.mesh.num_cells), sa.rptr(), sb.rptr(), self.t, dt,
            self.substeps, _lib.TRACER_SCHEMES[self.scheme], int(self.hint), self.tol, self.n, _lib.ptr(self._x),
            _lib.ptr(self._cell), _lib.ptr(self._status), _lib.ptr(self._age), _lib.ptr(self._path), _lib.ptr(self._t_exit))
        _lib.check(_lib.load().ox_tracer_advance(C.byref(args), _lib.current_stream()), "ox_tracer_advance")
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

    # ---- records ---------------------------------------------------------------------------------------------------------
    def record(self, capacity: int = 64) -> None:
        """Append positions and status (id order) to a device ring that doubles when full; ``capacity`` sizes the ring
        at the first record."""
        if int(capacity) < 1:
            raise ValueError(f"Tracers.record: capacity = {capacity}")
        dev, d = self._x.device, self.mesh.gdim
        if self._ring_x is None:
            self._ring_x = torch.full((int(capacity), self.n, d), math.nan, dtype=torch.float64, device=dev)
            self._ring_s = torch.full((int(capacity), self.n), -1, dtype=torch.int32, device=dev)
        k, cap = len(self._times), int(self._ring_x.shape[0])
        if k == cap:
            self._ring_x = torch.cat([self._ring_x, torch.full_like(self._ring_x, math.nan)])
            self._ring_s = torch.cat([self._ring_s, torch.full_like(self._ring_s, -1)])
        if self._ids is None:
            self._ring_x[k].copy_(self._x)
            self._ring_s[k].copy_(self._status)
        else:
            self._ring_x[k].index_copy_(0, self._ids, self._x)
            self._ring_s[k].index_copy_(0, self._ids, self._status)
        self._times.append(self.t)

    @property
    def n_records(self) -> int:
        return len(self._times)

    def trajectories(self):
        """(positions (n_records, n, gdim), status (n_records, n), times (n_records,)) on the host; a particle injected
        after a record has NaN positions and status -1 there."""
        k = len(self._times)
        d = self.mesh.gdim
        if self._ring_x is None:
            return np.zeros((0, self.n, d)), np.zeros((0, self.n), dtype=np.int32), np.zeros(0)
        return self._ring_x[:k].cpu().numpy(), self._ring_s[:k].cpu().numpy(), np.asarray(self._times, dtype=np.float64)

    def save(self, path) -> None:
        X, S, times = self.trajectories()
        np.savez(path, positions=X, status=S, times=times, final_positions=self.positions(), final_status=self.status(),
                 age=self.age(), path_length=self.path_length(), exit_time=self.exit_time(), cells=self.cells(), t=self.t)
