"""Flow diagnostics and running turbulence statistics, evaluated on the device beside the time step.

Both objects read the solver's ``u``, ``p`` and ``nut`` through ``rptr()`` (a sample never counts as a write), launch on
the current stream and never synchronise with the host inside ``sample()``.  A solver without them makes none of these
calls.  One GPU.

:class:`FlowDiagnostics` -- per ``sample(t, dt, nu)`` two launches: ``ox_flow_cells`` (one lane per cell) and
``ox_flow_reduce`` (one block), which writes one row of a device ring::

    volume          sum |cell|                          enstrophy   1/2 int |curl u|^2
    kinetic_energy  1/2 int |u|^2                       div_l2      sqrt(int (div u)^2)
    strain2         int 2 S:S                           div_net     int div u
    dissipation     int (nu + nut) 2 S:S                cfl_max     max over the cells of cfl

The integrals are exact for the element.  The optional per-cell ``fields`` are values at the cell's CENTROID::

    cfl         dt max_a |u(x_c) . grad lambda_a|       divergence   tr grad u
    shear_rate  sqrt(2 S:S)                             q_criterion  1/2 (W:W - S:S)
    vorticity   g[1][0] - g[0][1] (2-D) | curl u (3-D)

``cfl`` is the rate at which the flow crosses the cell in barycentric units: ``|u . grad lambda_a|`` is the reciprocal of
the time the centroid velocity needs to cross the cell along the height onto facet ``a``, so flat boundary-layer cells are
seen with their short height.  It is a P1 measure: the nodes of a P2 / P3 element are spaced about 2 / 3 times finer than
the cell.  ``cfl_max`` is NaN as soon as one cell's value is: a run that has blown up shows NaN, not the largest finite
value.

:class:`FlowStatistics` -- running weighted mean and covariance of ``u``, ``p`` and scalars AT THE DOFS (per dof in time;
nothing is averaged in space), one launch of ``ox_stats_accumulate`` per field and sample: West's (1979) incremental
update, which keeps the variance when the mean dominates (raw sums of squares would cancel).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .fem import Function

__all__ = ["FlowDiagnostics", "FlowStatistics", "FIELD_NAMES", "RING_COLUMNS"]

FIELD_NAMES = ("cfl", "shear_rate", "divergence", "q_criterion", "vorticity")
# the columns of a ring row / of cell_integrals (the first seven)
RING_COLUMNS = ("volume", "kinetic_energy", "strain2", "dissipation", "enstrophy", "div2", "div_net", "cfl_max")


def _one_gpu(solver, who: str, what: str):
    comm = getattr(solver._mesh, "comm", None)
    if comm is not None and getattr(comm, "size", 1) > 1:
        raise NotImplementedError(f"{who} on a mesh partition (comm.size > 1): {what} are built for one GPU")


class FlowDiagnostics:
    """Global diagnostics (a device ring, one row per sample) and derived per-cell fields of a ``FractionalStep_AB_CN``.

    Args:
        solver: the solver (one GPU: ``comm.size > 1`` raises ``NotImplementedError``)
        fields: names out of ``FIELD_NAMES`` that ``cell_field`` will be asked for (any one makes the kernel write all)
        capacity: initial length of the ring (it doubles when full)
        cell_integrals: keep the seven integrals per cell too (``cell_integrals()``: DG0 energy / dissipation maps)
    """

    def __init__(self, solver, fields=(), capacity: int = 64, cell_integrals: bool = False):
        _one_gpu(solver, "FlowDiagnostics", "the per-cell evaluation and the sums")
        fields = (fields,) if isinstance(fields, str) else tuple(fields)
        for f in fields:
            if f not in FIELD_NAMES:
                raise ValueError(f"FlowDiagnostics: unknown field {f!r} (known: {', '.join(FIELD_NAMES)})")
        if int(capacity) < 1:
            raise ValueError(f"FlowDiagnostics: capacity = {capacity}")
        self._solver = solver
        self.fields = fields
        self.gdim = d = solver._mesh.gdim
        self.n_cells = nc = int(solver._geom.shape[0])
        self.n_blocks = (nc + 255) // 256
        dev = solver._mesh.device
        self._nf = 4 + (1 if d == 2 else 3)

        def rows(*shape):
            return torch.zeros(shape, dtype=torch.float64, device=dev)

        self._fields = rows(nc, self._nf) if fields else None
        self._cint = rows(nc, 7) if cell_integrals else None
        self._partials = rows(self.n_blocks, 8)
        self.capacity = int(capacity)
        self._ring = rows(self.capacity, 8)
        self._times = []

    @property
    def n_samples(self) -> int:
        return len(self._times)

    def sample(self, t: float, dt: float, nu: float) -> None:
        """Evaluate the diagnostics of the solver's current ``u`` (and ``nut``) on the current stream -- no host
        synchronisation.  ``dt``: the step the CFL number is formed with; ``nu``: the viscosity of the dissipation."""
        dt, nu = float(dt), float(nu)
        if not (dt > 0.0 and np.isfinite(dt)):
            raise ValueError(f"FlowDiagnostics.sample: dt = {dt} (the CFL number needs dt > 0)")
        if not (nu >= 0.0 and np.isfinite(nu)):
            raise ValueError(f"FlowDiagnostics.sample: nu = {nu}")
        k = len(self._times)
        if k == self.capacity:  # the ring doubles (a device copy on the current stream)
            ring = torch.zeros((2 * self.capacity, 8), dtype=torch.float64, device=self._ring.device)
            ring[: self.capacity] = self._ring
            self._ring, self.capacity = ring, 2 * self.capacity
        S = self._solver
        Vi = S._Vi[0][0]
        lib, st = _lib.load(), _lib.current_stream()
        _lib.check(lib.ox_flow_cells(Vi.degree, C.byref(S._cells), _lib.ptr(Vi.cell_dofs), S._U.rptr(), _lib.ptr(S._nut), dt, nu,
                                     _lib.ptr(self._fields), _lib.ptr(self._cint), _lib.ptr(self._partials), st),
                   "ox_flow_cells")
        _lib.check(lib.ox_flow_reduce(self.n_blocks, _lib.ptr(self._partials), _lib.ptr(self._ring), self.capacity, k, st),
                   "ox_flow_reduce")
        self._times.append(float(t))

    def latest(self) -> torch.Tensor:
        """The ring row of the latest sample (``RING_COLUMNS``) on the device -- no synchronisation."""
        if not self._times:
            raise RuntimeError("FlowDiagnostics: no sample has been taken")
        return self._ring[len(self._times) - 1]

    def history(self) -> dict:
        """Host arrays over the samples: ``t, volume, kinetic_energy, dissipation, strain2, enstrophy, div_l2, div_net,
        cfl_max`` (this reads the ring back: it synchronises)."""
        r = self._ring[: len(self._times)].cpu().numpy()
        return dict(t=np.asarray(self._times, dtype=np.float64), volume=r[:, 0].copy(), kinetic_energy=r[:, 1].copy(),
                    dissipation=r[:, 3].copy(), strain2=r[:, 2].copy(), enstrophy=r[:, 4].copy(), div_l2=np.sqrt(r[:, 5]),
                    div_net=r[:, 6].copy(), cfl_max=r[:, 7].copy())

    def _mesh_order(self, a: torch.Tensor) -> torch.Tensor:
        out = torch.zeros((int(self._solver._mesh.num_cells),) + tuple(a.shape[1:]), dtype=torch.float64, device=a.device)
        out[self._solver._Vi[0][0].local_cells.to(torch.int64)] = a
        return out

    def cell_field(self, name: str) -> torch.Tensor:
        """A centroid field of the latest sample in the MESH's cell order (``vorticity`` in 3-D: ``(num_cells, 3)``)."""
        if name not in FIELD_NAMES:
            raise ValueError(f"FlowDiagnostics: unknown field {name!r} (known: {', '.join(FIELD_NAMES)})")
        if name not in self.fields:
            raise ValueError(f"FlowDiagnostics: {name!r} was not among fields={self.fields!r} when the object was built")
        if not self._times:
            raise RuntimeError("FlowDiagnostics: no sample has been taken")
        k = FIELD_NAMES.index(name)
        col = self._fields[:, 4:] if (k == 4 and self.gdim == 3) else self._fields[:, k]
        return self._mesh_order(col)

    def cell_integrals(self) -> torch.Tensor:
        """``(num_cells, 7)`` in the MESH's cell order: the first seven ``RING_COLUMNS`` per cell, latest sample."""
        if self._cint is None:
            raise RuntimeError("FlowDiagnostics: built without cell_integrals=True")
        return self._mesh_order(self._cint)

    def save(self, path) -> None:
        out = dict(self.history())
        for name in self.fields if self._times else ():
            out[name] = self.cell_field(name).cpu().numpy()
        if self._cint is not None and self._times:
            out["cell_integrals"] = self.cell_integrals().cpu().numpy()
        np.savez(path, **out)


class _Moments:
    """One field of FlowStatistics: where it is read (``storage``, first column, components) and its moments."""

    def __init__(self, name, storage, col, ncomp, n, mean_fn):
        self.name, self.storage, self.col, self.ncomp, self.n, self.mean = name, storage, col, ncomp, n, mean_fn
        self.cov = torch.zeros((mean_fn._storage.n_alloc, ncomp * (ncomp + 1) // 2), dtype=torch.float64,
                               device=mean_fn._storage.rdev().device)


class FlowStatistics:
    """Running weighted mean and covariance per dof of a ``FractionalStep_AB_CN``'s fields.

    Args:
        solver: the solver (one GPU)
        fields: out of ``"u"`` (all components, one launch: the Reynolds stresses ``<u_i' u_j'>``) and ``"p"``
        scalars: names of the solver's ``ScalarTransport`` fields
    """

    def __init__(self, solver, fields=("u", "p"), scalars=()):
        _one_gpu(solver, "FlowStatistics", "the moments per dof")
        fields = (fields,) if isinstance(fields, str) else tuple(fields)
        scalars = (scalars,) if isinstance(scalars, str) else tuple(scalars)
        self._solver = solver
        self._m = {}
        Vi, Q = solver._Vi[0][0], solver._Q
        for f in fields:
            if f == "u":
                self._m[f] = _Moments(f, solver._U, 0, solver._gdim, solver._n_u, Function(solver._V, "mean_u"))
            elif f == "p":
                self._m[f] = _Moments(f, solver._P, 0, 1, solver._n_q, Function(Q, "mean_p"))
            else:
                raise ValueError(f"FlowStatistics: unknown field {f!r} (known: 'u', 'p'; scalars go into scalars=)")
        for s in scalars:
            if s in self._m:
                raise ValueError(f"FlowStatistics: {s!r} is listed twice")
            try:
                c = solver.scalar(s)
            except KeyError as exc:
                raise ValueError(f"FlowStatistics: {exc.args[0]}") from None
            W = c.function_space
            self._m[s] = _Moments(s, c._storage, int(c._comp), 1, int(c._storage.n), Function(W, f"mean_{s}"))
        for m in self._m.values():
            if m.mean._storage.n != m.n:
                raise RuntimeError(f"FlowStatistics: {m.name!r} has {m.n} rows, its space {m.mean._storage.n}")
        self._Vi = Vi
        self._W = 0.0
        self.n_samples = 0

    @property
    def names(self):
        return tuple(self._m)

    @property
    def total_weight(self) -> float:
        return self._W

    def sample(self, dt: float) -> None:
        """Add the solver's current fields with weight ``dt > 0`` -- one launch per field on the current stream."""
        w = float(dt)
        if not (w > 0.0 and np.isfinite(w)):
            raise ValueError(f"FlowStatistics.sample: dt = {w} (a sample needs a weight > 0)")
        lib, st = _lib.load(), _lib.current_stream()
        for m in self._m.values():
            src = m.storage.rdev()
            x = C.c_void_p(src.data_ptr() + 8 * m.col)
            _lib.check(lib.ox_stats_accumulate(m.ncomp, m.n, x, int(src.shape[1]), w, self._W, m.mean._storage.ptr(),
                                               _lib.ptr(m.cov), st), "ox_stats_accumulate")
        self._W += w
        self.n_samples += 1

    def _get(self, name) -> _Moments:
        if name not in self._m:
            raise ValueError(f"FlowStatistics: no statistics of {name!r} (have: {', '.join(self._m)})")
        return self._m[name]

    def _need_weight(self):
        if not self._W > 0.0:
            raise RuntimeError("FlowStatistics: no sample has been taken since the statistics were reset")

    def mean(self, name: str) -> Function:
        """The running mean as a ``Function`` on the field's own space (``"u"``: the solver's blocked velocity space), so
        ``VTXWriter``, ``Function.eval`` and ``Probes`` work on it.  The object's own storage: it follows later samples."""
        self._need_weight()
        return self._get(name).mean

    def covariance(self, name: str) -> torch.Tensor:
        """``cov / W`` on the device: ``(n, k (k + 1) / 2)``, the upper triangle row by row (``00, 01, 02, 11, 12, 22``)."""
        self._need_weight()
        m = self._get(name)
        return m.cov[: m.n] / self._W

    def variance(self, name: str) -> torch.Tensor:
        """The variance of a one-component field, ``(n,)`` on the device."""
        m = self._get(name)
        if m.ncomp != 1:
            raise ValueError(f"FlowStatistics.variance: {name!r} has {m.ncomp} components (covariance() has them all)")
        return self.covariance(name)[:, 0]

    def tke(self) -> Function:
        """Turbulent kinetic energy ``1/2 tr <u' u'>`` as a ``Function`` on the velocity component space."""
        cov = self.covariance("u")
        d = self._get("u").ncomp
        diag = [0, 2] if d == 2 else [0, 3, 5]
        k = Function(self._Vi, "tke")
        acc = cov[:, diag[0]].clone()
        for c in diag[1:]:
            acc += cov[:, c]
        k._storage.dev()[: acc.shape[0], 0] = 0.5 * acc
        return k

    def reset(self) -> None:
        for m in self._m.values():
            m.mean._storage.dev().zero_()
            m.cov.zero_()
        self._W = 0.0
        self.n_samples = 0

    def save(self, path) -> None:
        out = dict(total_weight=np.float64(self._W), n_samples=np.int64(self.n_samples), names=np.array(list(self._m)))
        for m in self._m.values():
            out["mean_" + m.name] = m.mean._storage.rhost()
            out["cov_" + m.name] = m.cov[: m.n].cpu().numpy()
        np.savez(path, **out)

    @classmethod
    def load(cls, solver, path) -> "FlowStatistics":
        """The statistics ``save`` wrote, bound to ``solver`` (the same mesh, spaces and scalars): averaging goes on
        after a restart."""
        with np.load(path) as z:
            names = [str(s) for s in z["names"]]
            obj = cls(solver, fields=[s for s in names if s in ("u", "p")], scalars=[s for s in names if s not in ("u", "p")])
            for m in obj._m.values():
                mean, cov = z["mean_" + m.name], z["cov_" + m.name]
                if mean.shape != (m.n, m.ncomp) or cov.shape != (m.n, m.cov.shape[1]):
                    raise ValueError(f"FlowStatistics.load: {m.name!r} was saved with shapes {mean.shape}, {cov.shape}; the "
                                     f"solver has {(m.n, m.ncomp)}")
                dev = m.cov.device
                m.mean._storage.dev()[: m.n] = torch.from_numpy(np.ascontiguousarray(mean)).to(dev)
                m.cov[: m.n] = torch.from_numpy(np.ascontiguousarray(cov)).to(dev)
            obj._W = float(z["total_weight"])
            obj.n_samples = int(z["n_samples"])
        return obj
