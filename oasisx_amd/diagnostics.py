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

:class:`ProfileStatistics` -- running weighted mean and covariance AVERAGED OVER SLABS of cells:
profiles across the inhomogeneous direction of a channel or a mixing layer.  :func:`slab_bins` sorts the cells of a mesh
into the slabs between the planes of an axis; any other binning goes in as ``cell_bins``.  Per group of fields and sample
two launches, ``ox_profile_cells`` (one lane per cell, cells reached through a permutation sorted by bin) and
``ox_profile_update`` (one wave per bin); the moments are exact integrals of the discrete fields, not nodal means.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .fem import Function, VectorFunctionSpace, _same_layout

__all__ = ["FlowDiagnostics", "FlowStatistics", "ProfileStatistics", "slab_bins", "FIELD_NAMES", "RING_COLUMNS"]

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


# ---- slab-averaged statistics ------------------------------------------------------------------
def slab_bins(mesh, axis: int, edges=None, tol=None):
    """The slab of every cell along ``axis``: ``(bins, edges)`` with ``bins`` int64 in the MESH's cell order (host).

    ``edges=None``: the edges are the distinct vertex coordinates along ``axis`` (two coordinates within ``tol`` times the
    extent, default 1e-8 as in ``make_periodic``, count as one plane); every cell must lie between two consecutive
    planes, which lattice meshes do -- otherwise ``ValueError``.  ``edges`` given (strictly increasing, at least two): a
    cell goes to the bin of its centroid; outside ``[edges[0], edges[-1])`` it gets -1 and is never sampled.  A bin
    without a cell is a ``ValueError``.  Pure host logic on ``mesh.coords`` / ``mesh.cells``."""
    d = int(mesh.gdim)
    axis = int(axis)
    if not 0 <= axis < d:
        raise ValueError(f"slab_bins: axis {axis} on a {d}-D mesh")
    x = mesh.coords.cpu().numpy()[:, axis]
    cells = mesh.cells.cpu().numpy()
    xc = x[cells]  # (nc, d + 1)
    if edges is None:
        lo, hi = float(x.min()), float(x.max())
        atol = (1e-8 if tol is None else float(tol)) * (hi - lo)
        xs = np.sort(x)
        first = np.concatenate([[True], np.diff(xs) > atol])
        start = np.nonzero(first)[0]
        stop = np.concatenate([start[1:], [xs.shape[0]]])
        edges = np.array([0.5 * (xs[a] + xs[b - 1]) for a, b in zip(start, stop)])  # the middle of each cluster
        if edges.shape[0] < 2:
            raise ValueError(f"slab_bins: the mesh has no extent along axis {axis}")
        plane = np.cumsum(first) - 1  # plane of each sorted coordinate
        vplane = np.empty(x.shape[0], dtype=np.int64)
        vplane[np.argsort(x, kind="stable")] = plane
        pc = vplane[cells]
        bins = pc.min(axis=1)
        bad = np.nonzero(pc.max(axis=1) - bins != 1)[0]
        if bad.shape[0]:
            c = int(bad[0])
            raise ValueError(f"slab_bins: cell {c} spans the planes {edges[pc[c].min()]:.6g} .. {edges[pc[c].max()]:.6g} of axis "
                             f"{axis}: it does not lie between two consecutive vertex planes ({bad.shape[0]} such cells); "
                             "pass edges= to bin the cells by their centroids")
    else:
        edges = np.asarray(edges, dtype=np.float64).reshape(-1)
        if edges.shape[0] < 2 or not (np.diff(edges) > 0.0).all():
            raise ValueError("slab_bins: edges must be strictly increasing and at least two")
        cen = xc.mean(axis=1)
        bins = np.searchsorted(edges, cen, side="right").astype(np.int64) - 1
        bins[(cen < edges[0]) | (cen >= edges[-1])] = -1
    n_bins = edges.shape[0] - 1
    count = np.bincount(bins[bins >= 0], minlength=n_bins)
    if (count == 0).any():
        b = int(np.argmax(count == 0))
        raise ValueError(f"slab_bins: bin {b} ([{edges[b]:.6g}, {edges[b + 1]:.6g}) along axis {axis}) holds no cell")
    return bins.astype(np.int64), edges


def bin_chunk_plan(bins_mesh, local_cells, n_cells, n_bins, who):
    """The atomic-free plan of a sum over the cells of every bin, built on the device (shared by ``ProfileStatistics``
    and ``DynamicSmagorinsky``): ``order`` (the sampled cells, kernel numbering, stably sorted by bin), the chunk table
    ``{first entry, cells, bin, consecutive}`` of at most 256 entries each, none crossing a bin, and ``bin_chunk_ptr``.
    ``bins_mesh``: the bin of every cell in the MESH's cell order (-1: left out), ``local_cells``: the mesh cell of every
    kernel cell."""
    dev = bins_mesh.device
    if int(local_cells.shape[0]) != n_cells or int(local_cells.max()) >= int(bins_mesh.shape[0]):
        raise RuntimeError(f"{who}: the solver's cell order does not match its mesh")
    bk = bins_mesh[local_cells]  # bins in the kernel's cell order
    sel = torch.nonzero(bk >= 0).reshape(-1)
    order = sel[torch.sort(bk[sel], stable=True).indices]
    nb = n_bins
    count = torch.bincount(bk[sel], minlength=nb)
    nch = (count + 255) // 256
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    ptr = torch.cat([zero, torch.cumsum(nch, 0)])
    start = torch.cat([zero, torch.cumsum(count, 0)])
    cbin = torch.repeat_interleave(torch.arange(nb, device=dev), nch)
    off = start[cbin] + 256 * (torch.arange(int(ptr[-1]), device=dev) - ptr[cbin])
    length = torch.minimum(start[cbin + 1] - off, torch.full_like(off, 256))
    # breaks[i]: entries j <= i of order that do not continue their predecessor
    brk = torch.cat([zero, torch.cumsum((order[1:] - order[:-1] != 1).to(torch.int64), 0)])
    consecutive = (brk[off + length - 1] - brk[off]) == 0
    chunks = torch.stack([off, length, cbin, consecutive.to(torch.int64)], dim=1).to(torch.int32).contiguous()
    n_sampled = int(order.shape[0])
    lmin, lmax, lsum = torch.stack([length.min(), length.max(), length.sum()]).tolist()
    if not (1 <= lmin and lmax <= 256 and lsum == n_sampled):  # (the kernel's lanes index order by these)
        raise RuntimeError(f"{who}: chunks of {lmin} .. {lmax} cells covering {lsum} of {n_sampled}")
    return {"order": order.to(torch.int32).contiguous(), "chunks": chunks,
            "bin_chunk_ptr": ptr.to(torch.int32).contiguous(), "n_chunks": int(chunks.shape[0]), "n_sampled": n_sampled,
            "bins_kernel": bk}


def _tri_index(n, i, j):
    """Position of (i, j), i <= j, in the upper triangle of an n x n matrix stored row by row."""
    return i * n - i * (i - 1) // 2 + j - i


class _ProfileGroup:
    """One joint vector of ProfileStatistics: its members (name, first component, components), the dof table it is read
    through, its sources (storage, first column; leading dimension from the storage) and its running moments."""

    def __init__(self, members, degree, cell_dofs, sources, n_bins, dev, second=True):
        self.members, self.degree, self.cell_dofs, self.sources = members, int(degree), cell_dofs, sources
        self.nq = sum(m[2] for m in members)
        self.nv = self.nq * (self.nq + 1) // 2
        self.mean = torch.zeros((n_bins, self.nq), dtype=torch.float64, device=dev)
        self.m2 = torch.zeros((n_bins, self.nv), dtype=torch.float64, device=dev) if second else None  # (slab_mean: none)


class ProfileStatistics:
    """Running weighted mean and covariance of a ``FractionalStep_AB_CN``'s fields averaged over slabs of cells and time.

    For bin ``b`` with cells ``C_b``, ``V_b = sum |c|`` and samples of weight ``w_k``, ``W = sum w_k``::

        mean_b = sum_k w_k int_b q / (W V_b)        cov_b = sum_k w_k int_b (q - mean_b) (q - mean_b)^T / (W V_b)

    with the integrals of the discrete fields taken exactly (the element's mass matrix), not as nodal means.

    Args:
        solver: the solver (one GPU)
        axis, edges, tol: the bins are ``slab_bins(mesh, axis, edges, tol)`` -- or
        cell_bins: an int array in the MESH's cell order (-1: the cell is left out; ``n_bins = max + 1``); exactly one of
            ``axis`` and ``cell_bins`` is given
        fields: out of ``"u"`` and ``"p"``
        scalars: names of the solver's ``ScalarTransport`` fields (at most two).  With ``"u"`` they form ONE joint vector
            ``q = (u_0 .. u_{d-1}, c_1 ..)``, so the scalar fluxes ``<u_i' c'>`` come with the Reynolds stresses; without
            ``"u"`` each scalar stands alone.  ``"p"`` is a one-component group of its own.
    """

    def __init__(self, solver, axis=None, edges=None, cell_bins=None, fields=("u", "p"), scalars=(), tol=None):
        _one_gpu(solver, "ProfileStatistics", "the sums over the cells of a bin")
        if (axis is None) == (cell_bins is None):
            raise ValueError("ProfileStatistics: give exactly one of axis= (with optional edges=) and cell_bins=")
        if cell_bins is not None and edges is not None:
            raise ValueError("ProfileStatistics: edges= belongs to axis=, not to cell_bins=")
        fields = (fields,) if isinstance(fields, str) else tuple(fields)
        scalars = (scalars,) if isinstance(scalars, str) else tuple(scalars)
        for f in fields:
            if f not in ("u", "p"):
                raise ValueError(f"ProfileStatistics: unknown field {f!r} (known: 'u', 'p'; scalars go into scalars=)")
        if len(scalars) > 2:
            raise ValueError(f"ProfileStatistics: {len(scalars)} scalars (the joint vector takes at most two)")
        if len(set(fields)) != len(fields) or len(set(scalars)) != len(scalars) or set(fields) & set(scalars):
            raise ValueError("ProfileStatistics: a field is listed twice")
        mesh = solver._mesh
        self._solver = solver
        self.axis = None if axis is None else int(axis)
        if cell_bins is None:
            bins, e = slab_bins(mesh, axis, edges, tol)
            self.edges = e
        else:
            bins = np.asarray(cell_bins.cpu().numpy() if torch.is_tensor(cell_bins) else cell_bins)
            if bins.shape != (int(mesh.num_cells),) or not np.issubdtype(bins.dtype, np.integer):
                raise ValueError(f"ProfileStatistics: cell_bins must be {int(mesh.num_cells)} integers in the mesh's cell order")
            bins = bins.astype(np.int64)
            if bins.min() < -1 or bins.max() < 0:
                raise ValueError("ProfileStatistics: cell_bins holds values below -1, or no cell is sampled")
            self.edges = None
        self._bins = bins
        self.n_bins = nb = int(bins.max()) + 1
        count = np.bincount(bins[bins >= 0], minlength=nb)
        if (count == 0).any():
            raise ValueError(f"ProfileStatistics: bin {int(np.argmax(count == 0))} holds no cell")
        Vi, Q = solver._Vi[0][0], solver._Q
        self._Vi, self._Q = Vi, Q
        self.gdim = d = int(mesh.gdim)
        dev = solver._geom.device
        self._build_chunks(torch.from_numpy(bins).to(dev), Vi.local_cells.to(torch.int64).to(dev), int(solver._geom.shape[0]))
        # rows a field must have to be read through each dof table (read back once, here: slab_mean checks against it)
        self._rows = {id(V): (int(V.cell_dofs.max()) + 1 if V.cell_dofs.numel() else 0) for V in (Vi, Q)}
        # the groups
        self._groups, self._where = [], {}
        joint, src = [], []
        if "u" in fields:
            joint.append(("u", 0, d))
            src.append((solver._U, 0))
        cs = []
        for s in scalars:
            try:
                c = solver.scalar(s)
            except KeyError as exc:
                raise ValueError(f"ProfileStatistics: {exc.args[0]}") from None
            if not _same_layout(c.function_space, Vi):
                raise ValueError(f"ProfileStatistics: scalar {s!r} does not live on the velocity's element")
            cs.append((s, c))
        if joint:
            for s, c in cs:
                joint.append((s, sum(m[2] for m in joint), 1))
                src.append((c._storage, int(c._comp)))
            self._add_group(joint, Vi, src, dev)
        else:
            for s, c in cs:
                self._add_group([(s, 0, 1)], Vi, [(c._storage, int(c._comp))], dev)
        if "p" in fields:
            self._add_group([("p", 0, 1)], Q, [(solver._P, 0)], dev)
        if not self._groups:
            raise ValueError("ProfileStatistics: no field to average (fields and scalars are both empty)")
        self._vol = torch.zeros(nb, dtype=torch.float64, device=dev)
        self._vol_scratch = torch.zeros_like(self._vol)  # (where slab_mean's launch pair writes V_b)
        nq = max([d] + [g.nq for g in self._groups])  # (slab_mean of a velocity takes d components whatever is averaged)
        self._partials = torch.zeros((self.n_chunks, 1 + nq + nq * (nq + 1) // 2), dtype=torch.float64, device=dev)
        self._W = 0.0
        self.n_samples = 0

    # ---- set-up ------------------------------------------------------------------------------------------------------
    def _build_chunks(self, bins_mesh, local_cells, n_cells):
        """The chunk plan of ``bin_chunk_plan`` as this object's tables."""
        plan = bin_chunk_plan(bins_mesh, local_cells, n_cells, self.n_bins, "ProfileStatistics")
        self._order, self._chunks, self._bin_chunk_ptr = plan["order"], plan["chunks"], plan["bin_chunk_ptr"]
        self.n_chunks, self.n_sampled = plan["n_chunks"], plan["n_sampled"]

    def _add_group(self, members, space, sources, dev):
        d = self.gdim
        nq = sum(m[2] for m in members)
        if not (nq == 1 or d <= nq <= d + 2):
            raise NotImplementedError(f"ProfileStatistics: a joint vector of {nq} components on a {d}-D mesh")
        for st, col in sources:
            if st.n_alloc < self._rows[id(space)]:
                raise RuntimeError(f"ProfileStatistics: a field of {st.n_alloc} rows on a space of {self._rows[id(space)]} dofs")
        g = _ProfileGroup(members, space.degree, space.cell_dofs, sources, self.n_bins, dev)
        for name, c0, nc in members:
            self._where[name] = (g, c0, nc)
        self._groups.append(g)

    # ---- sampling ----------------------------------------------------------------------------------------------------
    @staticmethod
    def _source_args(sources):
        """(addresses, leading dimensions) of the sources ``(storage, first column)`` as the kernel gets them: a column
        inside a block is the block's address plus 8 bytes per column, read with the block's width as its stride."""
        devs = [s.rdev() for s, _ in sources]
        return [t.data_ptr() + 8 * col for t, (_, col) in zip(devs, sources)], [int(t.shape[1]) for t in devs]

    def _cells(self, g, sources, shift):
        """ox_profile_cells of one group: the chunk partial rows about ``shift`` (None: 0)."""
        lib, st = _lib.load(), _lib.current_stream()
        n = len(sources)
        addr, lds = self._source_args(sources)
        src, ld = (C.c_void_p * n)(*addr), (C.c_int64 * n)(*lds)
        _lib.check(lib.ox_profile_cells(g.degree, C.byref(self._solver._cells), _lib.ptr(g.cell_dofs), g.nq, n, src, ld,
                                        _lib.ptr(self._order), _lib.ptr(self._chunks), self.n_chunks, _lib.ptr(shift),
                                        _lib.ptr(self._partials), st), "ox_profile_cells")

    def _update(self, g, shift, w, W_old, seed, mean, m2, vol, sums=None):
        """ox_profile_update of one group: the partial rows summed per bin, then the merge (or the seed)."""
        _lib.check(_lib.load().ox_profile_update(g.nq, self.n_bins, _lib.ptr(self._bin_chunk_ptr), _lib.ptr(self._partials),
                                                 _lib.ptr(shift), w, W_old, int(seed), _lib.ptr(mean), _lib.ptr(m2),
                                                 _lib.ptr(vol), _lib.ptr(sums), _lib.current_stream()), "ox_profile_update")

    def _launch(self, g, sources, shift, w, W_old, seed, mean, m2, vol, sums=None):
        """The launch pair of one group."""
        self._cells(g, sources, shift)
        self._update(g, shift, w, W_old, seed, mean, m2, vol, sums)

    def sample(self, dt: float) -> None:
        """Add the solver's current fields with weight ``dt > 0``: two launches per group on the current stream, taken
        about the running mean; no host synchronisation.  The first sample runs the pair twice (seed, then accumulate), so
        a mean far larger than the fluctuations never meets a raw second moment."""
        w = float(dt)
        if not (w > 0.0 and np.isfinite(w)):
            raise ValueError(f"ProfileStatistics.sample: dt = {w} (a sample needs a weight > 0)")
        for g in self._groups:
            if self._W == 0.0:
                g.m2.zero_()
                self._launch(g, g.sources, None, 0.0, 0.0, True, g.mean, None, self._vol)
            self._launch(g, g.sources, g.mean, w, self._W, False, g.mean, g.m2, self._vol)
        self._W += w
        self.n_samples += 1

    def slab_mean(self, function) -> torch.Tensor:
        """One-shot slab means ``(n_bins, ncomp)`` of a ``Function`` on the velocity component space, the blocked
        velocity space or the pressure space (e.g. ``FlowStatistics.mean("u")``); the running state is untouched."""
        V = function.function_space
        blocked = isinstance(V, VectorFunctionSpace)
        Vs = V.scalar if blocked else V
        space = self._Vi if _same_layout(Vs, self._Vi) else (self._Q if _same_layout(Vs, self._Q) else None)
        if space is None:
            raise ValueError("ProfileStatistics.slab_mean: the function lives on neither the velocity nor the pressure space")
        st = function._storage
        nc = st.nc if function._comp is None else 1
        if nc not in (1, self.gdim):
            raise ValueError(f"ProfileStatistics.slab_mean: a function of {nc} components")
        if st.n_alloc < self._rows[id(space)]:
            raise RuntimeError("ProfileStatistics.slab_mean: the function has fewer rows than its space has dofs")
        g = _ProfileGroup([("f", 0, nc)], space.degree, space.cell_dofs, [(st, int(function._comp or 0))], self.n_bins,
                          self._vol.device, second=False)
        self._launch(g, g.sources, None, 0.0, 0.0, True, g.mean, None, self._vol_scratch)
        return g.mean

    # ---- results -----------------------------------------------------------------------------------------------------
    @property
    def names(self):
        return tuple(self._where)

    @property
    def total_weight(self) -> float:
        return self._W

    def _get(self, name):
        if name not in self._where:
            raise ValueError(f"ProfileStatistics: no statistics of {name!r} (have: {', '.join(self._where)})")
        return self._where[name]

    def _need_weight(self):
        if not self._W > 0.0:
            raise RuntimeError("ProfileStatistics: no sample has been taken since the statistics were reset")

    def coordinates(self):
        """The bin centres along ``axis`` (host), ``None`` with ``cell_bins``."""
        return None if self.edges is None else 0.5 * (self.edges[:-1] + self.edges[1:])

    def volume(self) -> torch.Tensor:
        """``V_b``, ``(n_bins,)`` on the device, as the latest sample summed it."""
        self._need_weight()
        return self._vol

    def mean(self, name: str) -> torch.Tensor:
        """``(n_bins, ncomp)`` on the device (a view of the running state)."""
        self._need_weight()
        g, c0, nc = self._get(name)
        return g.mean[:, c0:c0 + nc]

    def joint_covariance(self, name: str = "u") -> torch.Tensor:
        """``M2 / W`` of the whole group ``name`` belongs to: ``(n_bins, nq (nq + 1) / 2)``, upper triangle row by row."""
        self._need_weight()
        return self._get(name)[0].m2 / self._W

    def covariance(self, name: str) -> torch.Tensor:
        """``(n_bins, k (k + 1) / 2)``: the upper triangle of the field's own block, row by row (``00, 01, 02, 11, 12,
        22`` for ``"u"`` in 3-D: the Reynolds stresses)."""
        g, c0, nc = self._get(name)
        idx = [_tri_index(g.nq, c0 + i, c0 + j) for i in range(nc) for j in range(i, nc)]
        return self.joint_covariance(name)[:, idx]

    def variance(self, name: str) -> torch.Tensor:
        g, c0, nc = self._get(name)
        if nc != 1:
            raise ValueError(f"ProfileStatistics.variance: {name!r} has {nc} components (covariance() has them all)")
        return self.covariance(name)[:, 0]

    def tke(self) -> torch.Tensor:
        """Turbulent kinetic energy ``1/2 tr <u' u'>`` per bin, ``(n_bins,)``."""
        g, c0, nc = self._get("u")
        cov = self.joint_covariance("u")
        acc = cov[:, _tri_index(g.nq, c0, c0)].clone()
        for i in range(1, nc):
            acc += cov[:, _tri_index(g.nq, c0 + i, c0 + i)]
        return 0.5 * acc

    def flux(self, scalar: str) -> torch.Tensor:
        """The turbulent scalar flux ``<u_i' c'>``, ``(n_bins, d)``."""
        g, c0, nc = self._get(scalar)
        if "u" not in self._where or self._where["u"][0] is not g or scalar == "u":
            raise ValueError(f"ProfileStatistics.flux: {scalar!r} is not a scalar averaged jointly with 'u'")
        return self.joint_covariance("u")[:, [_tri_index(g.nq, i, c0) for i in range(self.gdim)]]

    def reset(self) -> None:
        for g in self._groups:
            g.mean.zero_()
            g.m2.zero_()
        self._vol.zero_()
        self._W = 0.0
        self.n_samples = 0

    def save(self, path) -> None:
        out = dict(total_weight=np.float64(self._W), n_samples=np.int64(self.n_samples), cell_bins=self._bins,
                   fields=np.array([n for n in self._where if n in ("u", "p")], dtype=str),
                   scalars=np.array([n for n in self._where if n not in ("u", "p")], dtype=str),
                   axis=np.int64(-1 if self.axis is None else self.axis), volume=self._vol.cpu().numpy())
        if self.edges is not None:
            out["edges"] = self.edges
        for k, g in enumerate(self._groups):
            out[f"mean_{k}"] = g.mean.cpu().numpy()
            out[f"m2_{k}"] = g.m2.cpu().numpy()
        np.savez(path, **out)

    @classmethod
    def load(cls, solver, path) -> "ProfileStatistics":
        """The statistics ``save`` wrote, bound to ``solver`` (the same mesh, spaces and scalars): averaging goes on
        after a restart, bit for bit."""
        with np.load(path) as z:
            obj = cls(solver, cell_bins=z["cell_bins"], fields=[str(s) for s in z["fields"]],
                      scalars=[str(s) for s in z["scalars"]])
            obj.axis = None if int(z["axis"]) < 0 else int(z["axis"])
            obj.edges = z["edges"].copy() if "edges" in z.files else None
            dev = obj._vol.device
            for k, g in enumerate(obj._groups):
                mean, m2 = z[f"mean_{k}"], z[f"m2_{k}"]
                if mean.shape != tuple(g.mean.shape) or m2.shape != tuple(g.m2.shape):
                    raise ValueError(f"ProfileStatistics.load: group {k} was saved with shapes {mean.shape}, {m2.shape}; this "
                                     f"object has {tuple(g.mean.shape)}, {tuple(g.m2.shape)}")
                g.mean.copy_(torch.from_numpy(np.ascontiguousarray(mean)).to(dev))
                g.m2.copy_(torch.from_numpy(np.ascontiguousarray(m2)).to(dev))
            obj._vol.copy_(torch.from_numpy(np.ascontiguousarray(z["volume"])).to(dev))
            obj._W = float(z["total_weight"])
            obj.n_samples = int(z["n_samples"])
        return obj
