"""Point location and evaluation, shaped after ``dolfinx.geometry``: ``bb_tree``, ``compute_collisions_points``,
``compute_colliding_cells``; and :class:`Probes`, a set of points sampled into a device-resident ring every time step.

The work is done by the library (csrc/ox_probe.hip): a uniform-grid locator over the straight simplices of the mesh
(``ox_locator_*``) and the evaluation of P1 / P2 / P3 fields at located points (``ox_eval_points`` /
``ox_probe_sample``).  There is no CPU path.

**Deviation from DOLFINx.**  Every point has zero or one link: the LOWEST cell id among the cells that contain it (all
barycentric coordinates >= -tol), where DOLFINx lists every colliding cell; a script that takes ``links(i)[0]`` behaves
the same.  The answer is the same on every run, for points on shared faces, edges and vertices too.

**Mesh partitions.**  Every rank holds the whole mesh and the same partition maps, so the owner of a point is decided
without communication: the rank locates among the cells of its window (``MeshPartition.win_cells``), takes the lowest
cell id c* that contains the point, and the owner is the rank that owns c*'s first vertex.  That rank has c* among its
local cells (c* touches a dof it owns) and sees every cell that shares a vertex with c* inside its two-ring window, so it
finds the same c*; every other rank that finds c* computes the same owner and drops the point.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .fem import DGSpace, Function, FunctionSpace, HighOrderLagrangeSpace, VectorFunctionSpace
from .native import _Handle

__all__ = ["bb_tree", "compute_collisions_points", "compute_colliding_cells", "AdjacencyList", "BoundingBoxTree",
           "Probes", "WallDistance", "DEFAULT_TOL"]

DEFAULT_TOL = 1e-10  # on the (dimensionless) barycentric coordinates


class AdjacencyList:
    """``dolfinx.graph.AdjacencyList``: ``links(i)``, ``array``, ``offsets``.  Here every node has zero or one link."""

    def __init__(self, array: np.ndarray, offsets: np.ndarray):
        self.array = np.asarray(array, dtype=np.int32)
        self.offsets = np.asarray(offsets, dtype=np.int32)
        self.num_nodes = int(self.offsets.shape[0]) - 1

    def links(self, i: int) -> np.ndarray:
        return self.array[self.offsets[i]:self.offsets[i + 1]]

    @classmethod
    def from_cells(cls, cells: torch.Tensor):
        """One node per entry of ``cells`` (a cell id, or -1 for no link)."""
        c = cells.cpu().numpy()
        hit = c >= 0
        return cls(c[hit], np.concatenate([[0], np.cumsum(hit)]))


def as_points(x, gdim: int, device) -> torch.Tensor:
    """(n, gdim) float64 tensor on ``device`` of points given as (n, 3) or (n, gdim) (or one point), numpy or torch."""
    if torch.is_tensor(x):
        t = x.to(device=device, dtype=torch.float64)
    else:
        a = np.asarray(x, dtype=np.float64)
        t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    if t.ndim == 1:
        t = t.reshape(1, -1)
    if t.ndim != 2 or int(t.shape[1]) not in (gdim, 3):
        raise ValueError(f"points must have shape (n, 3) or (n, {gdim}), got {tuple(t.shape)}")
    return t[:, :gdim].contiguous()


class BoundingBoxTree:
    """The locator of a mesh (all cells, or ``entities`` only): what ``bb_tree`` returns.  Owns the library object."""

    def __init__(self, mesh, entities=None, padding: float = 0.0, tol: float = DEFAULT_TOL):
        if not (0.0 <= float(tol) <= 1e-2):
            raise ValueError(f"tol = {tol}: a tolerance on barycentric coordinates, 0 <= tol <= 1e-2")
        if not float(padding) >= 0.0:
            raise ValueError(f"padding = {padding}")
        self.mesh, self.tol, self.padding = mesh, float(tol), float(padding)
        ids = None
        if entities is not None:
            ids = torch.as_tensor(entities).to(device=mesh.device, dtype=torch.int64).reshape(-1)
            if ids.numel() == 0:
                raise ValueError("bb_tree: empty list of entities")
            ids = torch.unique(ids)  # ascending: list order = cell id order
            if int(ids[0]) < 0 or int(ids[-1]) >= mesh.num_cells:
                raise ValueError("bb_tree: entities are cell ids of the mesh")
        self.entities = ids
        self.num_cells = mesh.num_cells if ids is None else int(ids.shape[0])
        if mesh.device.type != "cuda":
            raise _lib.OasisxHipError("bb_tree: the locator runs on the GPU (a mesh on a CUDA/HIP device); oasisx_amd has "
                                      "no CPU fallback")
        lib = _lib.load()
        h = C.c_void_p()
        _lib.check(lib.ox_locator_create(mesh.gdim, _lib.ptr(mesh.coords), mesh.num_vertices, _lib.ptr(mesh.cells),
                                         mesh.num_cells, _lib.ptr(ids), 0 if ids is None else int(ids.shape[0]),
                                         self.tol, self.padding, _lib.current_stream(), C.byref(h)), "ox_locator_create")
        # (destroyed in the creating process only: a forked child has no GPU context -- native._Handle)
        self._owner = _Handle(h, lib.ox_locator_destroy)
        self._h = h

    def info(self) -> dict:
        n, nb, nl = C.c_int64(), C.c_int64(), C.c_int64()
        per = (C.c_int * 3)()
        _lib.check(_lib.load().ox_locator_info(self._h, C.byref(n), C.byref(nb), C.byref(nl), per), "ox_locator_info")
        return {"cells": n.value, "bins": nb.value, "list": nl.value, "bins_per_axis": list(per)[: self.mesh.gdim]}

    def find(self, x, tol: float | None = None):
        """(cells, bary): per point the lowest containing mesh cell id (-1: none), int64 (n,), and its barycentric
        coordinates (n, gdim + 1), both on the device."""
        X = as_points(x, self.mesh.gdim, self.mesh.device)
        n = int(X.shape[0])
        cells = torch.empty(n, dtype=torch.int64, device=X.device)
        bary = torch.empty((n, self.mesh.gdim + 1), dtype=torch.float64, device=X.device)
        _lib.check(_lib.load().ox_locator_find(self._h, n, _lib.ptr(X), self.tol if tol is None else float(tol),
                                               _lib.ptr(cells), _lib.ptr(bary), _lib.current_stream()), "ox_locator_find")
        return cells, bary

    def bary(self, x, cells) -> torch.Tensor:
        """Barycentric coordinates (n, gdim + 1) of the points in the GIVEN mesh cells (NaN rows for -1)."""
        X = as_points(x, self.mesh.gdim, self.mesh.device)
        cd = torch.as_tensor(cells).to(device=X.device, dtype=torch.int64).reshape(-1).contiguous()
        if cd.shape[0] != X.shape[0]:
            raise ValueError(f"{int(X.shape[0])} points, {int(cd.shape[0])} cells")
        bary = torch.empty((int(X.shape[0]), self.mesh.gdim + 1), dtype=torch.float64, device=X.device)
        _lib.check(_lib.load().ox_locator_bary(self._h, int(X.shape[0]), _lib.ptr(X), _lib.ptr(cd), _lib.ptr(bary),
                                               _lib.current_stream()), "ox_locator_bary")
        return bary


def bb_tree(mesh, dim: int, entities=None, padding: float = 0.0, tol: float = DEFAULT_TOL) -> BoundingBoxTree:
    """``dolfinx.geometry.bb_tree``: the locator over the cells of ``mesh`` (``dim`` = the topological dimension only)."""
    if int(dim) != mesh.gdim:
        raise NotImplementedError(f"bb_tree: dim = {dim}; only trees of cells (dim = {mesh.gdim}) are built")
    return BoundingBoxTree(mesh, entities, padding, tol)


def compute_collisions_points(tree: BoundingBoxTree, x) -> AdjacencyList:
    """Per point the lowest cell id that contains it (zero or one link; see the module's note on DOLFINx)."""
    if not isinstance(tree, BoundingBoxTree):
        raise TypeError("compute_collisions_points: a tree from bb_tree")
    return AdjacencyList.from_cells(tree.find(x)[0])


def compute_colliding_cells(mesh, candidates: AdjacencyList, x) -> AdjacencyList:
    """``dolfinx.geometry.compute_colliding_cells``.  The candidates of ``compute_collisions_points`` are exact already
    (the locator tests the cells, not their boxes): they are returned as they are, after checking the shapes."""
    if not isinstance(candidates, AdjacencyList):
        raise TypeError("compute_colliding_cells: candidates from compute_collisions_points")
    n = int(as_points(x, mesh.gdim, x.device if torch.is_tensor(x) else "cpu").shape[0])
    if n != candidates.num_nodes:
        raise ValueError(f"compute_colliding_cells: {n} points, candidates for {candidates.num_nodes}")
    return candidates


# ---- wall distance ----------------------------------------------------------------------------------------------------
class WallDistance:
    """Distance to the nearest wall facet and that facet, for any point, on the device (``ox_walldist_*``,
    csrc/ox_probe.hip).

    Args:
        mesh: one GPU (``comm.size > 1`` raises ``NotImplementedError``)
        facets: ``None``: all exterior facets (on a ``make_periodic`` mesh without the identified faces);
            ``(meshtags, id)`` / ``(meshtags, (id, ...))``: the facets of those values; an array of facet ids.  An empty
            selection raises ``ValueError``.  Order: by tag, then by facet id (``wall.select_facets``) -- ``.facets``
        bins: bins per axis of the background grid instead of the computed ones; ``(1, 1, 1)`` searches every facet

    The distance is to the closest point of the facet (a segment or a triangle), not to its plane.  On a periodic mesh every
    query is the minimum over the images ``x + s * period``, ``s in {-1, 0, 1}`` per periodic axis.
    """

    def __init__(self, mesh, facets=None, bins=None, _selection=None):
        from .wall import select_facets

        comm = getattr(mesh, "comm", None)
        if comm is not None and getattr(comm, "size", 1) > 1:
            raise NotImplementedError("WallDistance on a mesh partition (comm.size > 1): the search is built for one GPU")
        d = mesh.gdim
        # (_selection: facet ids a caller has ordered by select_facets already -- VanDriest shares them with its FacetSet)
        ids = select_facets(mesh, facets, "WallDistance")[0] if _selection is None else np.asarray(_selection, dtype=np.int64)
        if ids.shape[0] == 0:
            raise ValueError("WallDistance: the selection holds no facet")
        fv, _ = mesh._entities(d - 1)
        if ids.min() < 0 or ids.max() >= fv.shape[0]:
            raise ValueError("WallDistance: facet ids are indices of the mesh's facets")
        b3 = None
        if bins is not None:
            b = [int(v) for v in np.atleast_1d(bins)]
            if len(b) not in (d, 3) or min(b) < 1 or max(b) > 1024:
                raise ValueError(f"WallDistance: bins = {bins!r}: {d} counts in 1..1024")
            b3 = (C.c_int * 3)(*(b[:d] + [1] * (3 - d)))
        self.mesh, self.gdim = mesh, d
        self.facets, self.n_facets = ids, int(ids.shape[0])
        per = getattr(mesh, "periodic", None)
        self._shifts = [None]
        if per is not None:
            import itertools

            period = np.asarray(per.period, dtype=np.float64).reshape(-1)
            self._shifts = []
            for s in itertools.product((0, -1, 1), repeat=len(per.axes)):  # (the unshifted search first)
                v = np.zeros(3)
                for k, sk in zip(per.axes, s):
                    v[k] = sk * period[k]
                self._shifts.append(v if any(s) else None)
        if mesh.device.type != "cuda":
            raise _lib.OasisxHipError("WallDistance: the search runs on the GPU (a mesh on a CUDA/HIP device); oasisx_amd "
                                      "has no CPU fallback")
        lib = _lib.load()
        xyz = mesh.coords[torch.from_numpy(fv[ids].astype(np.int64)).to(mesh.device)].to(torch.float64).contiguous()
        h = C.c_void_p()
        _lib.check(lib.ox_walldist_create(d, _lib.ptr(xyz), self.n_facets, b3, _lib.current_stream(), C.byref(h)),
                   "ox_walldist_create")
        self._owner = _Handle(h, lib.ox_walldist_destroy)
        self._h = h

    def info(self) -> dict:
        n, nb, nl = C.c_int64(), C.c_int64(), C.c_int64()
        per = (C.c_int * 3)()
        _lib.check(_lib.load().ox_walldist_info(self._h, C.byref(n), C.byref(nb), C.byref(nl), per), "ox_walldist_info")
        return {"facets": n.value, "bins": nb.value, "list": nl.value, "bins_per_axis": list(per)[: self.gdim]}

    def query(self, x):
        """(dist, nearest): per point the distance to the nearest wall facet, float64 (n,), and that facet's position in
        ``.facets``, int32 (n,) -- the lowest among facets at the same distance; both on the device.  A non-finite point:
        NaN and -1."""
        X = as_points(x, self.gdim, self.mesh.device)
        n = int(X.shape[0])
        dist = torch.empty(n, dtype=torch.float64, device=X.device)
        near = torch.empty(n, dtype=torch.int32, device=X.device)
        if n == 0:
            return dist, near
        lib, st = _lib.load(), _lib.current_stream()
        for k, s in enumerate(self._shifts):
            sh = None if s is None else (C.c_double * 3)(*s)
            _lib.check(lib.ox_walldist_query(self._h, n, _lib.ptr(X), sh, int(k > 0), _lib.ptr(dist), _lib.ptr(near), st),
                       "ox_walldist_query")
        return dist, near

    def cells(self):
        """(dist, nearest) at the cell centroids, in the mesh's cell order."""
        m = self.mesh
        return self.query(m.coords[m.cells.to(torch.int64)].mean(dim=1))

    def function(self, V) -> Function:
        """A ``Function`` on the scalar Lagrange space ``V`` holding the distance at ``V``'s dof coordinates."""
        Vs = scalar_space(V)
        if Vs is not V:
            raise TypeError("WallDistance.function: a scalar FunctionSpace")
        f = Function(V, name="wall_distance")
        dist, _ = self.query(V.x)
        f._storage.dev()[: int(dist.shape[0]), 0].copy_(dist)  # (device to device: nothing is read back)
        return f


# ---- spaces -----------------------------------------------------------------------------------------------------------
def scalar_space(V) -> FunctionSpace:
    """The scalar Lagrange space whose ``cell_dofs`` evaluate a field on ``V``; raises for spaces without a device path."""
    if isinstance(V, DGSpace):
        raise NotImplementedError("point evaluation of a discontinuous (DGSpace) field is not implemented")
    if isinstance(V, HighOrderLagrangeSpace):
        raise NotImplementedError("point evaluation on a HighOrderLagrangeSpace (equispaced, degree >= 3, boundary "
                                  "conditions only) is not implemented; FunctionSpace covers degree 1 to 3")
    Vs = V.scalar if isinstance(V, VectorFunctionSpace) else V
    if not isinstance(Vs, FunctionSpace):
        raise TypeError(f"point evaluation: a FunctionSpace or VectorFunctionSpace, not {type(V).__name__}")
    return Vs


def space_tree(Vs: FunctionSpace, tol: float = DEFAULT_TOL) -> BoundingBoxTree:
    """The locator a space evaluates through, cached on the mesh: all cells on one GPU, the cells of the rank's window
    on a mesh partition (the module's ownership rule needs the window, not just the local cells)."""
    part = Vs.part
    holder = Vs.mesh if part is None else part
    cache = holder.__dict__.setdefault("_probe_trees", {})
    tree = cache.get(float(tol))
    if tree is None:
        tree = BoundingBoxTree(Vs.mesh, None if part is None else part.win_cells, 0.0, tol)
        cache[float(tol)] = tree
    return tree


def kernel_position_table(Vs: FunctionSpace) -> torch.Tensor:
    """(num_cells,) device int64: mesh cell id -> position in the space's kernel cell order (-2: a cell the rank does not
    hold); built once per space."""
    inv = getattr(Vs, "_probe_cell_inv", None)
    if inv is None:
        inv = torch.full((Vs.mesh.num_cells,), -2, dtype=torch.int64, device=Vs.mesh.device)
        lc = Vs.local_cells.to(torch.int64)
        inv[lc] = torch.arange(int(lc.shape[0]), dtype=torch.int64, device=inv.device)
        Vs._probe_cell_inv = inv
    return inv


def kernel_positions(Vs: FunctionSpace, cells: torch.Tensor) -> torch.Tensor:
    """Position in the space's kernel cell order of mesh cell ids (device int64; -1 stays -1, a cell the rank does not
    hold gives -2)."""
    inv = kernel_position_table(Vs)
    ok = cells >= 0
    return torch.where(ok, inv[cells.clamp(0, Vs.mesh.num_cells - 1)], torch.full_like(cells, -1))


def owned_points(Vs: FunctionSpace, cells: torch.Tensor) -> torch.Tensor:
    """Mask of the located points this rank evaluates: all of them on one GPU; on a partition those whose cell's first
    vertex the rank owns."""
    ok = cells >= 0
    if Vs.part is None:
        return ok
    first = Vs.mesh.cells[cells.clamp_min(0), 0]
    return ok & (Vs.part.vown[first] == Vs.part.rank)


class PointPlan:
    """Located points prepared for one scalar space: kernel-cell positions and barycentric coordinates SORTED by cell
    position, and the permutation back to the caller's order -- what ``ox_eval_points`` / ``ox_probe_sample`` take."""

    def __init__(self, Vs: FunctionSpace, cells: torch.Tensor, bary: torch.Tensor):
        pos = kernel_positions(Vs, cells)
        if bool((pos == -2).any()):
            bad = cells[pos == -2][:8].tolist()
            raise ValueError(f"point evaluation: cells {bad} are not among the cells this rank holds (V.local_cells)")
        self.Vs, self.n = Vs, int(pos.shape[0])
        self.perm = torch.argsort(pos, stable=True)
        self.pos = pos[self.perm].contiguous()
        self.bary = bary[self.perm].contiguous()

    def args(self):
        Vs = self.Vs
        return (Vs.degree, Vs.mesh.gdim, _lib.ptr(Vs.cell_dofs), int(Vs.cell_dofs.shape[0]), int(Vs.n_local), self.n,
                _lib.ptr(self.pos), _lib.ptr(self.bary), _lib.ptr(self.perm))


def field_args(f: Function):
    """(read-only pointer, columns of the block, column or -1, number of values) of a Function's storage."""
    s = f._storage
    if f._comp is None:
        return s.rptr(), s.nc, -1, s.nc
    return s.rptr(), s.nc, int(f._comp), 1


def eval_function(f: Function, x, cells=None, tol: float = DEFAULT_TOL) -> torch.Tensor:
    """Values (n, value_size) of ``f`` at the points, on the device.  ``cells``: the mesh cell of every point (-1: NaN
    row); None: located first (on a mesh partition points of other ranks give NaN rows)."""
    Vs = scalar_space(f.function_space)
    X = as_points(x, Vs.mesh.gdim, Vs.mesh.device)
    cd = None
    if cells is not None:
        cd = torch.as_tensor(np.asarray(cells) if not torch.is_tensor(cells) else cells).to(
            device=X.device, dtype=torch.int64).reshape(-1)
        if cd.shape[0] != X.shape[0]:
            raise ValueError(f"eval: {int(X.shape[0])} points, {int(cd.shape[0])} cells")
        if bool((cd >= Vs.mesh.num_cells).any()) or bool((cd < -1).any()):
            raise ValueError("eval: cells are cell ids of the mesh (or -1)")
    tree = space_tree(Vs, tol)
    if cd is None:
        cd, bary = tree.find(X)
        cd = torch.where(owned_points(Vs, cd), cd, torch.full_like(cd, -1))
    else:
        bary = tree.bary(X, cd)
    plan = PointPlan(Vs, cd, bary)
    ptr, nc, col, nv = field_args(f)
    out = torch.empty((plan.n, nv), dtype=torch.float64, device=X.device)
    _lib.check(_lib.load().ox_eval_points(*plan.args(), ptr, nc, col, _lib.ptr(out), nv, 0, _lib.current_stream()),
               "ox_eval_points")
    return out


class Probes:
    """Points sampled every time step without leaving the device.

    ``Probes(points, functions)`` locates the points once and keeps cells, barycentric coordinates and the sort
    permutation on the device; ``sample(t)`` enqueues one ``ox_probe_sample`` per function on the current stream -- no
    host synchronisation, the fields are read through ``rptr()`` (sampling never counts as a write of ``u``) -- into slot
    k of a ring (capacity, n_local_points, n_values_total) that doubles when full.  ``array()`` brings the samples to
    the host.  On a mesh partition the object keeps the points this rank owns (``local_indices``); nothing is gathered
    across ranks.  A point no cell contains raises unless ``allow_missing`` (then its values are NaN); on a partition such
    a point cannot be told from another rank's without communication and is simply in no rank's ``local_indices``."""

    def __init__(self, points, functions, capacity: int = 64, tol: float = DEFAULT_TOL, allow_missing: bool = False):
        if isinstance(functions, Function):
            functions = [functions]
        functions = list(functions)
        if not functions or not all(isinstance(f, Function) for f in functions):
            raise TypeError("Probes: functions is a Function or a non-empty sequence of Functions")
        if int(capacity) < 1:
            raise ValueError(f"Probes: capacity = {capacity}")
        spaces = [scalar_space(f.function_space) for f in functions]
        mesh = spaces[0].mesh
        if any(V.mesh is not mesh for V in spaces):
            raise ValueError("Probes: every function must live on the same mesh")
        if any(V.part is not spaces[0].part for V in spaces):
            raise ValueError("Probes: every function must live on the same mesh partition")
        X = as_points(points, mesh.gdim, mesh.device)
        tree = space_tree(spaces[0], tol)
        cells, bary = tree.find(X)
        found = cells >= 0
        part = spaces[0].part
        # (on a partition a point outside the rank's window is another rank's point or outside the mesh: telling the two
        # apart needs the other ranks, so nothing is raised there; the union of local_indices says what was found)
        if part is None and not allow_missing and not bool(found.all()):
            bad = torch.nonzero(~found).reshape(-1)
            raise ValueError(f"Probes: {int(bad.shape[0])} point(s) lie in no cell of the mesh, the first at "
                             f"{X[bad[0]].tolist()} (allow_missing=True records NaN there)")
        keep = owned_points(spaces[0], cells) if part is not None else torch.ones_like(found)
        idx = torch.nonzero(keep).reshape(-1)
        self.functions = functions
        self.local_indices = idx.cpu().numpy()
        self.points = X[idx].cpu().numpy()
        self.cells = cells[idx].cpu().numpy()
        self.n_points = int(idx.shape[0])
        self.tol = float(tol)
        plans = {}
        self._jobs, off = [], 0
        for f, V in zip(functions, spaces):
            if id(V) not in plans:
                plans[id(V)] = PointPlan(V, cells[idx], bary[idx])
            nv = f._storage.nc if f._comp is None else 1
            self._jobs.append((f, plans[id(V)], off))
            off += nv
        self.n_values = off
        self.capacity = int(capacity)
        self._ring = torch.zeros((self.capacity, self.n_points, self.n_values), dtype=torch.float64, device=mesh.device)
        self._times = []

    @property
    def n_samples(self) -> int:
        return len(self._times)

    @property
    def times(self) -> np.ndarray:
        return np.asarray(self._times, dtype=np.float64)

    def sample(self, t: float = 0.0) -> None:
        k = len(self._times)
        if k == self.capacity:  # the ring doubles (a device copy on the current stream)
            ring = torch.zeros((2 * self.capacity,) + tuple(self._ring.shape[1:]), dtype=torch.float64, device=self._ring.device)
            ring[: self.capacity] = self._ring
            self._ring, self.capacity = ring, 2 * self.capacity
        lib, st = _lib.load(), _lib.current_stream()
        for f, plan, off in self._jobs:
            ptr, nc, col, _ = field_args(f)
            _lib.check(lib.ox_probe_sample(*plan.args(), ptr, nc, col, _lib.ptr(self._ring), self.capacity, k, self.n_values,
                                           off, st), "ox_probe_sample")
        self._times.append(float(t))

    def array(self) -> np.ndarray:
        """(n_samples, n_local_points, n_values_total) on the host."""
        return self._ring[: len(self._times)].cpu().numpy()

    def save(self, path) -> None:
        np.savez(path, values=self.array(), times=self.times, points=self.points, local_indices=self.local_indices,
                 cells=self.cells, names=np.asarray([f.name for f in self.functions]))
