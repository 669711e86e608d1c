"""Drag zones: the volume term ``-sigma(x, |u|) (u - u_t)`` of the momentum equation, on the device inside
``assemble_first`` (``csrc/ox_drag.hip``).

One term, three uses: porous media (Darcy-Forchheimer: stents, flow diverters, filters, canopies, screens), sponge or fringe
layers that pull the flow to a target field ``u_t`` in front of an outlet or behind an inlet, and solids by Brinkman
penalisation (an obstacle in a lattice mesh without meshing it; the force on it is a by-product).

For each cell c of a zone, with ``M_c`` its mass matrix on the velocity component space and ``x_c`` its centroid::

    sigma_c = darcy_c + forchheimer_c |u_ab(x_c) - u_t(x_c)|          (u_ab of this step)
    D       = sum_c sigma_c M_c
    A       <- A + theta D
    b_first <- b_first - (1 - theta) D u_1 + D u_t                     (per component)

``theta = drag_theta`` in [0.5, 1]; the default 1 is backward Euler: a penalised solid has ``sigma dt >> 1``, where
Crank-Nicolson rings.  The coefficient is isotropic (one ``A`` serves all components).  The projection keeps ``M``: inside a
stiff zone the end-of-step velocity differs from ``u_t`` by ``O(dt |grad dp|)``.

Three kernels: ``ox_drag_sigma`` (one lane per zone cell; skipped when every ``forchheimer`` is zero: ``sigma`` is then
written once), ``ox_drag_rows`` (one lane per row of the slices that touch a zone, one launch per width bin of the
pattern; the lane owns its row of ``A`` and of ``b_first``: no atomics, equal bits for equal inputs) and, for
``DragZone.sample``, ``ox_drag_force_cells`` with the per-tag sums of ``ox_wall_forces``.  The tables the feature adds are
of ``O(n_cells + n_rows)``.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib

__all__ = ["DragZone", "DragGroup", "check_zones"]


def _centroids(mesh, ids=None) -> np.ndarray:
    """(3, n) centroids of the mesh's cells (of the cells ``ids``), zero-padded: what the callables are handed."""
    cells = mesh.cells.to(torch.int64)
    if ids is not None:
        cells = cells[torch.as_tensor(np.asarray(ids, dtype=np.int64), device=cells.device)]
    cen = mesh.coords[cells].mean(dim=1).cpu().numpy()
    X = np.zeros((3, cen.shape[0]))
    X[: cen.shape[1]] = cen.T
    return X


def _check_coefficient(name, v):
    v = np.asarray(v, dtype=np.float64)
    if not np.isfinite(v).all() or (v < 0.0).any():
        raise ValueError(f"DragZone: {name} must be finite and >= 0 (min {float(np.min(v))}): a negative drag feeds the flow")


class DragZone:
    """Cells of the mesh with a drag ``-sigma (u - u_t)``, ``sigma = darcy + forchheimer |u - u_t|``.

    Args:
        cells: ``(celltags, id | ids)``: the cells of those values, one tag per id; an array of cell ids (the mesh's
            order): one tag 0; a callable ``f(x)`` on the cell centroids (``x: (3, ncells)``) that returns a bool mask:
            one tag 0
        darcy: ``alpha >= 0``: a float, a callable on the centroids of the zone's cells, or an array over the zone's cells
            (in the order of ``.cells``: by tag, then by cell id)
        forchheimer: ``beta >= 0``: the same
        target: ``u_t``: ``None`` (zero), a tuple of gdim floats, a callable ``f(x) -> (gdim, n)`` on dof coordinates
            (``x: (3, n)``) or a blocked Function of the solver's vector space.  It lives on the dofs of the zone's cells;
            where two zones share a dof, the target set last holds there
        rho: density, scales ``forces()``
        capacity: initial length of the ring of forces (it doubles when full)

    The zone is bound by ``FractionalStep_AB_CN(..., drag=zone)``.  ``.cells``, ``.cell_tags``, ``.tags`` then hold the
    selection (host arrays).
    """

    def __init__(self, cells, darcy=0.0, forchheimer=0.0, target=None, rho: float = 1.0, capacity: int = 64):
        self._cells_arg = cells
        self._darcy, self._forchheimer = self._coefficient("darcy", darcy), self._coefficient("forchheimer", forchheimer)
        self._target = target
        if isinstance(target, (tuple, list)) and not all(math.isfinite(float(v)) for v in target):
            raise ValueError(f"DragZone: target = {target}: finite numbers are expected")
        self.rho = float(rho)
        if not math.isfinite(self.rho) or not self.rho > 0.0:
            raise ValueError(f"DragZone: rho = {rho}")
        if int(capacity) < 1:
            raise ValueError(f"DragZone: capacity = {capacity}")
        self.capacity = int(capacity)
        self._group = None
        self._times = []
        self.cells = self.cell_tags = self.tags = None

    @staticmethod
    def _coefficient(name, v):
        if callable(v):
            return v
        if np.ndim(v) == 0:
            v = float(v)
            _check_coefficient(name, v)
            return v
        v = np.array(torch.as_tensor(v).detach().cpu().numpy(), dtype=np.float64).reshape(-1)
        _check_coefficient(name, v)
        return v

    # ---- what needs the mesh, but neither the library nor a GPU kernel ---------------------------------------------------
    def select(self, mesh):
        """(cell ids, tag index per cell, tag values): by tag, then by cell id.  An empty selection raises ``ValueError``."""
        arg = self._cells_arg
        nc = int(mesh.num_cells)
        if isinstance(arg, tuple) and len(arg) == 2 and hasattr(arg[0], "find"):
            mt, want = arg
            if mt.dim != mesh.gdim:
                raise ValueError(f"DragZone: the meshtags are of dimension {mt.dim}, cells have {mesh.gdim}")
            tags = np.atleast_1d(np.asarray(want, dtype=np.int64))
            if np.unique(tags).shape[0] != tags.shape[0]:
                raise ValueError("DragZone: a tag is listed twice")
            parts = [np.asarray(mt.find(np.int32(g)), dtype=np.int64) for g in tags]
            ids = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
            tag_of = np.concatenate([np.full(p.shape[0], k, dtype=np.int64) for k, p in enumerate(parts)])
        else:
            if callable(arg):
                mask = np.asarray(arg(_centroids(mesh)))
                if mask.dtype != np.bool_ or mask.shape != (nc,):
                    raise ValueError(f"DragZone: the cell marker must return a bool mask of {nc} cells "
                                     f"(got {mask.dtype}, shape {mask.shape})")
                ids = np.nonzero(mask)[0].astype(np.int64)
            else:
                ids = np.asarray(arg.cpu().numpy() if torch.is_tensor(arg) else arg, dtype=np.int64).reshape(-1)
            tag_of, tags = np.zeros(ids.shape[0], dtype=np.int64), np.array([0], dtype=np.int64)
        if ids.size == 0:
            raise ValueError("DragZone: the zone holds no cell")
        if ids.min() < 0 or ids.max() >= nc:
            raise ValueError(f"DragZone: a cell id outside 0 .. {nc - 1}")
        if np.unique(ids).shape[0] != ids.shape[0]:
            raise ValueError("DragZone: a cell is listed twice")
        order = np.lexsort((ids, tag_of))
        return ids[order], tag_of[order], tags

    def coefficients(self, mesh, ids):
        """(alpha, beta) per cell of ``ids``; negative or non-finite values raise ``ValueError``."""
        out = []
        for name, v in (("darcy", self._darcy), ("forchheimer", self._forchheimer)):
            n = ids.shape[0]
            if callable(v):
                a = np.broadcast_to(np.asarray(v(_centroids(mesh, ids)), dtype=np.float64), (n,)).copy()
            elif isinstance(v, float):
                a = np.full(n, v)
            else:
                if v.shape[0] != n:
                    raise ValueError(f"DragZone: {name} has {v.shape[0]} values, the zone has {n} cells")
                a = v.copy()
            _check_coefficient(name, a)
            out.append(a)
        return out

    # ---- bound ---------------------------------------------------------------------------------------------------------
    def _bound(self):
        if self._group is None:
            raise RuntimeError("DragZone: the zone is not the drag= of a solver yet")
        return self._group

    @property
    def n_samples(self) -> int:
        return len(self._times)

    def times(self) -> np.ndarray:
        return np.asarray(self._times, dtype=np.float64)

    def set_coefficients(self, darcy=None, forchheimer=None) -> None:
        """New ``darcy`` and / or ``forchheimer`` (forms as in the constructor), between steps: a ramped sponge.  Nothing
        is rebuilt; with every ``forchheimer`` zero, ``sigma`` is rewritten here."""
        if darcy is not None:
            self._darcy = self._coefficient("darcy", darcy)
        if forchheimer is not None:
            self._forchheimer = self._coefficient("forchheimer", forchheimer)
        if self._group is not None:
            self._group.write_coefficients(self)

    def set_target(self, target) -> None:
        """A new ``u_t`` (forms as in the constructor), between steps: a time-dependent target."""
        self._target = target
        if self._group is not None:
            self._group.write_target(self)

    def sample(self, t: float) -> None:
        """The force the fluid exerts on the medium of every tag, ``rho sum_c sigma_c int_c (u - u_t) dx``, of the solver's
        current ``u`` (read through ``rptr()``) with the ``sigma`` of the last ``assemble_first``: two launches on the
        current stream, no host synchronisation."""
        self._bound().sample(self, float(t))

    def forces(self) -> np.ndarray:
        """(n_samples, n_tags, gdim) on the host."""
        self._bound()
        return self._ring[: len(self._times)].cpu().numpy()

    def volume(self) -> np.ndarray:
        """Volume of the cells of every tag, (n_tags,)."""
        self._bound()
        return self._volume.copy()

    def save(self, path) -> None:
        np.savez(path, forces=self.forces(), times=self.times(), cells=self.cells, cell_tags=self.cell_tags, tags=self.tags,
                 volume=self.volume(), rho=self.rho)


def _zone_list(drag):
    if drag is None:
        return []
    zones = [drag] if isinstance(drag, DragZone) else list(drag)
    for z in zones:
        if not isinstance(z, DragZone):
            raise TypeError(f"drag=: a DragZone or a list of them is expected (got {type(z).__name__})")
    return zones


def check_zones(drag, mesh, rotational, theta):
    """The scope guards of ``drag=``, raised before the library is loaded or a collective is entered; returns per zone
    ``(ids, tag_of, tags, alpha, beta)``."""
    zones = _zone_list(drag)
    if not zones:
        return []
    comm = getattr(mesh, "comm", None)
    if comm is not None and getattr(comm, "size", 1) > 1:
        raise NotImplementedError("drag= on a mesh partition (comm.size > 1): the drag pass and the force sums are built "
                                  "for one GPU")
    if rotational:
        raise NotImplementedError("drag= with rotational=True: the rotational pressure update assumes the momentum "
                                  "operator M/dt + nu K/2; with a drag term it is not derived")
    theta = float(theta)
    if not (0.5 <= theta <= 1.0):
        raise ValueError(f"drag_theta = {theta}: a value in [0.5, 1] is expected (1: backward Euler, 0.5: Crank-Nicolson)")
    if len(set(map(id, zones))) != len(zones) or any(z._group is not None for z in zones):
        raise ValueError("drag=: a DragZone is bound to one solver, once")
    out, seen = [], np.zeros(int(mesh.num_cells), dtype=np.int32)
    for z in zones:
        ids, tag_of, tags = z.select(mesh)
        alpha, beta = z.coefficients(mesh, ids)
        seen[ids] += 1
        out.append((ids, tag_of, tags, alpha, beta))
    if seen.max() > 1:
        raise ValueError(f"drag=: cell {int(np.argmax(seen > 1))} lies in two zones: the coefficient of a cell has one owner")
    return out


class DragGroup:
    """The zones of one solver: the concatenated list of their cells (kernel positions, by zone, by tag, ascending), the
    coefficients per list entry, ``sigma`` per cell (kernel order, zero outside the zones), the target block and the
    slices of the velocity pattern with a row adjacent to a zone cell."""

    def __init__(self, solver, drag, theta, selections):
        from .fem import SLICE

        zones = _zone_list(drag)
        mesh = solver._mesh
        dev = mesh.device
        Vi = solver._Vi[0][0]
        d = mesh.gdim
        self._solver, self.zones, self.theta = solver, zones, float(theta)
        nc = int(solver._geom.shape[0])
        adet = solver._geom[:, d * d].cpu().numpy()
        vol = adet / math.factorial(d)
        kpos_all, off = [], 0
        for z, (ids, tag_of, tags, alpha, beta) in zip(zones, selections):
            kpos = Vi.kernel_cell_index(ids)
            if (kpos < 0).any():
                raise ValueError("DragZone: a cell is not among the cells of the solver's spaces")
            order = np.lexsort((kpos, tag_of))  # the kernel's order within a tag
            z.cells, z.cell_tags, z.tags = ids, (tags[tag_of] if ids.size else tag_of), tags
            z.n_cells, z.n_tags = int(ids.shape[0]), int(tags.shape[0])
            z._to_kernel = order
            z._off = off
            ptr = np.zeros(z.n_tags + 1, dtype=np.int64)
            ptr[1:] = np.cumsum(np.bincount(tag_of, minlength=z.n_tags))
            z._tag_ptr = torch.from_numpy(ptr).to(dev)
            z._volume = np.array([vol[kpos[tag_of == k]].sum() for k in range(z.n_tags)])
            z._ring = torch.zeros((z.capacity, z.n_tags, d), dtype=torch.float64, device=dev)
            z._times = []
            z._group = self
            kpos_all.append(kpos[order])
            off += z.n_cells
        kp = np.concatenate(kpos_all)
        self.n_zone_cells = int(kp.shape[0])
        self._zc = torch.from_numpy(kp.astype(np.int32)).to(dev)
        self._zc64 = self._zc.to(torch.int64)
        self._alpha = torch.zeros(self.n_zone_cells, dtype=torch.float64, device=dev)
        self._beta = torch.zeros(self.n_zone_cells, dtype=torch.float64, device=dev)
        self._sigma = torch.zeros(nc, dtype=torch.float64, device=dev)
        self._ft = torch.zeros((self.n_zone_cells, d), dtype=torch.float64, device=dev)
        self._ut = None
        # the slices with a row adjacent to a zone cell, ascending (chunks of the pair list: the temporaries stay small)
        in_zone = torch.zeros(nc + 1, dtype=torch.bool, device=dev)  # (the last entry serves the padding pairs)
        in_zone[self._zc64] = True
        adj = Vi.adj
        touched = torch.zeros(adj.n_slices, dtype=torch.bool, device=dev)
        ap = adj.adj_ptr.cpu().numpy()
        s0 = 0
        while s0 < adj.n_slices:
            s1 = int(min(adj.n_slices, max(s0 + 1, np.searchsorted(ap, ap[s0] + (1 << 26), side="right") - 1)))
            a, b = int(ap[s0]), int(ap[s1])
            if b > a:
                cell = adj.adj_cell[a:b].to(torch.int64)
                hit = in_zone[torch.where(cell >= 0, cell, torch.full_like(cell, nc))]
                counts = torch.from_numpy(np.diff(ap[s0:s1 + 1])).to(dev)
                sl = torch.repeat_interleave(torch.arange(s0, s1, device=dev), counts)
                touched[sl[hit]] = True
            s0 = s1
        # listed by the width bins of the pattern: a launch per bin, its accumulator as wide as the bin's rows
        P = Vi.pattern
        hit = touched[P.bin_slices.to(torch.int64)]
        self._slices = P.bin_slices[hit].to(torch.int32).contiguous()
        before = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(hit.to(torch.int64), 0)])
        self._bin_off = [int(v) for v in before[torch.as_tensor(np.asarray(P.bin_ptr, dtype=np.int64), device=dev)].tolist()]
        self._bin_width = [int(w) + (int(w) & 1) for w in np.asarray(P.bin_width)]
        self.n_slices_touched, self.n_slices = int(self._slices.shape[0]), int(adj.n_slices)
        self._w = None  # u_t - (1 - theta) u_1 where theta < 1
        assert SLICE == 64 and self._bin_off[-1] == self.n_slices_touched
        for z, (ids, tag_of, tags, alpha, beta) in zip(zones, selections):
            self._write_ab(z, alpha, beta)
        self._refresh()
        for z in zones:
            if z._target is not None:
                self.write_target(z)

    # ---- coefficients --------------------------------------------------------------------------------------------------
    def _write_ab(self, z, alpha, beta):
        dev = self._alpha.device
        seg = slice(z._off, z._off + z.n_cells)
        self._alpha[seg] = torch.from_numpy(alpha[z._to_kernel]).to(dev)
        self._beta[seg] = torch.from_numpy(beta[z._to_kernel]).to(dev)

    def _refresh(self):
        """``sigma <- alpha`` on the zones' cells (what it is where every ``forchheimer`` is zero, and before the first
        step elsewhere) and the flag that lets the sigma launch be skipped."""
        self.static = not bool((self._beta != 0.0).any())
        self._sigma[self._zc64] = self._alpha

    def write_coefficients(self, z):
        alpha, beta = z.coefficients(self._solver._mesh, z.cells)
        self._write_ab(z, alpha, beta)
        self._refresh()

    def write_target(self, z):
        from .fem import Function

        S = self._solver
        Vi = S._Vi[0][0]
        d, dev = S._gdim, self._alpha.device
        t = z._target
        if t is None and self._ut is None:
            return
        if self._ut is None:
            self._ut = torch.zeros((S._n_u, d), dtype=torch.float64, device=dev)
        seg = self._zc64[z._off: z._off + z.n_cells]
        dofs = torch.unique(Vi.cell_dofs.to(torch.int64)[seg].reshape(-1))
        if t is None:
            self._ut[dofs] = 0.0
        elif isinstance(t, Function):
            st = t._storage
            if t._comp is not None or st.nc != d or st.n != S._n_u:
                raise ValueError("DragZone: a target Function must be a blocked Function of the solver's vector space")
            self._ut[dofs] = st.rdev()[dofs]
        elif callable(t):
            x = Vi.x[dofs].cpu().numpy()
            X = np.zeros((3, x.shape[0]))
            X[:d] = x.T
            v = np.asarray(t(X), dtype=np.float64)
            if v.shape != (d, x.shape[0]):
                raise ValueError(f"DragZone: the target must return an array of shape ({d}, n) (got {v.shape})")
            if not np.isfinite(v).all():
                raise ValueError("DragZone: the target is not finite")
            self._ut[dofs] = torch.from_numpy(np.ascontiguousarray(v.T)).to(dev)
        else:
            v = np.asarray(t, dtype=np.float64).reshape(-1)
            if v.shape[0] != d or not np.isfinite(v).all():
                raise ValueError(f"DragZone: target = {t}: {d} finite numbers are expected")
            self._ut[dofs] = torch.from_numpy(v).to(dev)

    # ---- launches ------------------------------------------------------------------------------------------------------
    def launch_sigma(self):
        S = self._solver
        Vi = S._Vi[0][0]
        _lib.check(_lib.load().ox_drag_sigma(Vi.degree, C.byref(S._cells), _lib.ptr(Vi.cell_dofs), self.n_zone_cells,
                                             _lib.ptr(self._zc), _lib.ptr(self._alpha), _lib.ptr(self._beta),
                                             S._UAB.rptr(), _lib.ptr(self._ut), _lib.ptr(self._sigma),
                                             _lib.current_stream()), "ox_drag_sigma")

    def launch_rows(self):
        S = self._solver
        Vi = S._Vi[0][0]
        lib, st = _lib.load(), _lib.current_stream()
        w = self._ut  # theta = 1: the right-hand side is D u_t (None: nothing)
        if self.theta != 1.0:  # w = u_t - (1 - theta) u_1, one pass over the block
            if self._w is None:
                self._w = torch.zeros((S._n_u, S._gdim), dtype=torch.float64, device=self._sigma.device)
            w, n = self._w, S._n_u * S._gdim
            if self._ut is None:
                _lib.check(lib.ox_axpby(n, self.theta - 1.0, S._U1.rptr(), 0.0, S._U1.rptr(), _lib.ptr(w), st), "ox_axpby")
            else:
                _lib.check(lib.ox_axpby(n, 1.0, _lib.ptr(self._ut), self.theta - 1.0, S._U1.rptr(), _lib.ptr(w), st),
                           "ox_axpby")
        info, b = Vi.assembly_info(), S._BFIRST.ptr()
        for k, width in enumerate(self._bin_width):
            lo, hi = self._bin_off[k], self._bin_off[k + 1]
            if hi > lo:
                _lib.check(lib.ox_drag_rows(C.byref(S._cells), C.byref(info), S._A.ref(), hi - lo, _lib.ptr(self._slices[lo:hi]),
                                            width, _lib.ptr(self._sigma), self.theta, _lib.ptr(w), b, st), "ox_drag_rows")

    def add(self) -> None:
        """``sigma`` of this step's ``u_ab``, then ``A += theta D`` and the two terms of ``b_first``."""
        if not self.static:
            self.launch_sigma()
        self.launch_rows()
        self._solver._A.version += 1

    def sample(self, z, t):
        S = self._solver
        Vi = S._Vi[0][0]
        k = len(z._times)
        if k == z.capacity:  # the ring doubles (a device copy on the current stream)
            ring = torch.zeros((2 * z.capacity,) + tuple(z._ring.shape[1:]), dtype=torch.float64, device=z._ring.device)
            ring[: z.capacity] = z._ring
            z._ring, z.capacity = ring, 2 * z.capacity
        lib, st = _lib.load(), _lib.current_stream()
        seg = slice(z._off, z._off + z.n_cells)
        ft = self._ft[seg]
        _lib.check(lib.ox_drag_force_cells(Vi.degree, C.byref(S._cells), _lib.ptr(Vi.cell_dofs), z.n_cells,
                                           _lib.ptr(self._zc[seg]), _lib.ptr(self._sigma), S._U.rptr(), _lib.ptr(self._ut),
                                           _lib.ptr(ft), st), "ox_drag_force_cells")
        # ox_wall_forces writes -rho sum ft, the force on a wall; on the medium it is +rho sum ft
        _lib.check(lib.ox_wall_forces(S._gdim, z.n_tags, _lib.ptr(z._tag_ptr), _lib.ptr(ft), -z.rho, _lib.ptr(z._ring),
                                      z.capacity, k, st), "ox_wall_forces")
        z._times.append(t)

    def coefficient(self) -> torch.Tensor:
        """``sigma`` per cell in the MESH's cell order."""
        S = self._solver
        out = torch.zeros(int(S._mesh.num_cells), dtype=torch.float64, device=self._sigma.device)
        out[S._Vi[0][0].local_cells.to(torch.int64)] = self._sigma
        return out
