"""Outlet models on tagged exterior facets, on the device beside the time step: flow rates, lumped resistance and RCR
Windkessel pressures, and the backflow stabilisation of a pressure boundary.

On exterior facet f with outward unit normal n and measure ``|f|`` (``csrc/ox_outlet.hip``)::

    Q_tag = sum_{f in tag} |f| n . mean_f(u)                          Q > 0 leaves the domain
    Resistance:   P = p_distal + R Q
    Windkessel:   P = Pc + Rp Q,   C dPc/dt = Q - (Pc - p_distal) / Rd

The facet is affine, so the facet mean of a Lagrange field is exact (compile-time facet means of the basis).  A model is
the ``value`` of a :class:`oasisx_amd.PressureBC`; the coupling is explicit and of first order: in step n,
``assemble_first(dt, nu)`` takes Q of ``u1`` (the velocity of the last finished step) over the outlet's facets, advances
``Pc`` by backward Euler with that Q::

    Pc <- (Pc + (dt/C) (Q + p_distal/Rd)) / (1 + dt/(Rd C))

and writes ``h = (Pc + Rp Q) / rho`` on the outlet's pressure dofs (the step is kinematic, the parameters physical).  Two
launches per step for all the models of a solver (``ox_outlet_flux``, ``ox_outlet_update``), nothing is read back.

Backflow stabilisation, ``PressureBC(..., backflow=beta)``: ``-beta int_Gamma min(u_ab . n, 0) u . v ds`` in the momentum
equation of every component, Crank-Nicolson like the convection it tames: ``A += (beta/2) B``, ``b_first -= (beta/2) B u1``
with ``B_rs = sum_f int_f max(-u_ab . n, 0) phi_r phi_s ds``, by ``ox_outlet_backflow``: one lane per touched row, no atomics.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .wall import FacetSet, select_facets

__all__ = ["FlowRate", "Resistance", "Windkessel", "OutletModel"]

NPAR = 8  # OX_OUTLET_NPAR of csrc/ox_outlet.hip: kind, Rp, C, Rd, p_distal, rho, 2 reserved
RULE_POINTS = {1: 2, 2: 4, 3: 5}  # Gauss points per direction of the backflow term's facet rule, by velocity degree


# ---- lumped models -----------------------------------------------------------------------------------------------------
def _finite(name, v):
    v = float(v)
    if not math.isfinite(v):
        raise ValueError(f"{name} = {v}: a finite number is expected")
    return v


class OutletModel:
    """A lumped model of what lies beyond an outlet: the ``value`` of a ``PressureBC``.  The solver binds it; the state
    ``Pc`` and the history live on the device."""

    kind = 0

    def __init__(self, Rp, Cap, Rd, p_distal, p0, rho, capacity):
        who = type(self).__name__
        self.Rp, self.Rd = _finite(f"{who}: resistance", Rp), _finite(f"{who}: Rd", Rd)
        self.C = _finite(f"{who}: C", Cap)
        self.p_distal, self.rho = _finite(f"{who}: p_distal", p_distal), _finite(f"{who}: rho", rho)
        self.p0 = self.p_distal if p0 is None else _finite(f"{who}: p0", p0)
        if self.Rp < 0.0 or self.Rd < 0.0:
            raise ValueError(f"{who}: a resistance is negative (Rp = {self.Rp}, Rd = {self.Rd})")
        if not self.C > 0.0:
            raise ValueError(f"{who}: C = {self.C}: a positive compliance is expected")
        if not self.rho > 0.0:
            raise ValueError(f"{who}: rho = {self.rho}")
        if int(capacity) < 1:
            raise ValueError(f"{who}: capacity = {capacity}")
        self.capacity = int(capacity)
        self._group, self._k = None, -1

    def parameters(self) -> np.ndarray:
        """The model's row of the kernel's parameter table."""
        return np.array([self.kind, self.Rp, self.C, self.Rd, self.p_distal, self.rho, 0.0, 0.0], dtype=np.float64)

    def initial_h(self) -> float:
        """``h`` before the first step: ``P / rho`` at Q = 0."""
        return self.p0 / self.rho

    def _bind(self, group, k):
        self._group, self._k = group, k

    def _bound(self):
        if self._group is None:
            raise RuntimeError(f"{type(self).__name__}: the model is not the value of a PressureBC of a solver yet")
        return self._group

    def history(self) -> dict:
        """``dict(times, Q, P, Pc)``: one entry per ``assemble_first``, host arrays (one synchronisation); ``times`` is the
        running sum of ``dt``."""
        g = self._bound()
        n = len(g._times)
        H = g._hist[:n, self._k].cpu().numpy()
        return dict(times=np.asarray(g._times, dtype=np.float64), Q=H[:, 0].copy(), P=H[:, 1].copy(), Pc=H[:, 2].copy())

    def state(self) -> float:
        """The current ``Pc`` (one synchronisation)."""
        return float(self._bound()._state[self._k].item())

    def reset(self, p0=None) -> None:
        """``Pc <- p0`` (default: the model's initial value)."""
        if p0 is not None:
            self.p0 = _finite(f"{type(self).__name__}: p0", p0)
        if self._group is not None:
            self._group._state[self._k] = self.p0


class Resistance(OutletModel):
    """``P = p_distal + R Q``: the Windkessel without its capacitor."""

    kind = 1

    def __init__(self, R, p_distal: float = 0.0, rho: float = 1.0, capacity: int = 64):
        super().__init__(R, 1.0, 0.0, p_distal, None, rho, capacity)
        self.R = self.Rp


class Windkessel(OutletModel):
    """Three-element RCR Windkessel: ``P = Pc + Rp Q``, ``C dPc/dt = Q - (Pc - p_distal) / Rd``; ``p0``: the initial ``Pc``
    (default ``p_distal``)."""

    kind = 2

    def __init__(self, Rp, C, Rd, p_distal: float = 0.0, p0=None, rho: float = 1.0, capacity: int = 64):
        super().__init__(Rp, C, Rd, p_distal, p0, rho, capacity)


# ---- facets ------------------------------------------------------------------------------------------------------------
def _single_gpu(mesh, who):
    comm = getattr(mesh, "comm", None)
    if comm is not None and getattr(comm, "size", 1) > 1:
        raise NotImplementedError(f"{who} on a mesh partition (comm.size > 1): the facet sums are built for one GPU")


class _FacetSet(FacetSet):
    """The shared facet set with the per-facet flux buffer the outlet kernels write."""

    def __init__(self, solver, ids, tag_of, n_tags, who):
        super().__init__(solver, ids, tag_of, n_tags, who, "flow rates and outlet models")
        dev = solver._mesh.device
        if not self.n_facets:  # (never launched on; the update kernel is handed a valid pointer)
            self.rec = torch.zeros((1, 2), dtype=torch.int32, device=dev)
        self.flux = torch.zeros(max(self.n_facets, 1), dtype=torch.float64, device=dev)

    def launch_flux(self, solver, u_ptr):
        if self.n_facets:
            Vi = solver._Vi[0][0]
            _lib.check(_lib.load().ox_outlet_flux(Vi.degree, C.byref(solver._cells), _lib.ptr(Vi.cell_dofs), self.n_facets,
                                                  _lib.ptr(self.rec), u_ptr, _lib.ptr(self.flux), _lib.current_stream()),
                       "ox_outlet_flux")


def _grown(ring, capacity):
    """The ring with twice the capacity (a device copy on the current stream)."""
    out = torch.zeros((2 * capacity,) + tuple(ring.shape[1:]), dtype=ring.dtype, device=ring.device)
    out[:capacity] = ring
    return out


class FlowRate:
    """Flow rates ``Q_tag = sum_f |f| n . mean_f(u)`` through exterior facets of a ``FractionalStep_AB_CN`` solver.

    Args:
        solver: the solver (one GPU: ``comm.size > 1`` raises ``NotImplementedError``)
        facets: ``None``: all exterior facets, one tag 0; ``(meshtags, id)`` / ``(meshtags, (id, ...))``: the facets of
            those values, one tag per id; an array of facet ids: those facets, one tag 0.  Interior facets raise
            ``ValueError``
        capacity: initial length of the ring of rates (it doubles when full)

    The object's facet order is by tag, then by facet id (``.facets``, ``.facet_tags``); ``.tags``: the tag values;
    ``.normals`` (outward), ``.areas``: host arrays in that order.
    """

    def __init__(self, solver, facets=None, capacity: int = 64):
        mesh = solver._mesh
        _single_gpu(mesh, "FlowRate")
        if int(capacity) < 1:
            raise ValueError(f"FlowRate: capacity = {capacity}")
        ids, tag_of, tags = select_facets(mesh, facets, "FlowRate")
        self._solver = solver
        self._set = _FacetSet(solver, ids, tag_of, tags.shape[0], "FlowRate")
        self.facets, self.tags = ids, tags
        self.facet_tags = tags[tag_of] if ids.size else tag_of
        self.cells, self.local_facets = self._set.cells, self._set.local_facets
        self.normals, self.areas = self._set.normals, self._set.areas
        self.n_facets, self.n_tags = self._set.n_facets, self._set.n_tags
        self.capacity = int(capacity)
        self._ring = torch.zeros((self.capacity, self.n_tags), dtype=torch.float64, device=mesh.device)
        self._times = []

    @property
    def n_samples(self) -> int:
        return len(self._times)

    @property
    def times(self) -> np.ndarray:
        return np.asarray(self._times, dtype=np.float64)

    def sample(self, t: float, level: int = 0) -> None:
        """The rates of the solver's ``u`` (``level=0``) or ``u1`` (``level=1``) on the current stream: two launches, no
        host synchronisation; the block is read through ``rptr()``."""
        if level not in (0, 1):
            raise ValueError("FlowRate.sample: level is 0 (u) or 1 (u1)")
        k = len(self._times)
        if k == self.capacity:
            self._ring, self.capacity = _grown(self._ring, self.capacity), 2 * self.capacity
        S = self._solver
        self._set.launch_flux(S, (S._U if level == 0 else S._U1).rptr())
        _lib.check(_lib.load().ox_outlet_update(self.n_tags, _lib.ptr(self._set.tag_ptr), _lib.ptr(self._set.flux),
                                                _lib.ptr(self._ring), self.capacity, k, None, 0.0, None, None, None, None,
                                                None, 0, _lib.current_stream()), "ox_outlet_update")
        self._times.append(float(t))

    def rates(self) -> np.ndarray:
        """(n_samples, n_tags) on the host."""
        return self._ring[: len(self._times)].cpu().numpy()

    def facet_flux(self) -> torch.Tensor:
        """``|f| n . mean_f(u)`` per facet of the latest sample, (n_facets,) on the device."""
        return self._set.flux[: self.n_facets]

    def save(self, path) -> None:
        np.savez(path, rates=self.rates(), times=self.times, facets=self.facets, facet_tags=self.facet_tags, tags=self.tags,
                 normals=self.normals, areas=self.areas, facet_flux=self.facet_flux().cpu().numpy())


# ---- the solver's side -------------------------------------------------------------------------------------------------
class OutletGroup:
    """The lumped models of one solver: one tag per modelled ``PressureBC``, advanced together once per
    ``assemble_first`` (flux of ``u1``, update, ``h``)."""

    def __init__(self, solver, bcs):
        mesh = solver._mesh
        dev = mesh.device
        self.bcs = list(bcs)
        n = len(self.bcs)
        parts = [np.sort(np.asarray(b._facets, dtype=np.int64)) for b in self.bcs]
        ids = np.concatenate(parts)
        tag_of = np.concatenate([np.full(p.shape[0], k, dtype=np.int64) for k, p in enumerate(parts)])
        self._set = _FacetSet(solver, ids, tag_of, n, "PressureBC with an outlet model")
        self._solver = solver
        nq = int(solver._Q.n_local)
        self._h = torch.zeros((n, nq), dtype=torch.float64, device=dev)
        dof_ptr = np.zeros(n + 1, dtype=np.int64)
        dof_ptr[1:] = np.cumsum([b._dofs.shape[0] for b in self.bcs])
        dofs = np.concatenate([b._dofs for b in self.bcs]).astype(np.int32)
        self._dof_ptr = torch.from_numpy(dof_ptr).to(dev)
        self._dofs = torch.from_numpy(dofs if dofs.size else np.zeros(1, dtype=np.int32)).to(dev)
        models = [b._model for b in self.bcs]
        self._params = torch.from_numpy(np.stack([m.parameters() for m in models])).to(dev)
        self._state = torch.tensor([m.p0 for m in models], dtype=torch.float64, device=dev)
        self.capacity = min(m.capacity for m in models)
        self._ring = torch.zeros((self.capacity, n), dtype=torch.float64, device=dev)
        self._hist = torch.zeros((self.capacity, n, 3), dtype=torch.float64, device=dev)
        self._times, self._t = [], 0.0
        for k, (b, m) in enumerate(zip(self.bcs, models)):
            self._h[k].copy_(b._h)  # the outlet's nodal values become the group's row k: the kernel writes them there
            b._h = self._h[k]
            m._bind(self, k)

    def advance(self, dt: float) -> None:
        dt = float(dt)
        if not dt > 0.0:
            raise ValueError(f"outlet models: dt = {dt}")
        k = len(self._times)
        if k == self.capacity:
            self._ring, self._hist = _grown(self._ring, self.capacity), _grown(self._hist, self.capacity)
            self.capacity *= 2
        S = self._solver
        self._set.launch_flux(S, S._U1.rptr())
        _lib.check(_lib.load().ox_outlet_update(self._set.n_tags, _lib.ptr(self._set.tag_ptr), _lib.ptr(self._set.flux),
                                                _lib.ptr(self._ring), self.capacity, k, _lib.ptr(self._params), dt,
                                                _lib.ptr(self._state), _lib.ptr(self._hist), _lib.ptr(self._dof_ptr),
                                                _lib.ptr(self._dofs), _lib.ptr(self._h), int(self._h.shape[1]),
                                                _lib.current_stream()), "ox_outlet_update")
        self._t += dt
        self._times.append(self._t)


def facet_dofs(d: int, degree: int, a: int) -> np.ndarray:
    """The cell-local dofs that live on local facet a, ascending (``OX_OFD`` of csrc/fe_tables_o.h): the basis functions
    that do not vanish on the facet."""
    from .fem import _simplex_rule, lagrange_basis

    lam = _simplex_rule(d - 1, 3)[0]
    p = np.zeros((lam.shape[0], d + 1))
    p[:, [b for b in range(d + 1) if b != a]] = lam
    return np.nonzero(np.abs(lagrange_basis(d, degree, p)).max(axis=0) > 1e-12)[0]


class RowPairs:
    """The row-centric set-up of a facet pass over the velocity component space (shared by :class:`Backflow` and the
    scalars' flux / Robin pass, :mod:`oasisx_amd.scalar`): per touched owned row its (record, position among the record's
    facet dofs) pairs, by row and then by record, and -- with ``slots`` -- per pair the slots of (row, facet dof s) in the
    SELL value array of the space's pattern.  ``kpos`` / ``local_facets``: kernel cell and local facet per record (a facet
    may occur in several records)."""

    def __init__(self, Vi, kpos, local_facets, dev, who: str, slots: bool = True):
        from .fem import KV, SLICE

        d = int(Vi.mesh.gdim)
        nf = int(np.asarray(kpos).shape[0])
        table = np.stack([facet_dofs(d, Vi.degree, a) for a in range(d + 1)])  # (d + 1, nfd)
        nfd = table.shape[1]
        cd = Vi.cell_dofs.cpu().numpy()[kpos]  # (nf, nd)
        fd = np.take_along_axis(cd, table[local_facets], axis=1).astype(np.int64)  # (nf, nfd)
        row = fd.reshape(-1)
        fi = np.repeat(np.arange(nf, dtype=np.int64), nfd)
        loc = np.tile(np.arange(nfd, dtype=np.int64), nf)
        keep = row < Vi.n_owned
        row, fi, loc = row[keep], fi[keep], loc[keep]
        order = np.lexsort((fi, row))  # by row, then by record (= ascending facet id)
        row, fi, loc = row[order], fi[order], loc[order]
        rows, counts = np.unique(row, return_counts=True)
        row_ptr = np.zeros(rows.shape[0] + 1, dtype=np.int64)
        row_ptr[1:] = np.cumsum(counts)
        self.facet_dofs = fd
        self.n_rows, self.nfd, self.n_pairs = int(rows.shape[0]), int(nfd), int(row.shape[0])
        self.rows = torch.from_numpy(rows.astype(np.int32) if rows.size else np.zeros(1, dtype=np.int32)).to(dev)
        self.row_ptr = torch.from_numpy(row_ptr).to(dev)
        self.pair_facet = torch.from_numpy(fi.astype(np.int32) if fi.size else np.zeros(1, dtype=np.int32)).to(dev)
        self.pair_loc = torch.from_numpy(loc.astype(np.int32) if loc.size else np.zeros(1, dtype=np.int32)).to(dev)
        self.pair_off = None
        if not slots:
            return
        if not row.size:  # an empty facet set: nothing is looked up
            self.pair_off = torch.zeros(1, dtype=torch.int64, device=dev)
            return
        # slots of (row, facet dof s) in the SELL value array of the velocity pattern
        P = Vi.pattern
        r = torch.from_numpy(row).to(dev)
        rl = P.row_len.to(torch.int64)[r]
        W = int(rl.max().item()) if row.size else 0
        kk = torch.arange(W, device=dev, dtype=torch.int64)
        slots = (P.slice_ptr[r // SLICE].unsqueeze(1) + (kk // KV).unsqueeze(0) * (SLICE * KV)
                 + (r % SLICE).unsqueeze(1) * KV + (kk % KV).unsqueeze(0))
        valid = kk.unsqueeze(0) < rl.unsqueeze(1)
        cols = P.cols[slots.clamp(0, max(P.size - 1, 0))].to(torch.int64)
        want = torch.from_numpy(fd[fi]).to(dev)  # (n_pairs, nfd)
        off = torch.full(want.shape, -1, dtype=torch.int64, device=dev)
        for s in range(nfd):
            hit = (cols == want[:, s].unsqueeze(1)) & valid
            if not bool(hit.any(dim=1).all()):
                raise RuntimeError(f"{who}: an entry of the facet mass matrix is not in the velocity pattern")
            off[:, s] = torch.gather(slots, 1, hit.to(torch.int8).argmax(dim=1, keepdim=True)).squeeze(1)
        self.pair_off = off.contiguous() if off.numel() else torch.zeros(1, dtype=torch.int64, device=dev)


class Backflow:
    """The backflow pass of one solver: the facets of every ``PressureBC`` with ``backflow > 0`` in ascending facet id,
    ``beta`` per facet; per touched velocity row its (facet, position among the facet's dofs) pairs and the slots of
    ``A``'s value array, computed once from the velocity pattern (:class:`RowPairs`)."""

    def __init__(self, solver, bcs):
        mesh = solver._mesh
        dev = mesh.device
        ids = np.concatenate([np.asarray(b._facets, dtype=np.int64) for b in bcs])
        beta = np.concatenate([np.full(b._facets.shape[0], b.backflow, dtype=np.float64) for b in bcs])
        order = np.argsort(ids, kind="stable")
        ids, beta = ids[order], beta[order]
        self._set = _FacetSet(solver, ids, np.zeros(ids.shape[0], dtype=np.int64), 1, "PressureBC with backflow")
        self._solver = solver
        rp = RowPairs(solver._Vi[0][0], self._set.kpos, self._set.local_facets, dev, "backflow")
        self.n_rows, self.nfd = rp.n_rows, rp.nfd
        self.rows, self.row_ptr, self.pair_facet, self.pair_loc, self.pair_off = (rp.rows, rp.row_ptr, rp.pair_facet,
                                                                                  rp.pair_loc, rp.pair_off)
        self.beta = torch.from_numpy(beta if beta.size else np.zeros(1)).to(dev)

    def add(self) -> None:
        """``A += (beta/2) B``, ``b_first -= (beta/2) B u1`` with the ``u_ab`` block of this step."""
        S = self._solver
        Vi = S._Vi[0][0]
        _lib.check(_lib.load().ox_outlet_backflow(Vi.degree, C.byref(S._cells), _lib.ptr(Vi.cell_dofs), self.n_rows,
                                                  _lib.ptr(self.rows), _lib.ptr(self.row_ptr), _lib.ptr(self.pair_facet),
                                                  _lib.ptr(self.pair_loc), _lib.ptr(self.pair_off), self._set.n_facets,
                                                  _lib.ptr(self._set.rec), _lib.ptr(self.beta), S._UAB.rptr(),
                                                  S._U1.rptr(), _lib.ptr(S._A.vals), int(S._A.vals.shape[0]),
                                                  S._BFIRST.ptr(), _lib.current_stream()), "ox_outlet_backflow")
        S._A.version += 1
