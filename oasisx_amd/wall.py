"""Wall shear stress, traction and forces on tagged exterior facets, evaluated on the device beside the time step.

On exterior facet f of cell c (opposite local vertex a) with outward unit normal n and measure ``|f|``, in kinematic
units (``rho`` scales the forces)::

    t_f   = (1/|f|) int_f sigma n ds = -pbar n + nu_eff (gbar + gbar^T) n      gbar, pbar: facet means of grad u, p
    nu_eff = nu + nut[c]                                                         (nut only with a viscosity_model)
    wss_f = t_f - (t_f . n) n                                                    (outward n: the usual convention)
    F_tag = -rho sum_{f in tag} |f| t_f                                          (the force of the fluid ON the boundary)

The facet is affine, so the facet means are exact (compile-time facet means of the bases, csrc/fe_tables_f.h).  The stress
is always the symmetric ``sigma``, also with a viscosity model -- whose viscous term in the step is the Laplacian form
``div(nut grad u)`` (:mod:`oasisx_amd.viscosity`).  One launch of ``ox_wall_stress`` per sample (one lane per facet) and
one of ``ox_wall_forces`` (one block per tag); nothing is read back, ``u`` and ``p`` are read through ``rptr()``.

Time-averaged indices over the samples taken with ``dt > 0`` (total weight T)::

    TAWSS = (1/T) sum dt |wss|      mean_wss = (1/T) sum dt wss      OSI = (1 - |sum dt wss| / sum dt |wss|) / 2
    RRT   = 1 / ((1 - 2 OSI) TAWSS)
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

__all__ = ["WallStress", "facet_table", "select_facets", "FacetSet"]


def facet_table(mesh, facets, who: str = "WallStress", what: str = "wall stresses"):
    """(cell, opposite local vertex) of exterior facets: mesh cell ids and local vertex indices, in the order of
    ``facets``.  A facet that two cells share (or no cell has) raises ``ValueError`` (in the name of ``who``)."""
    import itertools

    d = mesh.gdim
    facets = np.asarray(facets, dtype=np.int64).reshape(-1)
    _, cf = mesh._entities(d - 1)
    if facets.size and (facets.min() < 0 or facets.max() > cf.max()):
        raise ValueError(f"{who}: facet ids are indices of the mesh's facets")
    if np.unique(facets).shape[0] != facets.shape[0]:
        raise ValueError(f"{who}: a facet is listed twice")
    counts = np.bincount(cf.ravel(), minlength=int(cf.max()) + 1)
    interior = facets[counts[facets] != 1]
    if interior.size:
        raise ValueError(f"{who}: {interior.size} of the facets are interior facets (the first: {int(interior[0])}); "
                         f"{what} are evaluated on exterior facets")
    per = getattr(mesh, "periodic", None)
    if per is not None and per.is_periodic_facet(facets).any():
        seam = facets[per.is_periodic_facet(facets)]
        raise ValueError(f"{who}: {seam.size} of the facets lie on an identified (periodic) face (the first: {int(seam[0])}); "
                         f"{what} are evaluated on exterior facets")
    combos = list(itertools.combinations(range(d + 1), d))
    opp_of_combo = np.array([[a for a in range(d + 1) if a not in c][0] for c in combos])
    fcell, fslot = np.nonzero(np.isin(cf, facets))
    fid = cf[fcell, fslot]
    order = np.argsort(fid)  # every id occurs once: exterior
    pos = np.searchsorted(fid[order], facets)
    sel = order[pos]
    return fcell[sel], opp_of_combo[fslot[sel]]


def select_facets(mesh, facets, who: str = "WallStress"):
    """(facet ids, tag index per facet, tag values) of a facet selection -- ``None``: all exterior facets, one tag 0;
    ``(meshtags, id | ids)``: one tag per id; an array of facet ids: one tag 0 -- ordered by tag, then by facet id."""
    d = mesh.gdim
    if facets is None:
        ids = np.asarray(mesh.exterior_facets(), dtype=np.int64)
        tag_of, tags = np.zeros(ids.shape[0], dtype=np.int64), np.array([0], dtype=np.int64)
    elif isinstance(facets, tuple) and len(facets) == 2 and hasattr(facets[0], "find"):
        mt, want = facets
        if mt.dim != d - 1:
            raise ValueError(f"{who}: the meshtags are of dimension {mt.dim}, facets have {d - 1}")
        tags = np.atleast_1d(np.asarray(want, dtype=np.int64))
        if np.unique(tags).shape[0] != tags.shape[0]:
            raise ValueError(f"{who}: a tag is listed twice")
        parts = [np.asarray(mt.find(np.int32(g)), dtype=np.int64) for g in tags]
        ids = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
        tag_of = np.concatenate([np.full(p.shape[0], k, dtype=np.int64) for k, p in enumerate(parts)])
    else:
        ids = np.asarray(facets.cpu().numpy() if torch.is_tensor(facets) else facets, dtype=np.int64).reshape(-1)
        tag_of, tags = np.zeros(ids.shape[0], dtype=np.int64), np.array([0], dtype=np.int64)
    order = np.lexsort((ids, tag_of))  # by tag, then by facet id
    return ids[order], tag_of[order], tags


class FacetSet:
    """Exterior facets of a solver's mesh, given sorted by tag: what the facet kernels read (``rec``: (kernel cell, local
    facet) per facet, ``tag_ptr``: the tags' segments; device tensors) and the host geometry from the same records
    (``normals`` outward, ``areas``, ``midpoints``).  Shared by ``WallStress`` and :mod:`oasisx_amd.outlet`."""

    def __init__(self, solver, ids, tag_of, n_tags, who: str = "WallStress", what: str = "wall stresses"):
        mesh = solver._mesh
        d = mesh.gdim
        fcell, fopp = facet_table(mesh, ids, who, what)
        kpos = solver._Vi[0][0].kernel_cell_index(fcell)
        if (kpos < 0).any():
            raise ValueError(f"{who}: a facet's cell is not among the cells of the solver's spaces")
        dev = mesh.device
        nf = int(ids.shape[0])
        self.facets, self.cells, self.local_facets, self.kpos = ids, fcell, fopp, kpos
        self.n_facets, self.n_tags = nf, int(n_tags)
        # geometry on the host, from the records the kernel reads
        geom = solver._geom[torch.from_numpy(kpos).to(dev)].cpu().numpy()  # (nf, gs)
        G = geom[:, : d * d].reshape(-1, d, d)
        G = np.concatenate([-G.sum(axis=1, keepdims=True), G], axis=1)
        Ga = G[np.arange(nf), fopp]
        ga = np.linalg.norm(Ga, axis=1)
        self.normals = -Ga / ga[:, None]
        self.areas = geom[:, d * d] * ga * (0.5 if d == 3 else 1.0)
        fv, _ = mesh._entities(d - 1)
        self.midpoints = mesh.coords.cpu().numpy()[fv[ids]].mean(axis=1)
        # device tables
        rec = np.stack([kpos, fopp], axis=1).astype(np.int32)
        self.rec = torch.from_numpy(np.ascontiguousarray(rec)).to(dev)
        ptr = np.zeros(self.n_tags + 1, dtype=np.int64)
        ptr[1:] = np.cumsum(np.bincount(tag_of, minlength=self.n_tags))
        self.tag_ptr = torch.from_numpy(ptr).to(dev)


class WallStress:
    """Traction, wall shear stress and forces on exterior facets of a ``FractionalStep_AB_CN`` solver.

    Args:
        solver: the solver (one GPU: ``comm.size > 1`` raises ``NotImplementedError``)
        facets: ``None``: all exterior facets, one tag 0; ``(meshtags, id)`` / ``(meshtags, (id, ...))``: the facets of
            those values, one tag per id; an array of facet ids: those facets, one tag 0.  Interior facets raise
            ``ValueError``
        rho: density, scales ``forces()``
        capacity: initial length of the forces ring (it doubles when full)

    The object's facet order is by tag, then by facet id (``.facets``, ``.facet_tags``).  ``.tags``: the tag values;
    ``.normals`` (outward), ``.areas``, ``.midpoints``: host arrays in that order.
    """

    def __init__(self, solver, facets=None, rho: float = 1.0, capacity: int = 64):
        mesh = solver._mesh
        comm = getattr(mesh, "comm", None)
        if comm is not None and getattr(comm, "size", 1) > 1:
            raise NotImplementedError("WallStress on a mesh partition (comm.size > 1): the facet evaluation and the force "
                                      "sums are built for one GPU")
        if int(capacity) < 1:
            raise ValueError(f"WallStress: capacity = {capacity}")
        d = mesh.gdim
        ids, tag_of, tags = select_facets(mesh, facets)
        fs = FacetSet(solver, ids, tag_of, tags.shape[0])
        self._solver = solver
        self.rho = float(rho)
        self.gdim = d
        self.facets = ids
        self.tags = tags
        self.facet_tags = tags[tag_of] if ids.size else tag_of
        self.cells, self.local_facets = fs.cells, fs.local_facets
        self.n_facets, self.n_tags = fs.n_facets, fs.n_tags
        dev = mesh.device
        self.normals, self.areas, self.midpoints = fs.normals, fs.areas, fs.midpoints
        self._rec, self._tag_ptr = fs.rec, fs.tag_ptr

        def rows(*shape):
            return torch.zeros(shape, dtype=torch.float64, device=dev)

        nf = self.n_facets
        self._t, self._wss, self._ft = rows(nf, d), rows(nf, d), rows(nf, d)
        self._acc_vec, self._acc_mag, self._acc_t = rows(nf, d), rows(nf), rows(nf, d)
        self._T = 0.0
        self.capacity = int(capacity)
        self._ring = rows(self.capacity, self.n_tags, d)
        self._times = []

    # ---- sampling ----------------------------------------------------------------------------------------------------
    @property
    def n_samples(self) -> int:
        return len(self._times)

    @property
    def times(self) -> np.ndarray:
        return np.asarray(self._times, dtype=np.float64)

    def sample(self, t: float, nu: float, dt: float = 0.0) -> None:
        """Evaluate traction, shear and forces of the solver's current ``u`` and ``p`` (and ``nut``) on the current
        stream -- no host synchronisation; ``dt > 0`` adds the sample to the statistics with weight ``dt``."""
        dt = float(dt)
        if not dt >= 0.0:
            raise ValueError(f"WallStress.sample: dt = {dt}")
        k = len(self._times)
        if k == self.capacity:  # the ring doubles (a device copy on the current stream)
            ring = torch.zeros((2 * self.capacity,) + tuple(self._ring.shape[1:]), dtype=torch.float64,
                               device=self._ring.device)
            ring[: self.capacity] = self._ring
            self._ring, self.capacity = ring, 2 * self.capacity
        S = self._solver
        Vi, Q = S._Vi[0][0], S._Q
        lib, st = _lib.load(), _lib.current_stream()
        if self.n_facets:
            _lib.check(lib.ox_wall_stress(Vi.degree, Q.degree, C.byref(S._cells), _lib.ptr(Vi.cell_dofs), _lib.ptr(Q.cell_dofs),
                                          self.n_facets, _lib.ptr(self._rec), S._U.rptr(), S._P.rptr(), _lib.ptr(S._nut),
                                          float(nu), dt, _lib.ptr(self._t), _lib.ptr(self._wss), _lib.ptr(self._ft),
                                          _lib.ptr(self._acc_vec), _lib.ptr(self._acc_mag), _lib.ptr(self._acc_t), st),
                       "ox_wall_stress")
        _lib.check(lib.ox_wall_forces(self.gdim, self.n_tags, _lib.ptr(self._tag_ptr), _lib.ptr(self._ft), self.rho,
                                      _lib.ptr(self._ring), self.capacity, k, st), "ox_wall_forces")
        self._T += dt
        self._times.append(float(t))

    def traction(self) -> torch.Tensor:
        """``t_f`` of the latest sample, (n_facets, gdim) on the device."""
        return self._t

    def wss(self) -> torch.Tensor:
        """``wss_f`` of the latest sample, (n_facets, gdim) on the device."""
        return self._wss

    def forces(self) -> np.ndarray:
        """(n_samples, n_tags, gdim) on the host: the force the fluid exerts on the facets of every tag."""
        return self._ring[: len(self._times)].cpu().numpy()

    # ---- statistics --------------------------------------------------------------------------------------------------
    @property
    def total_weight(self) -> float:
        return self._T

    def _need_weight(self):
        if not self._T > 0.0:
            raise RuntimeError("WallStress: no sample with dt > 0 has been taken since the statistics were reset")

    def tawss(self) -> torch.Tensor:
        self._need_weight()
        return self._acc_mag / self._T

    def mean_wss(self) -> torch.Tensor:
        self._need_weight()
        return self._acc_vec / self._T

    def mean_traction(self) -> torch.Tensor:
        self._need_weight()
        return self._acc_t / self._T

    def osi(self) -> torch.Tensor:
        """``0.5 (1 - |sum dt wss| / sum dt |wss|)``, 0 where the denominator is 0."""
        self._need_weight()
        v = self._acc_vec
        nrm = torch.sqrt((v * v).sum(dim=1))
        ok = self._acc_mag > 0.0
        ratio = torch.where(ok, nrm / torch.where(ok, self._acc_mag, torch.ones_like(nrm)), torch.ones_like(nrm))
        return 0.5 * (1.0 - torch.clamp(ratio, max=1.0))

    def rrt(self) -> torch.Tensor:
        """``1 / ((1 - 2 OSI) TAWSS)``, inf where the denominator is 0."""
        den = (1.0 - 2.0 * self.osi()) * self.tawss()
        ok = den > 0.0
        return torch.where(ok, 1.0 / torch.where(ok, den, torch.ones_like(den)), torch.full_like(den, float("inf")))

    def reset_statistics(self) -> None:
        for a in (self._acc_vec, self._acc_mag, self._acc_t):
            a.zero_()
        self._T = 0.0

    def save(self, path) -> None:
        out = dict(forces=self.forces(), times=self.times, facets=self.facets, facet_tags=self.facet_tags, tags=self.tags,
                   normals=self.normals, areas=self.areas, midpoints=self.midpoints, rho=self.rho,
                   traction=self._t.cpu().numpy(), wss=self._wss.cpu().numpy(), total_weight=self._T)
        if self._T > 0.0:
            out.update(tawss=self.tawss().cpu().numpy(), mean_wss=self.mean_wss().cpu().numpy(),
                       osi=self.osi().cpu().numpy(), rrt=self.rrt().cpu().numpy())
        np.savez(path, **out)
