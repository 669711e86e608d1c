"""Eddy-viscosity (LES) models, generalised-Newtonian laws and per-cell viscosities for ``FractionalStep_AB_CN(..., viscosity_model=...)``.

With a model the step's diffusion operator is ``nu K + K_nut``, ``K_nut = sum_c nut_c K_c`` (``K_c``: the stiffness
matrix of cell ``c``): the Laplacian form ``div(nut grad u)`` of a viscosity that is constant per cell (DESIGN.md
sections 4 and 14)::

    A = M/dt + C/2 + (nu K + K_nut)/2          b = (M/dt - C/2 - (nu K + K_nut)/2) u_1 + b0

The transposed term ``div(nut grad u^T)`` of the full stress ``nut (grad u + grad u^T)`` is an option of the solver:
``stress_form="laplacian"`` (the default) leaves it out, ``stress_form="full"`` subtracts it from ``b``, explicit in
``u_ab`` as Oasis does, with one row-centric vector kernel after the fused one (``ox_assemble_stress_transpose``,
DESIGN.md section 16); ``A`` stays component-decoupled::

    b[r][i] -= sum_c nut_c int_c sum_j d(u_ab)_j/dx_i d(phi_r)/dx_j

The generalised-Newtonian laws (:class:`CarreauYasuda`, :class:`Cross`, :class:`PowerLaw`) are functions of the shear rate
``gd = sqrt(2 S:S)``, ``S = sym(grad u_ab)`` at the cell centroid.  Each has a ``base_viscosity`` (its smallest value); the
kernel writes ``nut_c = nu(gd_c) - base_viscosity >= 0`` and the caller runs the step at ``nu = base_viscosity``, so
everything downstream of ``nut`` -- the fused kernel, ``eddy_viscosity()``, :class:`oasisx_amd.WallStress` -- is unchanged.

Per ``assemble_first``: one kernel writes ``nut_c`` from ``grad u_ab`` at the cell centroids (``ox_cell_viscosity``,
csrc/ox_viscosity.hip; :class:`CellViscosity` has nothing to evaluate), then the fused assembly kernel adds
``nut_c K_c`` to the convection rows it forms anyway (``ox_assemble_first`` with ``ox_first_args.nut``): no second pass over the pattern, no
second matrix.  ``Delta_c = |cell|^(1/gdim)``.

Wall damping: ``Smagorinsky(Cs, damping=VanDriest(walls))`` multiplies the length scale by
``D_c = 1 - exp(-y+_c / A_plus)``, ``y+_c = d_c u_tau,c / nu``: ``d_c`` the distance of the cell's centroid to the nearest
wall facet (:class:`oasisx_amd.geometry.WallDistance`, fixed when the solver is built) and ``u_tau,c = sqrt(|wss|)`` of that
facet, the kinematic facet-mean shear of ``u_ab`` with the molecular ``nu`` (one ``ox_wall_stress`` launch per
``assemble_first``), so that ``nut`` vanishes at the wall instead of peaking there.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

__all__ = ["Smagorinsky", "Wale", "CellViscosity", "CarreauYasuda", "Cross", "PowerLaw", "VanDriest", "DynamicSmagorinsky",
           "PatchFilter"]


def _coefficient(what, v):
    v = float(v)
    if not np.isfinite(v) or v < 0.0:
        raise ValueError(f"{what}: the model constant must be finite and >= 0 (got {v})")
    return v


def _cell_viscosity(solver, nut: torch.Tensor, *, model=0, coefficient=0.0, params=(), damping=None, cs2=None,
                    cs2_stride=0, n_coef=0, cell_bin=None, stream=None):
    """One ``ox_cell_viscosity`` launch: ``nut`` (kernel cell order) from the solver's ``u_ab`` on ``stream`` (``None``:
    torch's current stream).  The other keywords are the per-model fields of ``ox_viscosity_args`` (include/oasisx_hip.h):
    what a model does not read stays NULL / 0.  ``damping``: an ``ox_vandriest``; ``cs2``, ``cell_bin``: device addresses."""
    import ctypes as C

    Vi = solver._Vi[0][0]
    par = (C.c_double * len(params))(*params) if len(params) else None
    args = _lib.ox_viscosity_args(model, Vi.degree, _lib.ptr(Vi.cell_dofs), solver._UAB.rptr(), _lib.ptr(nut), coefficient,
                                  par, len(params), None if damping is None else C.pointer(damping), cs2, cs2_stride,
                                  n_coef, cell_bin)
    _lib.check(solver._lib.ox_cell_viscosity(C.byref(solver._cells), C.byref(args),
                                             _lib.current_stream() if stream is None else stream), "ox_cell_viscosity")


class _KernelModel:
    """A model whose ``nut`` is a function of ``grad u_ab`` at the cell centroid: evaluated by ``ox_cell_viscosity``."""

    model_id = None
    # nut is a turbulent viscosity that mixes scalars too: kappa_eff = kappa + nut / Sc_t (scalar.py)
    diffuses_scalars = True

    def check(self, gdim: int):
        pass

    def bind(self, solver):
        pass

    def evaluate(self, solver, nut: torch.Tensor, nu=None):
        _cell_viscosity(solver, nut, model=self.model_id, coefficient=self.coefficient)


class VanDriest:
    """Van Driest wall damping of the Smagorinsky length scale: ``D_c = 1 - exp(-y+_c / A_plus)``, ``y+_c = d_c u_tau,c / nu``.

    Args:
        facets: the walls -- ``None``: all exterior facets (on a ``make_periodic`` mesh without the identified faces);
            ``(meshtags, id | ids)``; an array of facet ids.  Interior facets raise ``ValueError``, as for ``WallStress``
        A_plus: the damping constant (26 in the channel-flow literature)
        u_tau: ``None``: ``sqrt(|wss|)`` of the nearest wall facet, evaluated from ``u_ab`` in every ``assemble_first``;
            a float: that constant friction velocity everywhere (no wall-stress launch)

    ``d_c`` and the nearest facet of every centroid are found once, when the solver is built."""

    def __init__(self, facets=None, A_plus: float = 26.0, u_tau=None):
        self.facets_arg = facets
        self.A_plus = float(A_plus)
        if not np.isfinite(self.A_plus) or self.A_plus <= 0.0:
            raise ValueError(f"VanDriest: A_plus must be finite and > 0 (got {A_plus})")
        self.u_tau = None if u_tau is None else float(u_tau)
        if self.u_tau is not None and (not np.isfinite(self.u_tau) or self.u_tau < 0.0):
            raise ValueError(f"VanDriest: u_tau must be finite and >= 0 (got {u_tau})")
        self.wall_distance = None
        self._nu = None

    def check(self, mesh):
        """What can be refused without the library: an empty wall selection."""
        from .wall import select_facets

        sel = select_facets(mesh, self.facets_arg, "VanDriest")
        if sel[0].shape[0] == 0:
            raise ValueError("VanDriest: the wall selection holds no facet")
        return sel

    def bind(self, solver):
        from .geometry import WallDistance
        from .wall import FacetSet

        mesh = solver._mesh
        ids, tag_of, tags = self.check(mesh)
        fs = FacetSet(solver, ids, tag_of, tags.shape[0], "VanDriest", "the friction velocity of the wall damping is")
        self.wall_distance = WallDistance(mesh, _selection=ids)
        self.facets, self.n_facets = ids, fs.n_facets
        self.cells, self.local_facets = fs.cells, fs.local_facets  # (mesh cell, opposite local vertex) per wall facet
        self._rec = fs.rec
        Vi = solver._Vi[0][0]
        lc = Vi.local_cells.to(torch.int64)
        cen = mesh.coords[mesh.cells.to(torch.int64)[lc]].mean(dim=1)
        self._dist, self._nearest = self.wall_distance.query(cen)  # kernel cell order
        d, dev = mesh.gdim, mesh.device
        self._t, self._wss, self._ft = (torch.zeros((fs.n_facets, d), dtype=torch.float64, device=dev) for _ in range(3))

    def evaluate(self, solver, coefficient: float, nut: torch.Tensor, nu):
        import ctypes as C

        if nu is None or not float(nu) > 0.0:
            raise ValueError(f"VanDriest: y+ needs the molecular viscosity (viscosity_assemble(nu), got nu = {nu})")
        nu = float(nu)
        Vi, Q = solver._Vi[0][0], solver._Q
        lib, st = solver._lib, _lib.current_stream()
        if self.u_tau is None:  # wss of u_ab with the molecular nu alone; the pressure drops out of the shear
            _lib.check(lib.ox_wall_stress(Vi.degree, Q.degree, C.byref(solver._cells), _lib.ptr(Vi.cell_dofs),
                                          _lib.ptr(Q.cell_dofs), self.n_facets, _lib.ptr(self._rec), solver._UAB.rptr(),
                                          solver._P.rptr(), None, nu, 0.0, _lib.ptr(self._t), _lib.ptr(self._wss),
                                          _lib.ptr(self._ft), None, None, None, st), "ox_wall_stress")
        vd = _lib.ox_vandriest(self._dist.data_ptr(), self._nearest.data_ptr(),
                               self._wss.data_ptr() if self.u_tau is None else None,
                               0.0 if self.u_tau is None else self.u_tau, nu, self.A_plus, self.n_facets)
        _cell_viscosity(solver, nut, model=0, coefficient=coefficient, damping=vd, stream=st)
        self._nu = nu

    def friction_velocity(self) -> torch.Tensor:
        """``u_tau`` per wall facet of the last ``assemble_first`` (the constant where one was given)."""
        if self.u_tau is not None:
            return torch.full((self.n_facets,), self.u_tau, dtype=torch.float64, device=self._dist.device)
        return torch.sqrt(torch.sqrt((self._wss * self._wss).sum(dim=1)))

    def wall_units(self, solver):
        """``(y_plus, damping)`` per cell of the last ``assemble_first``, device tensors in the MESH's cell order."""
        if self.wall_distance is None or self._nu is None:
            raise RuntimeError("VanDriest.wall_units: no assemble_first has run with this damping")
        yp_k = self._dist * self.friction_velocity()[self._nearest.to(torch.int64)] / self._nu
        lc = solver._Vi[0][0].local_cells.to(torch.int64)
        yp = torch.zeros(int(solver._mesh.num_cells), dtype=torch.float64, device=yp_k.device)
        yp[lc] = yp_k
        return yp, -torch.expm1(-yp / self.A_plus)

    def __repr__(self):
        return f"VanDriest(A_plus={self.A_plus}, u_tau={self.u_tau})"


class Smagorinsky(_KernelModel):
    """``nut_c = (Cs Delta_c)^2 sqrt(2 S:S)``, ``S = sym(grad u_ab)`` at the cell centroid.  2-D and 3-D, P1 / P2 / P3.
    ``damping``: a :class:`VanDriest` object: ``nut_c = (Cs Delta_c D_c)^2 sqrt(2 S:S)`` (the ``damping`` field);
    ``None``: the calls of the undamped model, nothing else."""

    model_id = 0

    def __init__(self, Cs: float = 0.1677, damping=None):
        self.coefficient = _coefficient("Smagorinsky", Cs)
        if damping is not None and not isinstance(damping, VanDriest):
            raise TypeError(f"Smagorinsky: damping is a VanDriest object or None (got {type(damping).__name__})")
        self.damping = damping

    def check_mesh(self, mesh):
        if self.damping is not None:
            self.damping.check(mesh)

    def bind(self, solver):
        if self.damping is not None:
            self.damping.bind(solver)

    def evaluate(self, solver, nut: torch.Tensor, nu=None):
        if self.damping is None:
            return super().evaluate(solver, nut)
        self.damping.evaluate(solver, self.coefficient, nut, nu)

    def __repr__(self):
        if self.damping is not None:
            return f"Smagorinsky(Cs={self.coefficient}, damping={self.damping!r})"
        return f"Smagorinsky(Cs={self.coefficient})"


class _Patches:
    """The vertex patches of a solver's mesh for the test filter: the vertex -> cell CSR over vertex CLASSES (on a
    ``make_periodic`` mesh the patches wrap around the seam), cells in the kernels' order and ascending within a vertex,
    and the cell -> vertex-class table.  Built once with torch, validated on the host before any launch."""

    def __init__(self, solver, who):
        mesh = solver._mesh
        Vi = solver._Vi[0][0]
        dev = solver._geom.device
        lc = Vi.local_cells.to(torch.int64).to(dev)
        self.n_cells = nc = int(solver._geom.shape[0])
        self.gdim = d = int(mesh.gdim)
        per = getattr(mesh, "periodic", None)
        self.n_vertices = nv = int(per.n_free_vertices) if per is not None else int(mesh.coords.shape[0])
        cv = mesh.topological_cells().to(dev).to(torch.int64)[lc]  # (nc, d + 1), kernel cell order
        if int(lc.shape[0]) != nc or nc * (d + 1) > 0x7FFFFFFF or nv > 0x7FFFFFFF:
            raise RuntimeError(f"{who}: {nc} cells, {nv} vertices do not fit the filter's int32 tables")
        flat = cv.reshape(-1)
        cell = torch.arange(nc, device=dev).repeat_interleave(d + 1)
        perm = torch.sort(flat, stable=True).indices  # stable: ascending cell id within a vertex
        count = torch.bincount(flat, minlength=nv)
        ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(count, 0)])
        idx = cell[perm]
        # the host check: monotone pointer, every index below n_cells, every vertex with at least one cell
        lo, hi, cmin, total = (int(v) for v in torch.stack([idx.min(), idx.max(), count.min(), ptr[-1]]).tolist())
        if int(flat.min()) < 0 or int(flat.max()) >= nv or int(count.shape[0]) != nv:
            raise ValueError(f"{who}: a cell names a vertex outside 0 .. {nv - 1}")
        if cmin < 1:
            raise ValueError(f"{who}: vertex {int(torch.argmin(count))} belongs to no cell (the test filter has no patch there)")
        if lo < 0 or hi >= nc or total != nc * (d + 1) or not bool((ptr[1:] > ptr[:-1]).all()):
            raise RuntimeError(f"{who}: the vertex -> cell table is inconsistent ({total} entries, cells {lo} .. {hi})")
        self.ptr, self.idx = ptr.to(torch.int32).contiguous(), idx.to(torch.int32).contiguous()
        self.cell_verts = cv.to(torch.int32).contiguous()
        self.n_idx = total
        self.max_patch = int(count.max())
        self.local_cells = lc


class PatchFilter:
    """The test filter of the dynamic procedure, the vertex-patch top hat, for per-cell data::

        q_v  = sum_{c in patch(v)} |c| q_c / sum_{c in patch(v)} |c|      q^_c = mean of q_v over the cell's vertices

    Vertices are mesh vertices (vertex classes on a periodic mesh), so the filter is the same for P1 / P2 / P3; boundary
    patches are one-sided; constants are preserved and the weights are positive.  ``apply(q)`` takes a device tensor
    ``(num_cells,)`` or ``(num_cells, k)`` in the MESH's cell order and returns the filtered tensor of the same shape:
    two launches (``ox_patch_filter_vertices``, ``ox_patch_filter_cells``), the ones ``average="local"`` runs.
    ``k = 1`` and ``k = 2`` are instantiated."""

    def __init__(self, solver, _patches=None):
        comm = getattr(solver._mesh, "comm", None)
        if comm is not None and getattr(comm, "size", 1) > 1:
            raise NotImplementedError("PatchFilter on a mesh partition (comm.size > 1): the patches are built for one GPU")
        self._solver = solver
        self._p = _patches if _patches is not None else _Patches(solver, "PatchFilter")
        p = self._p
        dev = solver._geom.device
        # |c| in kernel cell order, as the kernels form it from |det J|
        d = p.gdim
        adet = solver._geom[:, d * d]
        self._vol = (0.5 * adet if d == 2 else adet * (1.0 / 6.0)).contiguous()
        self._qv = torch.zeros((p.n_vertices, 2), dtype=torch.float64, device=dev)

    def _launch(self, k, q, out, vol=None, vol_stride=1):
        """q, out: (n_cells, k) contiguous, kernel cell order."""
        p, lib, st = self._p, self._solver._lib, _lib.current_stream()
        vol = _lib.ptr(self._vol) if vol is None else vol  # (or the address of the |c| column of the cell records)
        _lib.check(lib.ox_patch_filter_vertices(k, p.n_vertices, _lib.ptr(p.ptr), _lib.ptr(p.idx), p.n_cells, p.n_idx,
                                                _lib.ptr(q), vol, vol_stride, _lib.ptr(self._qv), st),
                   "ox_patch_filter_vertices")
        _lib.check(lib.ox_patch_filter_cells(k, p.gdim, p.n_cells, _lib.ptr(p.cell_verts), p.n_vertices, _lib.ptr(self._qv),
                                             _lib.ptr(out), st), "ox_patch_filter_cells")

    def apply(self, q: torch.Tensor) -> torch.Tensor:
        p = self._p
        nc_mesh = int(self._solver._mesh.num_cells)
        if not torch.is_tensor(q) or q.dtype != torch.float64 or q.dim() not in (1, 2) or int(q.shape[0]) != nc_mesh:
            raise ValueError(f"PatchFilter.apply: a float64 tensor ({nc_mesh},) or ({nc_mesh}, k) in the mesh's cell order is "
                             "expected")
        k = 1 if q.dim() == 1 else int(q.shape[1])
        if k not in (1, 2):
            raise NotImplementedError(f"PatchFilter.apply: k = {k} (k = 1 and k = 2 are instantiated)")
        qk = q.to(self._vol.device).reshape(nc_mesh, k)[p.local_cells].contiguous()
        out = torch.empty_like(qk)
        self._launch(k, qk, out)
        res = torch.zeros((nc_mesh, k), dtype=torch.float64, device=out.device)
        res[p.local_cells] = out
        return res.reshape(q.shape)


class DynamicSmagorinsky(_KernelModel):
    """The dynamic Smagorinsky model (Germano et al. 1991, Lilly 1992): ``nut_c = Cs2_c Delta_c^2 sqrt(2 S:S)`` with
    ``Cs2 = -(1/2) <Ld:M> / <M:M>`` from the step's ``u_ab``, clipped to ``[0, cs2_max]`` (0 where ``<M:M>`` is not
    positive); ``L = (u u^T)^ - u^ u^^T``, ``M = filter_ratio^2 Delta^2 |S^| S^ - (Delta^2 |S| S)^`` with the vertex-patch
    test filter ``^`` of :class:`PatchFilter`.  2-D and 3-D, P1 / P2 / P3.

    Args:
        average: ``"global"``: ``<.>`` sums ``|c| .`` over all cells, or over the cells of each bin where ``axis=`` /
            ``cell_bins=`` is given; ``"local"``: ``<.>`` is the test filter applied once more, a coefficient per cell
        axis, edges, tol: bins as ``slab_bins(mesh, axis, edges, tol)``
        cell_bins: bins as for ``ProfileStatistics`` (mesh cell order; -1: the cell gets ``Cs2 = 0``)
        filter_ratio: test-filter width over grid-filter width (> 1)
        cs2_max: the upper clip of ``Cs2`` (>= 0)
        update_every: ``Cs2`` is recomputed in the first ``assemble_first`` and every n-th after it; ``nut`` is recomputed
            from the stored ``Cs2`` in every step

    ``average="lagrangian"`` (Meneveau, Lund & Cabot 1996): ``Cs2 = F_LM / F_MM`` of two fields kept per
    vertex class, the averages of ``-2 (Ld:M)_v`` and ``4 (M:M)_v`` along the path lines with an exponentially fading
    memory: every update traces ``x_v - h u_v`` back (``h = update_every dt``, ``u_v`` the patch-mean ``u_ab``),
    interpolates the old fields there and relaxes them towards the sources with ``eps = (h/T) / (1 + h/T)``,
    ``T = time_scale Delta_v (F_LM F_MM)^(-1/8)`` (``ox_dynamic_lagrangian``).  Needs no homogeneous direction and has a
    memory: the model must be given ``dt`` (``assemble_first`` hands it on), and ``save`` / ``load`` carry the fields over
    a restart.

        cs2_initial: ``F_LM = cs2_initial F_MM`` in the first update (finite, >= 0)
        time_scale: the constant of the relaxation time ``T`` (1.5 in the paper; finite, > 0)
        cs2_floor: ``F_LM >= cs2_floor F_MM`` after every update, so that ``T`` stays finite (in ``[0, cs2_max]``)
    """

    model_id = 0
    damping = None
    AVERAGES = ("global", "local", "lagrangian")

    def __init__(self, average="global", axis=None, edges=None, cell_bins=None, filter_ratio=2.0, cs2_max=0.09,
                 update_every=1, tol=None, cs2_initial=0.0256, time_scale=1.5, cs2_floor=1e-24):
        if average not in self.AVERAGES:
            raise ValueError(f'DynamicSmagorinsky: average is "global", "local" or "lagrangian" (got {average!r})')
        if axis is not None and cell_bins is not None:
            raise ValueError("DynamicSmagorinsky: give at most one of axis= (with optional edges=) and cell_bins=")
        if average != "global" and (axis is not None or edges is not None or cell_bins is not None):
            raise ValueError(f'DynamicSmagorinsky: average="{average}" takes no bins (axis= / edges= / cell_bins= belong to '
                             '"global")')
        if edges is not None and axis is None:
            raise ValueError("DynamicSmagorinsky: edges= belongs to axis=")
        self.average = average
        self.axis = None if axis is None else int(axis)
        self.edges_arg, self.tol = edges, tol
        self.cell_bins_arg = cell_bins
        self.filter_ratio = float(filter_ratio)
        if not np.isfinite(self.filter_ratio) or self.filter_ratio <= 1.0:
            raise ValueError(f"DynamicSmagorinsky: filter_ratio must be finite and > 1 (got {filter_ratio})")
        self.cs2_max = float(cs2_max)
        if not np.isfinite(self.cs2_max) or self.cs2_max < 0.0:
            raise ValueError(f"DynamicSmagorinsky: cs2_max must be finite and >= 0 (got {cs2_max})")
        if int(update_every) != update_every or int(update_every) < 1:
            raise ValueError(f"DynamicSmagorinsky: update_every must be an integer >= 1 (got {update_every})")
        self.update_every = int(update_every)
        self.cs2_initial, self.time_scale, self.cs2_floor = float(cs2_initial), float(time_scale), float(cs2_floor)
        if not np.isfinite(self.cs2_initial) or self.cs2_initial < 0.0:
            raise ValueError(f"DynamicSmagorinsky: cs2_initial must be finite and >= 0 (got {cs2_initial})")
        if not np.isfinite(self.time_scale) or self.time_scale <= 0.0:
            raise ValueError(f"DynamicSmagorinsky: time_scale must be finite and > 0 (got {time_scale})")
        if not 0.0 <= self.cs2_floor <= self.cs2_max:
            raise ValueError(f"DynamicSmagorinsky: cs2_floor must lie in [0, cs2_max = {self.cs2_max}] (got {cs2_floor})")
        self.edges = None
        self.n_bins = None
        self.n_evaluations = 0  # assemble_first calls seen
        self.n_updates = 0      # of which recomputed Cs2
        self._patches = None

    # ---- what can be refused without the library
    def _bins_of(self, mesh):
        """(bins in mesh cell order or None, n_bins)."""
        nc = int(mesh.num_cells)
        if self.average != "global":
            return None, 0
        if self.axis is not None:
            from .diagnostics import slab_bins

            bins, self.edges = slab_bins(mesh, self.axis, self.edges_arg, self.tol)
        elif self.cell_bins_arg is not None:
            cb = self.cell_bins_arg
            bins = np.asarray(cb.cpu().numpy() if torch.is_tensor(cb) else cb)
            if bins.shape != (nc,) or not np.issubdtype(bins.dtype, np.integer):
                raise ValueError(f"DynamicSmagorinsky: cell_bins must be {nc} integers in the mesh's cell order")
            bins = bins.astype(np.int64)
            if bins.min() < -1 or bins.max() < 0:
                raise ValueError("DynamicSmagorinsky: cell_bins holds values below -1, or no cell is in a bin")
        else:
            bins = np.zeros(nc, dtype=np.int64)
        nb = int(bins.max()) + 1
        count = np.bincount(bins[bins >= 0], minlength=nb)
        if (count == 0).any():
            raise ValueError(f"DynamicSmagorinsky: bin {int(np.argmax(count == 0))} holds no cell")
        return bins, nb

    def check_mesh(self, mesh):
        self._bins_of(mesh)

    def bind(self, solver):
        from .diagnostics import bin_chunk_plan

        mesh = solver._mesh
        dev = solver._geom.device
        self._patches = p = _Patches(solver, "DynamicSmagorinsky")
        d, nc = p.gdim, p.n_cells
        ns = d * (d + 1) // 2
        self._nr, self._nm = d + ns + 2, d + 3 * ns
        f64 = dict(dtype=torch.float64, device=dev)
        self._rec = torch.zeros((nc, self._nr), **f64)
        self._mom = torch.zeros((p.n_vertices, self._nm), **f64)
        self._lm = torch.zeros((nc, 2), **f64)
        bins, nb = self._bins_of(mesh)
        self.n_bins = nb
        if self.average == "local":
            self._filter = PatchFilter(solver, _patches=p)
            self._lmf = torch.zeros((nc, 2), **f64)
            self._cs2 = torch.zeros(nc, **f64)
        elif self.average == "lagrangian":
            self._bind_lagrangian(solver)
        else:
            plan = bin_chunk_plan(torch.from_numpy(bins).to(dev), p.local_cells, nc, nb, "DynamicSmagorinsky")
            self._plan = plan
            self._cell_bin = plan["bins_kernel"].to(torch.int32).contiguous()
            self._partials = torch.zeros((plan["n_chunks"], 2), **f64)
            self._bins = torch.zeros((nb, 4), **f64)  # {sum |c| LM, sum |c| MM, Cs2 unclipped, Cs2 clipped}
        self.n_evaluations = self.n_updates = 0

    @property
    def needs_dt(self) -> bool:
        """``viscosity_assemble`` hands ``dt`` to a model that says so: the Lagrangian average traces back over it."""
        return self.average == "lagrangian"

    def _bind_lagrangian(self, solver):
        """The whole-mesh locator of the tracers, the master vertex of every class, ``Delta_v`` and the two field pairs."""
        from . import geometry as G

        mesh, p = solver._mesh, self._patches
        Vi = solver._Vi[0][0]
        dev = solver._geom.device
        d, nv, nc = p.gdim, p.n_vertices, p.n_cells
        f64 = dict(dtype=torch.float64, device=dev)
        self._loc_tol = G.DEFAULT_TOL
        self._tree = G.space_tree(Vi, self._loc_tol)
        self._cell_inv = G.kernel_position_table(Vi)
        per = getattr(mesh, "periodic", None)
        coords = mesh.coords.to(dev)
        self._periodic = [0, 0, 0]
        self._lo, self._hi, self._period = [0.0] * 3, [0.0] * 3, [0.0] * 3
        if per is None:
            self._xv = coords.contiguous()
        else:
            vm = np.asarray(per.vertex_master)
            free = np.nonzero(vm == np.arange(vm.shape[0]))[0]  # ascending master id: the order of the classes
            self._xv = coords[torch.from_numpy(free).to(dev)].contiguous()
            for k in per.axes:
                self._periodic[k] = 1
                self._lo[k], self._hi[k], self._period[k] = float(per.lo[k]), float(per.hi[k]), float(per.period[k])
        if tuple(self._xv.shape) != (nv, d):
            raise RuntimeError(f"DynamicSmagorinsky: {tuple(self._xv.shape)} master-vertex coordinates for {nv} vertex classes")
        # the hint: the first cell of every patch, as a mesh cell id (the locator's numbering)
        first = p.idx.to(torch.int64)[p.ptr[:-1].to(torch.int64)]
        self._hint = p.local_cells[first].contiguous()
        lib, st = solver._lib, _lib.current_stream()
        adet = solver._geom[:, d * d]
        vol = (0.5 * adet if d == 2 else adet * (1.0 / 6.0)).contiguous()  # |c| as the kernels form it from |det J|
        vv = torch.zeros(nv, **f64)
        _lib.check(lib.ox_patch_filter_vertices(1, nv, _lib.ptr(p.ptr), _lib.ptr(p.idx), nc, p.n_idx, _lib.ptr(vol),
                                                _lib.ptr(vol), 1, _lib.ptr(vv), st), "ox_patch_filter_vertices")
        self._delta_v = torch.pow(vv, 1.0 / d).contiguous()
        self._src = torch.zeros((nv, 2), **f64)               # {(LM)_v, (MM)_v}
        self._f = [torch.zeros((nv, 2), **f64) for _ in range(2)]  # {F_LM, F_MM}: the current pair is _f[_cur]
        self._cur = 0
        self._cs2v = torch.zeros(nv, **f64)
        self._status = torch.zeros(nv, dtype=torch.int32, device=dev)
        self._cs2 = torch.zeros(nc, **f64)

    def _update_lagrangian(self, solver, vol, dt):
        """Launches 4 to 6 of the Lagrangian update: the sources per vertex, the back-trace and relaxation, ``Cs2`` per cell."""
        import ctypes as C

        p, lib, st = self._patches, solver._lib, _lib.current_stream()
        h = self.update_every * float(dt)
        _lib.check(lib.ox_patch_filter_vertices(2, p.n_vertices, _lib.ptr(p.ptr), _lib.ptr(p.idx), p.n_cells, p.n_idx,
                                                _lib.ptr(self._lm), vol, self._nr, _lib.ptr(self._src), st),
                   "ox_patch_filter_vertices")
        old, new = self._f[self._cur], self._f[1 - self._cur]
        args = self.lagrangian_args(h, self.n_updates == 0, self._mom, self._nm, self._src, old, new, self._cs2v, self._status)
        _lib.check(lib.ox_dynamic_lagrangian(C.byref(args), st), "ox_dynamic_lagrangian")
        self._cur = 1 - self._cur
        _lib.check(lib.ox_patch_filter_cells(1, p.gdim, p.n_cells, _lib.ptr(p.cell_verts), p.n_vertices,
                                             _lib.ptr(self._cs2v), _lib.ptr(self._cs2), st), "ox_patch_filter_cells")

    def lagrangian_args(self, h, first, u, u_stride, src, f_old, f_new, cs2v, status):
        """The argument block of ``ox_dynamic_lagrangian`` on this model's tables, for the given device tensors."""
        p = self._patches
        A3, I3 = _lib.C.c_double * 3, _lib.C.c_int * 3
        return _lib.ox_lagrangian_args(
            self._tree._h, p.gdim, int(bool(first)), p.n_vertices, _lib.ptr(self._xv), _lib.ptr(u), int(u_stride),
            _lib.ptr(self._hint), _lib.ptr(self._cell_inv), int(self._cell_inv.shape[0]), _lib.ptr(p.cell_verts), p.n_cells,
            _lib.ptr(src), _lib.ptr(self._delta_v), _lib.ptr(f_old), _lib.ptr(f_new), _lib.ptr(cs2v), _lib.ptr(status),
            float(h), self.time_scale, self.cs2_floor, self.cs2_max, self.cs2_initial, self._loc_tol,
            I3(*self._periodic), A3(*self._lo), A3(*self._hi), A3(*self._period))

    # ---- per assemble_first
    def update_coefficient(self, solver, dt=None):
        """The launches that recompute ``Cs2`` from the solver's ``u_ab``."""
        import ctypes as C

        p, lib, st = self._patches, solver._lib, _lib.current_stream()
        Vi = solver._Vi[0][0]
        _lib.check(lib.ox_dynamic_cells(Vi.degree, C.byref(solver._cells), _lib.ptr(Vi.cell_dofs), solver._UAB.rptr(),
                                        _lib.ptr(self._rec), st), "ox_dynamic_cells")
        _lib.check(lib.ox_dynamic_vertices(p.gdim, p.n_vertices, _lib.ptr(p.ptr), _lib.ptr(p.idx), p.n_cells,
                                           _lib.ptr(self._rec), _lib.ptr(self._mom), st), "ox_dynamic_vertices")
        _lib.check(lib.ox_dynamic_products(p.gdim, p.n_cells, _lib.ptr(p.cell_verts), p.n_vertices, _lib.ptr(self._rec),
                                           _lib.ptr(self._mom), self.filter_ratio, _lib.ptr(self._lm), st),
                   "ox_dynamic_products")
        vol = C.c_void_p(self._rec.data_ptr() + 8 * (self._nr - 1))  # |c|: the last column of the cell records
        if self.average == "local":
            self._filter._launch(2, self._lm, self._lmf, vol=vol, vol_stride=self._nr)
            _lib.check(lib.ox_dynamic_clip(p.n_cells, _lib.ptr(self._lmf), self.cs2_max, _lib.ptr(self._cs2), st),
                       "ox_dynamic_clip")
        elif self.average == "lagrangian":
            self._update_lagrangian(solver, vol, dt)
        else:
            pl = self._plan
            _lib.check(lib.ox_dynamic_bin_sums(p.n_cells, _lib.ptr(self._lm), vol, self._nr, _lib.ptr(pl["order"]),
                                               _lib.ptr(pl["chunks"]), pl["n_chunks"], _lib.ptr(self._partials), st),
                       "ox_dynamic_bin_sums")
            _lib.check(lib.ox_dynamic_bin_coefficients(self.n_bins, _lib.ptr(pl["bin_chunk_ptr"]), _lib.ptr(self._partials),
                                                       self.cs2_max, _lib.ptr(self._bins), st),
                       "ox_dynamic_bin_coefficients")
        self.n_updates += 1

    def evaluate(self, solver, nut: torch.Tensor, nu=None, dt=None):
        import ctypes as C

        if self._patches is None:
            raise RuntimeError("DynamicSmagorinsky: the model is not bound to a solver")
        if self.average == "lagrangian":
            if dt is None or not np.isfinite(float(dt)) or float(dt) < 0.0:
                raise ValueError('DynamicSmagorinsky: average="lagrangian" traces the path lines back over the step: '
                                 f"viscosity_assemble(nu, dt) with a finite dt >= 0 (got dt = {dt})")
        if self.n_evaluations % self.update_every == 0:
            self.update_coefficient(solver, dt)
        self.n_evaluations += 1
        if self.average != "global":
            cs2, stride, n, cb = _lib.ptr(self._cs2), 1, self._patches.n_cells, None
        else:
            cs2, stride, n, cb = C.c_void_p(self._bins.data_ptr() + 8 * 3), 4, self.n_bins, _lib.ptr(self._cell_bin)
        _cell_viscosity(solver, nut, model=0, cs2=cs2, cs2_stride=stride, n_coef=n, cell_bin=cb)

    # ---- accessors
    def _need(self, what):
        if self._patches is None or self.n_updates == 0:
            raise RuntimeError(f"DynamicSmagorinsky.{what}: no assemble_first has run with this model")

    def _to_mesh_order(self, t):
        lc = self._patches.local_cells
        out = torch.zeros((int(lc.max()) + 1,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        out[lc] = t
        return out

    def coefficient_cells(self, solver=None) -> torch.Tensor:
        """``Cs2`` per cell (clipped), device tensor in the MESH's cell order."""
        self._need("coefficient_cells")
        if self.average != "global":
            ck = self._cs2
        else:
            cb = self._cell_bin.to(torch.int64)
            ck = torch.where(cb >= 0, self._bins[:, 3][cb.clamp_min(0)], torch.zeros_like(self._bins[:1, 3]))
        nc_mesh = int(solver._mesh.num_cells) if solver is not None else int(self._patches.local_cells.max()) + 1
        out = torch.zeros(nc_mesh, dtype=torch.float64, device=ck.device)
        out[self._patches.local_cells] = ck
        return out

    def bin_coefficients(self, clipped=True) -> torch.Tensor:
        """``Cs2`` per bin (length 1 for the global average), clipped or as the ratio stands."""
        self._need("bin_coefficients")
        if self.average != "global":
            raise RuntimeError(f'DynamicSmagorinsky.bin_coefficients: average="{self.average}" has a coefficient per cell')
        return self._bins[:, 3 if clipped else 2].clone()

    def bin_sums(self) -> torch.Tensor:
        """``(sum |c| LM, sum |c| MM)`` per bin, shape ``(n_bins, 2)``."""
        self._need("bin_sums")
        if self.average != "global":
            raise RuntimeError(f'DynamicSmagorinsky.bin_sums: average="{self.average}" has no bins')
        return self._bins[:, :2].clone()

    def products(self):
        """``(LM, MM)`` per cell, ``Ld:M`` and ``M:M``, device tensors in the MESH's cell order."""
        self._need("products")
        both = self._to_mesh_order(self._lm)
        return both[:, 0].contiguous(), both[:, 1].contiguous()

    # ---- the Lagrangian average: its fields, and their way over a restart
    def _need_lagrangian(self, what, updated=True):
        if self.average != "lagrangian":
            raise RuntimeError(f'DynamicSmagorinsky.{what}: average="{self.average}" keeps no fields along path lines')
        if self._patches is None or (updated and self.n_updates == 0):
            raise RuntimeError(f"DynamicSmagorinsky.{what}: no assemble_first has run with this model")

    def lagrangian_fields(self):
        """``(F_LM, F_MM)`` per vertex class (on a periodic mesh: per class of identified vertices), device tensors."""
        self._need_lagrangian("lagrangian_fields")
        f = self._f[self._cur]
        return f[:, 0].contiguous(), f[:, 1].contiguous()

    def vertex_coefficients(self) -> torch.Tensor:
        """``Cs2_v = F_LM / F_MM`` per vertex class, clipped to ``[0, cs2_max]``."""
        self._need_lagrangian("vertex_coefficients")
        return self._cs2v.clone()

    def backtrace_status(self) -> torch.Tensor:
        """int32 per vertex class of the last update: 0 a cell was found, 1 the path line left the mesh (the vertex kept
        its own old value), 2 a non-finite departure point or an index out of range (NaN)."""
        self._need_lagrangian("backtrace_status")
        return self._status.clone()

    def save(self, path) -> None:
        """The two fields, the coefficients and the counters as an ``.npz``: what a restarted run needs to go on bit for bit."""
        self._need_lagrangian("save", updated=False)
        f = self._f[self._cur]
        np.savez(path, fields=f.cpu().numpy(), cs2_vertices=self._cs2v.cpu().numpy(), cs2_cells=self._cs2.cpu().numpy(),
                 status=self._status.cpu().numpy(), n_evaluations=np.int64(self.n_evaluations),
                 n_updates=np.int64(self.n_updates), update_every=np.int64(self.update_every))

    def load(self, path) -> None:
        """What ``save`` wrote, into this model (bound to a solver on the same mesh, with the same ``update_every``)."""
        self._need_lagrangian("load", updated=False)
        with np.load(path) as z:
            f, cv, cc, st = z["fields"], z["cs2_vertices"], z["cs2_cells"], z["status"]
            nv, nc = self._patches.n_vertices, self._patches.n_cells
            if f.shape != (nv, 2) or cv.shape != (nv,) or cc.shape != (nc,) or st.shape != (nv,):
                raise ValueError(f"DynamicSmagorinsky.load: saved for {f.shape[0]} vertex classes and {cc.shape[0]} cells; the "
                                 f"solver has {nv} and {nc}")
            if int(z["update_every"]) != self.update_every:
                raise ValueError(f"DynamicSmagorinsky.load: saved with update_every = {int(z['update_every'])}, the model "
                                 f"has {self.update_every}")
            dev = self._cs2.device
            self._f[self._cur].copy_(torch.from_numpy(np.ascontiguousarray(f)).to(dev))
            self._cs2v.copy_(torch.from_numpy(np.ascontiguousarray(cv)).to(dev))
            self._cs2.copy_(torch.from_numpy(np.ascontiguousarray(cc)).to(dev))
            self._status.copy_(torch.from_numpy(np.ascontiguousarray(st)).to(dev))
            self.n_evaluations, self.n_updates = int(z["n_evaluations"]), int(z["n_updates"])

    def __repr__(self):
        if self.average == "lagrangian":
            return (f"DynamicSmagorinsky(lagrangian, filter_ratio={self.filter_ratio}, cs2_max={self.cs2_max}, "
                    f"update_every={self.update_every}, cs2_initial={self.cs2_initial}, time_scale={self.time_scale}, "
                    f"cs2_floor={self.cs2_floor})")
        where = self.average if self.axis is None and self.cell_bins_arg is None else (
            f"axis={self.axis}" if self.axis is not None else "cell_bins")
        return (f"DynamicSmagorinsky({where}, filter_ratio={self.filter_ratio}, cs2_max={self.cs2_max}, "
                f"update_every={self.update_every})")


class Wale(_KernelModel):
    """Wall-adapting local eddy viscosity (Nicoud & Ducros 1999), 3-D only.  With ``g = grad u_ab`` at the centroid,
    ``Sd = sym(g g) - tr(g g)/3 I``::

        nut_c = (Cw Delta_c)^2 (Sd:Sd)^(3/2) / ((S:S)^(5/2) + (Sd:Sd)^(5/4))        (0 where the denominator is 0)
    """

    model_id = 1

    def __init__(self, Cw: float = 0.325, damping=None):
        self.coefficient = _coefficient("Wale", Cw)
        if damping is not None:
            raise ValueError("Wale: wall damping is refused -- the model's operator vanishes at a wall by construction "
                             "(nut ~ y^3); damping= belongs to Smagorinsky")

    def check(self, gdim: int):
        if gdim != 3:
            raise ValueError(f"Wale: the model is defined for three-dimensional flow (the mesh has gdim = {gdim})")

    def __repr__(self):
        return f"Wale(Cw={self.coefficient})"


def _law_parameter(what, name, v, positive=False):
    v = float(v)
    if not np.isfinite(v):
        raise ValueError(f"{what}: {name} must be finite (got {v})")
    if positive and v <= 0.0:
        raise ValueError(f"{what}: {name} must be > 0 (got {v})")
    if not positive and v < 0.0:
        raise ValueError(f"{what}: {name} must be >= 0 (got {v})")
    return v


class _LawModel(_KernelModel):
    """A generalised-Newtonian law ``nu(gd)``, ``gd = sqrt(2 S:S)`` at the cell centroid: ``nut_c = nu(gd_c) -
    base_viscosity`` (models 2-4).  ``params``: the law's parameters in the order of include/oasisx_hip.h."""

    base_viscosity = None
    params = ()
    # nut = nu(gd) - base_viscosity is a property of the fluid's momentum, not a mixing of scalars
    diffuses_scalars = False

    def evaluate(self, solver, nut: torch.Tensor, nu=None):
        _cell_viscosity(solver, nut, model=self.model_id, params=self.params)


class CarreauYasuda(_LawModel):
    """``nu(gd) = nu_inf + (nu0 - nu_inf) (1 + (lam gd)^a)^((n - 1)/a)``; ``a = 2``: the Carreau law.
    ``base_viscosity = min(nu0, nu_inf)``.  2-D and 3-D, P1 / P2 / P3."""

    model_id = 2

    def __init__(self, nu0: float, nu_inf: float, lam: float, n: float, a: float = 2.0):
        w = "CarreauYasuda"
        self.nu0, self.nu_inf = _law_parameter(w, "nu0", nu0), _law_parameter(w, "nu_inf", nu_inf)
        self.lam = _law_parameter(w, "lam", lam)
        self.n, self.a = _law_parameter(w, "n", n, positive=True), _law_parameter(w, "a", a, positive=True)
        self.params = (self.nu0, self.nu_inf, self.lam, self.n, self.a)
        self.base_viscosity = min(self.nu0, self.nu_inf)

    def __repr__(self):
        return f"CarreauYasuda(nu0={self.nu0}, nu_inf={self.nu_inf}, lam={self.lam}, n={self.n}, a={self.a})"


class Cross(_LawModel):
    """``nu(gd) = nu_inf + (nu0 - nu_inf) / (1 + (lam gd)^m)``.  ``base_viscosity = min(nu0, nu_inf)``."""

    model_id = 3

    def __init__(self, nu0: float, nu_inf: float, lam: float, m: float):
        w = "Cross"
        self.nu0, self.nu_inf = _law_parameter(w, "nu0", nu0), _law_parameter(w, "nu_inf", nu_inf)
        self.lam, self.m = _law_parameter(w, "lam", lam), _law_parameter(w, "m", m, positive=True)
        self.params = (self.nu0, self.nu_inf, self.lam, self.m)
        self.base_viscosity = min(self.nu0, self.nu_inf)

    def __repr__(self):
        return f"Cross(nu0={self.nu0}, nu_inf={self.nu_inf}, lam={self.lam}, m={self.m})"


class PowerLaw(_LawModel):
    """``nu(gd) = min(max(k gd^(n - 1), nu_min), nu_max)``; at ``gd == 0``: ``nu_max`` for ``n < 1``, ``nu_min`` for
    ``n > 1``, the clipped ``k`` for ``n == 1``.  ``base_viscosity = nu_min`` (> 0: the step needs a viscosity)."""

    model_id = 4

    def __init__(self, k: float, n: float, nu_min: float, nu_max: float):
        w = "PowerLaw"
        self.k, self.n = _law_parameter(w, "k", k), _law_parameter(w, "n", n, positive=True)
        self.nu_min = _law_parameter(w, "nu_min", nu_min, positive=True)
        self.nu_max = _law_parameter(w, "nu_max", nu_max)
        if self.nu_min > self.nu_max:
            raise ValueError(f"PowerLaw: nu_min = {self.nu_min} > nu_max = {self.nu_max}")
        self.params = (self.k, self.n, self.nu_min, self.nu_max)
        self.base_viscosity = self.nu_min

    def __repr__(self):
        return f"PowerLaw(k={self.k}, n={self.n}, nu_min={self.nu_min}, nu_max={self.nu_max})"


class CellViscosity:
    """A fixed, non-negative additional viscosity per cell (sponge layers in front of outlets; a way to test the
    operator without a turbulence model).

    Args:
        value: a float, a callable ``f(x)`` on the cell centroids (``x: (3, ncells)``, the mesh's cell order) or an array
            of ``ncells`` values in the mesh's cell order.  Evaluated once, when the solver is built.
    """

    model_id = None
    diffuses_scalars = True

    def __init__(self, value):
        if callable(value):
            self.value = value
        elif np.ndim(value) == 0:
            self.value = float(value)
            self._check_values(np.asarray([self.value]))
        else:
            self.value = np.array(torch.as_tensor(value).detach().cpu().numpy(), dtype=np.float64).reshape(-1)
            self._check_values(self.value)
        self._kernel_order = None

    @staticmethod
    def _check_values(v):
        if not np.isfinite(v).all() or (v < 0.0).any():
            raise ValueError("CellViscosity: the values must be finite and >= 0 "
                             f"(min {float(np.min(v))}): a negative viscosity makes the step ill-posed")

    def values(self, mesh) -> np.ndarray:
        """The ``mesh.num_cells`` values in the mesh's cell order."""
        nc = int(mesh.num_cells)
        if callable(self.value):
            gdim = mesh.geometry.dim
            cen = mesh.coords[mesh.cells.to(torch.int64)].mean(dim=1).cpu().numpy()  # (nc, gdim)
            X = np.zeros((3, nc))
            X[:gdim] = cen.T
            v = np.broadcast_to(np.asarray(self.value(X), dtype=np.float64), (nc,)).copy()
        elif isinstance(self.value, float):
            v = np.full(nc, self.value)
        else:
            v = self.value
            if v.shape[0] != nc:
                raise ValueError(f"CellViscosity: {v.shape[0]} values for a mesh of {nc} cells")
        self._check_values(v)
        return v

    def check(self, gdim: int):
        pass

    def bind(self, solver):
        Vi = solver._Vi[0][0]
        v = torch.from_numpy(self.values(solver._mesh)).to(solver._mesh.device)
        self._kernel_order = v[Vi.local_cells.to(torch.int64)].contiguous()

    def evaluate(self, solver, nut: torch.Tensor, nu=None):
        nut.copy_(self._kernel_order)

    def __repr__(self):
        return f"CellViscosity({self.value!r})"


def check_model(model, mesh, rotational: bool, scalars) -> None:
    """The scope guards of ``viscosity_model=``; run before anything is built (and before the HIP library is loaded)."""
    if not isinstance(model, (_KernelModel, CellViscosity)):
        raise TypeError("viscosity_model: a Smagorinsky, DynamicSmagorinsky, Wale, CarreauYasuda, Cross, PowerLaw or "
                        "CellViscosity object is expected "
                        f"(got {type(model).__name__})")
    if rotational:
        raise NotImplementedError("viscosity_model with rotational=True: the xi nu div(u) term of the rotational pressure "
                                  "update is derived for a constant viscosity")
    if scalars:
        from .scalar import check_turbulent_schmidt

        check_turbulent_schmidt(model, scalars)
    comm = getattr(mesh, "comm", None)
    if comm is not None and getattr(comm, "size", 1) > 1:
        raise NotImplementedError("viscosity_model on a mesh partition (comm.size > 1): the per-cell viscosity is built for "
                                  "one GPU")
    model.check(mesh.geometry.dim)
    if getattr(model, "damping", None) is not None:
        model.check_mesh(mesh)  # an empty wall selection fails here
    if isinstance(model, DynamicSmagorinsky):
        model.check_mesh(mesh)  # bins that do not fit the mesh fail here
    if isinstance(model, CellViscosity):
        model.values(mesh)  # a callable or an array of the wrong length / sign fails here, not in the first step
