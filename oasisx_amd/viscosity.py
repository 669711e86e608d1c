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

Per ``assemble_first``: one kernel writes ``nut_c`` from ``grad u_ab`` at the cell centroids (``ox_eddy_viscosity``,
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

__all__ = ["Smagorinsky", "Wale", "CellViscosity", "CarreauYasuda", "Cross", "PowerLaw", "VanDriest"]


def _coefficient(what, v):
    v = float(v)
    if not np.isfinite(v) or v < 0.0:
        raise ValueError(f"{what}: the model constant must be finite and >= 0 (got {v})")
    return v


class _KernelModel:
    """A model whose ``nut`` is a function of ``grad u_ab`` at the cell centroid: evaluated by ``ox_eddy_viscosity``."""

    model_id = None
    # nut is a turbulent viscosity that mixes scalars too: kappa_eff = kappa + nut / Sc_t (scalar.py)
    diffuses_scalars = True

    def check(self, gdim: int):
        pass

    def bind(self, solver):
        pass

    def evaluate(self, solver, nut: torch.Tensor, nu=None):
        Vi = solver._Vi[0][0]
        import ctypes as C

        _lib.check(solver._lib.ox_eddy_viscosity(self.model_id, Vi.degree, C.byref(solver._cells), _lib.ptr(Vi.cell_dofs),
                                                 solver._UAB.rptr(), self.coefficient, _lib.ptr(nut),
                                                 _lib.current_stream()), "ox_eddy_viscosity")


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
        _lib.check(lib.ox_eddy_viscosity_damped(0, Vi.degree, C.byref(solver._cells), _lib.ptr(Vi.cell_dofs),
                                                solver._UAB.rptr(), coefficient, C.byref(vd), _lib.ptr(nut), st),
                   "ox_eddy_viscosity_damped")
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
    ``damping``: a :class:`VanDriest` object: ``nut_c = (Cs Delta_c D_c)^2 sqrt(2 S:S)`` (``ox_eddy_viscosity_damped``);
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
    base_viscosity`` (``ox_viscosity_law``).  ``params``: the law's parameters in the order of include/oasisx_hip.h."""

    base_viscosity = None
    params = ()
    # nut = nu(gd) - base_viscosity is a property of the fluid's momentum, not a mixing of scalars
    diffuses_scalars = False

    def evaluate(self, solver, nut: torch.Tensor, nu=None):
        Vi = solver._Vi[0][0]
        import ctypes as C

        par = (C.c_double * len(self.params))(*self.params)
        _lib.check(solver._lib.ox_viscosity_law(self.model_id, Vi.degree, C.byref(solver._cells), _lib.ptr(Vi.cell_dofs),
                                                solver._UAB.rptr(), par, len(self.params), _lib.ptr(nut),
                                                _lib.current_stream()), "ox_viscosity_law")


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
        raise TypeError("viscosity_model: a Smagorinsky, Wale, CarreauYasuda, Cross, PowerLaw or CellViscosity object is "
                        "expected "
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
    if isinstance(model, CellViscosity):
        model.values(mesh)  # a callable or an array of the wrong length / sign fails here, not in the first step
