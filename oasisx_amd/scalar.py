"""Passive scalars carried by ``FractionalStep_AB_CN`` (Oasis: ``scalar_components`` + Schmidt numbers).

Per step and scalar, with the extrapolated velocity ``u_ab`` of that step (so the scalar does not depend on the step's
pressure iteration and is solved once)::

    A_c = M/dt + C(u_ab)/2 + kappa K/2
    b_c = (M/dt - C/2 - kappa K/2) c_1 + b0_c  =  (2/dt) M c_1 - A_c c_1 + b0_c
    the scalar's own Dirichlet rows -> identity in A_c, boundary value in b_c;  solve A_c c = b_c;  c_1 <- c

Plain Galerkin unless the scalar states ``stabilization=`` (SUPG, below).  ``C(u_ab)`` is what the velocity step assembles anyway:
``A_c = A + (kappa - nu)/2 K`` with the velocity matrix ``A`` before its boundary rows, one streaming pass over the
values of the shared SELL-64 pattern (``ox_scalar_rows``, csrc/ox_scalar.hip) instead of a second element loop.

On a solver with a ``viscosity_model`` ``A`` also holds ``K_t / 2``, ``K_t = sum_c nut_c K_c``, and a
scalar with ``turbulent_schmidt=Sc_t`` has the diffusivity ``kappa + nut_c / Sc_t`` per cell::

    A_c = A + s K + t K_t,    s = (kappa - nu)/2,    t = (1/Sc_t - 1)/2        (a law's nut does not diffuse: t = -1/2)

``K_t`` is stored nowhere: ``ox_scalar_rows_cellvisc`` forms its rows once more in LDS (the stiffness contraction of the
fused kernel without its convection turns and gathers) and streams the slices as ``ox_scalar_rows`` does.  ``Sc_t = 1``
(``t = 0``) and a solver without a model run ``ox_scalar_rows``.

Scalars with the same diffusivity specification (``turbulent_schmidt`` included), the same set of Dirichlet rows and the same
matrix-changing part of their ``flux_bcs`` (below) form a GROUP: one matrix, solved in lock-step as the columns of one block solve (at most 3 columns; more open further groups).  One group costs one f64
value array of the velocity pattern in device memory.

A scalar with ``buoyancy=b`` drives the flow (Boussinesq): component ``i`` of the momentum equation
gains ``b_i (c* - reference)`` with ``c* = c_1 + 0.5 (c_1 - c_2)``, the scalar at the step's midpoint (``c* = c_1`` with
``extrapolate=False``)::

    b_first_i += b_i M (c* - reference)          summed over the coupled scalars, inside assemble_first

in one pass over ``M`` (``ox_buoyancy_rows``); ``A`` is not touched.  The coupling is explicit in ``c``.
:class:`ScalarFlux` evaluates the diffusive flux ``-kappa n . grad c`` through tagged exterior facets on the device.

Natural boundary conditions other than the insulated wall, ``flux_bcs=[FluxBC, RobinBC, ...]``: with
``n`` outward and ``kappa_eff`` whatever diffuses the scalar::

    FluxBC(q, facets):                  kappa_eff dc/dn = q                                   q > 0 ENTERS the domain
    RobinBC(h, c_inf, facets, beta):   -kappa_eff dc/dn = (h + beta max(-u_ab . n, 0)) (c - c_inf)

Crank-Nicolson in ``c``: ``A_c += H/2``, ``b_c += load - (H/2) c_1`` with ``H_rs = int hq phi_r phi_s ds`` and
``load_r = int (q + hq c_inf) phi_r ds``, by ``ox_scalar_boundary`` after ``ox_scalar_rows`` and before the group's Dirichlet
rows (which win on rim dofs): one lane per touched row, no atomics.

Convection-dominated scalars (cell Peclet number >> 1), ``stabilization=SUPG(scale, time_term)`` (streamline-upwind
Petrov-Galerkin).  Per cell ``c``, with ``k`` the element degree and ``G[a] = grad lambda_a``::

    w_c     = u_ab(x_c)                     the extrapolated velocity at the centroid
    q_c     = sum_a |w_c . G[a]|,   g_c = sum_a |G[a]|^2
    kappa_c = kappa + nut_c / Sc_t          (kappa without a viscosity model, with Sc_t = inf and with a law)
    tau_c   = scale ([time_term] (2/dt)^2 + (k q_c)^2 + (2 k^2 kappa_c g_c)^2)^(-1/2)         (Shakib)

(1-D P1: ``((2/dt)^2 + (2|w|/h)^2 + (4 kappa/h^2)^2)^(-1/2)``; nothing is divided by ``|w|``: ``w = 0`` gives a finite
``tau`` and no stabilising term, a ``w`` that is not finite gives NaN.)  The test function ``phi_i + tau_c w_c . grad phi_i``
is applied to the Crank-Nicolson residual, with the advecting velocity INSIDE the stabilising terms frozen at ``w_c`` and
the second-derivative term ``tau (w . grad phi_i) kappa lap c`` dropped (exactly zero for P1; for P2 / P3 a stated limit:
the scheme stays consistent to the order of that term).  With::

    N_ij = sum_c tau_c int_c (w_c . grad phi_i) phi_j,      S_ij = sum_c tau_c int_c (w_c . grad phi_i)(w_c . grad phi_j)
    A_c  = A + s K + t K_t + N/dt + S/2
    b_c  = (2/dt) M c_1 - A_c c_1 + b0_c + N ((2/dt) c_1 + f_h)          f_h: the nodal interpolant of ``source``

One per-cell launch (``ox_supg_cells``: ``w_c``, ``tau_c``) and ONE fused row launch per group (``ox_scalar_rows_supg``,
the sibling of ``ox_scalar_rows_cellvisc``: the same LDS accumulator and ``StiffTab`` contraction with
``nut_c G[a].G[b] + (tau_c/(2t))(w_c.G[a])(w_c.G[b])``, the time term from one more compile-time table, the right-hand side
term per lane in registers).  Flux / Robin pass, Dirichlet rows, solve and time levels are unchanged.  A scalar without
``stabilization=`` makes neither call.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .fem import FieldStorage, Function, Vector
from .ksp import KSPSolver
from .la import SellMatrix

__all__ = ["ScalarTransport", "ScalarFlux", "FluxBC", "RobinBC", "SUPG"]

MAX_COLUMNS = 3  # OX_MAXC: the columns ox_ksp_solve / ox_spmv take in lock-step


class SUPG:
    """Streamline-upwind Petrov-Galerkin stabilisation of a :class:`ScalarTransport` (module docstring, DESIGN.md
    section 32).

    Args:
        scale: a finite float > 0 that multiplies Shakib's ``tau`` (1: the standard parameter)
        time_term: ``True`` (default): ``(2/dt)^2`` stands under the root of ``tau``, so ``tau <= dt/2``; ``False``: the
            steady-state parameter
    """

    def __init__(self, scale: float = 1.0, time_term: bool = True):
        try:
            scale = float(scale)
        except (TypeError, ValueError):
            raise ValueError(f"SUPG: scale = {scale!r}: a finite float > 0 is expected") from None
        if not (np.isfinite(scale) and scale > 0.0):
            raise ValueError(f"SUPG: scale = {scale}: a finite float > 0 is expected")
        if not isinstance(time_term, (bool, np.bool_)):
            raise TypeError(f"SUPG: time_term = {time_term!r}: a bool is expected")
        self.scale, self.time_term = scale, bool(time_term)

    def key(self):
        return (self.scale, self.time_term)

    def __repr__(self):
        return f"SUPG(scale={self.scale}, time_term={self.time_term})"


class ScalarTransport:
    """One passive scalar ``c``: ``dc/dt + u . grad c = kappa lap c + source`` on the velocity component space.

    Args:
        name: key of ``FractionalStep_AB_CN.scalar(name)`` and of the iteration counts
        diffusivity: kappa, absolute -- or
        schmidt: Sc, kappa = nu / Sc with the ``nu`` handed to ``solve`` (exactly one of the two)
        bcs: list of :class:`oasisx_amd.DirichletBC` (time-dependent values through ``update_bc``, as for the velocity)
        source: a float, a callable ``f(x)``, a ``Function`` of the component space or a
            :class:`oasisx_amd.function.Expression` -- the four kinds of ``body_force``; assembled once
        initial: c(t0): a float, a callable ``f(x)`` or a ``Function`` of the component space (default 0)
        buoyancy: ``None`` (default): the scalar is passive.  A sequence of ``gdim`` finite floats ``b``: the momentum
            equation of component ``i`` gains the force ``b_i (c - reference)`` -- ``b = -beta g`` for a thermal expansion
            coefficient ``beta``, or ``(0, Ra Pr)`` in diffusion units.  The coupling is EXPLICIT in ``c`` and therefore
            conditionally stable: ``dt`` is bounded by the buoyancy (Brunt-Vaisala) time scale ``1 / sqrt(|b . grad c|)``
            beside the step's convective limit
        reference: the value of ``c`` at which the force vanishes
        extrapolate: ``True`` (default): the force is taken at the step's midpoint, ``c* = c_1 + 0.5 (c_1 - c_2)`` (second
            order; the group keeps a second time level ``c_2``, ``solver.scalar(name, level=2)``); ``False``: ``c* = c_1``,
            first order
        turbulent_schmidt: ``Sc_t``, for a solver with a ``viscosity_model`` (there it must be given: there is no default):
            a finite float > 0 -- the scalar's diffusivity is ``kappa + nut_c / Sc_t`` per cell -- or ``float("inf")``: no
            turbulent diffusivity.  With a generalised-Newtonian law (whose ``nut`` belongs to the momentum alone) only
            ``inf`` is accepted.  Without a ``viscosity_model`` it has no effect
        flux_bcs: list of :class:`FluxBC` / :class:`RobinBC`: prescribed fluxes, film and open-boundary conditions on
            exterior facets (one GPU).  Several conditions may share a facet: their ``q`` and ``h`` add.  Without them
            the natural condition is the insulated wall, and none of their calls is made
        stabilization: ``None`` (default): plain Galerkin.  :class:`SUPG`: the streamline-upwind Petrov-Galerkin scheme of
            the module docstring, for cell Peclet numbers far above 1 (``source`` is then interpolated at the dofs for
            the stabilised source term: an ``Expression`` source raises ``NotImplementedError``).  One GPU
    """

    def __init__(self, name, diffusivity=None, schmidt=None, bcs=(), source=0.0, initial=None, buoyancy=None,
                 reference=0.0, extrapolate=True, turbulent_schmidt=None, flux_bcs=(), stabilization=None):
        if not isinstance(name, str) or not name:
            raise ValueError("ScalarTransport: name must be a non-empty string")
        if (diffusivity is None) == (schmidt is None):
            raise ValueError(f"ScalarTransport {name!r}: give exactly one of diffusivity (kappa) and schmidt (kappa = nu / Sc)")
        val = float(diffusivity if schmidt is None else schmidt)
        if not np.isfinite(val) or val < 0.0 or (schmidt is not None and val == 0.0):
            raise ValueError(f"ScalarTransport {name!r}: diffusivity must be >= 0, a Schmidt number > 0 (got {val})")
        self.name = name
        self.diffusivity = None if diffusivity is None else val
        self.schmidt = None if schmidt is None else val
        self.bcs = list(bcs)
        from .bcs import DirichletBC

        for bc in self.bcs:
            if not isinstance(bc, DirichletBC):
                raise TypeError(f"ScalarTransport {name!r}: bcs holds DirichletBC objects (got {type(bc).__name__})")
        self.flux_bcs = list(flux_bcs)
        for bc in self.flux_bcs:
            if not isinstance(bc, (FluxBC, RobinBC)):
                raise TypeError(f"ScalarTransport {name!r}: flux_bcs holds FluxBC and RobinBC objects (got "
                                f"{type(bc).__name__})")
        from .function import Expression

        if not (callable(source) or isinstance(source, (Function, Expression))):
            source = float(source)
        self.source = source
        if initial is not None and not (callable(initial) or isinstance(initial, Function)):
            initial = float(initial)
        self.initial = initial
        if buoyancy is not None:
            buoyancy = tuple(float(b) for b in buoyancy)
            if not all(np.isfinite(b) for b in buoyancy):
                raise ValueError(f"ScalarTransport {name!r}: buoyancy = {buoyancy}: finite numbers are expected")
        self.buoyancy = buoyancy
        self.reference = float(reference)
        if not np.isfinite(self.reference):
            raise ValueError(f"ScalarTransport {name!r}: reference = {self.reference}: a finite number is expected")
        self.extrapolate = bool(extrapolate)
        if turbulent_schmidt is not None:
            try:
                turbulent_schmidt = float(turbulent_schmidt)
            except (TypeError, ValueError):
                raise ValueError(f"ScalarTransport {name!r}: turbulent_schmidt = {turbulent_schmidt!r}: a float > 0 or "
                                 "float('inf') is expected") from None
            if not turbulent_schmidt > 0.0:  # (NaN too)
                raise ValueError(f"ScalarTransport {name!r}: turbulent_schmidt = {turbulent_schmidt}: a float > 0 or "
                                 "float('inf') is expected")
        self.turbulent_schmidt = turbulent_schmidt
        if stabilization is not None and not isinstance(stabilization, SUPG):
            raise TypeError(f"ScalarTransport {name!r}: stabilization is None or a SUPG object (got "
                            f"{type(stabilization).__name__})")
        if stabilization is not None and isinstance(self.source, Expression):
            raise NotImplementedError(f"ScalarTransport {name!r}: stabilization= with an Expression source: the stabilised "
                                      "source term needs a nodal interpolant (a float, a callable f(x) or a Function)")
        self.stabilization = stabilization

    def inverse_turbulent_schmidt(self) -> float:
        """``1 / Sc_t``; 0 for ``inf`` (and where none was given)."""
        return 0.0 if self.turbulent_schmidt is None else 1.0 / self.turbulent_schmidt

    def kappa(self, nu: float) -> float:
        return self.diffusivity if self.schmidt is None else float(nu) / self.schmidt

    def _spec(self):
        spec = ("kappa", self.diffusivity) if self.schmidt is None else ("schmidt", self.schmidt)
        spec += (("turbulent_schmidt", self.turbulent_schmidt),)
        if self.stabilization is not None:  # (a scalar without it keeps the key it had)
            spec += (("supg",) + self.stabilization.key(),)
        return spec


# ---- flux and Robin conditions -----------------------------------------------------------------------------------------
def _datum(who, what, f):
    """A float (checked finite) or a callable ``f(x)``, as given."""
    if callable(f):
        return f
    v = float(f)
    if not np.isfinite(v):
        raise ValueError(f"{who}: {what} = {v}: a finite number is expected")
    return v


def _nodal(who, what, f, X, nonneg=False):
    """The datum at the points ``X: (3, npts)``: (npts,) float64; non-finite (and, with ``nonneg``, negative) values raise
    ``ValueError``."""
    npts = X.shape[1]
    v = np.broadcast_to(np.asarray(f(X) if callable(f) else f, dtype=np.float64), (npts,)).copy()
    if not np.isfinite(v).all():
        raise ValueError(f"{who}: {what} is not finite at {int((~np.isfinite(v)).sum())} of {npts} facet dofs")
    if nonneg and (v < 0.0).any():
        raise ValueError(f"{who}: {what} must be >= 0 (min {v.min()})")
    return v


class _FacetCondition:
    """Common part of :class:`FluxBC` and :class:`RobinBC`: the facet selection and the link to the group's pass."""

    def __init__(self, facets):
        self.facets = facets
        self._bound = []  # (pass of a scalar group, block): set when a solver takes the scalar

    def facet_ids(self, mesh) -> np.ndarray:
        """The exterior facets of the selection on ``mesh``, ascending; interior facets and facets on an identified
        (periodic) face raise ``ValueError``."""
        from .wall import facet_table, select_facets

        who = type(self).__name__
        ids, _, _ = select_facets(mesh, self.facets, who)
        ids = np.sort(ids)
        facet_table(mesh, ids, who, "flux and Robin conditions")
        return ids

    def update(self) -> None:
        """Re-evaluate the condition's callables at the facet dofs (time-dependent data: ``FractionalStep_AB_CN.solve``
        calls it where it calls ``update_bc`` of the Dirichlet conditions).  The values are used as they are: for second
        order in time return the value at the step's midpoint."""
        for bp, block in self._bound:
            bp.evaluate(block)


class FluxBC(_FacetCondition):
    """A prescribed diffusive flux on exterior facets: ``kappa_eff dc/dn = q`` with ``n`` outward, so a positive ``q``
    ENTERS the domain -- the opposite sign to :class:`ScalarFlux`, which reports the flux that leaves.  Independent of
    ``kappa`` (neither ``schmidt=`` nor ``turbulent_schmidt=`` changes it).

    Args:
        q: a float or a callable ``f(x)`` on ``x: (3, npts)``, evaluated at the facets' dofs of the scalar's space and
            interpolated on the facet
        facets: what :func:`oasisx_amd.wall.select_facets` takes: ``(meshtags, id | ids)``, an array of exterior facet
            ids (``None``: all exterior facets).  Interior facets and identified (periodic) facets raise ``ValueError``
    """

    def __init__(self, q, facets):
        super().__init__(facets)
        self.q = _datum("FluxBC", "q", q)


class RobinBC(_FacetCondition):
    """``-kappa_eff dc/dn = (h + advective max(-u_ab . n, 0)) (c - c_inf)`` on exterior facets, ``n`` outward.  ``h > 0``:
    a film (Biot) condition or first-order surface uptake; ``h = 0, advective = 1``: the open-boundary condition -- nothing
    on outflow, inflow carries ``c_inf`` (the scalar's counterpart of ``PressureBC(..., backflow=)``).  Crank-Nicolson in
    ``c``; the advective part takes the step's extrapolated velocity ``u_ab`` (explicit).  Independent of ``kappa``.

    Args:
        h: the film coefficient, a float or a callable ``f(x)``; ``>= 0`` wherever it is evaluated
        c_inf: the ambient value, a float or a callable ``f(x)``
        facets: as for :class:`FluxBC`
        advective: ``beta`` in ``[0, 1]``
    """

    def __init__(self, h, c_inf, facets, advective: float = 0.0):
        super().__init__(facets)
        self.h = _datum("RobinBC", "h", h)
        if not callable(self.h) and self.h < 0.0:
            raise ValueError(f"RobinBC: h = {self.h}: the film coefficient must be >= 0")
        self.c_inf = _datum("RobinBC", "c_inf", c_inf)
        self.advective = _datum("RobinBC", "advective", advective)
        if callable(self.advective) or not 0.0 <= self.advective <= 1.0:
            raise ValueError(f"RobinBC: advective = {advective!r}: a float in [0, 1] is expected")

    def _matrix_key(self, ids):
        """What of the condition changes the group's matrix: facets, ``h`` (a float, or the identity of the callable) and
        ``advective``."""
        return (ids.tobytes(), ("callable", id(self.h)) if callable(self.h) else ("float", self.h), self.advective)


def flux_key(scalar, mesh):
    """The matrix-changing part of a scalar's ``flux_bcs`` on ``mesh`` (its Robin conditions in list order) and the facet
    ids of every condition; a scalar with only ``FluxBC`` has the key of one with none."""
    ids = [bc.facet_ids(mesh) for bc in scalar.flux_bcs]
    return tuple(bc._matrix_key(i) for bc, i in zip(scalar.flux_bcs, ids) if isinstance(bc, RobinBC)), ids


def group_key(scalar, rows, mesh):
    """(key of the scalar's group, facet ids per condition): the diffusivity specification, the Dirichlet rows and -- only
    where the scalar has Robin conditions -- their matrix-changing part.  ``FluxBC`` changes no matrix and no key."""
    key, ids = (scalar._spec(), np.asarray(rows, dtype=np.int64).tobytes()), []
    if scalar.flux_bcs:
        robin, ids = flux_key(scalar, mesh)
        if robin:
            key += (robin,)
    return key, ids


def group_scalars(keyed_scalars, max_columns=None):
    """``[(key, rows, scalar), ...]`` -> ``[(rows, members), ...]``: scalars of equal key in lock-step, at most
    ``MAX_COLUMNS`` per group, in the order of first appearance."""
    max_columns = MAX_COLUMNS if max_columns is None else max_columns
    keyed = {}
    for key, rows, s in keyed_scalars:
        keyed.setdefault(key, (rows, []))[1].append(s)
    out = []
    for rows, members in keyed.values():
        for i in range(0, len(members), max_columns):
            out.append((rows, members[i:i + max_columns]))
    return out


class BoundaryPass:
    """The flux / Robin pass of one scalar group: one record per (facet, condition), sorted by facet id, then by the
    condition's place in its scalar's list (then by column); the Robin conditions, equal across the members but for
    ``c_inf``, give one record per facet.  Nodal data per record: ``q`` and ``c_inf`` per column, ``h`` and ``beta`` for
    the group.  The row-centric tables are :class:`oasisx_amd.outlet.RowPairs`."""

    def __init__(self, solver, group, facet_ids):
        from .outlet import RowPairs, _single_gpu
        from .wall import FacetSet

        mesh = solver._mesh
        _single_gpu(mesh, "ScalarTransport with flux_bcs")
        dev = mesh.device
        Vi = solver._Vi[0][0]
        members = group.members
        self._solver, self._group, self.nc = solver, group, len(members)
        # blocks: (kind, the RobinBC of every column | the FluxBC, facet ids, place in the scalar's list, column | -1)
        self.blocks = []
        robin = [[(p, bc) for p, bc in enumerate(m.flux_bcs) if isinstance(bc, RobinBC)] for m in members]
        for k, (p, _) in enumerate(robin[0]):
            self.blocks.append(("robin", [r[k][1] for r in robin], facet_ids[0][p], p, -1))
        for j, m in enumerate(members):
            for p, bc in enumerate(m.flux_bcs):
                if isinstance(bc, FluxBC):
                    self.blocks.append(("flux", bc, facet_ids[j][p], p, j))
        ids = np.concatenate([b[2] for b in self.blocks] + [np.zeros(0, np.int64)])
        place = np.concatenate([np.full(b[2].shape[0], b[3], np.int64) for b in self.blocks] + [np.zeros(0, np.int64)])
        col = np.concatenate([np.full(b[2].shape[0], b[4], np.int64) for b in self.blocks] + [np.zeros(0, np.int64)])
        blk = np.concatenate([np.full(b[2].shape[0], k, np.int64) for k, b in enumerate(self.blocks)] + [np.zeros(0, np.int64)])
        order = np.lexsort((col, place, ids))  # by facet id, then by the order of the list, then by column
        self.record_facets, blk = ids[order], blk[order]
        self._records_of = [np.nonzero(blk == k)[0] for k in range(len(self.blocks))]  # (ascending facet id inside a block)
        uniq, inv = np.unique(self.record_facets, return_inverse=True)
        fs = FacetSet(solver, uniq, np.zeros(uniq.shape[0], dtype=np.int64), 1, "ScalarTransport flux_bcs",
                      "flux and Robin conditions")
        ne = int(self.record_facets.shape[0])
        self.n_records = ne
        kpos, lf = fs.kpos[inv], fs.local_facets[inv]
        self.robin = bool(robin[0])
        self.adv = any(bc.advective > 0.0 for _, bc in robin[0])
        rp = RowPairs(Vi, kpos, lf, dev, "ScalarTransport flux_bcs", slots=self.robin)
        self.pairs, self.nfd = rp, rp.nfd
        rec = np.stack([kpos, lf], axis=1).astype(np.int32) if ne else np.zeros((1, 2), dtype=np.int32)
        self.rec = torch.from_numpy(np.ascontiguousarray(rec)).to(dev)
        # the coordinates of the records' facet dofs, (3, ne * nfd)
        x = Vi.x.cpu().numpy()[rp.facet_dofs.reshape(-1)]
        self._X = np.zeros((3, x.shape[0]))
        self._X[: x.shape[1]] = x.T
        n1 = max(ne, 1)
        self._q, self._c = np.zeros((n1, self.nfd, self.nc)), np.zeros((n1, self.nfd, self.nc))
        self._h, self._beta = np.zeros((n1, self.nfd)), np.zeros(n1)
        self.q, self.c_inf = torch.from_numpy(self._q).to(dev), torch.from_numpy(self._c).to(dev)
        self.h, self.beta = torch.from_numpy(self._h).to(dev), torch.from_numpy(self._beta).to(dev)
        self._dirty = False
        for k, b in enumerate(self.blocks):
            for bc in (b[1] if b[0] == "robin" else [b[1]]):
                bc._bound.append((self, k))
            self.evaluate(k, first=True)

    def evaluate(self, k: int, first: bool = False) -> None:
        """The nodal data of block k on the host (``first``: the constants too); they go to the device with the next
        pass."""
        kind, bcs, _, _, col = self.blocks[k]
        recs = self._records_of[k]
        nfd = self.nfd
        if not recs.size:  # an empty facet set
            return
        X = self._X.reshape(3, -1, nfd)[:, recs].reshape(3, -1)
        if kind == "flux":
            if first or callable(bcs.q):
                self._q[recs, :, col] = _nodal("FluxBC", "q", bcs.q, X).reshape(-1, nfd)
                self._dirty = True
            return
        for j, bc in enumerate(bcs):
            if first or callable(bc.c_inf):
                self._c[recs, :, j] = _nodal("RobinBC", "c_inf", bc.c_inf, X).reshape(-1, nfd)
                self._dirty = True
        if first or callable(bcs[0].h):
            self._h[recs] = _nodal("RobinBC", "h", bcs[0].h, X, nonneg=True).reshape(-1, nfd)
            self._dirty = True
        if first:
            self._beta[recs] = bcs[0].advective

    def add(self) -> None:
        """``A_c += H/2``, ``b_c += load - (H/2) c_1`` with the ``u_ab`` block of this step (``ox_scalar_boundary``)."""
        S, g = self._solver, self._group
        if self._dirty:
            for dst, src in ((self.q, self._q), (self.c_inf, self._c), (self.h, self._h), (self.beta, self._beta)):
                dst.copy_(torch.from_numpy(src))
            self._dirty = False
        if not self.n_records:
            return
        Vi = S._Vi[0][0]
        rp = self.pairs
        a = _lib.ox_scalar_bc_args()
        a.degree, a.nc, a.robin, a.adv = Vi.degree, self.nc, int(self.robin), int(self.adv)
        a.n_rows = rp.n_rows
        a.rows, a.row_ptr = rp.rows.data_ptr(), rp.row_ptr.data_ptr()
        a.pair_facet, a.pair_loc = rp.pair_facet.data_ptr(), rp.pair_loc.data_ptr()
        a.n_facets, a.facet_rec, a.q = self.n_records, self.rec.data_ptr(), self.q.data_ptr()
        if self.robin:
            a.pair_off, a.h, a.c_inf = rp.pair_off.data_ptr(), self.h.data_ptr(), self.c_inf.data_ptr()
            a.c1 = g.C1.rdev().data_ptr()
            a.a_vals, a.a_size = g.Ac.vals.data_ptr(), int(g.Ac.vals.shape[0])
        if self.adv:
            a.beta, a.uab = self.beta.data_ptr(), S._UAB.rdev().data_ptr()
        a.b, a.n_dofs = g.B.dev().data_ptr(), int(S._n_u)
        _lib.check(S._lib.ox_scalar_boundary(C.byref(S._cells), _lib.ptr(Vi.cell_dofs), C.byref(a), _lib.current_stream()),
                   "ox_scalar_boundary")
        if self.robin:
            g.Ac.version += 1


def check_turbulent_schmidt(model, scalars) -> None:
    """The scope guard of ``viscosity_model=`` with ``scalars=`` (run by ``viscosity.check_model``, before the library is
    loaded): every scalar states its turbulent Schmidt number, and with a model whose ``nut`` does not mix scalars
    (``diffuses_scalars = False``: the generalised-Newtonian laws) that number is ``inf``."""
    for s in scalars:
        if not isinstance(s, ScalarTransport):
            raise TypeError(f"scalars: a list of ScalarTransport (got {type(s).__name__})")
        if s.turbulent_schmidt is None:
            raise NotImplementedError(f"viscosity_model with scalars=: ScalarTransport {s.name!r} has no turbulent_schmidt=: "
                                      "the turbulent diffusivity of a scalar is a modelling decision with no default here "
                                      "(kappa + nut / Sc_t; float('inf') for none)")
        if not model.diffuses_scalars and s.turbulent_schmidt != float("inf"):
            raise ValueError(f"ScalarTransport {s.name!r}: turbulent_schmidt = {s.turbulent_schmidt} with {model!r}: the "
                             "law's nut = nu(gd) - base_viscosity is a property of the fluid's momentum and does not "
                             "diffuse scalars; turbulent_schmidt must be float('inf')")


def turbulent_factor(solver, member) -> float:
    """``t`` of ``A_c = A + s K + t K_t``: ``(1/Sc_t - 1)/2`` where the model's ``nut`` diffuses scalars, ``-1/2`` (``K_t``
    taken out again) where it does not."""
    if not solver._viscosity_model.diffuses_scalars:
        return -0.5
    return 0.5 * (member.inverse_turbulent_schmidt() - 1.0)


class ScalarGroup:
    """Scalars that share one operator: the columns of one block solve."""

    def __init__(self, solver, members, rows: np.ndarray, options):
        Vi = solver._Vi[0][0]
        dev = solver._mesh.device
        self.members = members
        nc = len(members)
        self.nc = nc
        n = solver._n_u
        self.C, self.C1, self.B0, self.B, self.AC1 = (FieldStorage(n, nc, dev) for _ in range(5))
        self.c = [Function(Vi, m.name, self.C, j) for j, m in enumerate(members)]
        self.c1 = [Function(Vi, m.name + "_1", self.C1, j) for j, m in enumerate(members)]
        # a second time level, only where a coupled member extrapolates its force to the step's midpoint
        self.C2, self.c2 = None, None
        if any(m.buoyancy is not None and m.extrapolate for m in members):
            self.C2 = FieldStorage(n, nc, dev)
            self.c2 = [Function(Vi, m.name + "_2", self.C2, j) for j, m in enumerate(members)]
        self.rows_dev = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(dev)
        self.Ac = SellMatrix(Vi.pattern, symmetric=False, name="A_" + "+".join(m.name for m in members))
        self.ksp = KSPSolver(solver._mesh.comm, options, prefix="scalar_transport")
        self.ksp.setOperators(self.Ac)
        self.ksp.setOptions(self.Ac)
        self.reasons = None
        self.ax0_valid = False  # AC1 holds A_c c_1 of the last assembly and has not been used yet
        self.boundary = None  # the flux / Robin pass (BoundaryPass), where a member has flux_bcs
        # SUPG (equal across the members: it is part of the group's key): the nodal source f_h and the per-cell record
        # of ox_supg_cells, a structure of arrays in kernel cell order: w_c (gdim rows), then tau_c
        self.stabilization = members[0].stabilization
        self.FH = self.supg_rec = None
        if self.stabilization is not None:
            self.FH = FieldStorage(n, nc, dev)
            self.supg_rec = torch.zeros((solver._gdim + 1, int(solver._geom.shape[0])), dtype=torch.float64, device=dev)

    def wants_ax0(self) -> bool:
        o = self.ksp._options
        return bool(o.get("ksp_initial_guess_nonzero", False)) and str(o.get("ksp_type", "")).lower() != "preonly"

    def bc_vector(self, j: int) -> Vector:
        return Vector(self.B, j)


def build_groups(solver, scalars, options):
    """Validate the scalars of a solver, create their Dirichlet data and sort them into groups."""
    Vi = solver._Vi[0][0]
    for s in scalars:
        if not isinstance(s, ScalarTransport):
            raise TypeError(f"scalars: a list of ScalarTransport (got {type(s).__name__})")
    names = [s.name for s in scalars]
    dup = sorted({n for n in names if names.count(n) > 1})
    if dup:
        raise ValueError(f"scalars: duplicate names {dup}")
    gdim = solver._gdim
    for s in scalars:
        if s.buoyancy is not None and len(s.buoyancy) != gdim:
            raise ValueError(f"ScalarTransport {s.name!r}: buoyancy has {len(s.buoyancy)} entries, the mesh has {gdim} "
                             "directions")
    for s in scalars:
        for what, f in (("source", s.source), ("initial", s.initial)):
            if isinstance(f, Function) and getattr(f.function_space, "scalar", f.function_space) is not Vi:
                raise ValueError(f"ScalarTransport {s.name!r}: a Function {what} must live on the velocity component space")
    from .fem import shared_marker_evaluations

    with shared_marker_evaluations():
        for s in scalars:
            for bc in s.bcs:
                bc.create_bc(Vi)
    keyed, facet_ids = [], {}
    for s in scalars:
        rows = np.unique(np.concatenate([np.asarray(bc._dofs, dtype=np.int64) for bc in s.bcs] + [np.zeros(0, np.int64)]))
        rows = rows[rows < Vi.n_owned]
        key, facet_ids[s.name] = group_key(s, rows, solver._mesh)
        keyed.append((key, rows, s))
    groups = []
    for rows, members in group_scalars(keyed):
        g = ScalarGroup(solver, members, rows, options)
        if any(m.flux_bcs for m in members):
            g.boundary = BoundaryPass(solver, g, [facet_ids[m.name] for m in members])
        groups.append(g)
    return groups


def set_initial(solver, group: ScalarGroup):
    """c(t0) into every time level, b0_c = int source v dx (once)."""
    Vi = solver._Vi[0][0]
    for j, s in enumerate(group.members):
        f = s.initial
        if isinstance(f, Function):
            group.C1.dev()[:, j] = f._storage.rdev()[:, 0 if f._comp is None else f._comp]
        elif callable(f):
            group.c1[j].interpolate(f)
        elif f is not None and f != 0.0:
            group.C1.dev()[: Vi.n_local, j] = float(f)
        group.B0.dev()[: Vi.n_owned, j] = solver._source_vector(s.source, f"ScalarTransport {s.name!r}: source")
        if group.FH is not None:  # f_h, the nodal interpolant of the source
            f = s.source
            if isinstance(f, Function):
                group.FH.dev()[:, j] = f._storage.rdev()[:, 0 if f._comp is None else f._comp]
            elif callable(f):
                Function(Vi, s.name + "_source", group.FH, j).interpolate(f)
            else:
                group.FH.dev()[: Vi.n_local, j] = float(f)
    group.C.dev().copy_(group.C1.rdev())
    if group.C2 is not None:
        group.C2.dev().copy_(group.C1.rdev())


def buoyancy_terms(groups):
    """The ``ox_buoy_term`` records of the coupled scalars of a solver, in the order of the groups and their columns, in
    launches of at most ``MAX_COLUMNS`` terms: a list of ctypes arrays (the blocks never move: built once)."""
    terms = []
    for g in groups:
        for j, m in enumerate(g.members):
            if m.buoyancy is None:
                continue
            t = _lib.ox_buoy_term()
            t.c1 = g.C1.rdev().data_ptr()
            t.c2 = g.C2.rdev().data_ptr() if m.extrapolate else None
            t.nc, t.col, t.ref = g.nc, j, m.reference
            for i in range(3):
                t.coef[i] = m.buoyancy[i] if i < len(m.buoyancy) else 0.0
            terms.append((g, t))
    out = []
    for i in range(0, len(terms), MAX_COLUMNS):
        chunk = terms[i:i + MAX_COLUMNS]
        out.append(((_lib.ox_buoy_term * len(chunk))(*[t for _, t in chunk]), [g for g, _ in chunk]))
    return out


def add_buoyancy(solver, launches):
    """``b_first_i += sum_t b_t,i M (c*_t - reference_t)``: one pass over ``M`` per launch (``ox_buoyancy_rows``)."""
    st = _lib.current_stream()
    for arr, groups in launches:
        for g in groups:  # blocks checked out to the host go back to the device first; read-only from here
            g.C1.rptr()
            if g.C2 is not None:
                g.C2.rptr()
        _lib.check(solver._lib.ox_buoyancy_rows(solver._M.ref(), solver._gdim, len(arr), arr, solver._BFIRST.ptr(), st),
                   "ox_buoyancy_rows")


def assemble(solver, group: ScalarGroup, dt: float, nu: float):
    """A_c, b_c and (optionally) A_c c_1 of one group from the velocity matrix BEFORE its boundary rows."""
    lib, st = solver._lib, _lib.current_stream()
    kappa = group.members[0].kappa(nu)
    au = group.AC1.ptr() if group.wants_ax0() else None
    if group.boundary is not None and group.boundary.robin:
        au = None  # A_c changes after the row kernel: its A_c c_1 by-product is not asked for
    t = 0.0 if solver._viscosity_model is None else turbulent_factor(solver, group.members[0])
    if group.stabilization is not None:  # SUPG: tau_c and w_c per cell, then the sibling of the cell-viscosity rows
        Vi = solver._Vi[0][0]
        solver._scalar_rows_open = group
        try:
            solver.scalar_stabilization_assemble(dt, nu)
        finally:
            solver._scalar_rows_open = None
        _lib.check(lib.ox_scalar_rows_supg(C.byref(solver._cells), C.byref(Vi.assembly_info()), solver._A.ref(),
                                           solver._M.ref(), solver._K.ref(), group.Ac.ref(),
                                           _lib.ptr(solver._nut) if t != 0.0 else None, _lib.ptr(group.supg_rec),
                                           0.5 * (kappa - float(nu)), t, float(dt), group.nc, group.C1.rptr(),
                                           group.B0.rptr(), group.FH.rptr(), group.B.ptr(), au,
                                           int(solver._row_blocks and Vi.pattern.n_row_blocks > 0), st),
                   "ox_scalar_rows_supg")
    elif t == 0.0:  # no model, or Sc_t = 1: the scalar's operator differs from A by a multiple of K alone
        _lib.check(lib.ox_scalar_rows(solver._A.ref(), solver._M.ref(), solver._K.ref(), group.Ac.ref(),
                                      0.5 * (kappa - float(nu)), float(dt), group.nc, group.C1.rptr(), group.B0.rptr(),
                                      group.B.ptr(), au, st), "ox_scalar_rows")
    else:  # A_c = A + s K + t K_t: the rows of K_t = sum_c nut_c K_c once more, in LDS
        Vi = solver._Vi[0][0]
        _lib.check(lib.ox_scalar_rows_cellvisc(C.byref(solver._cells), C.byref(Vi.assembly_info()), solver._A.ref(),
                                               solver._M.ref(), solver._K.ref(), group.Ac.ref(), _lib.ptr(solver._nut),
                                               0.5 * (kappa - float(nu)), t, float(dt), group.nc, group.C1.rptr(),
                                               group.B0.rptr(), group.B.ptr(), au,
                                               int(solver._row_blocks and Vi.pattern.n_row_blocks > 0), st),
                   "ox_scalar_rows_cellvisc")
    group.Ac.version += 1
    if group.boundary is not None:  # before the identity rows: Dirichlet rows win on rim dofs
        solver._scalar_rows_open = group
        try:
            solver.scalar_boundary_assemble()
        finally:
            solver._scalar_rows_open = None
    if group.rows_dev.shape[0] > 0:  # identity rows; (A_c c_1)[row] = c_1[row] there, in the same launch
        group.Ac.zero_rows(group.rows_dev, 1.0, au, group.C1.rptr() if au is not None else None, group.nc)
    for j, s in enumerate(group.members):
        for bc in s.bcs:
            bc.apply(group.bc_vector(j))
    group.ax0_valid = au is not None


def stabilization_cells(solver, group: ScalarGroup, dt: float, nu: float):
    """``w_c`` and ``tau_c`` of a stabilised group from the ``u_ab`` block (and the ``nut``) of this step
    (``ox_supg_cells``)."""
    Vi = solver._Vi[0][0]
    m, sp = group.members[0], group.stabilization
    model = solver._viscosity_model
    inv = m.inverse_turbulent_schmidt() if model is not None and model.diffuses_scalars else 0.0
    _lib.check(solver._lib.ox_supg_cells(Vi.degree, C.byref(solver._cells), _lib.ptr(Vi.cell_dofs), solver._UAB.rptr(),
                                         _lib.ptr(solver._nut) if inv != 0.0 else None, float(m.kappa(nu)), inv, float(dt),
                                         sp.scale, int(sp.time_term), _lib.ptr(group.supg_rec), _lib.current_stream()),
               "ox_supg_cells")


def solve(solver, group: ScalarGroup):
    lib, st = solver._lib, _lib.current_stream()
    n = solver._n_u * group.nc
    guess = bool(group.ksp._options.get("ksp_initial_guess_nonzero", False))
    ax0 = None
    if guess:  # the initial guess is c_1, whatever was written to c since: the product A_c c_1 of the assembly holds
        _lib.check(lib.ox_axpby(n, 1.0, group.C1.rptr(), 0.0, None, group.C.ptr(), st), "ox_axpby")
        if group.ax0_valid:
            ax0 = group.AC1
    group.ax0_valid = False
    group.reasons = np.asarray(group.ksp.solve_block(group.B, group.C, ax0=ax0), dtype=np.int32)
    if group.C2 is not None:  # c_2 <- c_1
        _lib.check(lib.ox_axpby(n, 1.0, group.C1.rptr(), 0.0, None, group.C2.ptr(), st), "ox_axpby")
    _lib.check(lib.ox_axpby(n, 1.0, group.C.rptr(), 0.0, None, group.C1.ptr(), st), "ox_axpby")  # c_1 <- c
    return group.reasons


class ScalarFlux:
    """Diffusive flux ``q_f = -kappa n . mean_f(grad c)`` (on a solver with a ``viscosity_model``: ``kappa + nut_c / Sc_t``
    of the facet's cell, with the ``nut`` of the last ``assemble_first``; ``ox_scalar_flux_cells``) of one scalar of a ``FractionalStep_AB_CN`` solver through
    exterior facets, evaluated on the device beside the time step: the Nusselt / Sherwood number of a wall is
    ``totals()`` over the wall's area and the reference flux.  ``n`` points outward: a positive flux leaves the domain.

    The facet is affine, so the facet mean of the gradient is exact (compile-time facet means of the basis,
    ``csrc/fe_tables_f.h``); for P1 it is the cell's constant gradient, first order in ``h``.  Limits: one GPU; exterior
    facets; the DIFFUSIVE flux only -- on an open boundary the advective part ``c u . n`` is not included.

    Args:
        solver: the solver (one GPU: ``comm.size > 1`` raises ``NotImplementedError``)
        scalar: the name of one of the solver's scalars
        facets: ``None``: all exterior facets, one tag 0; ``(meshtags, id)`` / ``(meshtags, (id, ...))``: the facets of
            those values, one tag per id; an array of facet ids: those facets, one tag 0.  Interior facets raise
            ``ValueError``
        capacity: initial length of the ring of totals (it doubles when full)

    The object's facet order is by tag, then by facet id (``.facets``, ``.facet_tags``).  ``.tags``: the tag values;
    ``.normals`` (outward), ``.areas``, ``.midpoints``: host arrays in that order.
    """

    def __init__(self, solver, scalar: str, facets=None, capacity: int = 64):
        from .wall import FacetSet, select_facets

        mesh = solver._mesh
        comm = getattr(mesh, "comm", None)
        if comm is not None and getattr(comm, "size", 1) > 1:
            raise NotImplementedError("ScalarFlux on a mesh partition (comm.size > 1): the facet evaluation and the sums "
                                      "are built for one GPU")
        if scalar not in solver._scalar_index:
            raise KeyError(f"ScalarFlux: no scalar named {scalar!r} (have: {sorted(solver._scalar_index)})")
        if int(capacity) < 1:
            raise ValueError(f"ScalarFlux: capacity = {capacity}")
        ids, tag_of, tags = select_facets(mesh, facets, "ScalarFlux")
        fs = FacetSet(solver, ids, tag_of, tags.shape[0], "ScalarFlux", "scalar fluxes")
        self._solver, self.scalar = solver, scalar
        self._group, self._col = solver._scalar_index[scalar]
        self.facets, self.tags = ids, tags
        self.facet_tags = tags[tag_of] if ids.size else tag_of
        self.cells, self.local_facets = fs.cells, fs.local_facets
        self.n_facets, self.n_tags = fs.n_facets, fs.n_tags
        self.normals, self.areas, self.midpoints = fs.normals, fs.areas, fs.midpoints
        self._rec, self._tag_ptr = fs.rec, fs.tag_ptr
        dev = mesh.device
        n = max(self.n_facets, 1)  # (the sums are handed a valid pointer also without facets)
        self._q, self._fq, self._cbar, self._acc = (torch.zeros(n, dtype=torch.float64, device=dev) for _ in range(4))
        self._T = 0.0
        self.capacity = int(capacity)
        self._ring = torch.zeros((self.capacity, self.n_tags), dtype=torch.float64, device=dev)
        self._times = []

    @property
    def n_samples(self) -> int:
        return len(self._times)

    @property
    def times(self) -> np.ndarray:
        return np.asarray(self._times, dtype=np.float64)

    @property
    def total_weight(self) -> float:
        return self._T

    def sample(self, t: float, nu: float, dt: float = 0.0) -> None:
        """Evaluate the flux of the scalar's current ``c`` (``kappa`` from ``nu`` for a Schmidt number) on the current
        stream: two launches (``ox_scalar_flux``, then the per-tag sums of ``|f| q`` by ``ox_outlet_update``), no host
        synchronisation; ``c`` is read through ``rptr()``.  ``dt > 0`` adds the sample to the time average with weight
        ``dt``."""
        dt = float(dt)
        if not dt >= 0.0:
            raise ValueError(f"ScalarFlux.sample: dt = {dt}")
        k = len(self._times)
        if k == self.capacity:  # the ring doubles (a device copy on the current stream)
            ring = torch.zeros((2 * self.capacity, self.n_tags), dtype=torch.float64, device=self._ring.device)
            ring[: self.capacity] = self._ring
            self._ring, self.capacity = ring, 2 * self.capacity
        S, g = self._solver, self._group
        Vi = S._Vi[0][0]
        lib, st = _lib.load(), _lib.current_stream()
        kappa = g.members[self._col].kappa(nu)
        model = S._viscosity_model
        if self.n_facets and model is not None:  # kappa + nut_c / Sc_t of the facet's cell, nut of the last assemble_first
            inv = g.members[self._col].inverse_turbulent_schmidt() if model.diffuses_scalars else 0.0
            _lib.check(lib.ox_scalar_flux_cells(Vi.degree, C.byref(S._cells), _lib.ptr(Vi.cell_dofs), self.n_facets,
                                                _lib.ptr(self._rec), g.C.rptr(), g.nc, self._col, float(kappa),
                                                _lib.ptr(S._nut), inv, dt, _lib.ptr(self._q), _lib.ptr(self._fq),
                                                _lib.ptr(self._cbar), _lib.ptr(self._acc), st), "ox_scalar_flux_cells")
        elif self.n_facets:
            _lib.check(lib.ox_scalar_flux(Vi.degree, C.byref(S._cells), _lib.ptr(Vi.cell_dofs), self.n_facets,
                                          _lib.ptr(self._rec), g.C.rptr(), g.nc, self._col, float(kappa), dt, _lib.ptr(self._q),
                                          _lib.ptr(self._fq), _lib.ptr(self._cbar), _lib.ptr(self._acc), st), "ox_scalar_flux")
        _lib.check(lib.ox_outlet_update(self.n_tags, _lib.ptr(self._tag_ptr), _lib.ptr(self._fq), _lib.ptr(self._ring),
                                        self.capacity, k, None, 0.0, None, None, None, None, None, 0, st), "ox_outlet_update")
        self._T += dt
        self._times.append(float(t))

    def flux(self) -> torch.Tensor:
        """``q_f`` of the latest sample, (n_facets,) on the device."""
        return self._q[: self.n_facets]

    def facet_mean(self) -> torch.Tensor:
        """The facet means of ``c`` of the latest sample, (n_facets,) on the device."""
        return self._cbar[: self.n_facets]

    def history(self) -> np.ndarray:
        """(n_samples, n_tags) on the host: ``sum_{f in tag} |f| q_f`` of every sample (one synchronisation)."""
        return self._ring[: len(self._times)].cpu().numpy()

    def totals(self) -> np.ndarray:
        """(n_tags,) on the host: ``sum_{f in tag} |f| q_f`` of the latest sample."""
        if not self._times:
            raise RuntimeError("ScalarFlux: no sample has been taken")
        return self._ring[len(self._times) - 1].cpu().numpy()

    def mean_flux(self) -> torch.Tensor:
        """The time average ``(1/T) sum dt q_f`` over the samples taken with ``dt > 0``."""
        if not self._T > 0.0:
            raise RuntimeError("ScalarFlux: no sample with dt > 0 has been taken since the statistics were reset")
        return self._acc[: self.n_facets] / self._T

    def reset_statistics(self) -> None:
        self._acc.zero_()
        self._T = 0.0

    def save(self, path, vtu=None, time: float = 0.0) -> None:
        """History and per-facet fields as ``.npz``; ``vtu``: a path for the facets' surface with ``flux`` and
        ``facet_mean`` (and ``mean_flux``) as cell data (:func:`oasisx_amd.io.write_facet_vtu`)."""
        out = dict(history=self.history(), times=self.times, facets=self.facets, facet_tags=self.facet_tags, tags=self.tags,
                   normals=self.normals, areas=self.areas, midpoints=self.midpoints, flux=self.flux().cpu().numpy(),
                   facet_mean=self.facet_mean().cpu().numpy(), total_weight=self._T)
        if self._T > 0.0:
            out.update(mean_flux=self.mean_flux().cpu().numpy())
        np.savez(path, **out)
        if vtu is not None:
            from .io import write_facet_vtu

            data = {k: out[k] for k in ("flux", "facet_mean", "mean_flux") if k in out}
            write_facet_vtu(vtu, self._solver._mesh, self.facets, data, time=time)
