"""Passive scalars carried by ``FractionalStep_AB_CN`` (Oasis: ``scalar_components`` + Schmidt numbers).

Per step and scalar, with the extrapolated velocity ``u_ab`` of that step (so the scalar does not depend on the step's
pressure iteration and is solved once)::

    A_c = M/dt + C(u_ab)/2 + kappa K/2
    b_c = (M/dt - C/2 - kappa K/2) c_1 + b0_c  =  (2/dt) M c_1 - A_c c_1 + b0_c
    the scalar's own Dirichlet rows -> identity in A_c, boundary value in b_c;  solve A_c c = b_c;  c_1 <- c

Plain Galerkin, no coupling back into the momentum equation.  ``C(u_ab)`` is what the velocity step assembles anyway:
``A_c = A + (kappa - nu)/2 K`` with the velocity matrix ``A`` before its boundary rows, one streaming pass over the
values of the shared SELL-64 pattern (``ox_scalar_rows``, csrc/ox_scalar.hip) instead of a second element loop.

Scalars with the same diffusivity specification and the same set of Dirichlet rows form a GROUP: one matrix, solved in
lock-step as the columns of one block solve (at most 3 columns; more open further groups).  One group costs one f64
value array of the velocity pattern in device memory.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .fem import FieldStorage, Function, Vector
from .ksp import KSPSolver
from .la import SellMatrix

__all__ = ["ScalarTransport"]

MAX_COLUMNS = 3  # OX_MAXC: the columns ox_ksp_solve / ox_spmv take in lock-step


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
    """

    def __init__(self, name, diffusivity=None, schmidt=None, bcs=(), source=0.0, initial=None):
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
        from .function import Expression

        if not (callable(source) or isinstance(source, (Function, Expression))):
            source = float(source)
        self.source = source
        if initial is not None and not (callable(initial) or isinstance(initial, Function)):
            initial = float(initial)
        self.initial = initial

    def kappa(self, nu: float) -> float:
        return self.diffusivity if self.schmidt is None else float(nu) / self.schmidt

    def _spec(self):
        return ("kappa", self.diffusivity) if self.schmidt is None else ("schmidt", self.schmidt)


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
        self.rows_dev = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(dev)
        self.Ac = SellMatrix(Vi.pattern, symmetric=False, name="A_" + "+".join(m.name for m in members))
        self.ksp = KSPSolver(solver._mesh.comm, options, prefix="scalar_transport")
        self.ksp.setOperators(self.Ac)
        self.ksp.setOptions(self.Ac)
        self.reasons = None
        self.ax0_valid = False  # AC1 holds A_c c_1 of the last assembly and has not been used yet

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
    for s in scalars:
        for what, f in (("source", s.source), ("initial", s.initial)):
            if isinstance(f, Function) and getattr(f.function_space, "scalar", f.function_space) is not Vi:
                raise ValueError(f"ScalarTransport {s.name!r}: a Function {what} must live on the velocity component space")
    from .fem import shared_marker_evaluations

    with shared_marker_evaluations():
        for s in scalars:
            for bc in s.bcs:
                bc.create_bc(Vi)
    keyed = {}
    for s in scalars:
        rows = np.unique(np.concatenate([np.asarray(bc._dofs, dtype=np.int64) for bc in s.bcs] + [np.zeros(0, np.int64)]))
        rows = rows[rows < Vi.n_owned]
        keyed.setdefault((s._spec(), rows.tobytes()), (rows, []))[1].append(s)
    groups = []
    for rows, members in keyed.values():
        for i in range(0, len(members), MAX_COLUMNS):
            groups.append(ScalarGroup(solver, members[i:i + MAX_COLUMNS], rows, options))
    return groups


def set_initial(solver, group: ScalarGroup):
    """c(t0) into both time levels, b0_c = int source v dx (once)."""
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
    group.C.dev().copy_(group.C1.rdev())


def assemble(solver, group: ScalarGroup, dt: float, nu: float):
    """A_c, b_c and (optionally) A_c c_1 of one group from the velocity matrix BEFORE its boundary rows."""
    lib, st = solver._lib, _lib.current_stream()
    kappa = group.members[0].kappa(nu)
    au = group.AC1.ptr() if group.wants_ax0() else None
    _lib.check(lib.ox_scalar_rows(solver._A.ref(), solver._M.ref(), solver._K.ref(), group.Ac.ref(),
                                  0.5 * (kappa - float(nu)), float(dt), group.nc, group.C1.rptr(), group.B0.rptr(),
                                  group.B.ptr(), au, st), "ox_scalar_rows")
    group.Ac.version += 1
    if group.rows_dev.shape[0] > 0:  # identity rows; (A_c c_1)[row] = c_1[row] there, in the same launch
        group.Ac.zero_rows(group.rows_dev, 1.0, au, group.C1.rptr() if au is not None else None, group.nc)
    for j, s in enumerate(group.members):
        for bc in s.bcs:
            bc.apply(group.bc_vector(j))
    group.ax0_valid = au is not None


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
    _lib.check(lib.ox_axpby(n, 1.0, group.C.rptr(), 0.0, None, group.C1.ptr(), st), "ox_axpby")  # c_1 <- c
    return group.reasons
