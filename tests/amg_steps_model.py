"""Reference of the AMG V-cycle and of AMG-preconditioned CG in extended precision, and the mesh-free operators they are
run on (plain numpy / scipy: importable without a GPU).  Used by tests/test_amg_steps_host.py (CPU: the preconditions)
and tests/test_gpu_amg_steps.py (GPU: ``Hierarchy.apply`` and ``KSPSolver`` with ``pc_type gamg`` against this model).

``helical_laplacian`` gives operators with an exact row count: the weighted graph Laplacian of a 2-D grid of width m
wrapped helically (node i is joined to i + 1 and to i + m: bands 0, +-1, +-m, at most 5 entries per row).  They are
weakly diagonally dominant on purpose: on a strictly dominant matrix (``reduction_systems.banded_system``) the smoother
alone nearly solves the system, the coarse correction barely moves z and a wrong deep level would hide.

``vcycle`` is the textbook recursive V-cycle written from the description in oasisx_amd/amg.py's header -- Chebyshev-
Jacobi pre-smoothing from x = 0, restriction of the residual, recursion, prolongation, post-smoothing with the same
polynomial, the dense (pseudo-)inverse at the bottom -- on what ``amg.build_levels`` produced (A, dinv, P, R, cheb, inv),
cast to the working precision; it does not call ``amg.vcycle_numpy``.  ``amg_cg_trace`` is left-preconditioned CG in the
conventions of the device solve (csrc/ox_ksp.hip, mgcg_solve): the residual is the recurrence's r_k, the norm tested is
|z_k| = |B r_k|, the reference norm of the relative test is |B b| for a zero and for a nonzero guess alike.

Extended precision: ``np.longdouble`` where it is wider than float64, exact dot products otherwise (``EXTENDED`` and
``_dot`` of tests/krylov_steps_model.py).
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from tests.krylov_steps_model import EXTENDED, _dot  # noqa: F401  (EXTENDED: re-exported for the tests)

KINDS = ("dirichlet", "neumann", "dict")
DICT_WEIGHTS = np.array([1.0, 1.125, 1.25, 1.5])
IDENTITY_EVERY = 97


def helical_laplacian(n: int, m: int, kind: str, seed: int = 0) -> sp.csr_matrix:
    """scipy CSR (sorted indices), bands 0, +-1, +-m: the graph Laplacian of the helically wrapped grid with edge weights
    1 + 0.5 rand ("dirichlet", "neumann") or from DICT_WEIGHTS ("dict": few distinct values and inverse diagonals, so
    that ``SellMatrix.freeze`` builds a value dictionary).  "neumann" is the Laplacian itself: singular, the constants
    its null space.  "dirichlet" and "dict" add 1 to the diagonal of the first and last m rows and turn every 97th row
    into an identity row (row and column zeroed, 1 on the diagonal: what ox_zero_rows_cols leaves of a Dirichlet row, a
    singleton of ``amg.aggregate`` and an empty row of P)."""
    assert kind in KINDS and 1 < m < n - 1
    rng = np.random.default_rng(3000 + seed)
    if kind == "dict":
        w1, wm = DICT_WEIGHTS[rng.integers(0, 4, n - 1)], DICT_WEIGHTS[rng.integers(0, 4, n - m)]
    else:
        w1, wm = 1.0 + 0.5 * rng.random(n - 1), 1.0 + 0.5 * rng.random(n - m)
    ident = np.zeros(n, dtype=bool)
    if kind != "neumann":
        # the identity rows leave the graph with their edges: their neighbours stay weakly dominant (a pinned node every
        # 97 rows would screen the operator, and the deep levels would no longer matter)
        ident[IDENTITY_EVERY - 1::IDENTITY_EVERY] = True
        w1 = np.where(ident[:-1] | ident[1:], 0.0, w1)
        wm = np.where(ident[:-m] | ident[m:], 0.0, wm)
    d = np.zeros(n)
    d[:-1] += w1
    d[1:] += w1
    d[:-m] += wm
    d[m:] += wm
    if kind != "neumann":
        d[:m] += 1.0
        d[-m:] += 1.0
        d[ident] = 1.0
    A = sp.diags([-wm, -w1, d, -w1, -wm], [-m, -1, 0, 1, m], format="csr")
    A.eliminate_zeros()
    A.sort_indices()
    return A


# ---- the hierarchies of the tests: name -> (n, m, kind, seed, gamg options, tail_rows of the V-cycle cases) -----------
BIG_N, BIG_M = 198437, 445  # reduction_systems.rows_for_parts(776): more than 768 partial rows in both kinds of sums
CASES = {
    "one": (1061, 29, "dirichlet", 1, {"pc_mg_levels": 1}, (0,)),
    "two-deg1": (12709, 131, "dirichlet", 2, {"pc_mg_levels": 2, "mg_levels_ksp_max_it": 1}, (0, 16384)),
    "two-deg1-dict": (12709, 131, "dict", 3, {"pc_mg_levels": 2, "mg_levels_ksp_max_it": 1}, (16384,)),
    "five": (BIG_N, BIG_M, "dirichlet", 4, {}, (0, 1, 32768)),
    "five-dict": (BIG_N, BIG_M, "dict", 5, {}, ()),
    "five-neumann-deg3": (BIG_N, BIG_M, "neumann", 6, {"mg_levels_ksp_max_it": 3}, (0,)),
    "deg8": (1061, 29, "neumann", 7, {"mg_levels_ksp_max_it": 8, "pc_gamg_coarse_eq_limit": 10}, (0, 1)),
    "deg9": (1061, 29, "neumann", 7, {"mg_levels_ksp_max_it": 9, "pc_gamg_coarse_eq_limit": 10}, (0, 1)),
}
VCYCLE_CASES = [(name, tail) for name, c in CASES.items() for tail in c[5]]
_BUILT = {}


def system(name: str):
    """(A csr, levels of amg.build_levels, kind) of a case, built once."""
    if name not in _BUILT:
        from oasisx_amd import amg

        n, m, kind, seed, options, _ = CASES[name]
        A = helical_laplacian(n, m, kind, seed)
        _BUILT[name] = (A, amg.build_levels(A, options), kind)
    return _BUILT[name]


def right_hand_sides(name: str, nc: int, seed: int) -> np.ndarray:
    """(n, nc) ``signed_unit_vectors``; mean-free columns for the singular (Neumann) operators."""
    from tests import reduction_systems as RS

    b = RS.signed_unit_vectors(CASES[name][0], nc, seed)
    return b - b.mean(axis=0) if CASES[name][2] == "neumann" else b


# ---- the V-cycle -----------------------------------------------------------------------------------------------------
class CastLevel:
    def __init__(self, lev, dtype, last):
        self.A = sp.csr_matrix(lev.A).astype(dtype)
        self.dinv = np.asarray(lev.dinv).astype(dtype)
        self.P = self.R = self.cheb = self.inv = None
        if last:
            self.inv = np.asarray(lev.inv).astype(dtype)
        else:
            self.P, self.R = sp.csr_matrix(lev.P).astype(dtype), sp.csr_matrix(lev.R).astype(dtype)
            self.cheb = [(dtype(cd), dtype(cr)) for cd, cr in lev.cheb]


class CastLevels(list):
    """The hierarchy of ``amg.build_levels`` in one working precision (every float64 value converts exactly)."""

    def __init__(self, levels, dtype):
        super().__init__(CastLevel(lev, dtype, i == len(levels) - 1) for i, lev in enumerate(levels))
        self.dtype = dtype


def cast_levels(levels, dtype) -> CastLevels:
    if isinstance(levels, CastLevels) and levels.dtype == dtype:
        return levels
    return CastLevels(levels, dtype)


def _smooth(L, b, x):
    """Chebyshev-Jacobi: r = D^-1 (b - A x); d = c_d d + c_r r; x += d, for every (c_d, c_r) (the first c_d is 0)."""
    d = np.zeros_like(b)
    for cd, cr in L.cheb:
        r = L.dinv * (b - L.A @ x)
        d = cd * d + cr * r
        x = x + d
    return x


def vcycle(levels, b, dtype=np.longdouble, lvl: int = 0):
    """z = B b: one symmetric V-cycle in ``dtype``."""
    levels = cast_levels(levels, dtype)
    L = levels[lvl]
    b = np.asarray(b).astype(dtype)
    if lvl == len(levels) - 1:
        return L.inv @ b
    x = _smooth(L, b, np.zeros_like(b))
    xc = vcycle(levels, L.R @ (b - L.A @ x), dtype, lvl + 1)
    return _smooth(L, b, x + L.P @ xc)


def without_prolongation(levels, j: int, dtype=np.float64) -> CastLevels:
    """The hierarchy whose correction from level j >= 1 never arrives: P of level j - 1 zeroed (the sensitivity check)."""
    out = CastLevels(levels, dtype)
    out[j - 1].P = out[j - 1].P * dtype(0)
    return out


# ---- AMG-CG ----------------------------------------------------------------------------------------------------------
def amg_cg_trace(A, levels, b, x0, kmax: int, dtype=np.longdouble):
    """[(x_k, |B b|, |B r_k|) for k = 0..kmax] of CG on A x = b preconditioned by the V-cycle B, from x0 (None: zero);
    r_k is the recurrence's residual."""
    levels = cast_levels(levels, dtype)
    Aw = sp.csr_matrix(A).astype(dtype)
    b = np.asarray(b).astype(dtype)
    sq = lambda v: np.sqrt(_dot(v, v, dtype))
    bn = sq(vcycle(levels, b, dtype))
    if x0 is None:
        x, r = np.zeros_like(b), b.copy()
    else:
        x = np.asarray(x0).astype(dtype)
        r = b - Aw @ x
    z = vcycle(levels, r, dtype)
    p = z.copy()
    rz = _dot(r, z, dtype)
    out = [(x.copy(), bn, sq(z))]
    for _ in range(kmax):
        q = Aw @ p
        alpha = rz / _dot(p, q, dtype)
        x = x + alpha * p
        r = r - alpha * q
        z = vcycle(levels, r, dtype)
        rz_new = _dot(r, z, dtype)
        out.append((x.copy(), bn, sq(z)))
        p = z + (rz_new / rz) * p
        rz = rz_new
    return out


def stopping_iteration(trace, rtol: float, atol: float = 0.0) -> int:
    """First k >= 0 with |z_k| <= max(rtol |B b|, atol) (-1: none in the trace)."""
    for k, (_, bn, zn) in enumerate(trace):
        if zn <= atol or zn <= rtol * bn:
            return k
    return -1


# ---- the references of the tests: computed once per process, never modified -----------------------------------------
RHS_SEED, GUESS_SEED, SCHEDULE_SEED = 11, 12, 27
CG_SYSTEMS = ("five", "five-dict", "five-neumann-deg3", "two-deg1", "one")
# the schedule test solves the "five" system with this right-hand side to this tolerance: the model stops at iteration
# SCHEDULE_ITS with |z| / |B b| a factor 2 away from the tolerance before and after (held by test_amg_steps_host.py)
SCHEDULE_RTOL, SCHEDULE_ITS = 3.13e-7, 15
ATOL_FACTOR = 1.5  # the reasons test: ksp_atol = ATOL_FACTOR |z_2| of the "five" trace, |z_1| another factor above it
_REF = {}


def guess_of(name: str) -> np.ndarray:
    from tests import reduction_systems as RS

    return 0.25 * RS.signed_unit_vectors(CASES[name][0], 1, GUESS_SEED)[:, 0]


def cast_system(name: str, dtype) -> CastLevels:
    key = ("c", name, dtype)
    if key not in _REF:
        _REF[key] = cast_levels(system(name)[1], dtype)
    return _REF[key]


def reference_vcycles(name: str, dtype=np.longdouble):
    """(b of two columns, [B b1, B b2]) of a case."""
    key = ("v", name, dtype)
    if key not in _REF:
        b = right_hand_sides(name, 2, RHS_SEED)
        cast = cast_system(name, dtype)
        _REF[key] = (b, [vcycle(cast, b[:, c], dtype) for c in range(2)])
    return _REF[key]


def reference_trace(name: str, guess: bool, dtype=np.longdouble, kmax: int | None = None, seed: int = RHS_SEED):
    """(b, x0 or None, trace) of a case: k = 0..3 from a zero guess, 0..2 from ``guess_of`` (the one-level case: the
    first iteration solves the system, the recurrence ends there: kmax 1)."""
    if kmax is None:
        kmax = 1 if name == "one" else (2 if guess else 3)
    key = ("t", name, guess, dtype, kmax, seed)
    if key not in _REF:
        b = right_hand_sides(name, 1, seed)[:, 0]
        x0 = guess_of(name) if guess else None
        _REF[key] = (b, x0, amg_cg_trace(system(name)[0], cast_system(name, dtype), b, x0, kmax, dtype))
    return _REF[key]
