"""Smoothed-aggregation algebraic multigrid: PETSc's ``pc_type gamg`` for one-column CG solves on one GPU.

The hierarchy is built on the host from the operator's scipy copy (``SellMatrix.to_scipy``):

  * strength of connection: |a_ij| > pc_gamg_threshold * sqrt(|a_ii a_jj|), i != j (threshold 0: every nonzero);
  * aggregation: a distance-2 maximal independent set (MIS-2) of the strength graph, computed in vectorised rounds with
    a fixed hash of the row index as priority (the same aggregates on every run); every root collects its neighbours,
    the rows two steps away join the largest-numbered aggregate among their neighbours.  Rows without off-diagonal
    entries (the identity rows ``bcs_p`` leaves behind) are singletons: they belong to no aggregate;
  * tentative prolongator from the constant near-nullspace (P_tent[i, agg(i)] = 1), smoothed once:
    P = (I - omega D^-1 A) P_tent with omega = 4 / (3 lambda_max(D^-1 A))  (pc_gamg_agg_nsmooths = 1);
  * R = P^T stored explicitly, Galerkin coarse operators R A P;
  * coarsening stops at pc_gamg_coarse_eq_limit rows or pc_mg_levels levels; the coarsest level is solved with a dense
    (pseudo-)inverse, which for a singular operator (pure Neumann pressure) annihilates the constants;
  * every other level is smoothed by Chebyshev-Jacobi of degree mg_levels_ksp_max_it on [0.1, 1.1] lambda_max (PETSc
    GAMG's smoother defaults); lambda_max(D^-1 A) comes from a Lanczos estimate with a fixed start vector.

On a mesh-partitioned operator (PETSc's ``pc_type bjacobi`` + ``sub_pc_type gamg``: one block per rank) the hierarchy
is built the same way from the rank's owned-by-owned block ``A_rr`` (``owned_block``: rows and columns < n_owned, ghost
columns dropped), with a level-0 matrix of its own (``Hierarchy(..., block=True)``).  On two ranks or more that block of
a pure-Neumann operator is SPD -- a principal submatrix of a matrix whose null space is the constants --, so the
row-sum test finds it nonsingular and the coarse inverse is not projected.

The device side (``csrc/ox_amg.hip``) runs a symmetric V-cycle -- the same Chebyshev polynomial before and after the
coarse correction, R = P^T -- so that it is a valid CG preconditioner.  ``Hierarchy.vcycle_numpy`` is the same cycle in
numpy (tests).
"""
from __future__ import annotations

import ctypes as C
import time

import numpy as np
import scipy.sparse as sp
import torch

from . import _lib

__all__ = ["Hierarchy", "build_levels", "owned_block", "vcycle_numpy"]

DEFAULTS = {"pc_gamg_threshold": 0.0, "pc_gamg_agg_nsmooths": 1, "pc_gamg_coarse_eq_limit": 50, "pc_mg_levels": 10,
            "mg_levels_ksp_max_it": 2}
LANCZOS_STEPS = 12
CHEB_LO, CHEB_HI = 0.1, 1.1
MAX_DEGREE = 8  # OX_MG_MAX_DEGREE of include/oasisx_hip.h
MAX_COARSE_ROWS = 4096


def _closed_max(indptr, indices, v):
    """m[i] = max(v[i], max over the neighbours j of i of v[j])."""
    m = v.copy()
    nz = np.diff(indptr) > 0
    if indices.size:
        red = np.maximum.reduceat(v[indices], indptr[:-1][nz])
        m[nz] = np.maximum(m[nz], red)
    return m


def _strength_graph(A: sp.csr_matrix, theta: float):
    """Strength graph (CSR without diagonal, symmetric) and the singleton mask (rows without off-diagonal entries)."""
    A = A.tocoo()
    off = (A.row != A.col) & (A.data != 0.0)
    n = A.shape[0]
    singleton = np.bincount(A.row[off], minlength=n) == 0
    d = np.abs(A.diagonal())
    r, c, v = A.row[off], A.col[off], np.abs(A.data[off])
    keep = v > theta * np.sqrt(d[r] * d[c]) if theta > 0 else np.ones(r.shape, dtype=bool)
    G = sp.csr_matrix((np.ones(int(keep.sum()), dtype=np.int8), (r[keep], c[keep])), shape=(n, n))
    G = ((G + G.T) > 0).tocsr()
    G.sort_indices()
    return G, singleton


def _priority(n: int) -> np.ndarray:
    """Distinct fixed priorities: a multiplicative hash of the index, ties impossible (the index is appended)."""
    i = np.arange(n, dtype=np.uint64)
    h = (i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    return (h.astype(np.int64) << np.int64(31)) | i.astype(np.int64)


def aggregate(A: sp.csr_matrix, theta: float = 0.0):
    """MIS-2 aggregation.  Returns agg (int64 [n], -1 for singletons) and the number of aggregates."""
    n = A.shape[0]
    G, singleton = _strength_graph(A, theta)
    ip, ix = G.indptr, G.indices
    key = _priority(n)
    state = np.zeros(n, dtype=np.int8)  # 0 undecided, 1 root, -1 covered
    state[singleton] = -1
    while True:
        und = state == 0
        if not und.any():
            break
        k = np.where(und, key, np.int64(-1))
        m2 = _closed_max(ip, ix, _closed_max(ip, ix, k))
        new = und & (k == m2)
        state[new] = 1
        isroot = (state == 1).astype(np.int8)
        near = _closed_max(ip, ix, _closed_max(ip, ix, isroot)) > 0
        state[und & near & ~new] = -1
    roots = np.flatnonzero(state == 1)
    agg = np.full(n, -1, dtype=np.int64)
    agg[roots] = np.arange(roots.size)
    # distance 1: the (unique) neighbouring root; then the rest: the largest aggregate id among the neighbours
    for _ in range(n + 1):
        todo = (agg < 0) & ~singleton
        if not todo.any():
            break
        cand = _closed_max(ip, ix, agg)
        upd = todo & (cand >= 0)
        if not upd.any():  # (a component of the strength graph without root cannot exist after a maximal MIS-2)
            raise RuntimeError("amg: aggregation left rows without aggregate")
        agg[upd] = cand[upd]
    return agg, int(roots.size)


def tentative_prolongator(agg: np.ndarray, nagg: int) -> sp.csr_matrix:
    n = agg.shape[0]
    rows = np.flatnonzero(agg >= 0)
    return sp.csr_matrix((np.ones(rows.size), (rows, agg[rows])), shape=(n, nagg))


def lambda_max(A: sp.csr_matrix, dinv: np.ndarray, steps: int = LANCZOS_STEPS) -> float:
    """Largest Ritz value of D^-1/2 A D^-1/2 after ``steps`` Lanczos steps from a fixed start vector."""
    n = A.shape[0]
    s = np.sqrt(np.abs(dinv))
    v = 1.0 + 0.5 * np.sin(np.arange(n, dtype=np.float64) * 0.7548776662)  # fixed, not an eigenvector of anything
    v /= np.linalg.norm(v)
    v_old = np.zeros(n)
    alphas, betas = [], []
    beta = 0.0
    for _ in range(min(steps, n)):
        w = s * (A @ (s * v))
        a = float(w @ v)
        w = w - a * v - beta * v_old
        alphas.append(a)
        beta = float(np.linalg.norm(w))
        if beta <= 1e-14 * abs(a):
            break
        betas.append(beta)
        v_old, v = v, w / beta
    k = len(alphas)
    T = np.diag(alphas) + np.diag(betas[: k - 1], 1) + np.diag(betas[: k - 1], -1)
    return float(np.linalg.eigvalsh(T)[-1])


def cheb_coefficients(lmax_est: float, degree: int):
    """(c_d, c_r) of every step of the Chebyshev-Jacobi smoother on [0.1, 1.1] lambda_max:
    r = D^-1 (b - A x);  d = c_d d + c_r r;  x += d  (step 1: c_d = 0)."""
    lo, hi = CHEB_LO * lmax_est, CHEB_HI * lmax_est
    theta, delta = 0.5 * (hi + lo), 0.5 * (hi - lo)
    sigma = theta / delta
    rho = 1.0 / sigma
    out = [(0.0, 1.0 / theta)]
    for _ in range(1, degree):
        rn = 1.0 / (2.0 * sigma - rho)
        out.append((rn * rho, 2.0 * rn / delta))
        rho = rn
    return out


def _coarse_inverse(A: sp.csr_matrix, singular: bool, scale: float = 0.0) -> np.ndarray:
    """Dense (pseudo-)inverse.  ``singular``: the operator's null space is the constants (pure Neumann pressure,
    propagated from the fine level: A_c 1 = R A P 1 = R A 1 = 0): the inverse on the mean-free subspace, which
    annihilates the constants.  (``scale``: the size of the level above's diagonal -- any positive shift of the
    constants gives the same result; a coarsest level of one row holds rounding noise only.)"""
    D = A.toarray()
    D = 0.5 * (D + D.T)
    n = D.shape[0]
    if n == 0:
        return D
    one = np.ones(n)
    if singular:
        s = max(float(np.abs(np.diag(D)).max()), scale) or 1.0
        Q = np.eye(n) - np.outer(one, one) / n
        inv = Q @ np.linalg.inv(D + (s / n) * np.outer(one, one)) @ Q
    else:
        w, V = np.linalg.eigh(D)
        big = np.abs(w) > 1e-12 * np.abs(w).max()
        inv = (V[:, big] / w[big]) @ V[:, big].T
    return 0.5 * (inv + inv.T)


def owned_block(M: sp.spmatrix) -> sp.csr_matrix:
    """The owned-by-owned block of a rank's rows: ``M`` is (n_owned, n_local) with the owned columns first (a partitioned
    ``SellMatrix.to_scipy()``); the ghost columns (>= n_owned) are dropped."""
    M = sp.csr_matrix(M)
    n = M.shape[0]
    if M.shape[1] < n:
        raise ValueError(f"amg: a block of {M.shape[0]} x {M.shape[1]} has fewer columns than rows")
    return sp.csr_matrix(M[:, :n])


class Level:
    def __init__(self, A, dinv, P=None, R=None, cheb=None, lmax=None, agg=None):
        self.A, self.dinv, self.P, self.R, self.cheb, self.lmax, self.agg = A, dinv, P, R, cheb, lmax, agg


def build_levels(A: sp.csr_matrix, options: dict | None = None):
    """Host hierarchy: list of Level (the last one coarsest, with ``inv``)."""
    o = dict(DEFAULTS)
    o.update({k: v for k, v in (options or {}).items() if k in DEFAULTS})
    theta = float(o["pc_gamg_threshold"])
    nsmooth = int(o["pc_gamg_agg_nsmooths"])
    limit = max(1, int(o["pc_gamg_coarse_eq_limit"]))
    max_levels = max(1, int(o["pc_mg_levels"]))
    degree = min(MAX_DEGREE, max(1, int(o["mg_levels_ksp_max_it"])))
    A = sp.csr_matrix(A, dtype=np.float64)
    A.eliminate_zeros()
    A.sort_indices()
    levels = []
    # the constants in the null space (pure Neumann): the coarsest inverse must annihilate them
    singular = bool(np.abs(A @ np.ones(A.shape[0])).max() <= 1e-12 * max(abs(A).max(), 1e-300))
    while True:
        d = A.diagonal()
        dinv = np.where(d != 0.0, 1.0 / np.where(d != 0.0, d, 1.0), 1.0)
        lev = Level(A, dinv)
        levels.append(lev)
        n = A.shape[0]
        if n <= limit or len(levels) >= max_levels:
            break
        agg, nagg = aggregate(A, theta)
        if nagg == 0 or nagg >= n:
            break
        lev.agg = agg
        lev.lmax = lambda_max(A, dinv)
        lev.cheb = cheb_coefficients(lev.lmax, degree)
        P = tentative_prolongator(agg, nagg)
        for _ in range(nsmooth):
            omega = 4.0 / (3.0 * lev.lmax)
            P = (P - omega * (sp.diags(dinv) @ (A @ P))).tocsr()
        P.eliminate_zeros()
        P.sort_indices()
        R = P.T.tocsr()
        R.sort_indices()
        Ac = (R @ A @ P).tocsr()
        Ac = 0.5 * (Ac + Ac.T)  # (the product's rounding is not symmetric bit for bit; the operator is)
        Ac = sp.csr_matrix(Ac)
        Ac.eliminate_zeros()
        Ac.sort_indices()
        lev.P, lev.R = P, R
        A = Ac
    if A.shape[0] > MAX_COARSE_ROWS:
        raise ValueError(f"amg: the coarsest level has {A.shape[0]} rows (more than {MAX_COARSE_ROWS} for its dense "
                         f"inverse): raise pc_mg_levels")
    scale = float(np.abs(levels[-2].A.diagonal()).max()) if len(levels) > 1 else 0.0
    levels[-1].inv = _coarse_inverse(A, singular, scale)
    return levels


def vcycle_numpy(levels, b: np.ndarray, lvl: int = 0) -> np.ndarray:
    """z = B b: the device V-cycle in numpy (same smoother, same order of phases)."""
    L = levels[lvl]
    if lvl == len(levels) - 1:
        return L.inv @ b
    A, dinv = L.A, L.dinv
    k = len(L.cheb)
    cd, cr = L.cheb[0]
    d = cr * dinv * b
    x = d.copy()
    for j in range(1, k):
        cd, cr = L.cheb[j]
        r = dinv * (b - A @ x)
        d = cd * d + cr * r
        x = x + d
    xc = vcycle_numpy(levels, L.R @ (b - A @ x), lvl + 1)
    x = x + L.P @ xc
    for j in range(k):
        cd, cr = L.cheb[j]
        r = dinv * (b - A @ x)
        d = cr * r if j == 0 else cd * d + cr * r
        x = x + d
    return x


# ---------------------------------------------------------------------------------------------------------------------
# device hierarchy
class _DevMat:
    """Plain-f64 SELL-64 copy of a scipy CSR matrix (fem.build_sell + values_from_csr)."""

    def __init__(self, M: sp.csr_matrix, device):
        from .fem import build_sell

        M = sp.csr_matrix(M)
        M.sort_indices()
        n_rows, n_cols = M.shape
        rl = np.diff(M.indptr).astype(np.int64)
        rows = np.repeat(np.arange(n_rows, dtype=np.int64), rl)
        keys = torch.from_numpy(rows * n_cols + M.indices.astype(np.int64)).to(device)
        self.pattern = build_sell(n_rows, n_cols, keys, torch.from_numpy(rl).to(device),
                                  torch.from_numpy(M.indptr.astype(np.int64)).to(device))
        self.vals = self.pattern.values_from_csr(M)
        self.struct = self.pattern.struct(self.vals, compress=False)
        self.nnz = int(M.nnz)


class Hierarchy:
    """Host levels + their device copies + the library's ``ox_mg`` handle."""

    def __init__(self, A, options: dict | None = None, tail_rows: int = 0, block: bool = False):
        """``A``: the fine-level ``la.SellMatrix`` (its own storage -- value dictionary, pair slots, windows -- stays in
        use on the fine level).  ``block``: the hierarchy of ``owned_block(A)`` (a mesh-partitioned operator: the
        rank's block of pc_type bjacobi), whose level 0 is a plain-f64 copy of that block: the cycle's fine-level
        vectors have n_owned entries and no mat-vec of the cycle reads a ghost column.  A block of no rows has no
        device hierarchy (``handle`` None)."""
        t0 = time.perf_counter()
        self.A = A
        self.block = bool(block)
        dev = A.vals.device
        M = A.to_scipy()
        if self.block:
            M = owned_block(M)
            if M.shape[0] == 0:
                self.levels, self.handle, self._keep = [], None, []
                self.setup_host_s = self.setup_s = time.perf_counter() - t0
                self.nnz, self.rows = [], []
                return
        self.levels = build_levels(M, options)
        self.setup_host_s = time.perf_counter() - t0
        lib = _lib.load()
        L = len(self.levels)
        self._keep = []
        arr = (_lib.ox_mg_level * L)()
        for i, lev in enumerate(self.levels):
            dinv = torch.from_numpy(lev.dinv).to(dev)
            self._keep.append(dinv)
            arr[i].dinv = dinv.data_ptr()
            arr[i].n_rows = lev.A.shape[0]
            if i == 0 and not self.block:
                arr[i].A = A.struct
            elif i < L - 1:
                m = _DevMat(lev.A, dev)
                self._keep.append(m)
                arr[i].A = m.struct
            if i < L - 1:
                P, R = _DevMat(lev.P, dev), _DevMat(lev.R, dev)
                self._keep += [P, R]
                arr[i].P, arr[i].R = P.struct, R.struct
                arr[i].degree = len(lev.cheb)
                for j, (cd, cr) in enumerate(lev.cheb):
                    arr[i].cheb[2 * j], arr[i].cheb[2 * j + 1] = cd, cr
        inv = torch.from_numpy(np.ascontiguousarray(self.levels[-1].inv)).to(dev)
        self._keep.append(inv)
        h = C.c_void_p()
        _lib.check(lib.ox_mg_create(L, arr, _lib.ptr(inv), int(tail_rows), C.byref(h)), "ox_mg_create")
        self.handle = h
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        self.setup_s = time.perf_counter() - t0
        self.nnz = [int(lev.A.nnz) for lev in self.levels]
        self.rows = [int(lev.A.shape[0]) for lev in self.levels]

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            try:
                _lib.load().ox_mg_destroy(h)
            except Exception:
                pass
            self.handle = None

    def kernels_per_cycle(self) -> int:
        return int(_lib.load().ox_mg_kernels_per_cycle(self.handle)) if self.handle is not None else 0

    def apply(self, r: torch.Tensor, z: torch.Tensor):
        """z = B r (one V-cycle) on device vectors of the fine level's rows."""
        _lib.check(_lib.load().ox_mg_apply(self.handle, _lib.ptr(r), _lib.ptr(z), _lib.current_stream()), "ox_mg_apply")

    def vcycle_numpy(self, b: np.ndarray) -> np.ndarray:
        return vcycle_numpy(self.levels, b)

    def cycle_bytes(self) -> float:
        """HBM bytes of one V-cycle, roughly (12 B per stored entry of every mat-vec, 8 B per vector element pass)."""
        tot = 0.0
        for i, lev in enumerate(self.levels[:-1]):
            k = len(lev.cheb)
            tot += 12.0 * (2 * k) * lev.A.nnz + 12.0 * (lev.P.nnz + lev.R.nnz) + 8.0 * 12 * lev.A.shape[0]
        return tot
