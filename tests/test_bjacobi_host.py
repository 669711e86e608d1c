"""CPU: pc_type bjacobi + sub_pc_type gamg -- how KSPSolver resolves the options (fake operators), the owned-by-owned
block of a partitioned operator and its hierarchy, and a numpy model of the block-Jacobi V-cycle preconditioned CG."""
import logging

import numpy as np
import pytest
import scipy.sparse as sp

BJ = {"ksp_type": "cg", "pc_type": "bjacobi", "sub_pc_type": "gamg", "ksp_rtol": 1e-8}


class _Comm:
    def __init__(self, size):
        self.size = size


def _op(partitioned: bool):
    class _Pattern:
        dist = object() if partitioned else None
        n_rows = 10

    class _Op:
        pattern = _Pattern()
        symmetric = True

    return _Op()


def _audit(caplog, opts, partitioned=True, nc=1, size=8):
    from oasisx_amd.ksp import KSPSolver

    ksp = KSPSolver(_Comm(size), dict(opts))
    ksp.setOperators(_op(partitioned))
    with caplog.at_level(logging.WARNING, logger="oasisx"):
        caplog.clear()
        ksp._audit_options(nc)
    return ksp, [r.getMessage() for r in caplog.records if r.levelno >= logging.WARNING]


@pytest.mark.parametrize("partitioned", [True, False])
def test_bjacobi_gamg_with_cg_is_honoured_silently(caplog, partitioned):
    extra = {"sub_ksp_type": "preonly", "pc_bjacobi_blocks": 8 if partitioned else 1, "sub_pc_gamg_threshold": 0.0,
             "sub_pc_gamg_agg_nsmooths": 1, "sub_pc_gamg_coarse_eq_limit": 50, "sub_pc_mg_levels": 10,
             "sub_mg_levels_ksp_max_it": 2}
    ksp, warned = _audit(caplog, dict(BJ, **extra), partitioned)
    assert ksp._bjacobi_gamg(1) and not ksp._gamg(1) and not ksp._pc_none()
    assert warned == []


@pytest.mark.parametrize("opts,nc,needle", [
    ({"sub_pc_type": None}, 1, "sub_pc_type unset (PETSc's default: ilu): runs jacobi"),
    ({"sub_pc_type": "ilu"}, 1, "sub_pc_type=ilu is not available on the device: runs jacobi"),
    ({"ksp_type": "bcgs"}, 1, "ksp_type=bcgs, 1 column(s)): runs jacobi"),
    ({"ksp_type": "gmres"}, 1, "ksp_type=gmres, 1 column(s)): runs jacobi"),
    ({}, 2, "ksp_type=cg, 2 column(s)): runs jacobi"),
])
def test_bjacobi_fallbacks_warn_and_run_jacobi(caplog, opts, nc, needle):
    o = dict(BJ, **opts)
    o = {k: v for k, v in o.items() if v is not None}
    ksp, warned = _audit(caplog, o, nc=nc)
    assert not ksp._bjacobi_gamg(nc) and not ksp._gamg(nc) and not ksp._pc_none()
    assert len([w for w in warned if "bjacobi" in w]) == 1 and needle in " ".join(warned), warned
    # once per solver
    with caplog.at_level(logging.WARNING, logger="oasisx"):
        caplog.clear()
        ksp._audit_options(nc)
    assert "bjacobi" not in caplog.text


@pytest.mark.parametrize("opts,needle", [
    ({"pc_bjacobi_blocks": 4}, "pc_bjacobi_blocks=4: runs one block per rank (8)"),
    ({"sub_ksp_type": "gmres"}, "sub_ksp_type=gmres is not available: runs preonly (one V-cycle per block)"),
])
def test_bjacobi_block_options_warn_but_keep_the_vcycle(caplog, opts, needle):
    ksp, warned = _audit(caplog, dict(BJ, **opts))
    assert ksp._bjacobi_gamg(1)
    assert len(warned) == 1 and needle in warned[0], warned


def test_bjacobi_jacobi_and_none_are_silent_remaps(caplog):
    ksp, warned = _audit(caplog, dict(BJ, sub_pc_type="jacobi"))
    assert warned == [] and not ksp._bjacobi_gamg(1) and not ksp._pc_none()
    ksp, warned = _audit(caplog, dict(BJ, sub_pc_type="none", pc_bjacobi_blocks=4))  # (any blocking: the same pc)
    assert warned == [] and not ksp._bjacobi_gamg(1) and ksp._pc_none()
    # an inner Krylov solve per block does not exist on these paths either: reported, preonly runs
    for sub in ("jacobi", "none"):
        ksp, warned = _audit(caplog, dict(BJ, sub_pc_type=sub, sub_ksp_type="gmres"))
        assert len(warned) == 1 and f"sub_ksp_type=gmres is not available: runs preonly (pc_type {sub}" in warned[0]
        assert ksp._pc_none() == (sub == "none")


def test_a_rank_without_owned_rows_has_an_empty_block_hierarchy():
    """A rank that owns no rows: no device hierarchy (ox_ksp_solve gets ``mg = NULL`` and still takes part in every
    exchange and all-reduce), a six-launch iteration, and the check interval still goes through the all-reduce."""
    import torch

    from oasisx_amd import _lib
    from oasisx_amd.ksp import KSPSolver

    class _Pattern:
        dist = object()
        n_rows, n_cols, nnz = 0, 5, 0

    class _Empty:
        pattern = _Pattern()
        symmetric = True
        version = 0
        struct = b""
        vals = torch.empty(0, dtype=torch.float64)

        def ref(self):
            return None

        def to_scipy(self):
            return sp.csr_matrix((0, 5))

    class _MaxComm(_Comm):
        calls = []

        def allreduce(self, v, op=None):
            self.calls.append((v, op))
            return v

    comm = _MaxComm(8)
    ksp = KSPSolver(comm, dict(BJ))
    ksp.setOperators(_Empty())
    H = ksp._hierarchy()
    assert H.block and H.handle is None and H.levels == [] and H.rows == []
    assert H.kernels_per_cycle() == 0 and H.cycle_bytes() == 0.0
    assert ksp._interval_for(1, _lib.KSP_CG_MG) == 16 and comm.calls == [(16, "max")]
    assert ksp._cg_kernels_per_iteration() == 6


def test_partitioned_gamg_still_resolves_to_jacobi(caplog):
    ksp, warned = _audit(caplog, {"ksp_type": "cg", "pc_type": "gamg"})
    assert not ksp._gamg(1) and not ksp._bjacobi_gamg(1)
    assert len(warned) == 1 and "pc_type=gamg" in warned[0] and "partitioned" in warned[0] and "runs jacobi" in warned[0]
    assert "pc_type bjacobi with sub_pc_type gamg" in warned[0]
    # the gamg keys next to bjacobi / the sub_ keys next to gamg are not those of the path
    _, warned = _audit(caplog, dict(BJ, pc_gamg_threshold=0.0))
    assert len(warned) == 1 and "pc_gamg_threshold" in warned[0]


# ---------------------------------------------------------------------------------------------------------------------
def _p1_neumann(N):
    """P1 stiffness matrix of the unit square split into 2 N^2 triangles (pure Neumann: A 1 = 0) and the vertices."""
    xs = np.linspace(0.0, 1.0, N + 1)
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    pts = np.stack([X.ravel(), Y.ravel()], 1)
    v = lambda i, j: i * (N + 1) + j
    tris = []
    for i in range(N):
        for j in range(N):
            tris.append((v(i, j), v(i + 1, j), v(i + 1, j + 1)))
            tris.append((v(i, j), v(i + 1, j + 1), v(i, j + 1)))
    tris = np.asarray(tris)
    rows, cols, vals = [], [], []
    for t in tris:
        P = pts[t]
        Bm = np.array([[P[1, 0] - P[0, 0], P[2, 0] - P[0, 0]], [P[1, 1] - P[0, 1], P[2, 1] - P[0, 1]]])
        area = 0.5 * abs(np.linalg.det(Bm))
        G = np.linalg.inv(Bm).T @ np.array([[-1.0, 1.0, 0.0], [-1.0, 0.0, 1.0]])
        K = area * G.T @ G
        rows.append(np.repeat(t, 3))
        cols.append(np.tile(t, 3))
        vals.append(K.ravel())
    n = pts.shape[0]
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A.sum_duplicates()
    return A, pts


def _parts(pts, k):
    """k parts of contiguous coordinate order (slabs along x, then y)."""
    order = np.lexsort((pts[:, 1], pts[:, 0]))
    return [np.sort(p) for p in np.array_split(order, k)]


def _local_rows(A, owned):
    """The rank's (n_owned, n_local) rows as a partitioned SellMatrix holds them: owned columns first, then the ghosts."""
    R = A[owned]
    ghosts = np.setdiff1d(np.unique(R.indices), owned)
    return R[:, np.concatenate([owned, ghosts])].tocsr(), ghosts


@pytest.mark.parametrize("k", [2, 3, 8])
def test_owned_block_is_the_spd_submatrix(k):
    from oasisx_amd.amg import build_levels, owned_block

    A, pts = _p1_neumann(24)
    assert np.abs(A @ np.ones(A.shape[0])).max() < 1e-12
    for owned in _parts(pts, k):
        M, ghosts = _local_rows(A, owned)
        assert ghosts.size > 0 and M.shape == (owned.size, owned.size + ghosts.size)
        B = owned_block(M)
        ref = A[owned][:, owned]
        assert B.shape == ref.shape and abs(B - ref).max() == 0.0
        np.linalg.cholesky(B.toarray())  # SPD: a principal submatrix of the Neumann matrix, not the whole of it
        levels = build_levels(B, {"pc_gamg_coarse_eq_limit": 20})
        Ac, inv = levels[-1].A.toarray(), levels[-1].inv
        # nonsingular: the coarse inverse is the inverse, not the projection that annihilates the constants
        assert np.abs(inv @ Ac - np.eye(Ac.shape[0])).max() < 1e-8
        assert np.abs(inv @ np.ones(Ac.shape[0])).max() > 1e-3


def _bj_apply(blocks, r):
    from oasisx_amd.amg import vcycle_numpy

    z = np.zeros_like(r)
    for owned, levels in blocks:
        z[owned] = vcycle_numpy(levels, r[owned])
    return z


def _pcg(A, b, prec, rtol=1e-10, max_it=5000):
    """The one-column PCG of OX_KSP_CG_MG: the same recurrences and the test |B r| <= rtol |B b|."""
    x = np.zeros_like(b)
    r = b.copy()
    z = prec(r)
    bn = np.linalg.norm(z)
    p = z.copy()
    rz = r @ z
    for it in range(1, max_it + 1):
        q = A @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        z = prec(r)
        if np.linalg.norm(z) <= rtol * bn:
            return x, it
        rz, rz_old = r @ z, rz
        p = z + (rz / rz_old) * p
    raise AssertionError("no convergence")


def _blocks(A, pts, k, opts):
    from oasisx_amd.amg import build_levels, owned_block

    out = []
    for owned in _parts(pts, k):
        M, _ = _local_rows(A, owned)
        out.append((owned, build_levels(owned_block(M), opts)))
    return out


def test_block_jacobi_vcycle_pcg_model():
    from oasisx_amd.amg import build_levels, vcycle_numpy

    A, pts = _p1_neumann(32)
    n = A.shape[0]
    opts = {"pc_gamg_coarse_eq_limit": 20}
    rng = np.random.default_rng(7)
    b = np.cos(3.0 * pts[:, 0]) * (1.0 + pts[:, 1]) + np.sin(2.0 * pts[:, 1])
    b -= b.mean()
    ref = np.linalg.solve(A.toarray() + np.ones((n, n)) / n, b)  # the mean-free solution
    ref -= ref.mean()
    dinv = 1.0 / A.diagonal()
    _, it_jac = _pcg(A, b, lambda r: dinv * r)
    its = {}
    for k in (2, 3, 8):
        blocks = _blocks(A, pts, k, opts)
        u, v = rng.standard_normal(n), rng.standard_normal(n)
        Bu, Bv = _bj_apply(blocks, u), _bj_apply(blocks, v)
        assert abs(Bu @ v - u @ Bv) <= 1e-12 * abs(Bu @ v)  # B symmetric
        x, its[k] = _pcg(A, b, lambda r: _bj_apply(blocks, r))
        x -= x.mean()
        assert np.abs(x - ref).max() <= 1e-7 * np.abs(ref).max(), k
        assert its[k] < it_jac, (its, it_jac)
    # one part: the one block is the whole (singular) operator -- plain gamg
    one = _blocks(A, pts, 1, opts)
    levels = build_levels(A, opts)
    _, it1 = _pcg(A, b, lambda r: _bj_apply(one, r))
    _, itg = _pcg(A, b, lambda r: vcycle_numpy(levels, r))
    assert it1 == itg, (it1, itg)
