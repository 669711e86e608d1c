"""CPU: the host side of pc_type gamg (oasisx_amd/amg.py) -- aggregation, prolongators, Galerkin coarse operators, the
coarsest inverse and the numpy V-cycle -- on small P1 / P2 Laplacians of the oracle's forms."""
import numpy as np
import pytest
import scipy.sparse as sp

from oasisx_amd import amg
from oracle import ipcs_oracle as O


def _laplacian(dim, N, deg, dirichlet):
    if dim == 2:
        coords, cells = O.create_rectangle_mesh((0.0, 0.0), (1.0, 1.0), (N, N))
    else:
        coords, cells = O.create_box_mesh((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (N, N, N))
    F = O.Forms(coords, cells, deg, deg)
    A = F.stiffness_q().tocsr()
    if dirichlet:
        # what ox_zero_rows_cols leaves for the pressure's Dirichlet rows: row and column zeroed, 1 on the diagonal
        x = F.x_q
        bd = ((np.abs(x) < 1e-12) | (np.abs(x - 1.0) < 1e-12)).any(axis=1) & (x[:, 0] < 0.5)
        D = sp.diags(bd.astype(np.float64))
        I = sp.identity(A.shape[0]) - D
        A = (I @ A @ I + D).tocsr()
    return A


CASES = [(3, 5, 1, True), (3, 5, 1, False), (2, 8, 2, True), (2, 8, 2, False), (3, 3, 2, True)]


@pytest.mark.parametrize("dim,N,deg,dirichlet", CASES)
def test_aggregates_partition_the_non_singleton_rows(dim, N, deg, dirichlet):
    A = _laplacian(dim, N, deg, dirichlet)
    Ae = A.copy()
    Ae.eliminate_zeros()
    off = np.diff(Ae.indptr) - (Ae.diagonal() != 0)
    agg, nagg = amg.aggregate(Ae)
    single = off == 0
    assert (single.any()) == dirichlet
    assert (agg[single] == -1).all()  # singletons: no aggregate
    assert (agg[~single] >= 0).all() and (agg < nagg).all()  # every other row in exactly one
    assert np.unique(agg[~single]).size == nagg  # no empty aggregate
    P = amg.tentative_prolongator(agg, nagg)
    one = P @ np.ones(nagg)
    assert np.array_equal(one, (~single).astype(np.float64))  # reproduces the constants on the aggregated rows


@pytest.mark.parametrize("dim,N,deg,dirichlet", CASES)
def test_galerkin_coarse_operators(dim, N, deg, dirichlet):
    A = _laplacian(dim, N, deg, dirichlet)
    levels = amg.build_levels(A, {"pc_gamg_coarse_eq_limit": 10})
    assert len(levels) >= 2
    for fine, coarse in zip(levels[:-1], levels[1:]):
        ref = (fine.P.T @ fine.A @ fine.P).toarray()
        Ac = coarse.A.toarray()
        assert np.abs(Ac - ref).max() <= 1e-13 * np.abs(ref).max()
        assert np.abs(Ac - Ac.T).max() <= 1e-13 * np.abs(Ac).max()
        assert (fine.R != fine.P.T).nnz == 0  # R = P^T, stored
        assert fine.A.shape[0] > coarse.A.shape[0]
        assert 0.5 < fine.lmax < 4.0 and len(fine.cheb) == 2


@pytest.mark.parametrize("dim,N,deg", [(3, 5, 1), (2, 8, 2)])
def test_singular_coarsest_inverse_annihilates_constants(dim, N, deg):
    A = _laplacian(dim, N, deg, False)
    assert np.abs(A @ np.ones(A.shape[0])).max() < 1e-12  # pure Neumann: singular
    levels = amg.build_levels(A)
    inv, Ac = levels[-1].inv, levels[-1].A.toarray()
    n = inv.shape[0]
    assert len(levels) >= 2 and n > 1
    assert np.abs(inv @ np.ones(n)).max() <= 1e-12 * np.abs(inv).max()
    # a pseudo-inverse on the mean-free subspace
    Q = np.eye(n) - np.ones((n, n)) / n
    assert np.abs(Ac @ inv @ Ac - Ac).max() <= 1e-10 * np.abs(Ac).max()
    assert np.abs(inv @ Ac - Q).max() <= 1e-10


@pytest.mark.parametrize("dim,N,deg,dirichlet", CASES)
def test_vcycle_is_symmetric_and_positive(dim, N, deg, dirichlet):
    A = _laplacian(dim, N, deg, dirichlet)
    levels = amg.build_levels(A, {"pc_gamg_coarse_eq_limit": 10})
    n = A.shape[0]
    B = np.column_stack([amg.vcycle_numpy(levels, e) for e in np.eye(n)])
    assert np.abs(B - B.T).max() <= 1e-11 * np.abs(B).max()
    if not dirichlet:  # positive on the mean-free subspace (the constants are A's null space)
        Q = np.eye(n) - np.ones((n, n)) / n
        w = np.linalg.eigvalsh(Q @ (0.5 * (B + B.T)) @ Q)
        assert (w[1:] > 0).all() and abs(w[0]) < 1e-10 * w[-1]
    else:
        assert np.linalg.eigvalsh(0.5 * (B + B.T))[0] > 0


def test_vcycle_preconditioned_cg_converges_fast():
    A = _laplacian(3, 10, 1, True)
    levels = amg.build_levels(A)
    b = np.cos(np.arange(A.shape[0]) * 0.37)
    x = np.zeros_like(b)
    r = b.copy()
    z = amg.vcycle_numpy(levels, r)
    p, rz, bn = z.copy(), r @ z, np.linalg.norm(z)
    for it in range(1, 100):
        q = A @ p
        a = rz / (p @ q)
        x += a * p
        r -= a * q
        z = amg.vcycle_numpy(levels, r)
        if np.linalg.norm(z) <= 1e-8 * bn:
            break
        rz, rz_old = r @ z, rz
        p = z + rz / rz_old * p
    assert it <= 15
    assert np.linalg.norm(A @ x - b) <= 1e-6 * np.linalg.norm(b)


def test_setup_is_deterministic():
    A = _laplacian(3, 6, 1, True)
    L1, L2 = amg.build_levels(A), amg.build_levels(A.copy())
    assert len(L1) == len(L2)
    for a, b in zip(L1, L2):
        assert (a.A != b.A).nnz == 0 and np.array_equal(a.dinv, b.dinv)
        if a.P is not None:
            assert np.array_equal(a.agg, b.agg) and (a.P != b.P).nnz == 0 and a.cheb == b.cheb
    assert np.array_equal(L1[-1].inv, L2[-1].inv)


def test_options_change_the_hierarchy():
    A = _laplacian(3, 6, 1, True)
    assert len(amg.build_levels(A, {"pc_mg_levels": 1})) == 1  # the dense solve alone
    three = amg.build_levels(A, {"mg_levels_ksp_max_it": 3, "pc_gamg_coarse_eq_limit": 10})
    assert len(three[0].cheb) == 3
    lo = amg.build_levels(A, {"pc_gamg_threshold": 0.0})
    hi = amg.build_levels(A, {"pc_gamg_threshold": 0.2})
    assert lo[1].A.shape[0] != hi[1].A.shape[0]
    with pytest.raises(ValueError):
        amg.build_levels(_laplacian(3, 16, 1, True), {"pc_mg_levels": 1})
