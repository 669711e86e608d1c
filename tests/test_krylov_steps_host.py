"""CPU: the extended-precision k-step reference of the Jacobi-CG / Jacobi-BiCGStab solvers (tests/krylov_steps_model.py)
against the oracle's own solvers cut at ``max_it``, and the mesh-free test systems of tests/test_gpu_reduction_sizes.py:
strictly diagonally dominant, of the kind each says it is, with partial-row counts that follow the library's formulas."""
import numpy as np
import pytest

from oracle import ipcs_oracle as O
from tests import krylov_steps_model as K
from tests import reduction_systems as RS


def test_the_model_sums_in_more_than_double_precision():
    from fractions import Fraction

    assert K.DOT_EPS < (1e-18 if K.EXTENDED else 3e-16)
    # the exact dot product: cancellation that float64 accumulation loses
    x = np.array([1e16, 1.0, -1e16, 0.1])
    y = np.array([1.0, 0.3, 1.0, 0.7])
    assert K.exact_dot(x, y) == float(sum(Fraction(float(a)) * Fraction(float(c)) for a, c in zip(x, y)))
    p, e = K.two_product(np.array([1.0 + 2.0**-30]), np.array([1.0 + 2.0**-30]))
    assert p[0] == 1.0 + 2.0**-29 and e[0] == 2.0**-60


@pytest.mark.parametrize("kind", RS.KINDS)
def test_k_step_iterates_equal_the_oracle_cut_at_max_it(kind):
    n, k = 997, 5
    A = RS.banded_system(n, kind, seed=3)
    b = RS.signed_unit_vectors(n, 2, seed=3)
    x0 = 0.25 * RS.signed_unit_vectors(n, 1, seed=4)[:, 0]
    for guess in (None, x0):
        if kind != "nonsym":
            xo, reason, its, rn = O.jacobi_cg(A, b[:, 0], x0=guess, rtol=1e-30, atol=1e-50, max_it=k)
            xm, bn, rm = K.jacobi_cg_steps(A, b[:, 0], guess, k)
            assert reason == O.DIVERGED_ITS and its == k
            assert np.abs(xm.astype(np.float64) - xo).max() <= 1e-13 * np.abs(xo).max()
            assert abs(float(rm) - rn) <= 1e-13 * float(bn)
            assert abs(float(bn) - np.linalg.norm(b[:, 0] / A.diagonal())) <= 1e-14 * float(bn)
        xo, reason, its, rn = O.jacobi_bicgstab(A, b[:, 1], x0=guess, rtol=1e-30, atol=1e-50, max_it=k)
        xm, bn, rm = K.jacobi_bicgstab_steps(A, b[:, 1], guess, k)
        assert reason == O.DIVERGED_ITS and its == k
        assert np.abs(xm.astype(np.float64) - xo).max() <= 1e-13 * np.abs(xo).max()
        assert abs(float(rm) - rn) <= 1e-13 * float(bn)
        # the recurrence norm of the merged-reduction form is the true norm in exact arithmetic
        tr = K.jacobi_bicgstab_trace(A, b[:, 1], guess, k)
        assert all(abs(float(t[3] - t[2])) <= 1e-15 * float(t[1]) for t in tr)


def test_the_float64_run_of_the_model_stays_within_1e_13_of_the_extended_one():
    n = 4099
    for kind, steps in (("sym", K.jacobi_cg_trace), ("dict", K.jacobi_cg_trace), ("nonsym", K.jacobi_bicgstab_trace)):
        A = RS.banded_system(n, kind, seed=1)
        b = RS.signed_unit_vectors(n, 1, seed=1)[:, 0]
        hi, lo = steps(A, b, None, 3), steps(A, b, None, 3, dtype=np.float64)
        for h, l in zip(hi, lo):
            assert l[0].dtype == np.float64
            assert np.abs(h[0] - l[0]).max() <= 1e-13 * max(np.abs(h[0]).max(), 1e-300)
            assert abs(h[2] - l[2]) <= 1e-13 * h[1]


@pytest.mark.parametrize("kind", RS.KINDS)
@pytest.mark.parametrize("n", [8, 997, 194341])
def test_the_systems_are_strictly_diagonally_dominant_and_of_their_kind(kind, n):
    A = RS.banded_system(n, kind, seed=n % 7)
    m = RS.band_offset(n)
    assert A.shape == (n, n) and A.has_sorted_indices and (A.diagonal() > 0).all()
    assert RS.dominance(A) > 0.15
    assert set(np.unique(A.tocoo().col - A.tocoo().row)) == {-m, -1, 0, 1, m}
    asym = abs(A - A.T).max()
    assert (asym > 0.05) if kind == "nonsym" else (asym == 0.0)
    nd = np.unique(A.diagonal()).size
    if kind == "dict":
        assert np.unique(A.data).size <= 12 and nd <= 8
    elif n > 300:
        assert nd > 256 and np.unique(A.data).size > 0.9 * A.nnz * (0.6 if kind == "sym" else 1.0)
    b = RS.signed_unit_vectors(n, 3, seed=1)
    assert (np.abs(b) >= 0.5).all() and (np.abs(b) <= 1.5).all()
    assert n < 100 or 0.4 < (b > 0).mean() < 0.6


def test_partial_row_counts_follow_the_library_formulas():
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oasisx_amd", "csrc", "ox_kernels.h")).read()
    # round8(ceil(n_slices / 4)) and the grid caps, as ox_kernels.h states them
    assert re.search(r"ngroups = \(n_slices \+ 3\) / 4;", src) and re.search(r"g8 = \(ngroups \+ 7\) & ~7;", src)
    m = re.search(r"return n >= \(\(int64_t\)1 << (\d+)\) \? (\d+) : (\d+);", src)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (24, 1024, 2048)
    for nparts in (8, 760, 776, 2568, 4104, 10248):
        n = RS.rows_for_parts(nparts)
        assert RS.spmv_parts(n) == nparts
        assert n % 64 == 37 and ((n + 63) // 64) % 4 == 1
    assert RS.vec_parts(194341) == 760 and RS.vec_parts(600000) == 2048 and RS.vec_parts(1 << 23) == 1024
    assert RS.vec_parts((1 << 23) - 1) == 2048
