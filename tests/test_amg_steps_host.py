"""CPU: the preconditions of tests/test_gpu_amg_steps.py -- what makes a miss of the device attributable to the device.

  * the recursive model V-cycle (tests/amg_steps_model.py) and the product's numpy twin (``amg.vcycle_numpy``) agree to
    1e-13 on every case, so that the device is compared with one cycle, not with one of two;
  * the float64 run of the model V-cycle and of the AMG-CG trace agrees with the extended-precision run to PRE = 1e-13
    (x relative to max |x|, the norms relative to |B b|): the systems themselves allow the device's TOL = 1e-12.
    Measured: V-cycle <= 2.5e-15, x_k (k <= 3) <= 1.4e-14, norms <= 9.9e-15 |B b|; the twins <= 8.8e-16;
  * sensitivity: zeroing the prolongation from any level j >= 1 moves z by at least 1e-2 relative, so a wrong deep level
    cannot stay under TOL.  Measured: 0.97 / 0.89 / 0.61 / 0.20 for the five-level Dirichlet hierarchy, 0.066 at the
    coarsest level of the Neumann one, 0.034 at the coarsest level of the degree-8 one;
  * shapes: the five-level hierarchies have the levels the device branches need (properties, not exact counts; measured
    198 437 / 26 953 / 1616 / 74 / 3 rows);
  * the schedule test's tolerance is a factor 2 away from the model's |z_k| / |B b| on both sides of the stopping
    iteration, and the ksp_atol of the reasons test separates |z_1| from |z_2| likewise.
"""
import numpy as np
import pytest

from oasisx_amd import amg
from tests import amg_steps_model as M
from tests import reduction_systems as RS

PRE = 1e-13
SENSITIVITY = 1e-2
NAMES = list(M.CASES)


def _rel(a, ref):
    return float(np.abs(np.asarray(a, dtype=np.longdouble) - ref).max() / np.abs(ref).max())


def test_the_operators_are_what_the_model_says():
    for name, (n, m, kind, seed, _, _) in M.CASES.items():
        A = M.system(name)[0]
        assert A.shape == (n, n) and abs(A - A.T).max() == 0.0 and np.diff(A.indptr).max() <= 5
        off = A.tocoo()
        assert set(np.unique(np.abs(off.row - off.col))) <= {0, 1, m}
        d = A.diagonal()
        slack = d - (np.asarray(abs(A).sum(axis=1)).ravel() - d)
        assert slack.min() > -1e-12 and (slack < 1e-12).mean() > 0.9  # weakly dominant: most rows with no slack at all
        single = np.diff(A.indptr) == 1
        if kind == "neumann":
            assert not single.any() and np.abs(A @ np.ones(n)).max() <= 1e-12 * abs(A).max()
        else:
            assert single.sum() == n // M.IDENTITY_EVERY and (d[single] == 1.0).all()
            agg = amg.aggregate(A)[0]
            assert (agg[single] == -1).all() and (agg[~single] >= 0).all()  # the singletons: empty rows of P
        if kind == "dict":
            assert np.unique(A.data).size <= 256 and np.unique(1.0 / d).size <= 256
        else:
            assert np.unique(d).size > 256


@pytest.mark.parametrize("name", NAMES)
def test_the_twins_agree(name):
    _, levels, _ = M.system(name)
    b, _ = M.reference_vcycles(name)
    for c in range(2):
        own = M.vcycle(M.cast_system(name, np.float64), b[:, c], np.float64)
        twin = amg.vcycle_numpy(levels, b[:, c])
        e = float(np.abs(own - twin).max() / np.abs(twin).max())
        print(f"{name} b{c + 1}: model against amg.vcycle_numpy {e:.2e}")
        assert e <= 1e-13


@pytest.mark.parametrize("name", NAMES)
def test_float64_vcycle_against_extended(name):
    b, hi = M.reference_vcycles(name)
    lo = M.reference_vcycles(name, np.float64)[1]
    for c in range(2):
        e = _rel(lo[c], hi[c])
        print(f"{name} b{c + 1}: float64 against extended {e:.2e}")
        assert e <= PRE


@pytest.mark.parametrize("name", M.CG_SYSTEMS)
def test_float64_amg_cg_against_extended(name):
    for guess in (False, True):
        hi = M.reference_trace(name, guess)[2]
        lo = M.reference_trace(name, guess, np.float64)[2]
        assert len(hi) == len(lo) == (2 if name == "one" else (3 if guess else 4))
        for k, (h, l) in enumerate(zip(hi, lo)):
            ex = _rel(l[0], h[0]) if k or guess else 0.0
            eb, er = float(abs(l[1] - h[1]) / h[1]), float(abs(l[2] - h[2]) / h[1])
            print(f"{name} guess={int(guess)} k={k}: x {ex:.2e}  |B b| {eb:.2e}  |z_k| {er:.2e}  (|z_k| / |B b| = {float(h[2] / h[1]):.3e})")
            assert ex <= PRE and eb <= PRE and er <= PRE


@pytest.mark.parametrize("name", [n for n in NAMES if n != "one"])
def test_every_level_moves_z(name):
    _, levels, _ = M.system(name)
    b, _ = M.reference_vcycles(name)
    z = M.reference_vcycles(name, np.float64)[1][0]
    for j in range(1, len(levels)):
        zj = M.vcycle(M.without_prolongation(levels, j), b[:, 0], np.float64)
        s = float(np.abs(zj - z).max() / np.abs(z).max())
        print(f"{name}: without the prolongation from level {j}: z moves by {s:.3g}")
        assert s >= SENSITIVITY


def test_shapes_reach_the_device_branches():
    assert M.BIG_N == RS.rows_for_parts(776) and RS.vec_parts(M.BIG_N) > 768 and RS.spmv_parts(M.BIG_N) > 768
    for name in ("five", "five-dict", "five-neumann-deg3"):
        rows = [lev.A.shape[0] for lev in M.system(name)[1]]
        print(name, rows)
        assert len(rows) >= 5 and rows[0] == M.BIG_N
        assert any(r > 2048 for r in rows[1:])  # a middle level on the grid
        tail = [r for r in rows if r <= 2048]
        assert 1024 < tail[0] <= 2048  # the default tail's first level: two rounds of the 1024-thread loop
        assert len(tail) >= 3 and all(r % 64 for r in rows)
        assert 16384 < rows[1] <= 32768  # tail_rows = 32768: that level in the tail too
    assert len(M.system("five-neumann-deg3")[1][0].cheb) == 3
    # two levels, degree 1: a coarsest level the dense solve and the tail loop need two rounds for; level 0 fits 16384
    for name in ("two-deg1", "two-deg1-dict"):
        levels = M.system(name)[1]
        rows = [lev.A.shape[0] for lev in levels]
        assert len(rows) == 2 and 1024 < rows[1] <= 4096 and 2048 < rows[0] <= 16384 and rows[0] > 12 * 1024
        assert all(r % 64 for r in rows) and len(levels[0].cheb) == 1 and levels[0].cheb[0][0] == 0.0
    assert [lev.A.shape[0] for lev in M.system("one")[1]] == [1061]
    for name in ("deg8", "deg9"):  # (9 clamps to 8)
        levels = M.system(name)[1]
        assert len(levels) >= 3 and all(len(lev.cheb) == amg.MAX_DEGREE == 8 for lev in levels[:-1])
        assert all(cd != 0.0 for cd, _ in levels[0].cheb[1:])


def test_the_model_stops_where_the_schedule_test_expects():
    tr = M.reference_trace("five", False, kmax=M.SCHEDULE_ITS, seed=M.SCHEDULE_SEED)[2]
    rel = [float(t[2] / t[1]) for t in tr]
    k = M.stopping_iteration(tr, M.SCHEDULE_RTOL)
    print("|z_k| / |B b|:", " ".join(f"{r:.3e}" for r in rel))
    assert k == M.SCHEDULE_ITS > 8  # (more than one batch of 8 iterations)
    assert all(r >= 2.0 * M.SCHEDULE_RTOL for r in rel[:k]) and rel[k] <= 0.5 * M.SCHEDULE_RTOL
    # the reasons test: ksp_atol = ATOL_FACTOR |z_2| ends the solve at iteration 2, not before
    tr = M.reference_trace("five", False)[2]
    atol = M.ATOL_FACTOR * float(tr[2][2])
    assert M.stopping_iteration(tr, 1e-30, atol) == 2
    assert float(tr[1][2]) >= 1.5 * atol and float(tr[2][2]) <= atol / 1.5
