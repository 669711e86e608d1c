"""CPU: the preconditions of tests/test_gpu_partitioned_cuts.py.

A one-rank plan whose only peer is the rank itself turns the local n x (n + ng) matrix of a partitioned operator into
A_eff = A_loc[:, :n] + A_loc[:, n:] S, S[j, send[j]] = 1, on owned vectors.  ``reduction_systems.ghosted`` moves the far
lower band of the rows from r0 on into ghost columns, so that A_eff is the system the k-step model already serves:

  * the fold is exact, entry for entry, for every system the GPU test uses;
  * the interior / boundary slice counts are what the GPU test's partial-row counts assume, neither a multiple of 4
    (both grids of the split mat-vec end in a partly filled block), and the send list is not monotone;
  * the float64 run of the model stays within PRE = 1e-13 of the extended one on these systems (checked inside
    ``cut_solves._Reference``).  Measured: at most 6.4e-16 over all columns and cuts; dominance at least 0.25;
  * the block-Jacobi AMG case: the hierarchy of the owned block has at least 2 levels, and AMG-CG with that
    preconditioner on A_eff satisfies the float64-against-extended bound of tests/test_amg_steps_host.py.
"""
import numpy as np
import pytest

from tests import amg_steps_model as M
from tests import cut_solves as CS
from tests import reduction_systems as RS
from tests.test_amg_steps_host import PRE as AMG_PRE


def test_split_parts_is_the_sum_of_two_rounded_grids():
    assert RS.split_parts(11, 18) == 16 and RS.split_parts(0, 29) == 8 == RS.spmv_parts(1829)
    assert RS.split_parts(4, 4) == 16 and RS.split_parts(32, 33) == 8 + 16
    n = RS.rows_for_parts(776)
    ni, nb = RS.slice_kinds(RS.ghosted(RS.banded_system(n, "dict", 0), RS.ghost_start(n), 0)[0])
    assert RS.split_parts(ni, nb) > 3 * 256  # the two-grid total stays beyond the 4-rows-in-flight threshold


@pytest.mark.parametrize("nparts,kind", CS.PART_SYSTEMS, ids=[f"{p}-{k}" for p, k in CS.PART_SYSTEMS])
def test_ghosted_systems_fold_back_exactly(nparts, kind):
    n = RS.rows_for_parts(nparts)
    m, r0 = RS.band_offset(n), CS.part_r0(nparts)
    Acsr, A_loc, send, ref = CS.part_system(nparts, kind)
    ng = n - r0
    assert A_loc.shape == (n, n + ng) and A_loc.has_sorted_indices and send.shape == (ng,)
    assert r0 > m and r0 % 64 not in (0, 63)
    D = RS.folded(A_loc, send) - Acsr
    D.eliminate_zeros()
    assert D.nnz == 0 and RS.folded(A_loc, send).nnz == Acsr.nnz
    # every ghost column is read by exactly one row, every row from r0 on reads exactly one; the send list is a
    # permutation of the rows r0 - m .. n - m - 1 and not monotone
    ghost = A_loc[:, n:].tocoo()
    assert np.array_equal(np.sort(ghost.col), np.arange(ng)) and np.array_equal(np.sort(ghost.row), np.arange(r0, n))
    assert np.array_equal(send[ghost.col], ghost.row - m)
    assert np.array_equal(np.sort(send), np.arange(r0 - m, n - m)) and (np.diff(send) < 0).sum() > ng // 4
    ni, nb = RS.slice_kinds(A_loc)
    assert ni == r0 // 64 and ni + nb == (n + 63) // 64 and ni % 4 != 0 and nb % 4 != 0
    if nparts == CS.SMALL:
        assert (n, m, r0, ni, nb) == (1829, 609, 725, 11, 18) and RS.split_parts(ni, nb) == 16
    assert RS.dominance(Acsr) > 0.15
    for guess in (False, True):
        for c in range(3):
            ref.get(c, guess)  # (asserts PRE)
    print(f"{nparts}-{kind}: n {n}, r0 {r0}, {ni} interior + {nb} boundary slices, split parts {RS.split_parts(ni, nb)}, "
          f"dominance {RS.dominance(Acsr):.2f}, float64 against extended {ref.worst_pre:.1e}")


def test_the_block_jacobi_amg_case():
    n, m = M.CASES[CS.AMG_PART][:2]
    A, A_loc, send, levels, b = CS.amg_part_system()
    r0 = CS.amg_part_r0()
    assert r0 > m and r0 % 64 not in (0, 63) and A_loc.shape == (n, 2 * n - r0)
    D = RS.folded(A_loc, send) - A
    D.eliminate_zeros()
    assert D.nnz == 0
    ni, nb = RS.slice_kinds(A_loc)
    assert ni == r0 // 64 and ni % 4 != 0 and nb % 4 != 0
    rows = [lev.A.shape[0] for lev in levels]
    assert len(levels) >= 2 and rows[0] == n
    assert (levels[0].A != A_loc[:, :n]).nnz == 0 and levels[0].A.nnz < A.nnz  # the block, not the operator
    hi = M.amg_cg_trace(A, levels, b, None, 2)
    lo = M.amg_cg_trace(A, levels, b, None, 2, dtype=np.float64)
    for k, (h, l) in enumerate(zip(hi, lo)):
        ex = float(np.abs(np.asarray(l[0], dtype=np.longdouble) - h[0]).max() / np.abs(h[0]).max()) if k else 0.0
        eb, er = float(abs(l[1] - h[1]) / h[1]), float(abs(l[2] - h[2]) / h[1])
        print(f"{CS.AMG_PART} r0 {r0} levels {rows} k={k}: x {ex:.2e}  |B b| {eb:.2e}  |z_k| {er:.2e}  "
              f"(|z_k| / |B b| = {float(h[2] / h[1]):.3e})")
        assert ex <= AMG_PRE and eb <= AMG_PRE and er <= AMG_PRE
