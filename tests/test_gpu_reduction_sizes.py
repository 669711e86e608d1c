"""GPU: the second stage of the Krylov reductions at the partial-row counts where it changes path.

Every Krylov scalar comes out of a two-stage ordered reduction: a mat-vec epilogue or an update kernel writes one row
of partial sums per block, one block sums the rows and runs the scalar logic.  That second stage branches on the number
of rows; below about 200 k matrix rows none of the branches is taken, and the suites that do cross them assert only
that solves converge -- which a Krylov method does with a slightly wrong scalar too, an iteration or two later.  Here
solves are CUT after k = 1, 2, 3 iterations (``ksp_rtol`` 1e-30, ``ksp_max_it`` k) and the k-th iterate and both norms
are compared with the extended-precision reference of tests/krylov_steps_model.py to 1e-12: a partial row lost or read
twice moves a sum by about 1 / nparts >= 1e-5 relative and the iterate with it.

Operators: mesh-free banded matrices (bands 0, +-1, +-m; ``reduction_systems.banded_system``) through
``fem.build_sell`` + ``SellMatrix`` + ``values_from_csr``, so that n_rows is exact; the mat-vec is pinned to the lane =
row kernel (``set_levels(7)``), whose epilogue writes round8(ceil(n_slices / 4)) partial rows.  n_rows = 64 (4 (nparts
- 1)) + 37: n_rows % 64 != 0 and n_slices % 4 != 0.  The vector kernels write min(ceil(n / 256), 2048) rows.

    branch (source)                                            threshold            nparts    n_rows
    -- none: the control                                       <= 3 * 256              760     194 341
    4 rows in flight, ksp_gather_t / ox_gather_partials        > 3 * 256 = 768         776     198 437
    second round of ksp_gather_rows<., 10>, 256 threads        > 10 * 256 = 2560      2568     657 189
    1024-thread reduction block (ox_red_threads)               > 4096                 4104   1 050 405
    second round of ksp_gather_rows<., 10>, 1024 threads;
      ``np_ > U * T`` of ksp_fold_point (folded CG);
      merged CG leaves its folded form (nbs1 > 10 * OX_FOLD_T) > 10 * 1024 = 10240   10248   2 623 269
    k_prereduce, last chunk partial, nparts * nv >= 16384:
      merged BiCGStab, 3 columns (nv = 15)                     >= 1093                1096     280 357
      BiCGStab, 3 columns (nv = 6)                             >= 2731                2736     700 197
      CG / single-reduction CG, 3 columns (nv = 3)             >= 5462                5464   1 398 565
    (the vector kernels' 2048 rows x 9 sums of a 3-column CG start are pre-reduced from 524 289 rows on as well)

The thresholds are read from the sources at test time (``test_the_sizes_cross_the_thresholds_the_sources_state``): a
retune fails that test instead of silently un-crossing a branch.  One CG system has <= 256 distinct values ("dict"):
``SellMatrix.freeze`` gives it a value dictionary and the solver a dictionary of dinv, so the folded kernels run their
``CODE = true`` instantiation.  The FE case (2-D P1 rectangle, 1096 x 1096 vertices, default levels) runs the same checks
on the LDS-window mat-vec, whose partial rows are window blocks (2347 blocks, a grid of 2352).  Its set-up -- mesh,
space and window stream -- was measured at 0.3 s on an MI355X, each of its two cases at about 4 s in all, so the size
the issue names was kept.

What a cut returns.  Every method returns the k-th iterate (the standard CG's last ``x += alpha p`` is applied by the
host once the device reports the end; the merged BiCGStab's by ``bcgsm_finish``).  The norm reported is the one the
method tests: |D^-1 r_k| of the recurrence residual for the CG forms and BiCGStab -- equal to the true residual's to
rounding --, and for the merged-reduction BiCGStab the recurrence norm sqrt(s.s - 2 omega t.s + omega^2 t.t)
(csrc/ox_ksp_dev.h, PH_BCGSM_B: ``double rr = fma(om, fma(om, tt, -2.0 * ts), ss)``; the stored residual is tested only
for columns that norm declared converged, PH_BCGSM_FIN), which is compared with the same expression of the model.

Known uncovered branches: the merged CG's own pre-reduction (PH_CGM_IT: from 4 * 16384 sums, i.e. more than 8 M rows).
The partitioned synchronisation points (k_ksp_reduce + k_ksp_logic, k_ksp_scalar_p2p) are cut at 776, 1096 and 4104
partial rows on one-rank plans by tests/test_gpu_partitioned_cuts.py, which shares this file's helpers through
tests/cut_solves.py; sums over more than one rank's contribution remain with the multi-rank rehearsals.

Mutation check.  Run once on an MI355X, never committed: five mutant libraries built from scratch copies of the sources,
each making ONE gather loop skip one partial row, each run against the cases below and the 760-row control.  Every
mutant left the control (760-sym, 760-nonsym) passing and made the cases of its branch miss by 1e-6 .. 5e-3 in x:
    ox_gather_partials, 4-in-flight loop (thread 5 drops its 2nd row)   reached through k_reduce_partials only, so caught by
        tests/test_gpu_blas1.py: test_dot_against_the_exact_sum[*-2097153], [1-16777219] and test_remove_mean[*-1000003-777];
        every smaller ox_dot / ox_remove_mean case and the control passed
    ksp_gather_t, 4-in-flight loop (thread 5 drops its 2nd row)         776-sym, 776-nonsym, 776-dict, 4104-sym (all methods
        but the one-column bcgs)
    ksp_gather_rows, second round (thread 3 drops its 1st row there)    2568-sym, 2568-nonsym, 10248-sym, 10248-dict,
        10248-nonsym (the one-column cg, cg_merged, cg_merged_fold, bcgs, bcgs_merged); 776-* passed
    k_prereduce (chunk 1 drops its last row)                            1096-nonsym, 2736-nonsym (bcgs, bcgs_merged nc=3),
        5464-sym (cg and cg_single nc=3)
    ksp_fold_point, the np_ > U * T loop (thread 2 drops its 1st row)   10248-sym and 10248-dict, cg_fold and cg_fold1 only
        (the unfolded methods of the same cases passed)
"""
import numpy as np
import pytest
import torch

from tests import reduction_systems as RS
from tests.cut_solves import METHODS, PRE, TOL, _check_cuts, _Reference, _sell, _thresholds  # noqa: F401

CONTROL, IN_FLIGHT, ROUND2, WIDE, ROUND2_WIDE = 760, 776, 2568, 4104, 10248
PRERED_MBCGS3, PRERED_BCGS3, PRERED_CG3 = 1096, 2736, 5464

CG_1 = [(m, 1) for m in ("cg", "cg_fold1", "cg_fold", "cg_single", "cg_merged", "cg_merged_fold")]
CG_ALL = CG_1 + [("cg", 3), ("cg_single", 3)]  # (with 3 columns the fold setting and the merged form do not apply)
BCGS_1 = [("bcgs", 1), ("bcgs_merged", 1)]
BCGS_ALL = BCGS_1 + [("bcgs", 3), ("bcgs_merged", 3)]

CASES = [
    (CONTROL, "sym", CG_ALL), (CONTROL, "nonsym", BCGS_ALL),
    (IN_FLIGHT, "sym", CG_ALL), (IN_FLIGHT, "nonsym", BCGS_ALL), (IN_FLIGHT, "dict", CG_1),
    (PRERED_MBCGS3, "nonsym", [("bcgs_merged", 3), ("bcgs", 3)]),
    (ROUND2, "sym", CG_ALL), (ROUND2, "nonsym", BCGS_ALL),
    (PRERED_BCGS3, "nonsym", [("bcgs", 3), ("bcgs_merged", 3)]),
    (WIDE, "sym", CG_ALL), (WIDE, "nonsym", BCGS_ALL),
    (PRERED_CG3, "sym", [("cg", 3), ("cg_single", 3)]),
    (ROUND2_WIDE, "sym", CG_1), (ROUND2_WIDE, "dict", [("cg_fold", 1), ("cg_fold1", 1), ("cg", 1)]),
    (ROUND2_WIDE, "nonsym", BCGS_1),
]


def test_the_sizes_cross_the_thresholds_the_sources_state():
    T = _thresholds()
    small, wide, U = T["red_small"], T["red_wide"], T["rows_u"]
    for nparts in (CONTROL, IN_FLIGHT, ROUND2, WIDE, ROUND2_WIDE, PRERED_MBCGS3, PRERED_BCGS3, PRERED_CG3):
        n = RS.rows_for_parts(nparts)  # (asserts n % 64 != 0, n_slices % 4 != 0 and the row count)
        assert RS.spmv_parts(n) == nparts
    # the control takes none of the branches, in the mat-vec's rows and in the vector kernels'
    nc_ = RS.rows_for_parts(CONTROL)
    assert max(CONTROL, RS.vec_parts(nc_)) <= 3 * small and CONTROL * T["max_nv"] < T["prered_min"]
    # 4 rows in flight: some thread of a 256-thread block has p + 3 T < nparts; still one round of U rows, 256 threads
    assert 3 * small < IN_FLIGHT <= CONTROL + 16 and IN_FLIGHT <= U * small and IN_FLIGHT <= T["wide_from"]
    # second round of U rows per thread in a 256-thread block
    assert U * small < ROUND2 <= U * small + 8 and ROUND2 <= T["wide_from"]
    # the 1024-thread block, whose 4-in-flight loop runs as well, in one round of U rows
    assert T["wide_from"] < WIDE <= T["wide_from"] + 8 and 3 * wide < WIDE <= U * wide
    # second round in a 1024-thread block; the folded CG's surplus loop; the merged CG leaves its folded form
    assert U * wide < ROUND2_WIDE <= U * wide + 8
    assert T["fold_u"] * T["fold_t"] < ROUND2_WIDE < T["prered_min"] and T["cgm_fold_rows"] * T["fold_t"] < ROUND2_WIDE
    # pre-reduction: the smallest grid with nparts * nv >= OX_PRERED_MIN, its last chunk partial; nv = sums per column of
    # the point times 3 columns: PH_BCGSM_B 5, PH_BCGS_2 2, PH_CG_A 1
    for nparts, nv in ((PRERED_MBCGS3, 15), (PRERED_BCGS3, 6), (PRERED_CG3, 3)):
        assert (nparts - 8) * nv < T["prered_min"] <= nparts * nv and nparts % T["chunk"] != 0
        assert nv <= T["max_nv"]
    # out of reach here: the merged CG's own pre-reduction
    assert ROUND2_WIDE * 2 < T["cgm_prered"] * T["prered_min"]
    # the vector kernels' rows: capped at 2048 (no second round in a 256-thread block, never the wide block)
    assert RS.vec_parts(RS.rows_for_parts(ROUND2_WIDE)) == 2048 <= min(U * small, T["wide_from"])


@pytest.mark.gpu
@pytest.mark.parametrize("nparts,kind,runs", CASES, ids=[f"{p}-{k}" for p, k, _ in CASES])
def test_cut_solves_match_the_extended_precision_iterates(hip, nparts, kind, runs):
    from oasisx_amd import _lib

    n = RS.rows_for_parts(nparts)
    Acsr = RS.banded_system(n, kind, seed=nparts % 89)
    assert RS.dominance(Acsr) > 0.15
    A = _sell(Acsr, symmetric=kind != "nonsym")
    if kind == "dict":
        assert A.freeze(pairs="never") and A.vcode is not None
    A.set_levels(7)  # the lane = row kernel (no pair slots, no LDS windows): nparts partial rows
    assert A.pattern.n_slices % 4 != 0 and n % 64 != 0 and RS.spmv_parts(n) == nparts
    # the library's own word on the one threshold it reports: the merged CG folds up to 10 * OX_FOLD_T partial rows
    T = _thresholds()
    assert hip.ox_ksp_kernels_per_iteration(_lib.KSP_CG_MERGED, A.ref(), 1, 8, -1, 0) == \
        (2 if nparts <= T["cgm_fold_rows"] * T["fold_t"] else 3)
    ref = _Reference(Acsr, RS.signed_unit_vectors(n, 3, seed=nparts), 0.25 * RS.signed_unit_vectors(n, 3, seed=nparts + 1),
                     bicgstab=kind == "nonsym")
    print(f"nparts {nparts} ({kind}): n_rows {n}, vector-kernel rows {RS.vec_parts(n)}")
    misses = _check_cuts(A, ref, runs, n, dict_dinv=kind == "dict")
    assert not misses, "\n".join(misses)


# ---- the FE case: the LDS-window mat-vec, whose partial rows are window blocks -----------------------------------
FE_N = 1095  # cells per side: 1096^2 = 1 201 216 vertices (set-up measured at 0.3 s on an MI355X: not shrunk)


def _hash01(a, b):
    """Deterministic pseudo-random numbers in [0, 1) from two integer arrays."""
    v = np.sin(a.astype(np.float64) * 12.9898 + b.astype(np.float64) * 78.233) * 43758.5453
    return v - np.floor(v)


_FE = {}


def _fe_space():
    if "V" not in _FE:
        import time

        from oasisx_amd import fem
        from oasisx_amd import mesh as M

        t0 = time.time()
        mesh = M.create_rectangle(None, [[-1.0, -1.0], [1.0, 1.0]], [FE_N, FE_N])
        V = fem.FunctionSpace(mesh, 1)
        assert V.build_windows()
        torch.cuda.synchronize()
        P = V.pattern
        rows, k = P.slot_rows_k()
        rl = np.zeros(P.n_slices * 64, dtype=np.int64)
        rl[: P.n_rows] = P.row_len.cpu().numpy()
        _FE.update(V=V, rows=rows, cols=P.cols.cpu().numpy().astype(np.int64), real=k < rl[rows])
        print(f"FE set-up: {P.n_rows} rows, {P.n_wblocks} window blocks, {time.time() - t0:.1f} s")
    return _FE


def _fe_matrix(symmetric):
    """Strictly diagonally dominant values on the P1 pattern: off-diagonals in -[0.2, 0.5) from a hash of the entry's
    (row, column) -- of the unordered pair for the symmetric matrix --, diagonal (1.5 .. 2) x the row's absolute sum + 0.1."""
    from oasisx_amd.la import SellMatrix

    F = _fe_space()
    P, rows, cols, real = F["V"].pattern, F["rows"], F["cols"], F["real"]
    lo, hi = (np.minimum(rows, cols), np.maximum(rows, cols)) if symmetric else (rows, cols)
    off = real & (rows != cols)
    vals = np.where(off, -(0.2 + 0.3 * _hash01(lo, hi)), 0.0)
    s = np.bincount(rows[off], weights=np.abs(vals[off]), minlength=P.n_slices * 64)
    dg = real & (rows == cols)
    vals[dg] = s[rows[dg]] * (1.5 + 0.5 * _hash01(rows[dg], rows[dg] + 7)) + 0.1
    A = SellMatrix(P, symmetric=symmetric)
    A.vals.copy_(torch.from_numpy(vals).cuda())
    A.version += 1
    return A, A.to_scipy()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,runs", [("sym", [("cg_fold", 1), ("cg", 1), ("cg_merged_fold", 1), ("cg", 3), ("cg_single", 3)]),
                                       ("nonsym", [("bcgs", 1), ("bcgs", 3), ("bcgs_merged", 3)])], ids=["sym", "nonsym"])
def test_cut_solves_on_the_window_stream_grid(hip, kind, runs):
    T = _thresholds()
    A, Acsr = _fe_matrix(kind == "sym")
    P = A.pattern
    n = P.n_rows
    assert n == (FE_N + 1) ** 2 and A._struct.n_wblocks == P.n_wblocks > 0 and A.levels is None  # default levels: windows
    grid = (P.n_wblocks + 7) & ~7
    assert 3 * T["red_small"] < grid != RS.spmv_parts(n)  # window blocks, not slice groups, and more than 768 of them
    assert RS.dominance(Acsr) > 0.15
    asym = abs(Acsr - Acsr.T).max()
    assert asym == 0.0 if kind == "sym" else asym > 0.05
    ref = _Reference(Acsr, RS.signed_unit_vectors(n, 3, seed=5), 0.25 * RS.signed_unit_vectors(n, 3, seed=6),
                     bicgstab=kind == "nonsym")
    print(f"FE {kind}: n_rows {n}, window grid {grid}")
    misses = _check_cuts(A, ref, runs, n)
    assert not misses, "\n".join(misses)
