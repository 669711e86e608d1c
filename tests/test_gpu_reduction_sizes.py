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

Known uncovered branches: the merged CG's own pre-reduction (PH_CGM_IT: from 4 * 16384 sums, i.e. more than 8 M rows),
and the partitioned synchronisation points (k_ksp_reduce + k_ksp_logic, k_ksp_scalar_p2p) at these sizes.

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
import os
import re

import numpy as np
import pytest
import torch

from tests import krylov_steps_model as K
from tests import reduction_systems as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12  # the bound test_single_reduction_cg_nonzero_guess_and_max_it puts on a cut solve
PRE = 1e-13  # float64 run of the recurrence against the extended one: the systems themselves allow TOL

CONTROL, IN_FLIGHT, ROUND2, WIDE, ROUND2_WIDE = 760, 776, 2568, 4104, 10248
PRERED_MBCGS3, PRERED_BCGS3, PRERED_CG3 = 1096, 2736, 5464

METHODS = {
    "cg": {"ksp_type": "cg", "ksp_cg_single_reduction": False, "ksp_cg_merged_reduction": False, "ksp_cg_fold_blocks": 0},
    "cg_fold1": {"ksp_type": "cg", "ksp_cg_single_reduction": False, "ksp_cg_merged_reduction": False, "ksp_cg_fold_blocks": 1},
    "cg_fold": {"ksp_type": "cg", "ksp_cg_single_reduction": False, "ksp_cg_merged_reduction": False},
    "cg_single": {"ksp_type": "cg", "ksp_cg_single_reduction": True, "ksp_cg_merged_reduction": False},
    "cg_merged": {"ksp_type": "cg", "ksp_cg_single_reduction": False, "ksp_cg_merged_reduction": True, "ksp_cg_fold_blocks": 0},
    "cg_merged_fold": {"ksp_type": "cg", "ksp_cg_single_reduction": False, "ksp_cg_merged_reduction": True},
    "bcgs": {"ksp_type": "bcgs", "ksp_bcgs_merged_reduction": False},
    "bcgs_merged": {"ksp_type": "bcgs", "ksp_bcgs_merged_reduction": True},
}
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


def _sources():
    rd = lambda *p: open(os.path.join(ROOT, *p)).read()
    return rd("oasisx_amd", "csrc", "ox_kernels.h"), rd("oasisx_amd", "csrc", "ox_ksp.hip")


def _thresholds():
    """The numbers the second stage branches on, as the sources state them."""
    kh, ksp = _sources()

    def one(pattern, text, what):
        found = set(re.findall(pattern, text))
        assert len(found) == 1, f"{what}: {sorted(found)} -- the sources no longer read as this test expects"
        return int(found.pop())

    T = {
        "red_small": one(r"#define OX_RED_THREADS_SMALL (\d+)", kh, "OX_RED_THREADS_SMALL"),
        "red_wide": one(r"#define OX_RED_THREADS (\d+)", kh, "OX_RED_THREADS"),
        "wide_from": one(r"ox_red_threads\(int nparts\) \{ return nparts > (\d+) \? OX_RED_THREADS : OX_RED_THREADS_SMALL", kh,
                         "ox_red_threads"),
        "max_nv": one(r"#define OX_MAX_NV (\d+)", kh, "OX_MAX_NV"),
        "chunk": one(r"#define OX_PRERED_CHUNK (\d+)", ksp, "OX_PRERED_CHUNK"),
        "prered_min": one(r"#define OX_PRERED_MIN (\d+)", ksp, "OX_PRERED_MIN"),
        "fold_t": one(r"#define OX_FOLD_T (\d+)", ksp, "OX_FOLD_T"),
        "rows_u": one(r"ksp_gather_rows<[^;]*?, (\d+)>\(partial", ksp, "rows per thread of ksp_gather_rows"),
        "fold_u": one(r"ksp_fold_point<1, (\d+), PH_CG_A", ksp, "U of the folded CG's first point"),
        "cgm_prered": one(r"PH == PH_CGM_IT \? (\d+) \* OX_PRERED_MIN", ksp, "merged CG's pre-reduction factor"),
        "cgm_fold_rows": one(r"nbs1 <= (\d+) \* OX_FOLD_T", ksp, "folded merged CG's row limit"),
    }
    # the branch conditions themselves
    assert len(re.findall(r"for \(; p \+ 3 \* T < nparts; p \+= 4 \* T\)", kh + ksp)) == 2  # ox_gather_partials, ksp_gather_t
    assert re.search(r"for \(int p0 = threadIdx\.x; p0 < nparts; p0 \+= U \* T\)", ksp)  # ksp_gather_rows
    assert re.search(r"if \(np_ > U \* T\)", ksp) and re.search(r"if \(\(int64_t\)nparts \* nv >= prered_min\)", ksp)
    assert re.search(r"if \(npin >= OX_PRERED_MIN\)", ksp)
    return T


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


def _sell(Acsr, symmetric):
    """SellMatrix of a scipy CSR matrix with sorted indices, without a mesh."""
    from oasisx_amd import fem
    from oasisx_amd.la import SellMatrix

    n = Acsr.shape[0]
    rl = np.diff(Acsr.indptr).astype(np.int64)
    keys = np.repeat(np.arange(n, dtype=np.int64), rl) * n + Acsr.indices
    P = fem.build_sell(n, n, torch.from_numpy(keys).cuda(), torch.from_numpy(rl).cuda(),
                       torch.from_numpy(Acsr.indptr.astype(np.int64)).cuda())
    A = SellMatrix(P, symmetric=symmetric)
    A.vals.copy_(P.values_from_csr(Acsr))
    A.version += 1
    return A


class _Reference:
    """Extended-precision traces of one system, column by column, computed once and kept unchanged; the float64 run of
    the same recurrence is held to PRE first (a device miss cannot be blamed on the system)."""

    def __init__(self, Acsr, b, x0, bicgstab):
        self.A, self.b, self.x0 = Acsr, b, x0
        self.trace = K.jacobi_bicgstab_trace if bicgstab else K.jacobi_cg_trace
        self._t = {}

    def get(self, c, guess):
        key = (c, guess)
        if key not in self._t:
            kmax, x0 = (2, self.x0[:, c]) if guess else (3, None)
            hi = self.trace(self.A, self.b[:, c], x0, kmax)
            lo = self.trace(self.A, self.b[:, c], x0, kmax, dtype=np.float64)
            for k, (h, l) in enumerate(zip(hi, lo)):
                ex = float(np.abs(h[0] - l[0]).max() / max(np.abs(h[0]).max(), np.finfo(np.float64).tiny))
                er = float(abs(h[2] - l[2]) / h[1])
                assert ex <= PRE and er <= PRE, f"the system does not allow {PRE:g} on the CPU: column {c}, k = {k}: {ex:.2e}, {er:.2e}"
            self._t[key] = [(np.asarray(h[0], dtype=np.float64), float(h[1]), float(h[2]), float(h[-1])) for h in hi]
        return self._t[key]


def _check_cuts(A, ref, runs, n, dict_dinv=False):
    """Every (method, columns) of ``runs``: k = 1, 2, 3 from a zero guess and k = 2 from a nonzero one; returns the list of
    misses (empty: all within TOL) and prints every figure."""
    from oasisx_amd import _lib
    from oasisx_amd.fem import FieldStorage
    from oasisx_amd.ksp import KSPSolver

    misses = []
    for method, nc in runs:
        B = FieldStorage(n, nc, "cuda")
        B.dev()[:] = torch.from_numpy(ref.b[:, :nc]).cuda()
        x0 = torch.from_numpy(np.ascontiguousarray(ref.x0[:, :nc])).cuda()
        ksp = KSPSolver(None, dict(METHODS[method], pc_type="jacobi", ksp_rtol=1e-30))
        ksp.setOperators(A)
        recurrence_norm = method == "bcgs_merged"
        for k, guess in ((1, False), (2, False), (3, False), (2, True)):
            ksp.updateOptions({"ksp_max_it": k, "ksp_initial_guess_nonzero": guess})
            X = FieldStorage(n, nc, "cuda")
            if guess:
                X.dev().copy_(x0)
            reasons = ksp.solve_block(B, X)
            if dict_dinv:
                assert ksp._dcode is not None, "the dictionary of dinv was not built: CODE = true is not what runs"
            res, xs = ksp.last_result, X.dev().cpu().numpy()
            for c in range(nc):
                xr, bn, rn_true, rn_rec = ref.get(c, guess)[k]
                rn = rn_rec if recurrence_norm else rn_true
                ex = float(np.abs(xs[:, c] - xr).max() / np.abs(xr).max())
                eb = abs(res.bnorm[c] - bn) / bn
                er = abs(res.rnorm[c] - rn) / bn
                tag = f"{method} nc={nc} c={c} k={k} guess={int(guess)}"
                print(f"  {tag}: reason {reasons[c]} its {res.its[c]}  x {ex:.2e}  bnorm {eb:.2e}  rnorm {er:.2e}")
                if reasons[c] != _lib.DIVERGED_ITS or res.its[c] != k:
                    misses.append(f"{tag}: reason {reasons[c]}, {res.its[c]} iterations")
                if not (ex <= TOL and eb <= TOL and er <= TOL):
                    misses.append(f"{tag}: x {ex:.2e} bnorm {eb:.2e} rnorm {er:.2e}")
    return misses


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
