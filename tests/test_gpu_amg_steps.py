"""GPU: the AMG V-cycle (``Hierarchy.apply``: ox_mg_create, k_mg_phase, k_mg_tail) and the AMG-preconditioned CG
(``KSPSolver`` with ``pc_type gamg``: mgcg_solve, k_mgcg_*) held to the extended-precision model of
tests/amg_steps_model.py, to TOL = 1e-12 in the relative max-norm -- the bound ``test_device_vcycle_matches_numpy``
uses; the float64 run of the model sits three orders below it (tests/test_amg_steps_host.py, which also holds that
every level of every hierarchy moves z by at least 1e-2: a wrong deep level cannot stay under TOL).

tests/test_gpu_amg.py compares the cycle with numpy on three FE operators of at most 2197 rows at degree 2 and asks of
the solve that it converges in at most 30 iterations to 1e-7 of a Jacobi solve -- which CG does with a wrong beta, a
wrong |B b| or a lost partial row too.  Here the cycle runs in every layout ``ox_mg_create`` can give it, and solves are
CUT after k iterations (``ksp_rtol`` 1e-30, ``ksp_max_it`` k) and compared iterate by iterate.

V-cycle layouts (operators: ``amg_steps_model.helical_laplacian`` through fem.build_sell + SellMatrix + values_from_csr):

    case                 rows of the levels             tail_rows   branch it reaches
    one                  1061                           0           c == 0: the dense inverse alone
    two-deg1             12 709 / 1848                  0           d2 == nullptr in the restriction; no pre-smoothing step;
                                                                    the cd == 0 step after the prolongation; dense solve
                                                                    and tail loop beyond 1024 rows
                                                        16384       lt == 0: level 0 by mg_row from the caller's
                                                                    cols / vals, 13 rounds of the tail loop
    two-deg1-dict        same, frozen                   16384       ... of a matrix that also carries value codes
    five                 198 437 / 26 953 / 1616 /      0           a middle level on the grid, a grid restriction into
                         74 / 3                                     the tail, whose first level needs two rounds
                                                        1           every level on the grid
                                                        32768       the 27 k-row level in the tail
    five-neumann-deg3    198 437 / 27 011 / 1555 /      0           projected coarse inverse; c_d of the third step
                         67 / 3
    deg8, deg9           1061 / 99 / 7                  0, 1        the whole cheb[] array (9 clamps to 8)

Every case fills z with NaN before each call (every row must be written) and runs the cycle on b1, b2 and b1 again: all
three within TOL, the third equal to the first bit for bit (the hierarchy keeps d, x, b, y between calls).

AMG-CG: cuts after k = 1, 2, 3 iterations from a zero guess and after 2 from a nonzero one (with and without the
caller's A x0) on the five-level Dirichlet system, its dictionary twin frozen with pair slots (the mat-vec with the dot
epilogue and the cycle's level-0 products run k_spmv_ps), the Neumann degree-3 and the two-level degree-1 system;
the one-level solve; the same cut through pc_type bjacobi + sub_pc_type gamg, bit for bit; five schedules (check
interval 1 / 3 / 8, run-ahead off / on) with identical bits and the model's stopping iteration; ksp_atol and
ksp_error_if_not_converged.  n = 198 437 gives 776 partial rows in the vector kernels' and in the mat-vec's sums: the
4-rows-in-flight gather of PH_CG_INIT (3 sums), PH_CG_A and PH_CG_B (2 sums).

Not covered: the reductions above 2560 partial rows for these phases, and sums over more than one rank's contribution
(``OX_KSP_CG_MG`` on a partitioned operator is cut on one-rank plans by tests/test_gpu_partitioned_cuts.py).

Measured on an MI355X (worst over the cases; relative max-norm, norms relative to |B b|):
    V-cycle z 3.9e-15 (two-deg1, b2); cut solves x 6.7e-15 (five, k = 3), bnorm 1.1e-16, rnorm 4.7e-15 (five, k = 1);
    the one-level solve x 3.2e-15 against the model's x_1 and 8.0e-15 against the extended dense solve; x_15 of the
    schedule test 1.8e-15.  The cut with the library's own A x0 is bit-identical to the cut without; with scipy's
    product (another order of the row sums) it is not, and within TOL.

Mutation check (run once on an MI355X, never committed: mutant libraries built from scratch copies of the sources; each
only skips or mis-scales work, none changes an address):
    "old": tests/test_gpu_amg.py, 11 tests.  Misses are relative errors against TOL = 1e-12.
    (a) k_mg_tail stops at row 1023.  New: 16 of 21 fail -- V-cycle one, two-deg1 (both tails), two-deg1-dict, five
        tail 0 / 32768, five-neumann-deg3, deg8 / deg9 tail 0: z off by 0.57 .. 0.96 or rows left NaN (37 .. 11 685
        rows); every cut solve: x 0.66 .. 0.96, bnorm 0.17 .. 0.32; one-level solve, schedules, reasons.  five tail 1 and
        deg8 / deg9 tail 1 (nothing but the coarsest level in the tail) pass.  Old: all 11 pass.
    (b) MG_STEP ignores c_d.  New: every case of degree >= 2 fails (z 0.12 .. 0.15, cut x 0.05 .. 0.47); degree 1 and
        one level pass.  Old: 7 of 11 fail, test_device_vcycle_matches_numpy among them -- c_d is nonzero from the
        SECOND step on, so degree 2 sees it: this mutant was no gap.
    (b') ox_mg_create gives every step from the third on the second step's c_d.  New: five-neumann-deg3 (z 2.6e-2, cut
        x 6.8e-3 .. 2.2e-2), deg8 and deg9 with both tails (z 4.7e-2) fail, nothing else.  Old: all 11 pass.
    (c) k_mgcg_dots<true> sums z where it should sum zb.  New: the three nonzero-guess cuts of each of the four systems
        miss in bnorm alone, by 2.1e-4 .. 8.7e-4 (x and rnorm stay at 1e-15); every zero-guess cut passes.  Old: all 11
        pass (test_cg_gamg_nonzero_guess included).
    (d) k_mgcg_update2 takes beta = 0.  New: every k = 2 and k = 3 cut misses (x 3.9e-3 .. 0.16, rnorm 3.5e-3 .. 0.14),
        every k = 1 cut passes; the schedule test sees 29 iterations for the model's 15, the reasons test 3 for 2.
        Old: 10 of 11 pass; test_cg_gamg_iterations_do_not_grow alone notices, narrowly, by the growth of the iteration
        count (23 at N = 64 against 1.5 x 14 at N = 16; every solve stays under its 30).
    (e) k_mg_phase returns for MG_PROLONG whenever `done` is not null, i.e. in every cycle of the iteration loop but
        not in ox_mg_apply nor in the two cycles before the loop.  New: every V-cycle case passes; every cut misses --
        k = 1 in rnorm alone (0.49 .. 0.99, x at 1e-15), k >= 2 in x too (0.03 .. 0.54); schedules 460 iterations for
        15; reasons.  Old: 8 of 11 pass, test_device_vcycle_matches_numpy among them; three solve tests notice by
        their iteration counts.
    Removing a `done` check from one kernel alone is not a detectable mutant: an inactive column has alpha = beta = 0 and
        x is written by k_mgcg_update1 only, so the no-ops of a run-ahead batch are belt and braces (by reading the
        code; not run).
"""
import numpy as np
import pytest
import torch

from tests import amg_steps_model as M

pytestmark = pytest.mark.gpu

TOL = 1e-12
_CACHE = {}


def _sell(Acsr):
    """SellMatrix of a scipy CSR matrix with sorted indices, without a mesh (as tests/test_gpu_reduction_sizes.py)."""
    from oasisx_amd import fem
    from oasisx_amd.la import SellMatrix

    n = Acsr.shape[0]
    rl = np.diff(Acsr.indptr).astype(np.int64)
    keys = np.repeat(np.arange(n, dtype=np.int64), rl) * n + Acsr.indices
    P = fem.build_sell(n, n, torch.from_numpy(keys).cuda(), torch.from_numpy(rl).cuda(),
                       torch.from_numpy(Acsr.indptr.astype(np.int64)).cuda())
    A = SellMatrix(P, symmetric=True)
    A.vals.copy_(P.values_from_csr(Acsr))
    A.version += 1
    return A


def _matrix(name):
    """The device operator of a case, built once; the dictionary cases frozen."""
    key = ("A", name)
    if key not in _CACHE:
        A = _sell(M.system(name)[0])
        if M.CASES[name][2] == "dict":
            # five-dict: the pair-slot stream forced, so that k_spmv_ps carries the dot epilogue and the cycle's products
            assert A.freeze(pairs="always" if name == "five-dict" else "auto") and A.vcode is not None
            if name == "five-dict":
                assert A.ps_code is not None
        _CACHE[key] = A
    return _CACHE[key]


def _hierarchy(name, tail):
    from oasisx_amd.amg import Hierarchy

    key = ("H", name, tail)
    if key not in _CACHE:
        H = Hierarchy(_matrix(name), M.CASES[name][4], tail_rows=tail)
        # the device runs the hierarchy the model was computed on
        levels = M.system(name)[1]
        assert H.rows == [lev.A.shape[0] for lev in levels]
        assert all(np.array_equal(a.dinv, b.dinv) and (a.A != b.A).nnz == 0 for a, b in zip(H.levels, levels))
        assert np.array_equal(H.levels[-1].inv, levels[-1].inv)
        _CACHE[key] = H
    return _CACHE[key]


def _err(x, ref):
    return float(np.abs(x - ref).max() / np.abs(ref).max())


# ---- the V-cycle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tail", M.VCYCLE_CASES, ids=[f"{n}-tail{t}" for n, t in M.VCYCLE_CASES])
def test_vcycle_layouts_match_the_extended_model(hip, name, tail):
    H = _hierarchy(name, tail)
    b, ref = M.reference_vcycles(name)
    n = b.shape[0]
    bd = [torch.from_numpy(np.ascontiguousarray(b[:, c])).cuda() for c in range(2)]
    got = []
    for c in (0, 1, 0):
        z = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        H.apply(bd[c], z)
        got.append((c, z.cpu().numpy()))
    errs = []
    for i, (c, z) in enumerate(got):
        assert np.isfinite(z).all(), f"{name} tail_rows {tail}, call {i + 1}: {int((~np.isfinite(z)).sum())} rows not written"
        errs.append(_err(z, np.asarray(ref[c], dtype=np.float64)))
    print(f"{name} tail_rows {tail}: levels {H.rows}, {H.kernels_per_cycle()} kernels; z(b1) {errs[0]:.2e}  z(b2) {errs[1]:.2e}  "
          f"z(b1) again {errs[2]:.2e}")
    assert max(errs) <= TOL
    assert np.array_equal(got[0][1], got[2][1]), "the cycle on b1 after a cycle on b2 differs from the first one: stale state"


def test_tail_rows_change_the_layout(hip):
    """What the table above says of ``tail_rows``, in the library's own kernel counts."""
    k = {t: _hierarchy("five", t).kernels_per_cycle() for t in (0, 1, 32768)}
    assert k[32768] < k[0] < k[1], k
    assert _hierarchy("one", 0).kernels_per_cycle() == 1
    assert _hierarchy("two-deg1", 16384).kernels_per_cycle() == 1 < _hierarchy("two-deg1", 0).kernels_per_cycle()
    assert _hierarchy("two-deg1-dict", 16384).kernels_per_cycle() == 1
    assert _hierarchy("deg8", 1).kernels_per_cycle() > 2 * 8 * 2 and _hierarchy("deg8", 0).kernels_per_cycle() == 1
    assert _hierarchy("deg9", 1).kernels_per_cycle() == _hierarchy("deg8", 1).kernels_per_cycle()


# ---- AMG-CG -----------------------------------------------------------------------------------------------------------
def _solver(name, **options):
    from oasisx_amd.ksp import KSPSolver

    ksp = KSPSolver(None, dict({"ksp_type": "cg", "pc_type": "gamg", "ksp_rtol": 1e-30, "ksp_atol": 1e-50}, **M.CASES[name][4],
                               **options))
    ksp.setOperators(_matrix(name))
    return ksp


def _field(v):
    from oasisx_amd.fem import FieldStorage

    F = FieldStorage(v.shape[0], 1, "cuda")
    F.dev()[:, 0] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).cuda()
    return F


def _solve(ksp, b, x0=None, ax0=None):
    """(reason, its, x, bnorm, rnorm) of one solve."""
    from oasisx_amd.fem import FieldStorage

    B = _field(b)
    X = _field(x0) if x0 is not None else FieldStorage(b.shape[0], 1, "cuda")
    reason = ksp.solve_block(B, X, ax0)[0]
    res = ksp.last_result
    return reason, int(res.its[0]), X.dev()[:, 0].cpu().numpy().copy(), float(res.bnorm[0]), float(res.rnorm[0])


def _cut_misses(tag, got, ref_k, k):
    from oasisx_amd import _lib

    reason, its, x, bn, rn = got
    xr, bnr, rnr = np.asarray(ref_k[0], dtype=np.float64), float(ref_k[1]), float(ref_k[2])
    ex, eb, er = _err(x, xr), abs(bn - bnr) / bnr, abs(rn - rnr) / bnr
    print(f"  {tag}: reason {reason} its {its}  x {ex:.2e}  bnorm {eb:.2e}  rnorm {er:.2e}")
    misses = []
    if reason != _lib.DIVERGED_ITS or its != k:
        misses.append(f"{tag}: reason {reason}, {its} iterations")
    if not (ex <= TOL and eb <= TOL and er <= TOL):
        misses.append(f"{tag}: x {ex:.2e} bnorm {eb:.2e} rnorm {er:.2e}")
    return misses


@pytest.mark.parametrize("name", ["five", "five-dict", "five-neumann-deg3", "two-deg1"])
def test_cut_solves_match_the_extended_iterates(hip, name):
    A = _matrix(name)
    if name == "five-dict":
        assert A.ps_code is not None and A.vcode is not None and A.levels is None  # pair slots present and allowed
    b, _, tr0 = M.reference_trace(name, False)
    _, x0, tr1 = M.reference_trace(name, True)
    print(f"{name}: levels {[lev.A.shape[0] for lev in M.system(name)[1]]}")
    ksp = _solver(name)
    misses = []
    for k in (1, 2, 3):
        ksp.updateOptions({"ksp_max_it": k, "ksp_initial_guess_nonzero": False})
        misses += _cut_misses(f"{name} k={k} guess=0", _solve(ksp, b), tr0[k], k)
    # the nonzero guess: |B b| is the norm of the relative test; the caller's A x0 replaces the solver's own product
    ksp.updateOptions({"ksp_max_it": 2, "ksp_initial_guess_nonzero": True})
    own = _solve(ksp, b, x0)
    ax0 = _field(np.zeros_like(x0))
    A.mult(_field(x0).dev(), ax0.dev(), 1)  # the library's own product: the order of the solver's
    given = _solve(ksp, b, x0, ax0=ax0)
    host = _solve(ksp, b, x0, ax0=_field(M.system(name)[0] @ x0))  # scipy's product: another order of the row sums
    misses += _cut_misses(f"{name} k=2 guess=1 ax0=None", own, tr1[2], 2)
    misses += _cut_misses(f"{name} k=2 guess=1 ax0=A x0 (device)", given, tr1[2], 2)
    misses += _cut_misses(f"{name} k=2 guess=1 ax0=A x0 (host)", host, tr1[2], 2)
    assert not misses, "\n".join(misses)
    assert np.array_equal(own[2], given[2]) and own[3:] == given[3:], "the caller's A x0 changes the bits of the solve"


def test_one_level_solve(hip):
    """The dense inverse is the preconditioner: one iteration solves the system."""
    from oasisx_amd import _lib

    b, _, tr = M.reference_trace("one", False)
    reason, its, x, bn, rn = _solve(_solver("one", ksp_rtol=1e-8), b)
    dense = np.asarray(M.vcycle(M.cast_system("one", np.longdouble), b, np.longdouble), dtype=np.float64)
    ex, ed, eb = _err(x, np.asarray(tr[1][0], dtype=np.float64)), _err(x, dense), abs(bn - float(tr[1][1])) / float(tr[1][1])
    print(f"one: reason {reason} its {its}  x against the model's x_1 {ex:.2e}, against the extended dense solve {ed:.2e}  "
          f"bnorm {eb:.2e}  rnorm / bnorm {rn / bn:.2e}")
    assert reason == _lib.CONVERGED_RTOL and its == 1
    assert ex <= TOL and ed <= TOL and eb <= TOL and rn <= 1e-8 * bn


def test_bjacobi_cut_is_the_gamg_cut(hip):
    b = M.reference_trace("five", False)[0]
    g = _solve(_solver("five", ksp_max_it=2), b)
    bj = _solve(_solver("five", pc_type="bjacobi", sub_pc_type="gamg", ksp_max_it=2), b)
    assert g[:2] == bj[:2] == (-3, 2)
    assert np.array_equal(g[2], bj[2]) and g[3:] == bj[3:]


def test_schedules_give_the_same_bits_and_the_model_iteration(hip):
    from oasisx_amd import _lib

    b, _, tr = M.reference_trace("five", False, kmax=M.SCHEDULE_ITS, seed=M.SCHEDULE_SEED)
    assert M.stopping_iteration(tr, M.SCHEDULE_RTOL) == M.SCHEDULE_ITS
    runs = {}
    ksp = _solver("five", ksp_rtol=M.SCHEDULE_RTOL)
    for every, ahead in ((1, False), (3, False), (8, False), (1, True), (8, True)):
        ksp.updateOptions({"ksp_run_ahead": ahead})
        ksp.check_every = every
        runs[(every, ahead)] = _solve(ksp, b)
        print(f"  check_every {every} run-ahead {int(ahead)}: reason {runs[(every, ahead)][0]} its {runs[(every, ahead)][1]}")
    first = runs[(1, False)]
    ex = _err(first[2], np.asarray(tr[M.SCHEDULE_ITS][0], dtype=np.float64))
    print(f"  x_{M.SCHEDULE_ITS} against the model {ex:.2e}")
    assert first[0] == _lib.CONVERGED_RTOL and first[1] == M.SCHEDULE_ITS
    for key, r in runs.items():
        assert r[:2] == first[:2] and np.array_equal(r[2], first[2]) and r[3:] == first[3:], key


def test_reasons(hip):
    from oasisx_amd import _lib
    from oasisx_amd.ksp import KSPConvergenceError

    b, _, tr = M.reference_trace("five", False)
    atol = M.ATOL_FACTOR * float(tr[2][2])
    ksp = _solver("five", ksp_atol=atol)
    reason, its, x, bn, rn = _solve(ksp, b)
    assert reason == _lib.CONVERGED_ATOL and its == M.stopping_iteration(tr, 1e-30, atol) == 2
    assert _err(x, np.asarray(tr[2][0], dtype=np.float64)) <= TOL and abs(rn - float(tr[2][2])) <= TOL * float(tr[2][1])
    ksp.updateOptions({"ksp_atol": 1e-50, "ksp_max_it": 2, "ksp_error_if_not_converged": True})
    with pytest.raises(KSPConvergenceError):
        _solve(ksp, b)
