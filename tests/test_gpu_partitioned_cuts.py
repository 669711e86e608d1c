"""GPU: the partitioned Krylov paths held to the extended-precision k-step iterates, on ONE GPU and in one process.

A partitioned operator changes every route a Krylov scalar takes: other methods by default (merged BiCGStab, single-
reduction or merged CG, never the folded forms), a mat-vec split into an interior and a boundary launch over slice lists
(``ox_spmv_dist``; the second launch writes its partial rows at ``partial + nb_int * nv``, and the row count is the sum
of two grids each rounded to 8: ``ox_spmv_dist_nparts``), synchronisation points that carry an all-reduce (k_ksp_reduce
+ all-reduce + k_ksp_logic, or k_ksp_scalar_p2p with the window all-reduce inside the kernel), vectors with a ghost block
that no dot product may include, and a scatter-forward of x after the solve.  The rehearsals that run this path compare
whole time steps at 1e-7 .. 1e-8 and let iteration counts differ by one: a lost partial row or a ghost row in a norm
moves a scalar by 1e-2 .. 1e-5 and passes there as one more iteration.

Here the plan has one rank whose only peer is the rank itself: ghost column j receives owned row send[j], so the local
n x (n + ng) matrix acts on owned vectors as A_eff = A_loc[:, :n] + A_loc[:, n:] S.  ``reduction_systems.ghosted`` moves
the far lower band of the rows from r0 on into ghost columns (through a permutation: the send list is not monotone), so
A_eff is, entry for entry, a system the model of tests/krylov_steps_model.py already serves
(tests/test_partitioned_systems_host.py), and the cuts of tests/cut_solves.py apply unchanged: k = 1, 2, 3 from a zero
guess and k = 2 from a nonzero one; x, bnorm and rnorm to TOL = 1e-12; reason DIVERGED_ITS, its == k.  The ghost rows of
b and of the guess hold values of magnitude 1e3; after each solve the ghost block of x must be x[send] bit for bit and
``ox_dist_status`` 0.

Transports, each built the way the product or an existing test builds it:
    rccl      one-rank communicator, the plan claims two ranks so that ``ox_allreduce_impl`` does not take its one-rank
              shortcut: pack kernel, grouped ncclSend / ncclRecv to self, k_ksp_reduce, ncclAllReduce, k_ksp_logic
    p2p       the rank's own window (as ``parallel.SelfLoopComm``), waits bounded by 15 s, conservative release:
              k_halo_push / k_halo_pull, k_ksp_scalar_p2p
    p2p-fast  the same with ``ox_dist_set_p2p_release(plan, 0)``
    custom    ``ox_dist_create_custom``: halo_cb copies the packed send values into the ghost block device to device,
              allreduce_cb leaves its buffer alone; the stream-drain and callback branches
each with ``ox_dist_set_overlap`` 0 (exchange, then one launch) and 1 (interior launch, exchange, boundary launch).

Small case: n = 1829 (29 slices), m = 609, r0 = 725: 11 interior + 18 boundary slices, 8 partial rows without and 16 with
the overlap, most blocks of either grid padding.  The full product transports x overlap x levels (``set_levels(7)``: the
lane = row kernel; default: 16-bit columns, and on the dictionary matrix -- frozen with pairs="always" -- k_spmv_ps over
slice lists).  At a fixed overlap and level the iterates and norms of the four transports are bit-identical: with one
rank every all-reduce sums one contribution, and gather and logic are the same functions in k_ksp_reduce / k_ksp_logic
and in k_ksp_scalar_p2p.  ``ksp_cg_fold_blocks`` = 1 on a partitioned operator does not fold (``_cg_folded()`` False) and
gives the bits of the unfolded CG.

Threshold cases (thresholds read from the sources, crossings asserted with ``spmv_parts`` / ``split_parts``): 776 partial
rows (784 with the overlap: 4 rows in flight in ksp_gather_t inside the partitioned kernels), 1096 (k_prereduce ahead of
a partitioned point, 15 sums), 4104 (the 1024-thread block of k_ksp_reduce and k_ksp_scalar_p2p, where threads =
max(ox_red_threads, ox_p2p_ar_threads)), and the 760-row control.  r0 is about n / 3.

Block-Jacobi AMG on a partitioned operator (``OX_KSP_CG_MG`` with a halo plan): the "two-deg1" system of tests/amg_steps_model.py
(12 709 rows, m = 131) ghosted from r0 = 4245 (66 interior + 133 boundary slices; the float64-against-extended
precondition of tests/test_amg_steps_host.py holds there: tests/test_partitioned_systems_host.py), cut at k = 1 and 2
and compared with ``amg_cg_trace(A_eff, levels of the owned block A_loc[:, :n])`` to the TOL of
tests/test_gpu_amg_steps.py.

Measured on an MI355X (worst over transports, overlaps, levels, methods, columns and cuts; x in the relative max-norm,
norms relative to bnorm; wall time per parametrised test, the first test of a system carries its reference):
    case            x         bnorm     rnorm     wall time
    small sym       6.9e-16   1.7e-16   1.3e-16   1.1 s the first (library warm-up), then 0.1 s (4 transports each)
    small nonsym    3.8e-16   1.6e-16   1.0e-16   0.1 s
    small dict      6.2e-16   1.2e-16   3.1e-17   0.1 s
    760 sym         5.0e-16   1.5e-16   3.9e-17   0.5 s / 0.1 s
    760 nonsym      4.8e-16   1.5e-16   1.1e-16   0.6 s / 0.1 s
    776 sym         5.3e-16   1.5e-16   7.6e-17   0.5 s / 0.1 s
    776 nonsym      5.7e-16   1.5e-16   1.3e-16   0.6 s / 0.1 s
    1096 nonsym     4.9e-16   0         1.1e-16   0.8 s / 0.1 s
    4104 sym        4.4e-16   1.3e-16   3.3e-17   2.5 s / 0.3 s
    4104 nonsym     4.9e-16   0         3.2e-17   1.2 s / 0.2 s
    bjacobi + gamg  2.8e-15   1.7e-16   1.1e-16   0.8 s the first, then 0.2 .. 0.3 s
All 34 tests together: 17 s.  The four transports gave the same bits in every small case.

Mutation check.  Run once on an MI355X, never committed: five mutant libraries built from scratch copies of the sources,
ONE change each, none touching an address outside the existing arrays; each run against this file (34 tests) and against
the whole of tests/test_gpu_reduction_sizes.py, which passed (17 tests) with every one of them.  Misses against 1e-12:
    1. ox_spmv_dist hands its boundary launch ``partial`` instead of ``partial + nb_int * nv``.  12 fail: every overlap-1
       test -- the six small ones (all four transports), 776-sym and 776-nonsym on rccl and p2p, bjacobi + gamg on rccl
       and p2p: x 2.5e-3 .. 2.1e+1, rnorm 4.7e-5 .. 1.6e+1 (bnorm comes from a vector kernel and stays exact); the
       transports no longer agree bitwise either.  All 22 overlap-0 tests pass.
    2. ox_spmv_dist_nparts returns the interior grid only.  The same 12 overlap-1 tests fail: x 5.5e-3 .. 4.0e+2, rnorm
       2.2e-4 .. 1.9e+2.  All 22 overlap-0 tests pass.
    3. k_ksp_reduce ignores the second partial array (B).  12 fail: the eight small sym and dict tests (both overlaps,
       both levels) on rccl and custom -- the transports that reach k_ksp_reduce -- in cg_single and cg_merged, the only
       methods with a second array (reason -5 after 0 iterations, or 3 after 1; x 0.36 .. 1.4, rnorm 1.5e-2 .. 1.2), and
       760-sym, 776-sym (both overlaps) and 4104-sym on rccl.  Every nonsym test, every p2p threshold test and bjacobi +
       gamg pass: no second array, or another kernel.
    4. k_ksp_scalar_p2p zeroes vals[nv - 1] before the all-reduce.  23 fail: all twelve small tests (p2p and p2p-fast
       only), every p2p threshold test (760 .. 4104, both overlaps) and bjacobi + gamg on p2p: bnorm 1.0 (the last sum
       of the first point), x 0.38 .. 1.4, reason -5 after 0 iterations.  Every rccl test passes.
    5. The overlapped path launches the boundary slices before ox_halo_end_impl.  9 fail, all overlap 1 and p2p / p2p-fast
       only: the six small tests, 776-sym and 776-nonsym on p2p, bjacobi + gamg on p2p: x 9.5e-5 .. 6.1e+2 (the ghosts of
       the previous exchange; the 1e3 fill at the first mat-vec of a nonzero guess), rnorm 4.5e-5 .. 5.6e+1.  On the
       callback transport the mutant is no change (the exchange is complete when ox_halo_begin_impl returns); on rccl it
       is a race between the side stream's exchange and the boundary launch, which the exchange won in this run.  All
       22 overlap-0 tests pass.
"""
import contextlib
import ctypes as C
import time

import numpy as np
import pytest
import torch

from tests import amg_steps_model as M
from tests import cut_solves as CS
from tests import reduction_systems as RS
from tests.cut_solves import _check_cuts, _sell, _thresholds
from tests.test_gpu_amg_steps import _cut_misses  # (holds a cut to that suite's own TOL)

pytestmark = pytest.mark.gpu

TRANSPORTS = ("rccl", "p2p", "p2p-fast", "custom")
P2P_WAIT_S = 15.0
CALLBACKS = {"halo": 0, "allreduce": 0}  # calls the latest custom plan has received


# ---- one-rank plans ---------------------------------------------------------------------------------------------------
def _hip_runtime():
    """The HIP runtime this process already runs on (for the callback transport's device-to-device copy)."""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(paths) == 1, f"expected one HIP runtime in the process, found {sorted(paths)}"
    rt = C.CDLL(paths.pop())
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rt.hipMemcpy.restype = C.c_int
    rt.hipDeviceSynchronize.restype = C.c_int
    return rt


@pytest.fixture(scope="module")
def rccl_comm(hip):
    """One one-rank RCCL communicator for all plans of the module."""
    from oasisx_amd import _lib

    buf = C.create_string_buffer(128)
    _lib.check(hip.ox_comm_unique_id(buf), "ox_comm_unique_id")
    comm = C.c_void_p()
    _lib.check(hip.ox_comm_create(buf.raw, 0, 1, C.byref(comm)), "ox_comm_create")
    try:
        yield comm
    finally:
        torch.cuda.synchronize()
        hip.ox_comm_destroy(comm)
        CS._PART.clear()  # (the references of the large systems)


@contextlib.contextmanager
def one_rank_plan(hip, comm, transport, n, send, overlap):
    """An ox_dist of one rank whose only peer is the rank itself: ghost j receives owned row send[j]."""
    from oasisx_amd import _lib

    ng = int(len(send))
    send_idx = torch.from_numpy(np.asarray(send, dtype=np.int32)).cuda()
    peers = np.zeros(1, dtype=np.int32)
    off = np.asarray([0, ng], dtype=np.int64)
    pp, po = peers.ctypes.data_as(C.POINTER(C.c_int32)), off.ctypes.data_as(C.POINTER(C.c_int64))
    plan, keep = C.c_void_p(), [send_idx, peers, off]
    try:
        if transport == "rccl":
            # (two ranks claimed, as test_rccl_calls_of_the_halo_plan_run_on_a_self_loop: no one-rank shortcut)
            _lib.check(hip.ox_dist_create(comm, 0, 2, 1, pp, po, _lib.ptr(send_idx), po, n, ng, C.byref(plan)), "ox_dist_create")
        elif transport in ("p2p", "p2p-fast"):
            _lib.check(hip.ox_dist_create(comm, 0, 1, 1, pp, po, _lib.ptr(send_idx), po, n, ng, C.byref(plan)), "ox_dist_create")
            win, handle = C.c_void_p(), C.create_string_buffer(64)
            _lib.check(hip.ox_p2p_window_create(hip.ox_p2p_window_bytes(1, ng), C.byref(win), handle), "ox_p2p_window_create")
            wins = (C.c_void_p * 1)(win.value)
            zero, png = np.zeros(1, dtype=np.int64), np.asarray([ng], dtype=np.int64)
            rc = hip.ox_dist_enable_p2p(plan, win, wins, zero.ctypes.data_as(C.POINTER(C.c_int64)),
                                        png.ctypes.data_as(C.POINTER(C.c_int64)), P2P_WAIT_S)
            if rc:  # (the plan owns the window only once the call has succeeded)
                hip.ox_p2p_window_free(win)
            _lib.check(rc, "ox_dist_enable_p2p")
            if transport == "p2p-fast":
                _lib.check(hip.ox_dist_set_p2p_release(plan, 0), "ox_dist_set_p2p_release")
        else:
            rt = _hip_runtime()
            HALO = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int)
            ARED = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int)
            calls = CALLBACKS
            calls.update(halo=0, allreduce=0)

            def halo_cb(user, send_dev, ghost_dev, nc):  # (the library has drained its stream before the call)
                calls["halo"] += 1
                if rt.hipMemcpy(ghost_dev, send_dev, ng * nc * 8, 3) != 0:  # 3: hipMemcpyDeviceToDevice
                    return 1
                return 1 if rt.hipDeviceSynchronize() != 0 else 0

            def ared_cb(user, buf_dev, count):  # one rank: the sum over the ranks is the buffer as it is
                calls["allreduce"] += 1
                return 0

            cbs = (HALO(halo_cb), ARED(ared_cb))
            keep += [cbs]
            _lib.check(hip.ox_dist_create_custom(0, 2, 1, pp, po, _lib.ptr(send_idx), po, n, ng, C.cast(cbs[0], C.c_void_p),
                                                 C.cast(cbs[1], C.c_void_p), None, C.byref(plan)), "ox_dist_create_custom")
        _lib.check(hip.ox_dist_set_overlap(plan, int(overlap)), "ox_dist_set_overlap")
        yield plan
    finally:
        torch.cuda.synchronize()
        if plan.value:
            hip.ox_dist_destroy(plan)
        del keep


def _operator(hip, plan, A_loc, kind, levels7, r0):
    """The ghosted matrix on the plan, with the slice split the host test states."""
    n = A_loc.shape[0]
    A = _sell(A_loc, symmetric=kind != "nonsym", plan=plan, n_owned=n)
    P = A.pattern
    assert (P.n_interior, P.n_slices - P.n_interior) == RS.slice_kinds(A_loc) == (r0 // 64, P.n_slices - r0 // 64)
    assert P.ib_slices[: P.n_interior].tolist() == list(range(r0 // 64))
    if kind == "dict":
        assert A.freeze(pairs="always") and A.vcode is not None and A.ps_code is not None
    if levels7:
        A.set_levels(7)
    return A


# ---- the small case: every transport, overlap and level -------------------------------------------------------------
SMALL_RUNS = {
    "sym": [("cg", 1), ("cg_fold1", 1), ("cg_single", 1), ("cg_merged", 1), ("cg", 2), ("cg_single", 2), ("cg", 3), ("cg_single", 3)],
    "nonsym": [(m, nc) for nc in (1, 2, 3) for m in ("bcgs", "bcgs_merged")],
    "dict": [("cg", 1), ("cg_single", 1), ("cg_merged", 1), ("cg", 3)],
}
SMALL_CASES = [(kind, overlap, levels7) for kind in ("sym", "nonsym", "dict") for overlap in (0, 1) for levels7 in (True, False)]


@pytest.mark.parametrize("kind,overlap,levels7", SMALL_CASES,
                         ids=[f"{k}-overlap{o}-{'levels7' if l else 'default'}" for k, o, l in SMALL_CASES])
def test_small_partitioned_cuts_on_every_transport(hip, rccl_comm, kind, overlap, levels7):
    t0 = time.perf_counter()
    n = RS.rows_for_parts(CS.SMALL)
    Acsr, A_loc, send, ref = CS.part_system(CS.SMALL, kind)
    ni, nb = RS.slice_kinds(A_loc)
    assert (n, ni, nb) == (1829, 11, 18) and RS.spmv_parts(n) == 8 and RS.split_parts(ni, nb) == 16
    misses, kept = [], {}
    for transport in TRANSPORTS:
        with one_rank_plan(hip, rccl_comm, transport, n, send, overlap) as plan:
            A = _operator(hip, plan, A_loc, kind, levels7, CS.SMALL_R0)
            print(f"{kind} {transport} overlap {overlap} {'levels 7' if levels7 else 'default levels'}: "
                  f"{RS.split_parts(ni, nb) if overlap else RS.spmv_parts(n)} partial rows")
            kept[transport] = {}
            misses += [f"{transport}: {m}" for m in
                       _check_cuts(A, ref, SMALL_RUNS[kind], n, dict_dinv=kind == "dict", plan=plan, send=send, keep=kept[transport])]
            if transport == "custom":  # every mat-vec exchanged and every point all-reduced through the callbacks
                assert CALLBACKS["halo"] > 0 and CALLBACKS["allreduce"] > 0, CALLBACKS
            del A
    first = kept[TRANSPORTS[0]]
    for transport in TRANSPORTS[1:]:
        for key, (x, bn, rn) in kept[transport].items():
            x1, bn1, rn1 = first[key]
            if not (torch.equal(x, x1) and bn == bn1 and rn == rn1):
                misses.append(f"{transport} against {TRANSPORTS[0]}, {key}: not the same bits "
                              f"(x differs by {float((x - x1).abs().max()):.2e})")
    if kind == "sym":  # the fold setting is ignored on a partitioned operator: the bits of the unfolded CG
        for transport in TRANSPORTS:
            for k, guess in CS.CUTS:
                a, b = kept[transport][("cg_fold1", 1, k, guess)], kept[transport][("cg", 1, k, guess)]
                if not (torch.equal(a[0], b[0]) and a[1:] == b[1:]):
                    misses.append(f"{transport}: ksp_cg_fold_blocks = 1 changes the bits of a partitioned CG (k = {k})")
    print(f"wall time {time.perf_counter() - t0:.1f} s")
    assert not misses, "\n".join(misses)


# ---- the thresholds inside the partitioned kernels --------------------------------------------------------------------
CONTROL, IN_FLIGHT, PRERED_MBCGS3, WIDE = 760, 776, 1096, 4104
THRESHOLD_CASES = [
    (nparts, kind, runs, transport, overlap)
    for nparts, kind, runs, overlaps in (
        (CONTROL, "sym", [("cg", 1), ("cg_single", 3), ("cg_merged", 1)], (0,)),
        (CONTROL, "nonsym", [("bcgs_merged", 3)], (0,)),
        (IN_FLIGHT, "sym", [("cg", 1), ("cg_single", 1), ("cg_merged", 1), ("cg", 3), ("cg_single", 3)], (0, 1)),
        (IN_FLIGHT, "nonsym", [("bcgs_merged", 1), ("bcgs_merged", 3)], (0, 1)),
        (PRERED_MBCGS3, "nonsym", [("bcgs_merged", 3)], (0,)),
        (WIDE, "sym", [("cg_single", 3)], (0,)),
        (WIDE, "nonsym", [("bcgs_merged", 1)], (0,)),
    )
    for overlap in overlaps for transport in ("rccl", "p2p")
]


@pytest.mark.parametrize("nparts,kind,runs,transport,overlap", THRESHOLD_CASES,
                         ids=[f"{p}-{k}-{t}-overlap{o}" for p, k, _, t, o in THRESHOLD_CASES])
def test_partitioned_cuts_across_the_thresholds(hip, rccl_comm, nparts, kind, runs, transport, overlap):
    t0 = time.perf_counter()
    T = _thresholds()
    small, wide, U = T["red_small"], T["red_wide"], T["rows_u"]
    n = RS.rows_for_parts(nparts)
    r0 = CS.part_r0(nparts)
    Acsr, A_loc, send, ref = CS.part_system(nparts, kind)
    ni, nb = RS.slice_kinds(A_loc)
    parts = RS.split_parts(ni, nb) if overlap else RS.spmv_parts(n)
    assert ni % 4 and nb % 4 and (overlap or parts == nparts)
    if nparts == CONTROL:  # none of the branches, in the mat-vec's rows and in the vector kernels'
        assert max(parts, RS.vec_parts(n)) <= 3 * small and parts * T["max_nv"] < T["prered_min"]
    elif nparts == IN_FLIGHT:  # 4 rows in flight in a 256-thread block, one round of U rows; both grids together too
        assert 3 * small < parts <= U * small and parts <= T["wide_from"] and parts * T["max_nv"] < T["prered_min"]
    elif nparts == PRERED_MBCGS3:  # the smallest grid whose 15 sums per row are pre-reduced, its last chunk partial
        assert (parts - 8) * 15 < T["prered_min"] <= parts * 15 and parts % T["chunk"] != 0 and 15 <= T["max_nv"]
    else:  # the 1024-thread block, 4 rows in flight there as well
        assert T["wide_from"] < parts <= T["wide_from"] + 8 and 3 * wide < parts <= U * wide
    with one_rank_plan(hip, rccl_comm, transport, n, send, overlap) as plan:
        A = _operator(hip, plan, A_loc, kind, True, r0)
        print(f"nparts {nparts} ({kind}) {transport} overlap {overlap}: n_rows {n}, r0 {r0}, {ni} + {nb} slices, "
              f"{parts} partial rows, vector-kernel rows {RS.vec_parts(n)}")
        misses = _check_cuts(A, ref, runs, n, plan=plan, send=send)
        del A
    print(f"wall time {time.perf_counter() - t0:.1f} s")
    assert not misses, "\n".join(misses)


# ---- block-Jacobi AMG on a partitioned operator -----------------------------------------------------------------------
_AMG_REF = {}


def _amg_reference():
    if not _AMG_REF:
        A, A_loc, send, levels, b = CS.amg_part_system()
        _AMG_REF["trace"] = M.amg_cg_trace(A, levels, b, None, 2)
    return _AMG_REF["trace"]


@pytest.mark.parametrize("transport,overlap", [(t, o) for t in ("rccl", "p2p") for o in (0, 1)],
                         ids=[f"{t}-overlap{o}" for t in ("rccl", "p2p") for o in (0, 1)])
def test_block_jacobi_amg_cuts_on_a_partitioned_operator(hip, rccl_comm, transport, overlap):
    from oasisx_amd.fem import FieldStorage
    from oasisx_amd.ksp import KSPSolver

    t0 = time.perf_counter()
    A_eff, A_loc, send, levels, b = CS.amg_part_system()
    trace = _amg_reference()
    n, ng = A_loc.shape[0], len(send)
    send_dev = torch.from_numpy(send).cuda()
    options = {"sub_" + k: v for k, v in M.CASES[CS.AMG_PART][4].items()}
    misses = []
    with one_rank_plan(hip, rccl_comm, transport, n, send, overlap) as plan:
        A = _operator(hip, plan, A_loc, "sym", False, CS.amg_part_r0())
        ksp = KSPSolver(None, dict({"ksp_type": "cg", "pc_type": "bjacobi", "sub_pc_type": "gamg", "ksp_rtol": 1e-30,
                                    "ksp_atol": 1e-50}, **options))
        ksp.setOperators(A)
        H = ksp._hierarchy()  # the device runs the hierarchy of the owned block, the one the model was computed on
        assert H.block and H.rows == [lev.A.shape[0] for lev in levels] and len(H.rows) >= 2
        assert all(np.array_equal(a.dinv, c.dinv) and (a.A != c.A).nnz == 0 for a, c in zip(H.levels, levels))
        B = FieldStorage(n + ng, 1, "cuda")
        B.dev()[:n, 0] = torch.from_numpy(b).cuda()
        B.dev()[n:] = torch.from_numpy(CS.ghost_fill(ng, 1, 1)).cuda()
        for k in (1, 2):
            ksp.updateOptions({"ksp_max_it": k})
            X = FieldStorage(n + ng, 1, "cuda")
            reason = ksp.solve_block(B, X)[0]
            res, xd = ksp.last_result, X.dev()[:, 0]
            assert hip.ox_dist_status(plan) == 0
            if not torch.equal(xd[n:], xd[send_dev]):
                misses.append(f"k={k}: the ghost block of x is not x[send]")
            got = (reason, int(res.its[0]), xd[:n].cpu().numpy(), float(res.bnorm[0]), float(res.rnorm[0]))
            misses += _cut_misses(f"{CS.AMG_PART} bjacobi+gamg {transport} overlap {overlap} k={k}", got, trace[k], k)
        del ksp, A
    print(f"wall time {time.perf_counter() - t0:.1f} s")
    assert not misses, "\n".join(misses)
