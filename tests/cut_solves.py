"""Cut solves against the extended-precision k-step model: what tests/test_gpu_reduction_sizes.py (one GPU) and
tests/test_gpu_partitioned_cuts.py (one-rank plans whose only peer is the rank itself) share.  A solve is CUT after k
iterations (``ksp_rtol`` 1e-30, ``ksp_max_it`` k) and its k-th iterate and both norms are compared with
tests/krylov_steps_model.py to TOL.  Importable without a GPU; everything that touches the device is imported inside
the functions."""
import os
import re

import numpy as np
import torch

from tests import krylov_steps_model as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12  # the bound test_single_reduction_cg_nonzero_guess_and_max_it puts on a cut solve
PRE = 1e-13  # float64 run of the recurrence against the extended one: the systems themselves allow TOL
GHOST_FILL = 1.0e3  # magnitude of the ghost rows of b and of the nonzero guess: a sum that includes one misses grossly

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
CUTS = ((1, False), (2, False), (3, False), (2, True))  # (k, nonzero guess)


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


def _sell(Acsr, symmetric, plan=None, n_owned=None):
    """SellMatrix of a scipy CSR matrix with sorted indices, without a mesh.  ``plan`` (an ox_dist handle) and
    ``n_owned``: the local matrix of a partitioned operator, n_owned rows by n_owned + n_ghost columns -- the pattern
    carries the plan and its interior / boundary slice lists (``SellPattern.split_interior``)."""
    from oasisx_amd import fem
    from oasisx_amd.la import SellMatrix

    n, n_cols = Acsr.shape
    rl = np.diff(Acsr.indptr).astype(np.int64)
    keys = np.repeat(np.arange(n, dtype=np.int64), rl) * n_cols + Acsr.indices
    P = fem.build_sell(n, n_cols, torch.from_numpy(keys).cuda(), torch.from_numpy(rl).cuda(),
                       torch.from_numpy(Acsr.indptr.astype(np.int64)).cuda())
    if plan is not None:
        assert n_owned == n
        P.dist = plan
        P.split_interior(n_owned)
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
        self.worst_pre = 0.0  # largest float64-against-extended figure seen so far

    def get(self, c, guess):
        key = (c, guess)
        if key not in self._t:
            kmax, x0 = (2, self.x0[:, c]) if guess else (3, None)
            hi = self.trace(self.A, self.b[:, c], x0, kmax)
            lo = self.trace(self.A, self.b[:, c], x0, kmax, dtype=np.float64)
            for k, (h, l) in enumerate(zip(hi, lo)):
                ex = float(np.abs(h[0] - l[0]).max() / max(np.abs(h[0]).max(), np.finfo(np.float64).tiny))
                er = float(abs(h[2] - l[2]) / h[1])
                self.worst_pre = max(self.worst_pre, ex, er)
                assert ex <= PRE and er <= PRE, f"the system does not allow {PRE:g} on the CPU: column {c}, k = {k}: {ex:.2e}, {er:.2e}"
            self._t[key] = [(np.asarray(h[0], dtype=np.float64), float(h[1]), float(h[2]), float(h[-1])) for h in hi]
        return self._t[key]


def ghost_fill(ng, nc, seed):
    """(ng, nc) values of magnitude GHOST_FILL .. 2 GHOST_FILL with mixed signs."""
    rng = np.random.default_rng(5000 + seed)
    return GHOST_FILL * (1.0 + rng.random((ng, nc))) * np.where(rng.random((ng, nc)) < 0.5, -1.0, 1.0)


def _check_cuts(A, ref, runs, n, dict_dinv=False, plan=None, send=None, keep=None):
    """Every (method, columns) of ``runs``: k = 1, 2, 3 from a zero guess and k = 2 from a nonzero one; returns the list of
    misses (empty: all within TOL) and prints every figure.

    ``plan`` and ``send`` (partitioned operators): the vectors have n + len(send) rows, the ghost rows of B and of the
    nonzero guess are filled with values of magnitude GHOST_FILL, and after every solve the ghost block of X must equal
    X[send] bit for bit (the scatter-forward of ksp.py) and the plan must report no timed-out wait.  ``keep`` (a dict):
    receives (method, nc, k, guess) -> (X on the device, bnorm, rnorm) for comparisons between runs."""
    from oasisx_amd import _lib
    from oasisx_amd.fem import FieldStorage
    from oasisx_amd.ksp import KSPSolver

    ng = 0 if send is None else int(len(send))
    send_dev = torch.from_numpy(np.asarray(send, dtype=np.int64)).cuda() if ng else None
    misses = []
    for method, nc in runs:
        B = FieldStorage(n + ng, nc, "cuda")
        B.dev()[:n] = torch.from_numpy(ref.b[:, :nc]).cuda()
        x0 = torch.zeros(n + ng, nc, dtype=torch.float64, device="cuda")
        x0[:n] = torch.from_numpy(np.ascontiguousarray(ref.x0[:, :nc])).cuda()
        if ng:
            B.dev()[n:] = torch.from_numpy(ghost_fill(ng, nc, 1)).cuda()
            x0[n:] = torch.from_numpy(ghost_fill(ng, nc, 2)).cuda()
        ksp = KSPSolver(None, dict(METHODS[method], pc_type="jacobi", ksp_rtol=1e-30))
        ksp.setOperators(A)
        if plan is not None:
            assert not ksp._cg_folded(), "a partitioned operator must not fold its synchronisation points"
        recurrence_norm = method == "bcgs_merged"
        for k, guess in CUTS:
            ksp.updateOptions({"ksp_max_it": k, "ksp_initial_guess_nonzero": guess})
            X = FieldStorage(n + ng, nc, "cuda")
            if guess:
                X.dev().copy_(x0)
            reasons = ksp.solve_block(B, X)
            if dict_dinv:
                assert ksp._dcode is not None, "the dictionary of dinv was not built: CODE = true is not what runs"
            res, xd = ksp.last_result, X.dev()
            xs = xd.cpu().numpy()
            tag = f"{method} nc={nc} k={k} guess={int(guess)}"
            if plan is not None:
                assert _lib.load().ox_dist_status(plan) == 0, f"{tag}: a wait of the plan timed out"
                if not torch.equal(xd[n:], xd[send_dev]):
                    misses.append(f"{tag}: the ghost block of x is not x[send] (no scatter-forward after the solve)")
            if keep is not None:
                keep[(method, nc, k, guess)] = (xd[:n].clone(), [float(res.bnorm[c]) for c in range(nc)],
                                                [float(res.rnorm[c]) for c in range(nc)])
            for c in range(nc):
                xr, bn, rn_true, rn_rec = ref.get(c, guess)[k]
                rn = rn_rec if recurrence_norm else rn_true
                ex = float(np.abs(xs[:n, c] - xr).max() / np.abs(xr).max())
                eb = abs(res.bnorm[c] - bn) / bn
                er = abs(res.rnorm[c] - rn) / bn
                tag = f"{method} nc={nc} c={c} k={k} guess={int(guess)}"
                print(f"  {tag}: reason {reasons[c]} its {res.its[c]}  x {ex:.2e}  bnorm {eb:.2e}  rnorm {er:.2e}")
                if reasons[c] != _lib.DIVERGED_ITS or res.its[c] != k:
                    misses.append(f"{tag}: reason {reasons[c]}, {res.its[c]} iterations")
                if not (ex <= TOL and eb <= TOL and er <= TOL):
                    misses.append(f"{tag}: x {ex:.2e} bnorm {eb:.2e} rnorm {er:.2e}")
    return misses


# ---- partitioned operators: the systems of tests/test_gpu_partitioned_cuts.py (plain data and host builders) ---------
SMALL = 8  # partial rows of the small case's unsplit mat-vec: n = rows_for_parts(8) = 1829, 29 slices
SMALL_R0 = 64 * 11 + 21  # 11 interior slices, 18 boundary ones (the slice of r0 mixes both kinds of rows)
PART_SYSTEMS = [(SMALL, "sym"), (SMALL, "nonsym"), (SMALL, "dict"), (760, "sym"), (760, "nonsym"), (776, "sym"),
                (776, "nonsym"), (1096, "nonsym"), (4104, "sym"), (4104, "nonsym")]
AMG_PART = "two-deg1"  # the system of tests/amg_steps_model.py that the block-Jacobi AMG case ghosts
_PART = {}


def part_r0(nparts):
    from tests import reduction_systems as RS

    return SMALL_R0 if nparts == SMALL else RS.ghost_start(RS.rows_for_parts(nparts))


def part_system(nparts, kind):
    """(Acsr, A_loc, send, reference) of a partitioned case; systems, seeds and right-hand sides are those of
    tests/test_gpu_reduction_sizes.py.  The latest system only is kept (the references of the large ones are not small)."""
    from tests import reduction_systems as RS

    key = (nparts, kind)
    if _PART.get("key") != key:
        n = RS.rows_for_parts(nparts)
        Acsr = RS.banded_system(n, kind, seed=nparts % 89)
        A_loc, send = RS.ghosted(Acsr, part_r0(nparts), perm_seed=nparts)
        ref = _Reference(Acsr, RS.signed_unit_vectors(n, 3, seed=nparts), 0.25 * RS.signed_unit_vectors(n, 3, seed=nparts + 1),
                         bicgstab=kind == "nonsym")
        _PART.clear()
        _PART.update(key=key, value=(Acsr, A_loc, send, ref))
    return _PART["value"]


def amg_part_r0():
    from tests import amg_steps_model as M
    from tests import reduction_systems as RS

    n, m = M.CASES[AMG_PART][:2]
    return RS.ghost_start(n, m)


def amg_part_system():
    """(A, A_loc, send, levels, b) of the block-Jacobi AMG case: ``levels`` are those of the owned-by-owned block
    A_loc[:, :n], which is what the solver's preconditioner is built on; A = folded(A_loc, send) is the operator."""
    if "amg" not in _PART:
        from oasisx_amd import amg
        from tests import amg_steps_model as M
        from tests import reduction_systems as RS

        n, m, _, _, options, _ = M.CASES[AMG_PART]
        A = M.system(AMG_PART)[0]
        A_loc, send = RS.ghosted(A, amg_part_r0(), perm_seed=n, m=m)
        levels = amg.build_levels(amg.owned_block(A_loc), options)
        _PART["amg"] = (A, A_loc, send, levels, M.right_hand_sides(AMG_PART, 1, M.RHS_SEED)[:, 0])
    return _PART["amg"]
