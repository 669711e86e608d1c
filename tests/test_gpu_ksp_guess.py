"""GPU: ksp_guess_type fischer (csrc/ox_guess.hip) -- exact guesses on a two-dimensional solution family, the device
guess against the numpy model (tests/guess_model.py), bits and resets, pc_type gamg, FractionalStep_AB_CN on one GPU,
and mesh-partitioned runs on eight rank threads and two processes."""
import logging
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

JAC = {"ksp_type": "cg", "pc_type": "jacobi", "ksp_rtol": 1e-8, "ksp_atol": 1e-50}


def _mass(N):
    """Three-column P2 velocity mass matrix of the product's space (no boundary rows, as fracstep's M)."""
    from oasisx_amd import fem
    from oasisx_amd import mesh as M
    from oasisx_amd.la import SellMatrix
    from oracle import ipcs_oracle as O

    mesh = M.create_box(None, [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], [N, N, N])
    V = fem.FunctionSpace(mesh, 2, window=256)
    F = O.Forms(mesh.coords.cpu().numpy(), V.cells_in_kernel_order(), 2, 1, vd=V.cell_dofs.cpu().numpy(),
                qd=V.cells_in_kernel_order(), nv_dofs=V.num_dofs, nq_dofs=mesh.num_vertices)
    Mm = F.mass_v().tocsr()
    S = SellMatrix(V.pattern, symmetric=True)
    S.vals.copy_(V.pattern.values_from_csr(Mm))
    S.version += 1
    return V, S, Mm, V.x.cpu().numpy()


def _fs(arr):
    from oasisx_amd.fem import FieldStorage

    arr = np.asarray(arr, dtype=np.float64).reshape(arr.shape[0], -1)
    F = FieldStorage(arr.shape[0], arr.shape[1], "cuda")
    F.dev()[:, :] = torch.from_numpy(arr).cuda()
    return F


def _family(Acsr, n, nc, count=6, seed=0):
    rng = np.random.default_rng(seed)
    s1, s2 = rng.standard_normal((n, nc)), rng.standard_normal((n, nc))
    th = np.linspace(0.3, 2.9, count)
    sols = [np.cos(t) * s1 + np.sin(t) * s2 for t in th]
    return sols, [Acsr @ s for s in sols]


def _run_family(S, Acsr, opts, nc, warm, with_ax0=False, count=6):
    from oasisx_amd.ksp import KSPSolver

    n = Acsr.shape[0]
    sols, rhs = _family(Acsr, n, nc, count)
    ksp = KSPSolver(None, dict(opts, ksp_initial_guess_nonzero=warm))
    ksp.setOperators(S)
    X = _fs(np.zeros((n, nc)))
    its, dims = [], []
    rtol = float(opts.get("ksp_rtol", 1e-5))
    for i, (b, x) in enumerate(zip(rhs, sols)):
        # the first two solutions to 1e-12: then they span the family to far below the tolerance of the others
        ksp.updateOptions({"ksp_rtol": 1e-12 if i < 2 else rtol})
        B = _fs(b)
        if not warm:
            X.dev().zero_()
        ax0 = _fs(Acsr @ X.dev().cpu().numpy()) if (with_ax0 and warm) else None
        dims.append(ksp.guess_dim)
        reasons = ksp.solve_block(B, X, ax0=ax0)
        assert all(r > 0 for r in reasons), reasons
        its.append(max(ksp.iterations))
        got = X.dev().cpu().numpy()
        assert np.abs(got - x).max() <= 1e-6 * np.abs(x).max()
    return its, dims


@pytest.mark.parametrize("model", [1, 2])
@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("merged", [True, False])
def test_solution_family_poisson(hip, caplog, model, warm, merged):
    from tests.test_gpu_amg import _poisson

    V, S, Acsr, x = _poisson(10)
    opts = dict(JAC, ksp_cg_merged_reduction=merged)
    if not merged:
        opts["ksp_cg_fold_blocks"] = 0  # the five-kernel iteration
    base, _ = _run_family(S, Acsr, opts, 1, warm)
    with caplog.at_level(logging.WARNING, logger="oasisx"):
        caplog.clear()
        its, dims = _run_family(S, Acsr, dict(opts, ksp_guess_type="fischer", ksp_guess_fischer_model=f"{model},4"), 1,
                                warm)
    assert caplog.text == ""
    assert dims == [0, 1, 2, 3, 4, 1]
    assert all(i <= 1 for i in its[2:5]), (its, base)
    assert min(base[2:]) > 10, base


@pytest.mark.parametrize("model", [1, 2])
def test_solution_family_mass_three_columns(hip, model):
    V, S, Mm, x = _mass(3)
    base, _ = _run_family(S, Mm, JAC, 3, True, with_ax0=True, count=5)
    its, dims = _run_family(S, Mm, dict(JAC, ksp_guess_type="fischer", ksp_guess_fischer_model=(model, 8)), 3, True,
                            with_ax0=True, count=5)
    assert dims == [0, 1, 2, 3, 4]
    assert all(i <= 1 for i in its[2:]), (its, base)
    assert min(base[2:]) > 5, base


def test_device_guess_matches_numpy_model(hip):
    from oasisx_amd.ksp import KSPSolver
    from tests.guess_model import FischerModel
    from tests.test_gpu_amg import _poisson

    V, S, Acsr, x = _poisson(8)
    n = Acsr.shape[0]
    rng = np.random.default_rng(3)
    ksp = KSPSolver(None, dict(JAC, ksp_rtol=1e-10, ksp_initial_guess_nonzero=True, ksp_guess_type="fischer",
                               ksp_guess_fischer_model="1,3"))
    ksp.setOperators(S)
    G = FischerModel(Acsr, nc=1, model=1, size=3)
    X = _fs(rng.standard_normal(n))
    dims = []
    for step in range(7):
        b = Acsr @ (rng.standard_normal(n) + 0.3 * step) if step % 2 else rng.standard_normal(n)
        B = _fs(b)
        xw = X.dev().cpu().numpy()[:, 0].copy()
        dims.append(ksp.guess_dim)
        g = ksp._guess_for(1)
        ksp._guess_form(g, B, X, True, None)  # the guess alone (the solve below forms it again from x_w)
        x0 = X.dev().cpu().numpy()[:, 0].copy()
        X.dev()[:, 0] = torch.from_numpy(xw).cuda()
        ref = G.form(b, xw)
        ref = xw if ref is None else ref[:, 0]
        assert np.abs(x0 - ref).max() <= 1e-10 * np.abs(ref).max(), step
        assert ksp.solve_block(B, X)[0] > 0
        G.update(X.dev().cpu().numpy()[:, 0])
    assert dims == [0, 1, 2, 3, 1, 2, 3]


def test_bits_reset_and_failed_solve(hip):
    from oasisx_amd.ksp import KSPSolver
    from tests.test_gpu_amg import _poisson

    V, S, Acsr, x = _poisson(8)
    n = Acsr.shape[0]
    opts = dict(JAC, ksp_initial_guess_nonzero=True, ksp_guess_type="fischer", ksp_guess_fischer_model="1,4")
    rhs = [np.random.default_rng(s).standard_normal(n) for s in range(4)]

    def run(ksp, bs):
        X = _fs(np.zeros(n))
        for b in bs:
            ksp.solve_block(_fs(b), X)
        return X.dev().cpu().numpy().copy()

    k1, k2 = KSPSolver(None, dict(opts)), KSPSolver(None, dict(opts))
    k1.setOperators(S)
    k2.setOperators(S)
    assert np.array_equal(run(k1, rhs), run(k2, rhs))  # identical sequences, identical bits
    assert k1.guess_dim == 4
    # a failed solve leaves the basis unchanged
    k1.updateOptions({"ksp_max_it": 1})
    X = _fs(np.zeros(n))
    assert k1.solve_block(_fs(rhs[0] * 3.0 + 1.0), X)[0] == -3
    assert k1.guess_dim == 4
    k1.updateOptions({"ksp_max_it": 10000})
    # new values of the operator: the basis is dropped (bits of a fresh solver)
    S.vals.mul_(2.0)
    S.version += 1
    fresh = KSPSolver(None, dict(opts))
    fresh.setOperators(S)
    a, b = run(k1, rhs[:2]), run(fresh, rhs[:2])
    assert np.array_equal(a, b) and k1.guess_dim == fresh.guess_dim == 2


def test_gamg_solution_family(hip, caplog):
    from tests.test_gpu_amg import GAMG, _poisson

    V, S, Acsr, x = _poisson(10)
    base, _ = _run_family(S, Acsr, GAMG, 1, True)
    with caplog.at_level(logging.WARNING, logger="oasisx"):
        caplog.clear()
        its, dims = _run_family(S, Acsr, dict(GAMG, ksp_guess_type="fischer", ksp_guess_fischer_model="1,4"), 1, True)
    assert caplog.text == ""
    assert dims == [0, 1, 2, 3, 4, 1]
    assert all(i <= 1 for i in its[2:5]), (its, base)
    assert min(base[2:]) > 3, base


def _tg(opts_extra, steps=8, N=8):
    from tests.helpers import KRYLOV, make_hip_problem

    opts = {k: dict(v, ksp_initial_guess_nonzero=True) for k, v in KRYLOV.items()}
    for k in ("pressure", "scalar"):
        opts[k].update(opts_extra)
    S, clock, mesh = make_hip_problem(3, N, solver_options=opts)
    t, its = 0.0, []
    for _ in range(steps):
        t += 0.005
        clock["t"] = t
        S.solve(0.005, 0.01, max_iter=1)
        its.append(S.iteration_counts())
    torch.cuda.synchronize()
    return S, its


def test_ipcs_taylor_green_with_fischer(hip, caplog):
    S0, its0 = _tg({})
    with caplog.at_level(logging.WARNING, logger="oasisx"):
        caplog.clear()
        S1, its1 = _tg({"ksp_guess_type": "fischer", "ksp_guess_fischer_model": "1,4"})
    assert not [r for r in caplog.records if r.levelno >= logging.WARNING], caplog.text
    du = float(np.abs(S1._U1.dev().cpu().numpy() - S0._U1.dev().cpu().numpy()).max())
    dp = float(np.abs(S1._P.dev().cpu().numpy() - S0._P.dev().cpu().numpy()).max())
    assert du < 1e-8 and dp < 1e-7, (du, dp)
    upd0 = sum(sum(i["update"]) for i in its0[2:])
    upd1 = sum(sum(i["update"]) for i in its1[2:])
    pr0 = [i["pressure"][0] for i in its0]
    pr1 = [i["pressure"][0] for i in its1]
    print(f"\nupdate iterations, steps 3-8: {upd0} -> {upd1}; pressure per step {pr0} -> {pr1}")
    assert upd1 < upd0
    assert S1._solver_p.guess_dim == 4 and S1._solver_c.guess_dim == 4
    assert S1._M.version == S0._M.version and S1._Ap.version == S0._Ap.version


P_GUESS = {"ksp_guess_type": "fischer", "ksp_guess_fischer_model": "1,4"}


@pytest.mark.parametrize("pressure", ["jacobi", "bjacobi"])
def test_eight_rank_threads_with_fischer(hip, pressure):
    from tests.helpers import KRYLOV, run_rank_threads
    from tests.test_gpu_bjacobi import BJ_P, _index, _run

    pr = dict(KRYLOV["pressure"] if pressure == "jacobi" else BJ_P, **P_GUESS)
    G, gdiffs, gits = _run(3, 8, None, "box", pr, steps=4)
    xu, xq = G._Vi[0][0].x.cpu().numpy(), G._Q.x.cpu().numpy()
    ug, pg = G._U1.dev().cpu().numpy(), G._P.dev().cpu().numpy()[:, 0]
    assert G._solver_p.guess_dim == 4

    def rank_job(comm):
        S, diffs, its = _run(3, 8, comm, "box", pr, steps=4)
        Vi, Q = S._Vi[0][0], S._Q
        iu, iq = _index(xu, Vi.x.cpu().numpy()), _index(xq, Q.x.cpu().numpy())
        ul, pl = S._U1.dev().cpu().numpy(), S._P.dev().cpu().numpy()[:, 0]
        return {"du": float(np.abs(ul - ug[iu]).max()), "dp": float(np.abs(pl - pg[iq]).max()), "its": its,
                "k": S._solver_p.guess_dim}

    res, world = run_rank_threads(8, rank_job)
    its = res[0]["its"]
    print(f"\n{pressure}+fischer, pressure (iterations, reason) per step on 8 ranks: {its}; serial {gits}")
    for r in res:
        assert r["du"] < 1e-8 and r["dp"] < 1e-7, res
        assert r["its"] == its and all(reason > 0 for _, reason in its)
        assert r["k"] == 4


def _worker(rank, world, port, out):
    import torch.distributed as dist

    from tests.helpers import KRYLOV
    from tests.test_gpu_bjacobi import _index, _run

    os.environ["OX_TRANSPORT"] = "p2p"
    os.environ["OX_P2P_TIMEOUT_S"] = "30"
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oasisx_amd.parallel import init_comm

        comm = init_comm()
        pr = dict(KRYLOV["pressure"], **P_GUESS)
        S, diffs, its = _run(3, 6, comm, "box", pr, steps=4)
        G, gdiffs, _ = _run(3, 6, None, "box", pr, steps=4)
        Vi, Q = S._Vi[0][0], S._Q
        assert Vi.dist is not None and S._solver_p.guess_dim == 4
        iu, iq = _index(G._Vi[0][0].x.cpu().numpy(), Vi.x.cpu().numpy()), _index(G._Q.x.cpu().numpy(), Q.x.cpu().numpy())
        ug, pg = G._U1.dev().cpu().numpy(), G._P.dev().cpu().numpy()[:, 0]
        ul, pl = S._U1.dev().cpu().numpy(), S._P.dev().cpu().numpy()[:, 0]
        du, dp = float(np.abs(ul - ug[iu]).max()), float(np.abs(pl - pg[iq]).max())
        assert du < 1e-8 and dp < 1e-7, (du, dp)
        out[rank] = (du, dp, its)
    finally:
        dist.destroy_process_group()


def test_two_processes_p2p_with_fischer(hip):
    import torch.multiprocessing as mp

    from tests.test_gpu_bjacobi import _free_port

    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    assert len(out) == 2, dict(out)
    its = [v[2] for v in out.values()]
    assert its[0] == its[1] and all(reason > 0 for _, reason in its[0])
