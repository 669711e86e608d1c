"""GPU: pc_type bjacobi + sub_pc_type gamg -- one block per rank, each preconditioned by one V-cycle of the hierarchy of
the rank's owned-by-owned block (OX_KSP_CG_MG with a halo plan).  On one GPU the path is exactly pc_type gamg; on eight rank
threads (the 2 x 2 x 2 split) and on 2-3 processes the partitioned IPCS steps match the serial Jacobi run on owned and
ghost entries, with the same iteration counts on every rank."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BJ_P = {"ksp_type": "cg", "pc_type": "bjacobi", "sub_pc_type": "gamg", "ksp_rtol": 1e-11, "ksp_atol": 1e-30}


def test_one_gpu_bjacobi_gamg_is_gamg(hip, caplog):
    import logging

    from tests.test_gpu_amg import GAMG, _poisson, _rhs, _solve

    V, A, Acsr, x = _poisson(16)
    b = _rhs(x)
    xg, itg, rg, _ = _solve(V, A, b, GAMG)
    bj = {k: v for k, v in GAMG.items() if k != "pc_type"}
    with caplog.at_level(logging.WARNING, logger="oasisx"):
        caplog.clear()
        xb, itb, rb, ksp = _solve(V, A, b, dict(bj, pc_type="bjacobi", sub_pc_type="gamg", sub_ksp_type="preonly"))
    assert caplog.text == ""
    assert rb == rg == 2 and itb == itg and itg <= 30
    assert np.array_equal(xb, xg)  # the same iterates, the same bits
    assert not ksp._hierarchy().block
    # the sub_ options are the gamg options of the one block
    xg2, itg2, _, _ = _solve(V, A, b, dict(GAMG, pc_gamg_coarse_eq_limit=20, mg_levels_ksp_max_it=3))
    xb2, itb2, _, _ = _solve(V, A, b, dict(bj, pc_type="bjacobi", sub_pc_type="gamg", sub_pc_gamg_coarse_eq_limit=20,
                                           sub_mg_levels_ksp_max_it=3))
    assert itb2 == itg2 and np.array_equal(xb2, xg2)


def _q(x):
    return np.round((np.asarray(x, dtype=np.float64) + 1.0) * float(1 << 35)).astype(np.int64)


def _index(xg, xl):
    """Positions in the serial run's dofs (coordinates ``xg``) of the rank's dofs (coordinates ``xl``)."""
    kg = {tuple(k): i for i, k in enumerate(_q(xg).tolist())}
    return np.asarray([kg[tuple(k)] for k in _q(xl).tolist()])


def _run(dim, N, comm, kind, pressure, steps=2):
    """Taylor-Green P2-P1 (as tests/test_gpu_threads_rehearsal.py / test_gpu_dist_rehearsal.py), the pressure solved with
    ``pressure``.  Returns the solver, the steps' differences and, per step, the pressure iterations and converged reason
    of THAT step's solve."""
    import oasisx_amd as ox
    from oasisx_amd import mesh as M
    from oracle import ipcs_oracle as O
    from tests.helpers import KRYLOV, on_boundary, on_boundary3

    nu, dt = 0.01, 0.005
    box = [[-1.0] * dim, [1.0] * dim]
    if kind == "delaunay":
        mesh = M.create_delaunay_box(comm, box, N, seed=4)
    else:
        mesh = M.create_rectangle(comm, box, [N, N]) if dim == 2 else M.create_box(comm, box, [N, N, N])
    clock = {"t": 0.0}
    fns = [O.tg_u, O.tg_v, O.tg_w][:dim]
    marker = on_boundary if dim == 2 else on_boundary3
    bcs = [[ox.DirichletBC(lambda x, f=f: f(x, clock["t"], nu), ox.LocatorMethod.GEOMETRICAL, marker)] for f in fns]
    opts = {k: dict(v, ksp_initial_guess_nonzero=True) for k, v in KRYLOV.items()}
    opts["pressure"] = dict(pressure, ksp_initial_guess_nonzero=True)
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_u=bcs, bcs_p=[], solver_options=opts,
                                options={"sell_window": 128})
    for i, f in enumerate(fns):
        S._u2[i].interpolate(lambda x, f=f: f(x, -dt, nu))
        S._u1[i].interpolate(lambda x, f=f: f(x, 0.0, nu))
    S._p.interpolate(lambda x: O.tg_p(x, -dt / 2, nu))
    diffs, its = [], []
    for _ in range(steps):
        clock["t"] += dt
        diffs.append(S.solve(dt, nu, max_iter=1))
        its.append((int(S.iteration_counts()["pressure"][0]), int(S._solver_p.last_result.reason[0])))
    torch.cuda.synchronize()
    return S, diffs, its


@pytest.mark.parametrize("N,kind", [(8, "box"), (6, "delaunay")])
def test_eight_rank_threads_bjacobi_gamg(hip, N, kind):
    from oasisx_amd.fem import FieldStorage
    from tests.helpers import KRYLOV, run_rank_threads

    G, gdiffs, _ = _run(3, N, None, kind, KRYLOV["pressure"])
    xu, xq = G._Vi[0][0].x.cpu().numpy(), G._Q.x.cpu().numpy()
    ug, pg = G._U1.dev().cpu().numpy(), G._P.dev().cpu().numpy()[:, 0]

    def rank_job(comm):
        S, diffs, its = _run(3, N, comm, kind, BJ_P)
        Vi, Q = S._Vi[0][0], S._Q
        assert Vi.dist is not None and S._Ap.pattern.dist is not None
        iu, iq = _index(xu, Vi.x.cpu().numpy()), _index(xq, Q.x.cpu().numpy())
        ul, pl = S._U1.dev().cpu().numpy(), S._P.dev().cpu().numpy()[:, 0]
        ksp = S._solver_p
        assert ksp._bjacobi_gamg(1)
        # the device V-cycle of the rank's block against the numpy one, on a random owned vector
        H = ksp._hierarchy()
        assert H.block and H.rows[0] == Q.n_owned
        r = np.random.default_rng(comm.rank).standard_normal(Q.n_owned)
        z = torch.empty(Q.n_owned, dtype=torch.float64, device="cuda")
        H.apply(torch.from_numpy(r).cuda(), z)
        zr = H.vcycle_numpy(r)
        dv = float(np.abs(z.cpu().numpy() - zr).max() / np.abs(zr).max())
        # two identical solves of a consistent system b = A y (after the steps, whose counts were read above)
        n = Q.n_local
        Y, Bv = FieldStorage(n, 1, "cuda"), FieldStorage(n, 1, "cuda")
        Y.dev()[:n, 0] = torch.from_numpy(np.random.default_rng(100 + comm.rank).standard_normal(n)).cuda()
        S._Ap.mult(Y.dev(), Bv.dev())
        sols = []
        for _ in range(2):
            X = FieldStorage(n, 1, "cuda")
            ksp.solve_block(Bv, X)
            sols.append((X.dev()[:n, 0].cpu().numpy().copy(), ksp.iterations[0]))
        same = bool(np.array_equal(sols[0][0], sols[1][0]) and sols[0][1] == sols[1][1])
        return {"du": float(np.abs(ul - ug[iu]).max()), "dp": float(np.abs(pl - pg[iq]).max()), "diff": diffs[-1],
                "its": its, "dv": dv, "same": same}

    def jacobi_job(comm):
        return _run(3, N, comm, kind, KRYLOV["pressure"])[2]

    res, world = run_rank_threads(8, rank_job)
    jac, _ = run_rank_threads(8, jacobi_job)
    bj = res[0]["its"]
    print(f"\n{kind} N={N}: pressure (iterations, reason) per step on 8 ranks: bjacobi+gamg {bj}, jacobi {jac[0]}")
    for r in res:
        assert r["du"] < 1e-8 and r["dp"] < 1e-7, res  # owned AND ghost entries agree with the serial run
        assert abs(r["diff"] - gdiffs[-1]) < 1e-8 * max(1.0, abs(gdiffs[-1]))
        assert r["its"] == bj and all(reason > 0 for _, reason in bj)  # the steps' counts and reasons, on every rank
        assert r["dv"] <= 1e-12, r["dv"]
        assert r["same"]
    assert all(j == jac[0] for j in jac)
    # every step against Jacobi on the same split.  Measured: Delaunay N = 6 38, 39 against 86, 87
    # -- at most half; box N = 8 31, 32 against 50, 51.  There the owned blocks have 100-125 rows and block Jacobi has no
    # coarse space across the ranks: in a numpy model of this split (P1 Laplacian, octants, cold start, rtol 1e-11) EXACT
    # block solves need 27 iterations against the V-cycle's 32 and Jacobi's 69 -- the V-cycle is not what keeps the box
    # above half (27 / 32 of 31 is still more than half of 50).  The box is held to two thirds.
    limit = 1 / 2 if kind == "delaunay" else 2 / 3
    for (ib, _), (ij, _) in zip(bj, jac[0]):
        assert ib <= limit * ij, (bj, jac[0])
    assert len(set(world.allreduces)) == 1 and min(world.exchanges) > 0


def _free_port():
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, dim, N, transport, out):
    import torch.distributed as dist

    from tests.helpers import KRYLOV

    os.environ["OX_TRANSPORT"] = transport
    os.environ["OX_P2P_TIMEOUT_S"] = "30"
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oasisx_amd.parallel import init_comm

        comm = init_comm()
        assert comm.size == world and comm.handle is None
        S, diffs, its = _run(dim, N, comm, "box", BJ_P)
        G, gdiffs, _ = _run(dim, N, None, "box", KRYLOV["pressure"])
        Vi, Q = S._Vi[0][0], S._Q
        assert Vi.dist is not None and Vi.n_local > Vi.n_owned and S._solver_p._bjacobi_gamg(1)
        assert comm.active == {2: transport, 1: transport}, comm.active
        iu, iq = _index(G._Vi[0][0].x.cpu().numpy(), Vi.x.cpu().numpy()), _index(G._Q.x.cpu().numpy(), Q.x.cpu().numpy())
        ug, pg = G._U1.dev().cpu().numpy(), G._P.dev().cpu().numpy()[:, 0]
        ul, pl = S._U1.dev().cpu().numpy(), S._P.dev().cpu().numpy()[:, 0]
        # owned AND ghost entries agree with the serial run (ghosts are kept consistent)
        du, dp = float(np.abs(ul - ug[iu]).max()), float(np.abs(pl - pg[iq]).max())
        assert du < 1e-8 and dp < 1e-7, (du, dp)
        assert abs(diffs[-1] - gdiffs[-1]) < 1e-8 * max(1.0, abs(gdiffs[-1]))
        out[rank] = (du, dp, its)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("transport", ["p2p", "host"])
@pytest.mark.parametrize("dim,N,world", [(3, 6, 2), (2, 12, 3)])
def test_processes_bjacobi_gamg_match_serial(hip, dim, N, world, transport):
    import torch.multiprocessing as mp

    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), dim, N, transport, out), nprocs=world, join=True)
    assert len(out) == world, dict(out)
    its = [v[2] for v in out.values()]
    assert all(i == its[0] for i in its) and all(reason > 0 for _, reason in its[0])  # the same on every rank
