"""GPU: pc_type gamg -- the device V-cycle (ox_mg_apply) against the numpy one, CG + gamg against Jacobi-CG (iterations,
solution, bits, warnings), the cases that keep running jacobi, and FractionalStep_AB_CN with a gamg pressure solve."""
import logging

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GAMG = {"ksp_type": "cg", "pc_type": "gamg", "ksp_rtol": 1e-8, "ksp_atol": 1e-50}
JACOBI = {"ksp_type": "cg", "pc_type": "jacobi", "ksp_rtol": 1e-8, "ksp_atol": 1e-50}


def _poisson(N, deg=1, dirichlet=True, delaunay=False, freeze=False):
    """P1 / P2 Laplacian on the product's space (the pressure matrix's form), Dirichlet rows on two faces as
    ox_zero_rows_cols leaves them."""
    import scipy.sparse as sp

    from oasisx_amd import fem
    from oasisx_amd import mesh as M
    from oasisx_amd.la import SellMatrix
    from oracle import ipcs_oracle as O

    mesh = (M.create_delaunay_box(None, [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], N) if delaunay
            else M.create_box(None, [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], [N, N, N]))
    V = fem.FunctionSpace(mesh, deg, window=256)
    F = O.Forms(mesh.coords.cpu().numpy(), V.cells_in_kernel_order(), deg, 1, vd=V.cell_dofs.cpu().numpy(),
                qd=V.cells_in_kernel_order(), nv_dofs=V.num_dofs, nq_dofs=mesh.num_vertices)
    A = F.stiffness_v().tocsr()
    x = V.x.cpu().numpy()
    if dirichlet:
        bd = (np.abs(x[:, 0]) < 1e-12) | (np.abs(x[:, 2] - 1.0) < 1e-12)
        D = sp.diags(bd.astype(np.float64))
        I = sp.identity(A.shape[0]) - D
        A = (I @ A @ I + D).tocsr()
    S = SellMatrix(V.pattern, symmetric=True)
    S.vals.copy_(V.pattern.values_from_csr(A))
    S.version += 1
    if freeze:
        S.freeze()
    return V, S, A, x


def _rhs(x, mean_free=False):
    b = np.cos(3.0 * x[:, 0]) * (1.0 + x[:, 1]) + np.sin(2.0 * x[:, 2])
    return b - b.mean() if mean_free else b


def _solve(V, A, b, opts, guess=None):
    from oasisx_amd.fem import FieldStorage
    from oasisx_amd.ksp import KSPSolver

    ksp = KSPSolver(None, dict(opts))
    ksp.setOperators(A)
    B = FieldStorage(V.num_dofs, 1, "cuda")
    B.dev()[:, 0] = torch.from_numpy(b).cuda()
    X = FieldStorage(V.num_dofs, 1, "cuda")
    reason = ksp.solve_block(B, X)[0]
    return X.dev()[:, 0].cpu().numpy().copy(), ksp.iterations[0], reason, ksp


@pytest.mark.parametrize("N,deg,delaunay,freeze", [(8, 1, False, False), (12, 1, False, True), (4, 2, True, False)])
def test_device_vcycle_matches_numpy(hip, N, deg, delaunay, freeze):
    from oasisx_amd.amg import Hierarchy

    V, A, Acsr, x = _poisson(N, deg, delaunay=delaunay, freeze=freeze)
    # tail_rows = 1: every phase on the grid; default: the small levels in the single-workgroup tail
    for tail in (1, 0):
        H = Hierarchy(A, {"pc_gamg_coarse_eq_limit": 20}, tail_rows=tail)
        assert len(H.levels) >= (2 if delaunay else 3)
        b = _rhs(x)
        z = torch.empty(V.num_dofs, dtype=torch.float64, device="cuda")
        H.apply(torch.from_numpy(b).cuda(), z)
        ref = H.vcycle_numpy(b)
        assert np.abs(z.cpu().numpy() - ref).max() <= 1e-12 * np.abs(ref).max()
        assert H.kernels_per_cycle() > 0


def test_cg_gamg_iterations_do_not_grow(hip, caplog):
    its = {}
    for N in (16, 32, 64):
        V, A, Acsr, x = _poisson(N, freeze=N == 64)
        b = _rhs(x)
        with caplog.at_level(logging.INFO, logger="oasisx"):
            caplog.clear()
            xg, its[N], reason, ksp = _solve(V, A, b, dict(GAMG, pc_gamg_threshold=0.0, pc_gamg_agg_nsmooths=1,
                                                           pc_gamg_coarse_eq_limit=50, pc_mg_levels=10,
                                                           mg_levels_ksp_max_it=2))
        assert not [r for r in caplog.records if r.levelno >= logging.WARNING], caplog.text
        assert reason == 2 and its[N] <= 30, (N, its)
        if N == 64:
            xj, itj, rj, _ = _solve(V, A, b, dict(JACOBI, ksp_rtol=1e-12))
            assert rj == 2 and itj > 100
            assert np.abs(xg - xj).max() <= 1e-7 * np.abs(xj).max()
            assert np.linalg.norm(Acsr @ xg - b) <= 1e-6 * np.linalg.norm(b)
    assert its[64] <= 1.5 * its[16], its


def test_cg_gamg_pure_neumann_and_bits(hip):
    V, A, Acsr, x = _poisson(16, dirichlet=False)
    b = _rhs(x, mean_free=True)
    xg, itg, rg, _ = _solve(V, A, b, GAMG)
    xg2, itg2, _, _ = _solve(V, A, b, GAMG)
    assert rg == 2 and itg <= 30
    assert itg2 == itg and np.array_equal(xg, xg2)  # identical runs, identical bits
    xj, itj, rj, _ = _solve(V, A, b, dict(JACOBI, ksp_rtol=1e-12))
    assert rj == 2
    xg, xj = xg - xg.mean(), xj - xj.mean()
    assert np.abs(xg - xj).max() <= 1e-7 * np.abs(xj).max()


def test_cg_gamg_nonzero_guess(hip):
    V, A, Acsr, x = _poisson(16)
    b = _rhs(x)
    sol, its0, _, _ = _solve(V, A, b, dict(GAMG, ksp_rtol=1e-12))
    from oasisx_amd.fem import FieldStorage
    from oasisx_amd.ksp import KSPSolver

    ksp = KSPSolver(None, dict(GAMG, ksp_initial_guess_nonzero=True))
    ksp.setOperators(A)
    B = FieldStorage(V.num_dofs, 1, "cuda")
    B.dev()[:, 0] = torch.from_numpy(b).cuda()
    X = FieldStorage(V.num_dofs, 1, "cuda")
    X.dev()[:, 0] = torch.from_numpy(sol * (1.0 + 1e-6)).cuda()
    assert ksp.solve_block(B, X)[0] == 2 and ksp.iterations[0] < its0
    assert np.abs(X.dev()[:, 0].cpu().numpy() - sol).max() <= 1e-7 * np.abs(sol).max()


@pytest.mark.parametrize("kind", ["bcgs", "columns"])
def test_gamg_elsewhere_runs_jacobi_and_warns(hip, caplog, kind):
    from oasisx_amd.fem import FieldStorage
    from oasisx_amd.ksp import KSPSolver

    V, A, Acsr, x = _poisson(8)
    nc = 1 if kind == "bcgs" else 2
    kt = "bcgs" if kind == "bcgs" else "cg"
    B = FieldStorage(V.num_dofs, nc, "cuda")
    for c in range(nc):
        B.dev()[:, c] = torch.from_numpy(_rhs(x) * (c + 1)).cuda()
    out = {}
    for pc in ("gamg", "jacobi"):
        ksp = KSPSolver(None, {"ksp_type": kt, "pc_type": pc, "ksp_rtol": 1e-8})
        ksp.setOperators(A)
        X = FieldStorage(V.num_dofs, nc, "cuda")
        with caplog.at_level(logging.WARNING, logger="oasisx"):
            caplog.clear()
            ksp.solve_block(B, X)
        out[pc] = (X.dev().cpu().numpy().copy(), ksp.iterations[:nc], caplog.text)
    assert "pc_type=gamg" in out["gamg"][2] and "runs jacobi" in out["gamg"][2]
    assert out["gamg"][1] == out["jacobi"][1] and np.array_equal(out["gamg"][0], out["jacobi"][0])


def test_gamg_on_partitioned_operator_resolves_to_jacobi(caplog):
    """Host-level: an operator with a halo plan keeps the Jacobi path (with the warning)."""
    from oasisx_amd.ksp import KSPSolver

    class _Pattern:
        dist = object()
        n_rows = 10

    class _Op:
        pattern = _Pattern()
        symmetric = True

    ksp = KSPSolver(None, dict(GAMG))
    ksp.setOperators(_Op())
    assert not ksp._gamg(1)
    with caplog.at_level(logging.WARNING, logger="oasisx"):
        ksp._audit_options(1)
    assert "pc_type=gamg" in caplog.text and "partitioned" in caplog.text


def _tg_steps(options, steps=5, N=16):
    from tests.helpers import KRYLOV, make_hip_problem

    S, clock, mesh = make_hip_problem(3, N, 2, solver_options=options)
    t, its = 0.0, []
    for _ in range(steps):
        t += 0.005
        clock["t"] = t
        S.solve(0.005, 0.01, max_iter=1)
        its.append(S.iteration_counts()["pressure"][0])
    return S.u.x.array.copy(), S._p.x.array.copy(), its


def test_fractional_step_with_gamg_pressure(hip):
    from tests.helpers import KRYLOV

    gopt = dict(KRYLOV, pressure={"ksp_type": "cg", "pc_type": "gamg", "ksp_rtol": 1e-11, "ksp_atol": 1e-30})
    ug, pg, itg = _tg_steps(gopt)
    uj, pj, itj = _tg_steps(KRYLOV)
    assert max(itg) <= 30, itg
    assert np.abs(ug - uj).max() <= 1e-7 * max(np.abs(uj).max(), 1.0)
    pg, pj = pg - pg.mean(), pj - pj.mean()
    assert np.abs(pg - pj).max() <= 1e-7 * max(np.abs(pj).max(), 1.0)


def test_channel_with_pressure_bc_and_gamg(hip):
    import oasisx_amd as ox
    from oasisx_amd import mesh as M
    from tests.helpers import KRYLOV

    def run(options):
        mesh = M.create_unit_square(None, 24, 24)
        fd = 1
        left = M.locate_entities_boundary(mesh, fd, lambda x: np.isclose(x[0], 0))
        tb = M.locate_entities_boundary(mesh, fd, lambda x: np.isclose(x[1], 0) | np.isclose(x[1], 1))
        right = M.locate_entities_boundary(mesh, fd, lambda x: np.isclose(x[0], 1))
        facets = np.hstack([left, tb, right])
        values = np.hstack([np.full_like(left, 1), np.full_like(tb, 2), np.full_like(right, 3)]).astype(np.int32)
        srt = np.argsort(facets)
        tags = M.meshtags(mesh, fd, facets[srt], values[srt])
        bc_tb = ox.DirichletBC(0.0, ox.LocatorMethod.TOPOLOGICAL, (tags, 2))
        bc_in_x = ox.DirichletBC(lambda x: np.sin(np.pi * x[1]), ox.LocatorMethod.TOPOLOGICAL, (tags, 1))
        bc_in_y = ox.DirichletBC(0.0, ox.LocatorMethod.TOPOLOGICAL, (tags, 1))
        S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_u=[[bc_in_x, bc_tb], [bc_in_y, bc_tb]],
                                    bcs_p=[ox.PressureBC(4.0, (tags, 3))], solver_options=options,
                                    options={"sell_window": 128})
        its = []
        for _ in range(5):
            S.solve(0.01, 0.5, max_iter=1)
            its.append(S.iteration_counts()["pressure"][0])
        return S.u.x.array.copy(), S._p.x.array.copy(), its

    gopt = dict(KRYLOV, pressure={"ksp_type": "cg", "pc_type": "gamg", "ksp_rtol": 1e-11, "ksp_atol": 1e-30})
    ug, pg, itg = run(gopt)
    uj, pj, itj = run(KRYLOV)
    assert max(itg) <= 30, itg
    assert np.abs(ug - uj).max() <= 1e-7 * max(np.abs(uj).max(), 1.0)
    assert np.abs(pg - pj).max() <= 1e-7 * max(np.abs(pj).max(), 1.0)
