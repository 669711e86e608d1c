"""GPU: flux and Robin conditions of the scalars (``flux_bcs=[FluxBC, RobinBC]``, oasisx_amd/scalar.py,
``ox_scalar_boundary`` of csrc/ox_scalar.hip) against the numpy model of tests/scalar_bc_model.py, which is built on the
oracle's forms fed the device's numbering and pinned by tests/test_scalar_bc_host.py.  Sizes, bounds and helpers are those
of tests/test_gpu_scalar.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [(2, 6, 1), (2, 5, 2), (3, 3, 1), (3, 3, 2), (2, 4, 3)]


def top(x):
    return np.isclose(x[1], 1.0)


def bottom(x):
    return np.isclose(x[1], -1.0)


def right(x):
    return np.isclose(x[0], 1.0)


def lower_right(x):
    return np.isclose(x[0], 1.0) & (x[1] <= 1e-12)


def _facets(mesh, marker):
    from oasisx_amd import mesh as M

    return np.asarray(M.locate_entities_boundary(mesh, mesh.gdim - 1, marker), dtype=np.int64)


def _model_facets(S, mesh, ids):
    """(cell in the kernels' order, opposite local vertex) of mesh facets: what the model's conditions take."""
    from oasisx_amd.wall import facet_table

    cells, opp = facet_table(mesh, np.sort(np.asarray(ids, dtype=np.int64)))
    return S._Vi[0][0].kernel_cell_index(cells), opp


def _mesh(dim, N, mode="dictionary"):
    from oasisx_amd import mesh as M
    from tests.helpers import tg_mesh

    if mode == "delaunay":
        return M.create_delaunay_box(None, [[-1.0] * dim, [1.0] * dim], 6 if dim == 2 else 4, seed=2)
    return tg_mesh(dim, N)


def _update(sc):
    for bc in sc.bcs:
        bc.update_bc()
    for bc in sc.flux_bcs:
        bc.update()


def _assemble(S, clock, scalars, dt, nu):
    for bcl in S._bcs_u:
        for bc in bcl:
            bc.update_bc()
    for sc in scalars:
        _update(sc)
    S.assemble_first(dt, nu)
    return 1.5 * S._U1.rhost() - 0.5 * S._U2.rhost()


def _compare(g, col, A_ref, b_ref, what=""):
    dA = abs(g.Ac.to_scipy() - A_ref).max()
    db = np.abs(g.B.rhost()[:, col] - b_ref).max()
    print(f"{what}: dA = {dA:.3e} (max|A| = {abs(A_ref).max():.3e}), db = {db:.3e} (max|b| = {np.abs(b_ref).max():.3e})")
    assert dA <= 1e-12 * abs(A_ref).max(), dA
    assert db <= 1e-12 * np.abs(b_ref).max(), db


class Data:
    """Non-constant data of the conditions; c_inf moves with the clock."""

    def __init__(self):
        self.clock = {"t": 0.0}
        self.src = lambda x: 1.0 + x[0] * x[1]
        self.val = lambda x: 1.0 + x[0] + self.clock["t"]
        self.ini = lambda x: np.cos(2.0 * x[0]) + 0.5 * x[1]
        self.q = lambda x: 0.5 + x[0] - 0.3 * x[0] ** 2
        self.q2 = lambda x: -0.4 + x[1]
        self.h = lambda x: 1.0 + 0.5 * x[1] ** 2
        self.c_inf = lambda x: 0.3 - x[1] + 2.0 * self.clock["t"]


# ---- 1. operator and right-hand side, entry by entry -------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dictionary", "f64", "delaunay"])
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_operator_and_rhs_entry_by_entry(hip, dim, N, deg, mode):
    """After assemble_first: A_c and b_c equal the model's to 1e-12 max|.| (the bound of
    tests/test_gpu_scalar.py::test_operator_and_rhs_entry_by_entry) with kappa != nu, a source and non-constant callables:
    a FluxBC on y = -1 and a RobinBC(advective=0.7) on x = 1 meet in a corner, a Dirichlet side (y = 1) meets the Robin
    side and wins on the rim dofs, a second FluxBC lies on the lower half of the Robin side (two conditions per facet);
    u_ab . n = sin(pi y) changes sign along x = 1.  A Robin group hands no A_c c_1 on; two assemblies give equal bits."""
    import torch

    import oasisx_amd as ox
    from tests import scalar_bc_model as BM
    from tests.test_gpu_scalar import _dofs, _forms, _options, _problem

    dt, nu, kappa = 0.1, 0.5, 0.2
    D = Data()
    mesh = _mesh(dim, N, mode)
    fb, fr, fh = _facets(mesh, bottom), _facets(mesh, right), _facets(mesh, lower_right)
    assert fb.size and fr.size and 0 < fh.size < fr.size
    sc = ox.ScalarTransport("T", diffusivity=kappa, source=D.src, initial=D.ini,
                            bcs=[ox.DirichletBC(D.val, ox.LocatorMethod.GEOMETRICAL, top)],
                            flux_bcs=[ox.FluxBC(D.q, fb), ox.RobinBC(D.h, D.c_inf, fr, advective=0.7), ox.FluxBC(D.q2, fh)])
    S, clock, mesh = _problem(dim, N, deg, [sc], nu=nu, dt=dt, mesh=mesh, solver_options=_options(guess=True),
                              options={"value_dictionary": mode != "f64"})
    g = S._scalar_groups[0]
    bp = g.boundary
    assert bp.robin and bp.adv and bp.n_records == fb.size + fr.size + fh.size
    assert bp.pairs.n_pairs > bp.pairs.n_rows  # corner rows and the doubly covered facets carry several pairs
    F, x_v = _forms(S, mesh)
    conds = [BM.Flux(*_model_facets(S, mesh, fb), D.q), BM.Robin(*_model_facets(S, mesh, fr), D.h, D.c_inf, beta=0.7),
             BM.Flux(*_model_facets(S, mesh, fh), D.q2)]
    m = BM.ScalarBCModel(F, x_v, kappa, dofs=_dofs(x_v, top), value=D.val, source=D.src, conditions=conds)
    m.interpolate(D.ini)
    clock["t"] = D.clock["t"] = dt
    uab = _assemble(S, clock, [sc], dt, nu)
    un = uab[_dofs(x_v, right), 0]
    assert un.min() < -0.05 and un.max() > 0.05  # inflow and outflow along the Robin side
    A_ref, b_ref = m.assemble(uab, dt)
    assert abs(m.H).max() > 0.0 and np.abs(m.load).max() > 0.0
    _compare(g, 0, A_ref, b_ref, f"({dim},{N},P{deg},{mode})")
    rim = np.intersect1d(_dofs(x_v, top), _dofs(x_v, right))
    want = D.val(np.vstack([x_v[rim].T, np.zeros((3 - dim, rim.size))]))
    assert rim.size and np.abs(g.B.rhost()[rim, 0] - want).max() <= 1e-14  # the Dirichlet row wins on the rim
    assert not g.ax0_valid  # A_c changed after the row kernel
    a0, b0 = g.Ac.vals.clone(), g.B.rdev().clone()
    S.assemble_first(dt, nu)
    assert torch.equal(a0, g.Ac.vals) and torch.equal(b0, g.B.rdev())
    with pytest.raises(RuntimeError, match="inside assemble_first"):
        S.scalar_boundary_assemble()


def test_all_exterior_facets_full_and_partial_block(hip):
    """A RobinBC on every exterior facet of the 3-D N = 4 P2 box: 386 touched rows, a full block of 256 lanes and a
    partial one."""
    import oasisx_amd as ox
    from tests import scalar_bc_model as BM
    from tests.test_gpu_scalar import _forms, _options, _problem

    dt, nu, kappa = 0.1, 0.5, 0.2
    D = Data()
    mesh = _mesh(3, 4)
    sc = ox.ScalarTransport("T", diffusivity=kappa, source=D.src, initial=D.ini,
                            flux_bcs=[ox.RobinBC(D.h, D.c_inf, None, advective=0.7), ox.FluxBC(D.q, None)])
    S, clock, mesh = _problem(3, 4, 2, [sc], nu=nu, dt=dt, mesh=mesh, solver_options=_options())
    g = S._scalar_groups[0]
    assert g.boundary.pairs.n_rows == 386 and g.boundary.n_records == 2 * mesh.exterior_facets().shape[0]
    F, x_v = _forms(S, mesh)
    fc, fa = _model_facets(S, mesh, mesh.exterior_facets())
    m = BM.ScalarBCModel(F, x_v, kappa, source=D.src, conditions=[BM.Robin(fc, fa, D.h, D.c_inf, beta=0.7), BM.Flux(fc, fa, D.q)])
    m.interpolate(D.ini)
    clock["t"] = D.clock["t"] = dt
    uab = _assemble(S, clock, [sc], dt, nu)
    _compare(g, 0, *m.assemble(uab, dt), "all exterior facets")


@pytest.mark.parametrize("kind", ["flux", "robin"])
def test_empty_facet_set(hip, kind):
    import oasisx_amd as ox
    from tests.scalar_model import ScalarModel
    from tests.test_gpu_scalar import _forms, _options, _problem

    dt, nu, kappa = 0.1, 0.5, 0.2
    D = Data()
    none = np.zeros(0, dtype=np.int64)
    bc = ox.FluxBC(D.q, none) if kind == "flux" else ox.RobinBC(D.h, D.c_inf, none, advective=0.5)
    sc = ox.ScalarTransport("T", diffusivity=kappa, source=D.src, initial=D.ini, flux_bcs=[bc])
    S, clock, mesh = _problem(2, 5, 2, [sc], nu=nu, dt=dt, solver_options=_options())
    g = S._scalar_groups[0]
    assert g.boundary.n_records == 0 and g.boundary.pairs.n_rows == 0
    F, x_v = _forms(S, mesh)
    m = ScalarModel(F, x_v, kappa, source=D.src)
    m.interpolate(D.ini)
    clock["t"] = dt
    uab = _assemble(S, clock, [sc], dt, nu)
    _compare(g, 0, *m.assemble(uab, dt), f"empty {kind}")


def test_three_columns_in_lock_step(hip):
    """Three scalars whose Robin conditions differ only in c_inf, two of them with FluxBCs of their own: one group, one
    matrix, each column's b_c against its own model."""
    import oasisx_amd as ox
    from tests import scalar_bc_model as BM
    from tests.test_gpu_scalar import _forms, _options, _problem

    dt, nu, kappa = 0.1, 0.5, 0.2
    D = Data()
    mesh = _mesh(2, 5)
    fb, fr, fh = _facets(mesh, bottom), _facets(mesh, right), _facets(mesh, lower_right)
    cinf = [D.c_inf, 2.5, lambda x: x[1] ** 2]

    def make(h=D.h):
        rob = [ox.RobinBC(h, cinf[j], fr, advective=0.7) for j in range(3)]
        lists = [[ox.FluxBC(D.q, fb), rob[0]], [rob[1]], [rob[2], ox.FluxBC(D.q2, fh)]]
        return [ox.ScalarTransport(f"s{j}", diffusivity=kappa, source=D.src, initial=D.ini, flux_bcs=lists[j]) for j in range(3)]

    scalars = make()
    S, clock, mesh = _problem(2, 5, 2, scalars, nu=nu, dt=dt, mesh=mesh, solver_options=_options())
    assert len(S._scalar_groups) == 1 and S._scalar_groups[0].nc == 3
    g = S._scalar_groups[0]
    F, x_v = _forms(S, mesh)
    clock["t"] = D.clock["t"] = dt
    uab = _assemble(S, clock, scalars, dt, nu)
    mown = [[BM.Flux(*_model_facets(S, mesh, fb), D.q)], [], [BM.Flux(*_model_facets(S, mesh, fh), D.q2)]]
    for j in range(3):
        m = BM.ScalarBCModel(F, x_v, kappa, source=D.src,
                             conditions=mown[j] + [BM.Robin(*_model_facets(S, mesh, fr), D.h, cinf[j], beta=0.7)])
        m.interpolate(D.ini)
        _compare(g, j, *m.assemble(uab, dt), f"column {j}")
    S2, _, _ = _problem(2, 5, 2, make()[:2] + make(h=2.0)[2:], nu=nu, dt=dt, mesh=mesh, solver_options=_options())
    assert sorted(g.nc for g in S2._scalar_groups) == [1, 2]  # a different h: a matrix of its own


# ---- 2. the by-product rule --------------------------------------------------------------------------------------------
def test_flux_only_group_keeps_the_product(hip):
    """A FluxBC changes no matrix: with a nonzero initial guess the group still takes A_c c_1 from the row kernel, and it
    equals the mat-vec bit for bit; the scalar shares the group of a plain one."""
    import torch

    import oasisx_amd as ox
    from tests import scalar_bc_model as BM
    from tests.test_gpu_scalar import _forms, _options, _problem

    dt, nu, kappa = 0.1, 0.5, 0.2
    D = Data()
    mesh = _mesh(2, 5)
    fb = _facets(mesh, bottom)
    scalars = [ox.ScalarTransport("T", diffusivity=kappa, source=D.src, initial=D.ini, flux_bcs=[ox.FluxBC(D.q, fb)]),
               ox.ScalarTransport("plain", diffusivity=kappa, source=D.src, initial=D.ini)]
    S, clock, mesh = _problem(2, 5, 2, scalars, nu=nu, dt=dt, mesh=mesh, solver_options=_options(guess=True))
    assert len(S._scalar_groups) == 1
    g = S._scalar_groups[0]
    assert not g.boundary.robin and not g.boundary.adv
    F, x_v = _forms(S, mesh)
    clock["t"] = dt
    uab = _assemble(S, clock, scalars, dt, nu)
    for j, conds in enumerate([[BM.Flux(*_model_facets(S, mesh, fb), D.q)], []]):
        m = BM.ScalarBCModel(F, x_v, kappa, source=D.src, conditions=conds)
        m.interpolate(D.ini)
        _compare(g, j, *m.assemble(uab, dt), f"column {j}")
    assert g.ax0_valid
    y = torch.zeros_like(g.C1.rdev())
    g.Ac.mult(g.C1.rdev(), y, 2)
    assert torch.equal(y[: S._no_u], g.AC1.rdev()[: S._no_u])


# ---- 3. steps against the model ------------------------------------------------------------------------------------------
def _steps(S, clock, D, m, dt, nu, name="T", nut=False, steps=3):
    from tests.test_gpu_scalar import _c

    g = S._scalar_index[name][0]
    for k in range(steps):
        clock["t"] = D.clock["t"] = (k + 1) * dt
        S.solve(dt, nu, max_iter=1)
        assert not g.ax0_valid
        if nut:
            m.step(S._UAB.rhost(), dt, nut=S._nut.cpu().numpy())
        else:
            m.step(S._UAB.rhost(), dt)
        c = _c(S, name)
        rel = np.abs(c - m.c).max() / np.abs(m.c).max()
        its = S.iteration_counts()["scalar_transport"][name]
        print(f"step {k}: rel diff {rel:.3e}, iterations {its} (model {m.its})")
        assert m.reason > 0
        assert rel < 1e-8, (k, rel)
        assert abs(its - m.its) <= 1, (k, its, m.its)
        assert np.array_equal(c, _c(S, name, 1))  # c_1 <- c


def _conditions(mesh, D):
    """FluxBC on y = -1, RobinBC(advective=0.7) with a time-dependent c_inf on x = 1: the device's list and, given the
    solver, the model's."""
    import oasisx_amd as ox
    from tests import scalar_bc_model as BM

    fb, fr = _facets(mesh, bottom), _facets(mesh, right)
    dev = [ox.FluxBC(D.q, fb), ox.RobinBC(D.h, D.c_inf, fr, advective=0.7)]
    mod = lambda S: [BM.Flux(*_model_facets(S, mesh, fb), D.q),  # noqa: E731
                     BM.Robin(*_model_facets(S, mesh, fr), D.h, D.c_inf, beta=0.7)]
    return dev, mod


@pytest.mark.parametrize("dim,N", [(2, 8), (3, 4)])
@pytest.mark.parametrize("guess", [False, True])
def test_steps_match_the_model(hip, dim, N, guess):
    """3 steps, P2: relative max difference in c below 1e-8, iteration counts within +-1 of the model's (the bounds of
    tests/test_gpu_scalar.py::test_steps_match_the_model); c_inf depends on time through the clock."""
    import oasisx_amd as ox
    from tests import scalar_bc_model as BM
    from tests.test_gpu_scalar import _dofs, _forms, _options, _problem

    nu, dt, kappa = 0.01, 0.005, 0.03
    D = Data()
    D.src = lambda x: 0.5 + x[0]
    D.ini = lambda x: np.cos(np.pi * x[0]) * np.cos(np.pi * x[1])
    mesh = _mesh(dim, N)
    dev, mod = _conditions(mesh, D)
    sc = ox.ScalarTransport("T", diffusivity=kappa, source=D.src, initial=D.ini, flux_bcs=dev,
                            bcs=[ox.DirichletBC(D.val, ox.LocatorMethod.GEOMETRICAL, top)])
    so = _options(guess=guess)
    S, clock, mesh = _problem(dim, N, 2, [sc], nu=nu, dt=dt, mesh=mesh, solver_options=so)
    F, x_v = _forms(S, mesh)
    m = BM.ScalarBCModel(F, x_v, kappa, dofs=_dofs(x_v, top), value=D.val, source=D.src, options=so["scalar_transport"],
                         conditions=mod(S))
    m.interpolate(D.ini)
    _steps(S, clock, D, m, dt, nu)


# ---- 4., 5. fixed point and conservation in a fluid at rest --------------------------------------------------------------
def _rest_problem(dim, N, deg, scalars, mesh):
    """A fluid at rest: no-slip walls, zero fields; the scalar's solves at ksp_rtol 1e-12."""
    import oasisx_amd as ox
    from tests.helpers import on_boundary, on_boundary3
    from tests.test_gpu_scalar import TIGHT, _options

    marker = on_boundary if dim == 2 else on_boundary3
    bcs_u = [[ox.DirichletBC(0.0, ox.LocatorMethod.GEOMETRICAL, marker)] for _ in range(dim)]
    return ox.FractionalStep_AB_CN(mesh, ("Lagrange", deg), ("Lagrange", 2 if deg == 3 else 1), bcs_u=bcs_u, bcs_p=[],
                                   solver_options=_options(TIGHT), options={"sell_window": 256}, scalars=scalars)


@pytest.mark.parametrize("dim,N,deg", [(2, 8, 1), (2, 8, 2), (2, 4, 3), (3, 4, 2)])
def test_robin_fixed_point(hip, dim, N, deg):
    """c = 1 on x = -1, RobinBC(h, c_inf) on x = 1, nothing on the other sides, fluid at rest: the linear profile with
    -kappa c' = h (c - c_inf) is a fixed point of the discrete step.  Three steps at ksp_rtol 1e-12 stay within 1e-8
    relative; a wrong factor in H, the load or the Crank-Nicolson term moves it at first order (pinned on the model by
    tests/test_scalar_bc_host.py::test_fixed_point_drift_of_the_model)."""
    import oasisx_amd as ox
    from tests.test_gpu_scalar import _c, left
    from tests.test_scalar_bc_host import robin_profile

    kappa, h, c_inf, dt, nu = 0.3, 2.0, -0.5, 0.05, 0.01
    mesh = _mesh(dim, N)
    prof = robin_profile(kappa, h, c_inf)
    sc = ox.ScalarTransport("T", diffusivity=kappa, initial=prof, bcs=[ox.DirichletBC(1.0, ox.LocatorMethod.GEOMETRICAL, left)],
                            flux_bcs=[ox.RobinBC(h, c_inf, _facets(mesh, right))])
    S = _rest_problem(dim, N, deg, [sc], mesh)
    ref = _c(S, "T", 1)
    assert abs(ref.min() - prof(np.array([[1.0], [0.0], [0.0]]))[0]) < 1e-14 and ref.max() == 1.0
    for _ in range(3):
        S.solve(dt, nu, max_iter=1)
    drift = np.abs(_c(S, "T") - ref).max() / np.abs(ref).max()
    print(f"({dim},{N},P{deg}): drift {drift:.3e}")
    assert drift < 1e-8


@pytest.mark.parametrize("dim,N,deg", [(2, 8, 2), (3, 4, 2), (2, 4, 3)])
def test_flux_conservation(hip, dim, N, deg):
    """FluxBC(q) with a non-constant q on y = -1, no Dirichlet row, no source, fluid at rest, c(0) = 0:
    1^T M (c^n - c^0) = n dt sum_f int_f q_I ds to 1e-8 relative, M and the integral from the model's forms."""
    import oasisx_amd as ox
    from tests import scalar_bc_model as BM
    from tests.test_gpu_scalar import _c, _forms

    kappa, dt, nu, n = 0.3, 0.05, 0.01, 3
    q = lambda x: 1.0 + 0.5 * x[0] + x[0] ** 2  # noqa: E731
    mesh = _mesh(dim, N)
    fb = _facets(mesh, bottom)
    sc = ox.ScalarTransport("T", diffusivity=kappa, flux_bcs=[ox.FluxBC(q, fb)])
    S = _rest_problem(dim, N, deg, [sc], mesh)
    F, x_v = _forms(S, mesh)
    _, load, _ = BM.surface_terms(F, x_v, BM.Flux(*_model_facets(S, mesh, fb), q), np.zeros((F.nv, dim)))
    M = F.mass_v()
    c0 = _c(S, "T", 1)
    assert np.abs(c0).max() == 0.0
    for _ in range(n):
        S.solve(dt, nu, max_iter=1)
    one = np.ones(F.nv)
    gained, expected = one @ (M @ (_c(S, "T") - c0)), n * dt * load.sum()
    defect = abs(gained - expected) / abs(expected)
    print(f"({dim},{N},P{deg}): gained {gained:.12e}, expected {expected:.12e}, defect {defect:.3e}")
    assert expected > 0.05 and defect < 1e-8


# ---- 6. the open boundary ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N", [(2, 6), (3, 4)])
def test_open_boundary(hip, dim, N):
    """RobinBC(0, c_inf, advective=1) on x = 1, where u_ab . n = sin(pi y) flows out on y > 0 and in on y < 0: the rows
    whose facets see only outflow are bit-equal to a run without the condition, all rows match the model."""
    import oasisx_amd as ox
    from tests import scalar_bc_model as BM
    from tests.test_gpu_scalar import _forms, _options, _problem

    dt, nu, kappa = 0.1, 0.5, 0.2
    D = Data()
    out = []
    for with_bc in (False, True):
        mesh = _mesh(dim, N)
        fr = _facets(mesh, right)
        sc = ox.ScalarTransport("T", diffusivity=kappa, source=D.src, initial=D.ini,
                                flux_bcs=[ox.RobinBC(0.0, 1.5, fr, advective=1.0)] if with_bc else [])
        S, clock, mesh = _problem(dim, N, 2, [sc], nu=nu, dt=dt, mesh=mesh, solver_options=_options())
        clock["t"] = dt
        uab = _assemble(S, clock, [sc], dt, nu)
        g = S._scalar_groups[0]
        out.append((g.Ac.to_scipy().tocsr(), g.B.rhost()[:, 0].copy()))
    F, x_v = _forms(S, mesh)
    m = BM.ScalarBCModel(F, x_v, kappa, source=D.src, conditions=[BM.Robin(*_model_facets(S, mesh, fr), 0.0, 1.5, beta=1.0)])
    m.interpolate(D.ini)
    _compare(g, 0, *m.assemble(uab, dt), f"open boundary ({dim},{N})")
    (A0, b0), (A1, b1) = out
    on_side = np.isclose(x_v[:, 0], 1.0)
    outflow = np.nonzero(on_side & (x_v[:, 1] > 1e-9))[0]
    inflow = np.nonzero(on_side & (x_v[:, 1] < -1e-9))[0]
    assert outflow.size and inflow.size
    assert (A1[outflow] != A0[outflow]).nnz == 0 and np.array_equal(b1[outflow], b0[outflow])
    assert abs(m.H[outflow]).max() == 0.0 and np.abs(m.load[outflow]).max() == 0.0  # the model agrees: nothing on outflow
    assert all(abs(A1[r] - A0[r]).max() > 0.0 for r in inflow) and np.all(b1[inflow] != b0[inflow])
    rest = np.nonzero(~on_side)[0]
    assert (A1[rest] != A0[rest]).nnz == 0 and np.array_equal(b1[rest], b0[rest])


# ---- 7. no behaviour change ----------------------------------------------------------------------------------------------
def test_empty_flux_bcs_is_the_scalar_of_before(hip, monkeypatch):
    """flux_bcs=[] makes none of the new calls and gives u, p and c bit-equal to a solver built without the keyword."""
    import torch

    import oasisx_amd as ox
    from oasisx_amd import scalar as sc_mod
    from tests.test_gpu_scalar import _options, _problem, _step, left

    def boom(*a, **k):
        raise AssertionError("the boundary pass was built for a scalar without conditions")

    monkeypatch.setattr(sc_mod, "BoundaryPass", boom)
    nu, dt = 0.01, 0.005
    out = []
    for kw in ({}, {"flux_bcs": []}):
        scalars = [ox.ScalarTransport("a", schmidt=2.0, initial=lambda x: x[0], source=0.3,
                                      bcs=[ox.DirichletBC(1.0, ox.LocatorMethod.GEOMETRICAL, left)], **kw),
                   ox.ScalarTransport("b", diffusivity=0.05, initial=1.0, **kw)]
        S, clock, _ = _problem(3, 4, 2, scalars, nu=nu, dt=dt, solver_options=_options(guess=True))
        for _ in range(3):
            _step(S, clock, dt, nu)
        assert all(g.boundary is None for g in S._scalar_groups)
        out.append([S._U.rdev().clone(), S._P.rdev().clone()] + [g.C.rdev().clone() for g in S._scalar_groups])
    assert len(out[0]) == len(out[1]) == 4 and all(torch.equal(x, y) for x, y in zip(*out))


# ---- 8. compositions -----------------------------------------------------------------------------------------------------
def test_with_a_turbulent_schmidt_number(hip):
    """Under Smagorinsky with Sc_t = 0.7: the conditions do not depend on the diffusivity; three steps against the LES
    model with the same surface terms."""
    import oasisx_amd as ox
    from tests import scalar_bc_model as BM
    from tests.scalar_les_model import ScalarLesModel
    from tests.test_gpu_scalar import _dofs, _options
    from tests.test_gpu_scalar_les import _problem
    from tests.test_gpu_viscosity import _forms, _model_of

    nu, dt, kappa, sct = 0.01, 0.005, 0.03, 0.7
    D = Data()
    D.src = lambda x: 0.5 + x[0]
    D.ini = lambda x: np.cos(np.pi * x[0]) * np.cos(np.pi * x[1])
    mo = ox.Smagorinsky()
    mesh = _mesh(2, 8)
    dev, mod = _conditions(mesh, D)
    sc = ox.ScalarTransport("T", diffusivity=kappa, source=D.src, initial=D.ini, turbulent_schmidt=sct, flux_bcs=dev,
                            bcs=[ox.DirichletBC(D.val, ox.LocatorMethod.GEOMETRICAL, top)])
    S, clock, mesh = _problem(2, 8, 2, mo, [sc], nu, dt, guess=True, perturb=0.05, mesh=mesh)
    F, x_v, _ = _forms(S, mesh)
    m = BM.with_conditions(ScalarLesModel)(F, x_v, kappa, sct, model=_model_of(S, mo), dofs=_dofs(x_v, top), value=D.val,
                                           source=D.src, options=_options(guess=True)["scalar_transport"], conditions=mod(S))
    m.interpolate(D.ini)
    _steps(S, clock, D, m, dt, nu, nut=True)
    assert m.nut.max() > 0.0


def test_on_a_periodic_channel(hip):
    """The make_periodic channel (identified in x): a FluxBC on the lower wall and a RobinBC on the upper one, whose
    facets at the seam hold identified dofs; three steps against the model on the reduced space."""
    import oasisx_amd as ox
    from tests import scalar_bc_model as BM
    from tests.test_gpu_periodic import _channel_mesh, _forms, _set_fields, _solver, _walls
    from tests.test_gpu_scalar import _options

    nu, dt, kappa = 0.01, 0.005, 0.03
    D = Data()
    D.src = lambda x: 0.5 + x[1]
    D.ini = lambda x: np.cos(np.pi * x[1]) + 0.3 * np.sin(2.0 * np.pi * x[0] / 3.0)
    D.q = lambda x: 0.5 + 0.3 * np.cos(2.0 * np.pi * x[0] / 3.0)
    D.h = lambda x: 1.0 + 0.5 * np.sin(2.0 * np.pi * x[0] / 3.0) ** 2
    D.c_inf = lambda x: 0.3 + 0.2 * np.cos(2.0 * np.pi * x[0] / 3.0) + 2.0 * D.clock["t"]
    mesh = _channel_mesh(2)
    fb, ft = _facets(mesh, bottom), _facets(mesh, top)
    assert fb.size == 3 and ft.size == 3
    sc = ox.ScalarTransport("T", diffusivity=kappa, source=D.src, initial=D.ini,
                            flux_bcs=[ox.FluxBC(D.q, fb), ox.RobinBC(D.h, D.c_inf, ft, advective=0.7)])
    so = _options()
    S = _solver(mesh, 2, bcs_u=[[ox.DirichletBC(0.0, ox.LocatorMethod.GEOMETRICAL, _walls)] for _ in range(2)],
                solver_options=so, scalars=[sc])
    _set_fields(S, None, [lambda x: 1.0 - x[1] ** 2, lambda x: 0.0 * x[0]], lambda x: 0.0 * x[0])
    F, x_v, _ = _forms(S)
    m = BM.ScalarBCModel(F, x_v, kappa, source=D.src, options=so["scalar_transport"],
                         conditions=[BM.Flux(*_model_facets(S, mesh, fb), D.q),
                                     BM.Robin(*_model_facets(S, mesh, ft), D.h, D.c_inf, beta=0.7)])
    m.interpolate(D.ini)
    _steps(S, {"t": 0.0}, D, m, dt, nu)
    with pytest.raises(ValueError, match="identified"):
        _solver(mesh, 2, scalars=[ox.ScalarTransport("T", diffusivity=kappa, flux_bcs=[ox.FluxBC(1.0, mesh.periodic_facets()[:2])])])


def test_with_buoyancy(hip):
    """A scalar that drives the flow and exchanges heat through its boundary: three steps against the model fed the
    device's u_ab."""
    import oasisx_amd as ox
    from tests import scalar_bc_model as BM
    from tests.test_gpu_scalar import _dofs, _forms, _options, _problem

    nu, dt, kappa = 0.01, 0.005, 0.03
    D = Data()
    D.src = lambda x: 0.5 + x[0]
    D.ini = lambda x: np.cos(np.pi * x[0]) * np.cos(np.pi * x[1])
    mesh = _mesh(2, 8)
    dev, mod = _conditions(mesh, D)
    sc = ox.ScalarTransport("T", diffusivity=kappa, source=D.src, initial=D.ini, flux_bcs=dev, buoyancy=(0.0, 2.0), reference=0.1,
                            bcs=[ox.DirichletBC(D.val, ox.LocatorMethod.GEOMETRICAL, top)])
    so = _options()
    S, clock, mesh = _problem(2, 8, 2, [sc], nu=nu, dt=dt, mesh=mesh, solver_options=so)
    assert S._buoyancy
    F, x_v = _forms(S, mesh)
    m = BM.ScalarBCModel(F, x_v, kappa, dofs=_dofs(x_v, top), value=D.val, source=D.src, options=so["scalar_transport"],
                         conditions=mod(S))
    m.interpolate(D.ini)
    _steps(S, clock, D, m, dt, nu)


# ---- loud limits -----------------------------------------------------------------------------------------------------------
def test_construction_errors_at_the_solver(hip):
    import oasisx_amd as ox
    from tests.test_gpu_scalar import _problem

    mesh = _mesh(2, 4)
    fr = _facets(mesh, right)
    T = lambda fb: [ox.ScalarTransport("T", diffusivity=0.1, flux_bcs=fb)]  # noqa: E731
    with pytest.raises(ValueError, match=">= 0"):  # a callable h: checked where it is evaluated
        _problem(2, 4, 2, T([ox.RobinBC(lambda x: x[1], 0.0, fr)]), mesh=mesh)
    with pytest.raises(ValueError, match="not finite"):
        _problem(2, 4, 2, T([ox.FluxBC(lambda x: np.full_like(x[0], np.nan), fr)]), mesh=mesh)
    interior = np.setdiff1d(np.arange(mesh._entities(1)[0].shape[0]), mesh.exterior_facets())[:1]
    with pytest.raises(ValueError, match="interior"):
        _problem(2, 4, 2, T([ox.FluxBC(1.0, interior)]), mesh=mesh)
    clock_c = {"t": 0.0}
    bc = ox.RobinBC(1.0, lambda x: np.full_like(x[0], np.inf if clock_c["t"] >= 1.0 else 1.0), fr)
    S, _, _ = _problem(2, 4, 2, T([bc]), mesh=mesh)
    clock_c["t"] = 1.0
    with pytest.raises(ValueError, match="not finite"):  # update() re-evaluates
        bc.update()


# ---- 9. the demo -----------------------------------------------------------------------------------------------------------
def test_demo_prints_a_converging_error_table(hip, capsys):
    """demo/robin_slab_hip.py: the error against the series solution falls at an order above 2 from N = 4 to N = 8 (P2),
    and the wall flux of ScalarFlux agrees with h (c_wall - c_inf)."""
    from demo.robin_slab_hip import main

    rows = main(["-N", "4", "-N", "8"])
    out = capsys.readouterr().out
    assert "L2 error c" in out and "h (c_wall - c_inf)" in out
    (n0, e0, _, _), (n1, e1, flux, film) = rows
    assert (n0, n1) == (4, 8)
    assert np.log2(e0 / e1) > 2.0, (e0, e1)
    # the P2 facet gradient is of second order in the mesh width: at N = 8 within a few per cent of the film law
    assert flux > 0.0 and film > 0.0 and abs(flux - film) < 0.05 * abs(film), (flux, film)
