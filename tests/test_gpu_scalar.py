"""GPU: passive scalar transport in FractionalStep_AB_CN (oasisx_amd/scalar.py, csrc/ox_scalar.hip) against the numpy
model of tests/scalar_model.py, which is built on the oracle's forms and Krylov solver and pinned by
tests/test_scalar_host.py.  The model is fed the device's own numbering (fields compare index by index) and, per step,
the extrapolated velocity u_ab the device used: these tests are about the scalar step, the velocity has its own parity
tests."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BCGS = {"ksp_type": "bcgs", "pc_type": "jacobi", "ksp_rtol": 1e-11, "ksp_atol": 1e-30}
TIGHT = {"ksp_type": "bcgs", "pc_type": "jacobi", "ksp_rtol": 1e-12, "ksp_atol": 1e-30}


def left(x):
    return np.isclose(x[0], -1.0)


def bottom(x):
    return np.isclose(x[1], -1.0)


def _options(scalar=None, guess=False):
    from tests.helpers import KRYLOV

    o = {k: dict(v) for k, v in KRYLOV.items()}
    o["scalar_transport"] = dict(scalar or BCGS)
    if guess:
        o = {k: dict(v, ksp_initial_guess_nonzero=True) for k, v in o.items()}
    return o


def _problem(dim, N, deg, scalars, nu=0.01, dt=0.005, solver_options=None, options=None, mesh=None, low_memory=True):
    """The Taylor-Green set-up of tests.helpers.make_hip_problem with ``scalars=`` (and P3-P2, and a mesh handed in)."""
    import oasisx_amd as ox
    from oracle import ipcs_oracle as O
    from tests.helpers import on_boundary, on_boundary3, tg_mesh

    mesh = tg_mesh(dim, N) if mesh is None else mesh
    clock = {"t": 0.0}
    marker = on_boundary if dim == 2 else on_boundary3
    fns = [O.tg_u, O.tg_v, O.tg_w][:dim]
    bcs_u = [[ox.DirichletBC(lambda x, f=f: f(x, clock["t"], nu), ox.LocatorMethod.GEOMETRICAL, marker)] for f in fns]
    opts = {"sell_window": 256, "low_memory_version": low_memory}
    opts.update(options or {})
    kw = {} if scalars is None else {"scalars": scalars}
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", deg), ("Lagrange", 2 if deg == 3 else 1), bcs_u=bcs_u, bcs_p=[],
                                solver_options=solver_options or _options(), options=opts, **kw)
    for i, f in enumerate(fns):
        S._u2[i].interpolate(lambda x, f=f: f(x, -dt, nu))
        S._u1[i].interpolate(lambda x, f=f: f(x, 0.0, nu))
    S._p.interpolate(lambda x: O.tg_p(x, -dt / 2.0, nu))
    return S, clock, mesh


def _forms(S, mesh):
    """The oracle's forms on the device's mesh arrays and dof numbering."""
    from oracle import ipcs_oracle as O

    Vi, Q = S._Vi[0][0], S._Q
    F = O.Forms(mesh.coords.cpu().numpy(), Vi.cells_in_kernel_order(), Vi.degree, Q.degree, vd=Vi.cell_dofs.cpu().numpy(),
                qd=Q.cell_dofs.cpu().numpy(), nv_dofs=Vi.num_dofs, nq_dofs=Q.num_dofs)
    return F, Vi.x.cpu().numpy()


def _dofs(x_v, marker):
    X = np.zeros((3, x_v.shape[0]))
    X[: x_v.shape[1]] = x_v.T
    return np.nonzero(marker(X))[0]


def _c(S, name, level=0):
    f = S.scalar(name, level)
    return f._storage.rhost()[:, f._comp].copy()


def _step(S, clock, dt, nu):
    clock["t"] += dt
    S.solve(dt, nu, max_iter=1)


# ---- 4. operator and right-hand side, entry by entry -------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dictionary", "f64", "delaunay"])
@pytest.mark.parametrize("dim,N,deg", [(2, 6, 1), (2, 5, 2), (3, 3, 1), (3, 3, 2), (2, 4, 3)])
def test_operator_and_rhs_entry_by_entry(hip, dim, N, deg, mode):
    """After assemble_first: A_c (identity rows on the scalar's OWN Dirichlet dofs) and b_c equal the model's to
    1e-12 max|.| -- the bound tests/test_gpu_parity.py puts on A and b_first -- with kappa != nu, a nonzero source and
    Dirichlet rows on part of the boundary; with value dictionaries, with f64 values and on a Delaunay mesh.  The product
    A_c c_1 handed to the solver equals the mat-vec bit for bit."""
    import torch

    import oasisx_amd as ox
    from oasisx_amd import mesh as M
    from tests.scalar_model import ScalarModel

    dt, nu, kappa = 0.1, 0.5, 0.2
    clock_c = {"t": 0.0}
    src = lambda x: 1.0 + x[0] * x[1]  # noqa: E731
    val = lambda x: 1.0 + x[1] + clock_c["t"]  # noqa: E731
    ini = lambda x: np.cos(2.0 * x[0]) + 0.5 * x[1]  # noqa: E731
    sc = ox.ScalarTransport("T", diffusivity=kappa, source=src, initial=ini,
                            bcs=[ox.DirichletBC(val, ox.LocatorMethod.GEOMETRICAL, left)])
    mesh = None
    if mode == "delaunay":
        mesh = M.create_delaunay_box(None, [[-1.0] * dim, [1.0] * dim], 6 if dim == 2 else 4, seed=2)
    S, clock, mesh = _problem(dim, N, deg, [sc], nu=nu, dt=dt, mesh=mesh, solver_options=_options(guess=True),
                              options={"value_dictionary": mode != "f64"})
    if mode == "dictionary" and dim == 2 and deg <= 2:  # (elsewhere K may exceed 256 distinct values: then f64 is read)
        assert S._M.vcode is not None and S._K.vcode is not None  # the LDS-dictionary instantiation runs
    elif mode == "f64":
        assert S._M.vcode is None and S._K.vcode is None
    elif mode == "delaunay":
        assert not S._lattice
    F, x_v = _forms(S, mesh)
    m = ScalarModel(F, x_v, kappa, dofs=_dofs(x_v, left), value=val, source=src)
    m.interpolate(ini)
    assert np.abs(_c(S, "T", 1) - m.c1).max() <= 1e-14
    clock["t"] = clock_c["t"] = dt
    for bcl in S._bcs_u:
        for bc in bcl:
            bc.update_bc()
    for bc in sc.bcs:
        bc.update_bc()
    S.assemble_first(dt, nu)
    uab = 1.5 * S._U1.rhost() - 0.5 * S._U2.rhost()
    A_ref, b_ref = m.assemble(uab, dt)
    g = S._scalar_groups[0]
    dA = abs(g.Ac.to_scipy() - A_ref).max()
    db = np.abs(g.B.rhost()[:, 0] - b_ref).max()
    print(f"dA = {dA:.3e} (max|A| = {abs(A_ref).max():.3e}), db = {db:.3e} (max|b| = {np.abs(b_ref).max():.3e})")
    assert dA <= 1e-12 * abs(A_ref).max(), dA
    assert db <= 1e-12 * np.abs(b_ref).max(), db
    y = torch.zeros_like(g.C1.rdev())
    g.Ac.mult(g.C1.rdev(), y, 1)
    assert torch.equal(y[: S._no_u], g.AC1.rdev()[: S._no_u])
    with pytest.raises(RuntimeError, match="inside assemble_first"):
        S.scalar_assemble(dt, nu)


# ---- 5. no behaviour change ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("low_memory", [True, False])
def test_velocity_and_pressure_bit_identical_with_and_without_scalars(hip, low_memory):
    import torch

    import oasisx_amd as ox

    nu, dt = 0.01, 0.005
    out = []
    for with_scalars in (False, True):
        scalars = None
        if with_scalars:
            scalars = [ox.ScalarTransport("a", schmidt=2.0, initial=lambda x: x[0], source=0.3,
                                          bcs=[ox.DirichletBC(1.0, ox.LocatorMethod.GEOMETRICAL, left)]),
                       ox.ScalarTransport("b", diffusivity=0.05, initial=1.0)]
        S, clock, _ = _problem(3, 4, 2, scalars, nu=nu, dt=dt, solver_options=_options(guess=True), low_memory=low_memory)
        its, tokens = [], []
        for _ in range(3):
            _step(S, clock, dt, nu)
            ic = S.iteration_counts()
            its.append((tuple(ic["tentative"]), tuple(ic["pressure"]), tuple(ic["update"])))
            tokens.append(S._u_is_u1 == (S._U.generation, S._U1.generation))
        assert tokens == [True] * 3  # the A u1 shortcut of the next tentative solve is alive
        assert ("scalar_transport" in S.iteration_counts()) == with_scalars
        out.append((S._U.rdev().clone(), S._P.rdev().clone(), S._A.vals.clone(), its))
    (u0, p0, a0, i0), (u1, p1, a1, i1) = out
    assert torch.equal(u0, u1) and torch.equal(p0, p1) and torch.equal(a0, a1)
    assert i0 == i1, (i0, i1)


def test_empty_scalar_list_is_the_plain_solver(hip):
    S, clock, _ = _problem(2, 6, 2, [])
    assert S._scalar_groups == [] and "scalar_transport" not in S.iteration_counts()
    _step(S, clock, 0.005, 0.01)
    with pytest.raises(KeyError):
        S.scalar("T")


# ---- 6. steps against the model --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N", [(2, 8), (3, 4)])
@pytest.mark.parametrize("guess", [False, True])
def test_steps_match_the_model(hip, dim, N, guess):
    """3 steps, P2: relative max difference in c below 1e-8 (the bound test_full_steps_match_oracle_krylov puts on u),
    iteration counts within +-1 of the model's jacobi_bicgstab at the same tolerances."""
    import oasisx_amd as ox
    from tests.scalar_model import ScalarModel

    nu, dt, kappa = 0.01, 0.005, 0.03
    clock_c = {"t": 0.0}
    src = lambda x: 0.5 + x[0]  # noqa: E731
    val = lambda x: 1.0 + x[1] * (1.0 + clock_c["t"])  # noqa: E731
    ini = lambda x: np.cos(np.pi * x[0]) * np.cos(np.pi * x[1])  # noqa: E731
    sc = ox.ScalarTransport("T", diffusivity=kappa, source=src, initial=ini,
                            bcs=[ox.DirichletBC(val, ox.LocatorMethod.GEOMETRICAL, left)])
    so = _options(guess=guess)
    S, clock, mesh = _problem(dim, N, 2, [sc], nu=nu, dt=dt, solver_options=so)
    F, x_v = _forms(S, mesh)
    m = ScalarModel(F, x_v, kappa, dofs=_dofs(x_v, left), value=val, source=src, options=so["scalar_transport"])
    m.interpolate(ini)
    for k in range(3):
        clock_c["t"] = (k + 1) * dt
        _step(S, clock, dt, nu)
        m.step(S._UAB.rhost(), dt)
        c = _c(S, "T")
        rel = np.abs(c - m.c).max() / np.abs(m.c).max()
        its = S.iteration_counts()["scalar_transport"]["T"]
        print(f"step {k}: rel diff {rel:.3e}, iterations {its} (model {m.its})")
        assert m.reason > 0
        assert rel < 1e-8, (k, rel)
        assert abs(its - m.its) <= 1, (k, its, m.its)
        assert np.array_equal(c, _c(S, "T", 1))  # c_1 <- c


# ---- 7. several scalars, groups ----------------------------------------------------------------------------------------
def test_groups_and_independence(hip):
    """Two scalars with different Schmidt numbers and Dirichlet sets plus two with equal kappa and equal sets (one
    group, lock-step, different boundary values and sources): each equals its own single-scalar run to 1e-10."""
    import oasisx_amd as ox
    from oasisx_amd.la import SellMatrix

    nu, dt = 0.01, 0.005

    def make():
        G = ox.LocatorMethod.GEOMETRICAL
        ini = lambda x: np.cos(np.pi * x[0]) * np.cos(np.pi * x[1])  # noqa: E731
        return [ox.ScalarTransport("a", schmidt=1.0, initial=ini, bcs=[ox.DirichletBC(1.0, G, left)]),
                ox.ScalarTransport("b", schmidt=4.0, initial=ini, source=lambda x: x[1], bcs=[ox.DirichletBC(0.5, G, bottom)]),
                ox.ScalarTransport("c", diffusivity=0.03, initial=ini, bcs=[ox.DirichletBC(1.0, G, left)]),
                ox.ScalarTransport("d", diffusivity=0.03, initial=0.2, source=1.0, bcs=[ox.DirichletBC(2.0, G, left)])]

    def run(scalars):
        S, clock, _ = _problem(2, 8, 2, scalars, nu=nu, dt=dt, solver_options=_options(TIGHT))
        for _ in range(3):
            _step(S, clock, dt, nu)
        return S

    S = run(make())
    groups = S._scalar_groups
    assert len(groups) == 3 and sorted(g.nc for g in groups) == [1, 1, 2]
    assert S._scalar_index["c"][0] is S._scalar_index["d"][0]
    mats = {id(g.Ac) for g in groups}
    assert len(mats) == 3 and all(isinstance(g.Ac, SellMatrix) for g in groups)
    its = S.iteration_counts()["scalar_transport"]
    assert sorted(its) == ["a", "b", "c", "d"] and all(v > 0 for v in its.values())
    for i, name in enumerate("abcd"):
        S1 = run([make()[i]])
        ref = _c(S1, name)
        rel = np.abs(_c(S, name) - ref).max() / np.abs(ref).max()
        print(f"scalar {name}: rel diff to its single run {rel:.3e}")
        assert rel <= 1e-10, (name, rel)


def test_more_than_three_equal_scalars_open_a_second_group(hip):
    import oasisx_amd as ox

    S, clock, _ = _problem(2, 6, 2, [ox.ScalarTransport(f"s{i}", diffusivity=0.1, initial=float(i)) for i in range(4)])
    assert sorted(g.nc for g in S._scalar_groups) == [1, 3]
    _step(S, clock, 0.005, 0.01)
    for i in range(4):  # constants are preserved, column by column
        assert np.abs(_c(S, f"s{i}") - float(i)).max() < 1e-8


# ---- 8. constant preservation and the exact solution -------------------------------------------------------------------
@pytest.mark.parametrize("dim,N", [(2, 8), (3, 4)])
def test_constant_is_preserved(hip, dim, N):
    """c_1 = 1, no Dirichlet rows, no source: C 1 = K 1 = 0, the step returns 1 to solver tolerance (rtol 1e-12)."""
    import oasisx_amd as ox

    S, clock, _ = _problem(dim, N, 2, [ox.ScalarTransport("one", diffusivity=0.3, initial=1.0)],
                           solver_options=_options(TIGHT))
    for _ in range(3):
        _step(S, clock, 0.005, 0.01)
    d = np.abs(_c(S, "one") - 1.0).max()
    print("max |c - 1| =", d)
    assert d < 1e-9


def test_exact_solution_on_the_device(hip):
    """cos(pi x) cos(pi y) exp(-2 kappa pi^2 t) in the Taylor-Green flow, exact Dirichlet data, P2, N = 4, 8, 16: the
    device's L2 error at t = 0.05 is within 5 % of the model's at each N (both discretise identically; the margin is
    for the solver tolerance) and falls at an order above 2."""
    import oasisx_amd as ox
    from tests.helpers import on_boundary
    from tests.scalar_model import ScalarModel, exact_c

    nu, dt, kappa, steps = 0.01, 0.005, 0.05, 10
    errs = []
    for N in (4, 8, 16):
        clock_c = {"t": 0.0}
        val = lambda x: exact_c(x, clock_c["t"], kappa)  # noqa: E731
        sc = ox.ScalarTransport("c", diffusivity=kappa, initial=lambda x: exact_c(x, 0.0, kappa),
                                bcs=[ox.DirichletBC(val, ox.LocatorMethod.GEOMETRICAL, on_boundary)])
        S, clock, mesh = _problem(2, N, 2, [sc], nu=nu, dt=dt, solver_options=_options(TIGHT))
        F, x_v = _forms(S, mesh)
        m = ScalarModel(F, x_v, kappa, dofs=_dofs(x_v, on_boundary), value=val, options=TIGHT)
        m.interpolate(lambda x: exact_c(x, 0.0, kappa))
        for k in range(steps):
            clock_c["t"] = (k + 1) * dt
            _step(S, clock, dt, nu)
            m.step(S._UAB.rhost(), dt)
        ex = lambda x: exact_c(x, clock_c["t"], kappa)  # noqa: E731
        e_dev = float(np.sqrt(F.l2_error_sq(_c(S, "c"), ex)))
        e_mod = float(np.sqrt(F.l2_error_sq(m.c, ex)))
        print(f"N = {N}: L2 error device {e_dev:.6e}, model {e_mod:.6e}")
        assert abs(e_dev - e_mod) <= 0.05 * e_mod, (N, e_dev, e_mod)
        errs.append(e_dev)
    orders = [float(np.log2(errs[i] / errs[i + 1])) for i in range(2)]
    print("observed orders:", orders)
    assert all(o > 2.0 for o in orders), (errs, orders)


# ---- 9. reproducibility, the handed-in first mat-vec -------------------------------------------------------------------
def test_two_runs_are_bit_identical_and_ax0_changes_nothing(hip):
    import oasisx_amd as ox

    nu, dt = 0.01, 0.005

    def run(ax0=True):
        G = ox.LocatorMethod.GEOMETRICAL
        ini = lambda x: np.cos(np.pi * x[0]) * np.cos(np.pi * x[1])  # noqa: E731
        scalars = [ox.ScalarTransport("a", diffusivity=0.03, initial=ini, source=0.2, bcs=[ox.DirichletBC(1.0, G, left)]),
                   ox.ScalarTransport("b", diffusivity=0.03, initial=0.5, bcs=[ox.DirichletBC(2.0, G, left)])]
        S, clock, _ = _problem(3, 4, 2, scalars, nu=nu, dt=dt, solver_options=_options(TIGHT, guess=True))
        if not ax0:
            for g in S._scalar_groups:
                g.wants_ax0 = lambda: False  # the solver multiplies A_c c_1 itself
        its = []
        for _ in range(3):
            _step(S, clock, dt, nu)
            ic = S.iteration_counts()["scalar_transport"]
            its.append((ic["a"], ic["b"]))
        return np.stack([_c(S, "a"), _c(S, "b")], axis=1), its

    c0, its0 = run()
    c1, its1 = run()
    assert np.array_equal(c0, c1) and its0 == its1
    c2, its2 = run(ax0=False)
    rel = np.abs(c2 - c0).max() / np.abs(c0).max()
    print("ax0 on/off: rel diff", rel, "iterations", its0, its2)
    assert rel <= 1e-10
    assert all(abs(a - b) <= 1 for s0, s2 in zip(its0, its2) for a, b in zip(s0, s2))


# ---- 10. time-dependent boundary values, point evaluation ----------------------------------------------------------------
def test_time_dependent_dirichlet_value_eval_and_probes(hip):
    import oasisx_amd as ox

    nu, dt = 0.01, 0.005
    clock_c = {"t": 0.0}
    sc = ox.ScalarTransport("T", diffusivity=0.02, initial=1.0,
                            bcs=[ox.DirichletBC(lambda x: 1.0 + 10.0 * clock_c["t"] + 0.0 * x[0], ox.LocatorMethod.GEOMETRICAL,
                                                left)])
    S, clock, mesh = _problem(2, 8, 2, [sc], nu=nu, dt=dt, solver_options=_options(TIGHT))
    x_v = S._Vi[0][0].x.cpu().numpy()
    rows = _dofs(x_v, left)
    for k in range(3):
        clock_c["t"] = (k + 1) * dt
        _step(S, clock, dt, nu)
        assert np.abs(_c(S, "T")[rows] - (1.0 + 10.0 * clock_c["t"])).max() < 1e-9
    pts = np.zeros((40, 3))
    pts[:, :2] = x_v[::7][:40]
    nodal = _c(S, "T")[::7][:40]
    assert np.abs(S.scalar("T").eval(pts)[:, 0] - nodal).max() < 1e-12
    probes = ox.Probes(pts, [S.scalar("T")], capacity=2)
    probes.sample(clock["t"])
    assert np.abs(probes.array()[0, :, 0] - nodal).max() < 1e-12


# ---- 11. loud limits -----------------------------------------------------------------------------------------------------
def test_construction_errors(hip):
    import oasisx_amd as ox
    from oasisx_amd import fem
    from oasisx_amd.parallel import Comm
    from tests.helpers import tg_mesh

    T = lambda name="T", **k: ox.ScalarTransport(name, diffusivity=0.1, **k)  # noqa: E731
    with pytest.raises(ValueError, match="duplicate"):
        _problem(2, 4, 2, [T(), T()])
    with pytest.raises(TypeError):
        _problem(2, 4, 2, ["T"])
    mesh = tg_mesh(2, 4)
    other = fem.Function(fem.FunctionSpace(mesh, 2, window=256))
    with pytest.raises(ValueError, match="velocity component space"):
        _problem(2, 4, 2, [T(source=other)], mesh=mesh)
    with pytest.raises(ValueError, match="velocity component space"):
        _problem(2, 4, 2, [T(initial=other)], mesh=mesh)
    pmesh = tg_mesh(2, 4)
    pmesh.comm = Comm(0, 2, None, transport="host")
    with pytest.raises(NotImplementedError, match="partition"):
        _problem(2, 4, 2, [T()], mesh=pmesh)


def test_function_source_and_initial_on_the_component_space(hip):
    """A Function source is M f, a Function initial value is copied: the space is handed in as ``u_element``."""
    import oasisx_amd as ox
    from oasisx_amd import fem
    from tests.helpers import KRYLOV, on_boundary, tg_mesh

    mesh = tg_mesh(2, 5)
    Vi = fem.FunctionSpace(mesh, 2, window=256)
    f = fem.Function(Vi)
    f.interpolate(lambda x: 1.0 + x[0] * x[1])
    S = ox.FractionalStep_AB_CN(mesh, Vi, ("Lagrange", 1), bcs_p=[], solver_options=KRYLOV,
                                bcs_u=[[ox.DirichletBC(0.0, ox.LocatorMethod.GEOMETRICAL, on_boundary)] for _ in range(2)],
                                scalars=[ox.ScalarTransport("T", schmidt=2.0, source=f, initial=f)])
    F, x_v = _forms(S, mesh)
    g = S._scalar_groups[0]
    ref = F.mass_v() @ f.x.array
    assert np.abs(g.B0.rhost()[:, 0] - ref).max() <= 1e-13 * np.abs(ref).max()
    assert np.array_equal(_c(S, "T", 1), f.x.array) and np.array_equal(_c(S, "T"), f.x.array)


def test_demo_prints_a_converging_error_table(hip, capsys):
    """demo/scalar_transport_hip.py: the scalar's L2 error falls at an order above 2 from N = 4 to N = 8 (P2)."""
    from demo.scalar_transport_hip import main

    rows = main(["-N", "4", "-N", "8"])
    assert "L2 error c" in capsys.readouterr().out
    (n0, e0, _, _), (n1, e1, _, its) = rows
    assert (n0, n1) == (4, 8) and its > 0
    assert np.log2(e0 / e1) > 2.0, (e0, e1)
