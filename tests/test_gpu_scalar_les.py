"""GPU: scalars under a viscosity model -- ``ScalarTransport(turbulent_schmidt=...)`` beside ``viscosity_model=``
(oasisx_amd/scalar.py, ``ox_scalar_rows_cellvisc`` of csrc/ox_assemble.hip, ``ox_scalar_flux_cells`` of csrc/ox_scalar.hip,
DESIGN.md section 25) against the numpy model of tests/scalar_les_model.py, which tests/test_scalar_les_host.py pins.  The
model is fed the device's numbering and the device's own velocity blocks."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [(2, 6, 1), (2, 5, 2), (3, 3, 1), (3, 3, 2), (2, 4, 3), (3, 2, 3)]
INF = float("inf")
SRC = lambda x: 1.0 + x[0] * x[1]  # noqa: E731
INI = lambda x: np.cos(2.0 * x[0]) + 0.5 * x[1]  # noqa: E731


def _val(clock_c):
    return lambda x: 1.0 + x[1] + clock_c["t"]


def _scalar(clock_c, kappa, sct, name="T", dirichlet=True, **kw):
    import oasisx_amd as ox
    from tests.test_gpu_scalar import left

    bcs = [ox.DirichletBC(_val(clock_c), ox.LocatorMethod.GEOMETRICAL, left)] if dirichlet else []
    kw.setdefault("source", SRC)
    kw.setdefault("initial", INI)
    return ox.ScalarTransport(name, diffusivity=kappa, bcs=bcs, turbulent_schmidt=sct, **kw)


def _problem(dim, N, deg, model, scalars, nu, dt, guess=True, **kw):
    """tests/test_gpu_viscosity._problem (perturbed Taylor-Green levels) with ``scalars=`` and the scalar's Krylov options."""
    from tests.test_gpu_scalar import _options
    from tests.test_gpu_viscosity import _problem as vp

    so = kw.pop("solver_options", None) or _options(guess=guess)
    if scalars is not None:
        kw["scalars"] = scalars
    kw.setdefault("perturb", 0.3)
    return vp(dim, N, deg, model, nu=nu, dt=dt, solver_options=so, **kw)


def _assemble(S, clock, clock_c, dt, nu):
    from tests.test_gpu_buoyancy import _update_bcs

    clock["t"] = clock_c["t"] = dt
    _update_bcs(S)
    S.assemble_first(dt, nu)


def _les_model(S, mesh, model_obj, kappa, sct, clock_c, dirichlet=True, options=None, source=SRC, initial=INI):
    from tests.scalar_les_model import ScalarLesModel
    from tests.test_gpu_scalar import _dofs, left
    from tests.test_gpu_viscosity import _forms, _model_of

    F, x_v, _ = _forms(S, mesh)
    m = ScalarLesModel(F, x_v, kappa, sct, model=_model_of(S, model_obj), dofs=_dofs(x_v, left) if dirichlet else None,
                       value=_val(clock_c), source=source, options=options)
    m.interpolate(initial)
    return m


def _check_against(S, m, dt, what, share=True):
    """A_c, b_c of group 0 against the assembled model: 1e-12 max|.| (tests/test_gpu_scalar.py, test_gpu_parity.py); the
    turbulent term is not lost in the bound; the handed A_c c_1 equals the mat-vec bit for bit."""
    import torch

    g = S._scalar_groups[0]
    A_ref, b_ref = m.A, m.b
    dA = abs(g.Ac.to_scipy() - A_ref).max()
    db = np.abs(g.B.rhost()[:, 0] - b_ref).max()
    kw_share = abs(m.Kw).max() / (2.0 * m.sct) / abs(A_ref).max()
    print(f"{what}: dA = {dA:.3e} (max|A_c| = {abs(A_ref).max():.3e}, max|K_w/(2 Sc_t)| / max|A_c| = {kw_share:.2e}), "
          f"db = {db:.3e} (max|b_c| = {np.abs(b_ref).max():.3e})")
    if share:
        assert kw_share > 1e-4
    assert dA <= 1e-12 * abs(A_ref).max(), dA
    assert db <= 1e-12 * np.abs(b_ref).max(), db
    assert g.ax0_valid
    y = torch.zeros_like(g.C1.rdev())
    g.Ac.mult(g.C1.rdev(), y, 1)
    assert torch.equal(y[: S._no_u], g.AC1.rdev()[: S._no_u])


class Counting:
    """The library with a list of the calls of the two scalar row entries."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        if name in ("ox_scalar_rows", "ox_scalar_rows_cellvisc", "ox_scalar_flux", "ox_scalar_flux_cells"):
            self.calls.append(name)
        return getattr(self._lib, name)


def _counted(S, monkeypatch):
    from oasisx_amd import _lib

    proxy = Counting(_lib.load())
    monkeypatch.setattr(_lib, "_lib", proxy)
    monkeypatch.setattr(S, "_lib", proxy)
    return proxy


# ---- 1. A_c and b_c, entry by entry ------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_blocks", [False, True])
@pytest.mark.parametrize("mode", ["dictionary", "f64", "delaunay"])
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_operator_and_rhs_entry_by_entry(hip, dim, N, deg, mode, row_blocks):
    """After assemble_first with Smagorinsky on the perturbed field and with a non-constant CellViscosity, Sc_t = 0.7,
    kappa != nu, a source and Dirichlet rows on x = -1: A_c and b_c equal the model's to 1e-12 max|.|, A_c c_1 is the
    mat-vec's bits, and the velocity's A and b_first are the bits of the same solver without scalars."""
    import torch

    import oasisx_amd as ox
    from tests.test_gpu_viscosity import _delaunay, _sponge

    dt, nu, kappa, sct = 0.1, 0.5, 0.2, 0.7
    mesh = _delaunay(dim, N) if mode == "delaunay" else None
    opts = {"value_dictionary": mode != "f64", "assemble_row_blocks": row_blocks}
    for mo in (ox.Smagorinsky(), ox.CellViscosity(_sponge)):
        clock_c = {"t": 0.0}
        S, clock, mesh = _problem(dim, N, deg, mo, [_scalar(clock_c, kappa, sct)], nu, dt, mesh=mesh, options=opts)
        assert S._row_blocks == row_blocks and (not row_blocks or S._Vi[0][0].pattern.n_row_blocks > 0)
        if mode == "dictionary" and dim == 2 and deg <= 2:
            assert S._M.vcode is not None and S._K.vcode is not None  # the LDS-dictionary instantiation runs
        elif mode == "f64":
            assert S._M.vcode is None and S._K.vcode is None
        m = _les_model(S, mesh, mo, kappa, sct, clock_c)
        assert np.abs(S._scalar_groups[0].C1.rhost()[:, 0] - m.c1).max() <= 1e-14
        _assemble(S, clock, clock_c, dt, nu)
        m.assemble(S._UAB.rhost(), dt)
        _check_against(S, m, dt, repr(mo))
        P, pclock, _ = _problem(dim, N, deg, mo, None, nu, dt, mesh=mesh, options=opts)
        _assemble(P, pclock, {"t": 0.0}, dt, nu)
        assert torch.equal(S._A.vals, P._A.vals) and torch.equal(S._BFIRST.rdev(), P._BFIRST.rdev())


# ---- 2. pins that need no model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_blocks", [False, True])
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_zero_and_constant_cell_viscosity(hip, dim, N, deg, row_blocks):
    """CellViscosity(0.0) with Sc_t = 0.7: A_c.vals and b_c are the BITS of the run without a model.  CellViscosity(c) at
    nu, kappa, Sc_t: A_c and b_c of the run without a model at nu + c and diffusivity kappa + c / Sc_t, to 1e-12 max|.|."""
    import torch

    import oasisx_amd as ox

    dt, nu, kappa, sct, c = 0.1, 0.5, 0.2, 0.7, 0.37
    out = {}
    for key, model, nu_run, kap, s in (("plain", None, nu, kappa, None), ("zero", ox.CellViscosity(0.0), nu, kappa, sct),
                                       ("const", ox.CellViscosity(c), nu, kappa, sct),
                                       ("shifted", None, nu + c, kappa + c / sct, None)):
        clock_c = {"t": 0.0}
        S, clock, _ = _problem(dim, N, deg, model, [_scalar(clock_c, kap, s)], nu, dt, options={"assemble_row_blocks": row_blocks})
        _assemble(S, clock, clock_c, dt, nu_run)
        g = S._scalar_groups[0]
        out[key] = (g.Ac.vals.clone(), g.B.rdev().clone())
    assert torch.equal(out["zero"][0], out["plain"][0]) and torch.equal(out["zero"][1], out["plain"][1])
    for k in (0, 1):
        ref = out["shifted"][k]
        d = float((out["const"][k] - ref).abs().max())
        print(f"{'A_c' if k == 0 else 'b_c'}: max diff {d:.3e}, max|.| {float(ref.abs().max()):.3e}")
        assert d <= 1e-12 * float(ref.abs().max()), (k, d)
    assert not torch.equal(out["const"][0], out["plain"][0])


def test_unit_schmidt_number_runs_the_plain_pass(hip, monkeypatch):
    """Sc_t = 1: A_c = A + s K, no call of the new entry; the result agrees with the model.  Sc_t = 0.7: one call of the
    new entry per group and assemble_first, none of the plain one."""
    import oasisx_amd as ox

    dt, nu, kappa = 0.1, 0.5, 0.2
    for sct, want in ((1.0, ["ox_scalar_rows"]), (0.7, ["ox_scalar_rows_cellvisc"])):
        clock_c = {"t": 0.0}
        mo = ox.Smagorinsky()
        S, clock, mesh = _problem(2, 5, 2, mo, [_scalar(clock_c, kappa, sct)], nu, dt)
        m = _les_model(S, mesh, mo, kappa, sct, clock_c)
        proxy = _counted(S, monkeypatch)
        _assemble(S, clock, clock_c, dt, nu)
        monkeypatch.undo()
        assert proxy.calls == want, (sct, proxy.calls)
        m.assemble(S._UAB.rhost(), dt)
        _check_against(S, m, dt, f"Sc_t = {sct}")


def test_without_a_model_the_argument_changes_nothing(hip, monkeypatch):
    """No viscosity_model: turbulent_schmidt is accepted, the calls are today's and c, u, p are the bits of the run without
    the argument."""
    import torch

    dt, nu = 0.005, 0.01
    out = []
    for sct in (None, 0.7):
        clock_c = {"t": 0.0}
        S, clock, _ = _problem(2, 6, 2, None, [_scalar(clock_c, 0.03, sct)], nu, dt, perturb=0.0)
        proxy = _counted(S, monkeypatch)
        for k in range(2):
            clock["t"] = clock_c["t"] = (k + 1) * dt
            S.solve(dt, nu, max_iter=1)
        monkeypatch.undo()
        assert proxy.calls == ["ox_scalar_rows"] * 2
        out.append((S._scalar_groups[0].C.rdev().clone(), S._U.rdev().clone(), S._P.rdev().clone()))
        with pytest.raises(RuntimeError, match="viscosity_model"):
            S.scalar_diffusivity("T", nu)
    assert all(torch.equal(a, b) for a, b in zip(*out))


# ---- 3. laws -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N,deg", [(2, 5, 2), (3, 3, 2)])
def test_a_law_does_not_diffuse_the_scalar(hip, dim, N, deg):
    """CarreauYasuda with turbulent_schmidt = inf: A_c is ScalarModel's plain operator at kappa -- no trace of nut -- to
    1e-12 max|.|, while A differs from the plain A by more than 1e-6 max|A|."""
    import oasisx_amd as ox
    from tests.scalar_model import ScalarModel
    from tests.test_gpu_scalar import _dofs, left
    from tests.test_gpu_viscosity import _forms

    law = ox.CarreauYasuda(nu0=0.16, nu_inf=0.01, lam=3.313, n=0.3568)
    dt, nu, kappa = 0.1, law.base_viscosity, 0.2
    clock_c = {"t": 0.0}
    S, clock, mesh = _problem(dim, N, deg, law, [_scalar(clock_c, kappa, INF)], nu, dt)
    F, x_v, _ = _forms(S, mesh)
    m = ScalarModel(F, x_v, kappa, dofs=_dofs(x_v, left), value=_val(clock_c), source=SRC)
    m.interpolate(INI)
    _assemble(S, clock, clock_c, dt, nu)
    A_ref, b_ref = m.assemble(S._UAB.rhost(), dt)
    g = S._scalar_groups[0]
    dA, db = abs(g.Ac.to_scipy() - A_ref).max(), np.abs(g.B.rhost()[:, 0] - b_ref).max()
    P, pclock, _ = _problem(dim, N, deg, None, None, nu, dt, mesh=mesh)
    _assemble(P, pclock, {"t": 0.0}, dt, nu)
    dplain = abs(S._A.to_scipy() - P._A.to_scipy()).max()
    amax = abs(P._A.to_scipy()).max()
    print(f"dA_c = {dA:.3e} of {abs(A_ref).max():.3e}, db_c = {db:.3e} of {np.abs(b_ref).max():.3e}; |A - A_plain| = "
          f"{dplain:.3e} of {amax:.3e}")
    assert float(S._nut.max()) > 0.0
    assert dA <= 1e-12 * abs(A_ref).max() and db <= 1e-12 * np.abs(b_ref).max()
    assert dplain > 1e-6 * amax
    assert np.array_equal(S.scalar_diffusivity("T", nu).cpu().numpy(), np.full(int(mesh.num_cells), kappa))


# ---- 4. whole steps ----------------------------------------------------------------------------------------------------
def _run_steps(dim, N, guess, steps=3, check=True):
    import oasisx_amd as ox

    nu, dt, kappa, sct = 0.01, 0.005, 0.03, 0.7
    clock_c = {"t": 0.0}
    mo = ox.Smagorinsky()
    src = lambda x: 0.5 + x[0]  # noqa: E731
    ini = lambda x: np.cos(np.pi * x[0]) * np.cos(np.pi * x[1])  # noqa: E731
    sc = _scalar(clock_c, kappa, sct, source=src, initial=ini)
    S, clock, mesh = _problem(dim, N, 2, mo, [sc], nu, dt, guess=guess, perturb=0.05)
    m = None
    if check:
        from tests.test_gpu_scalar import _options

        m = _les_model(S, mesh, mo, kappa, sct, clock_c, options=_options(guess=guess)["scalar_transport"], source=src,
                       initial=ini)
    g = S._scalar_groups[0]
    for k in range(steps):
        clock["t"] = clock_c["t"] = (k + 1) * dt
        S.solve(dt, nu, max_iter=1)
        if not check:
            continue
        m.step(S._UAB.rhost(), dt, nut=S._nut.cpu().numpy())
        c = g.C.rhost()[:, 0]
        rel = np.abs(c - m.c).max() / np.abs(m.c).max()
        its = S.iteration_counts()["scalar_transport"]["T"]
        print(f"step {k}: rel diff {rel:.3e}, iterations {its} (model {m.its}), max nut {m.nut.max():.3e}")
        assert m.reason > 0 and m.nut.max() > 0.0
        assert rel < 1e-8, (k, rel)
        assert abs(its - m.its) <= 1, (k, its, m.its)
        assert np.array_equal(c, g.C1.rhost()[:, 0])  # c_1 <- c
    return S


@pytest.mark.parametrize("guess", [False, True])
@pytest.mark.parametrize("dim,N", [(2, 8), (3, 4)])
def test_steps_match_the_model(hip, dim, N, guess):
    """Three P2-P1 steps with Smagorinsky and Sc_t = 0.7 against the model stepped with the device's u_ab and nut:
    relative max difference in c below 1e-8, iterations within +-1, c_1 == c."""
    _run_steps(dim, N, guess)


def test_two_runs_are_bit_identical(hip):
    import torch

    a, b = (_run_steps(3, 4, True, check=False) for _ in range(2))
    for x, y in ((a._scalar_groups[0].C, b._scalar_groups[0].C), (a._U, b._U), (a._P, b._P)):
        assert torch.equal(x.rdev(), y.rdev())
    assert torch.equal(a._scalar_groups[0].Ac.vals, b._scalar_groups[0].Ac.vals)


# ---- 5. groups ---------------------------------------------------------------------------------------------------------
def test_groups(hip, monkeypatch):
    """Two scalars equal except Sc_t: two groups, two launches per assemble_first, different fields.  Three scalars with
    equal specifications: one group of three columns, one launch per assemble_first; every column agrees with the one-column
    group of the other run to 1e-8 relative, the bound of the steps (the columns of a block solve stop together, so the
    iteration counts -- and the last bits -- may differ from a solve of their own)."""
    import oasisx_amd as ox

    nu, dt, kappa = 0.01, 0.005, 0.03

    def run(scts):
        clock_c = {"t": 0.0}
        scalars = [_scalar(clock_c, kappa, s, name=f"T{i}") for i, s in enumerate(scts)]
        S, clock, _ = _problem(2, 6, 2, ox.Smagorinsky(Cs=0.5), scalars, nu, dt)
        proxy = _counted(S, monkeypatch)
        for k in range(2):
            clock["t"] = clock_c["t"] = (k + 1) * dt
            S.solve(dt, nu, max_iter=1)
        monkeypatch.undo()
        return S, proxy.calls

    S, calls = run([0.7, 0.35])
    assert len(S._scalar_groups) == 2 and calls == ["ox_scalar_rows_cellvisc"] * 4
    c0, c1 = (S.scalar(n)._storage.rhost()[:, 0] for n in ("T0", "T1"))
    assert np.abs(c0 - c1).max() > 1e-6 * np.abs(c0).max()
    S3, calls = run([0.7, 0.7, 0.7])
    assert len(S3._scalar_groups) == 1 and S3._scalar_groups[0].nc == 3 and calls == ["ox_scalar_rows_cellvisc"] * 2
    C = S3._scalar_groups[0].C.rhost()
    for j in range(3):
        assert np.abs(C[:, j] - c0).max() <= 1e-8 * np.abs(c0).max()  # (lock-step columns stop together: the steps' bound)


# ---- 6. periodic -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_blocks", [False, True])
@pytest.mark.parametrize("dim,N,deg", [(2, 6, 2), (3, 4, 2)])
def test_periodic_box(hip, dim, N, deg, row_blocks):
    """The make_periodic box: check 1 against the model on the reduced space (no Dirichlet rows: every face is identified),
    by width bins and by row blocks; the velocity's A and b_first are the bits of the same solver without scalars."""
    import torch

    import oasisx_amd as ox
    from tests.scalar_les_model import ScalarLesModel
    from tests.test_gpu_periodic import _forms, _perturbed_tg, _set_fields, _solver, _tg_mesh
    from tests.test_gpu_scalar import _options

    nu, dt, kappa, sct = 0.5, 0.1, 0.2, 0.7
    mo = ox.Smagorinsky()
    src = lambda x: 0.5 + x[0]  # noqa: E731  (linear, as in tests/test_gpu_periodic.py: no quadrature rule enters the comparison)
    ini = lambda x: np.cos(np.pi * x[0]) * np.cos(np.pi * x[1]) + 0.2 * np.sin(np.pi * x[dim - 1])  # noqa: E731
    sc = ox.ScalarTransport("T", diffusivity=kappa, source=src, initial=ini, turbulent_schmidt=sct)
    opts = {"assemble_row_blocks": row_blocks}
    S = _solver(_tg_mesh(dim, N), deg, solver_options=_options(guess=True), options=opts, scalars=[sc], viscosity_model=mo)
    assert S._row_blocks == row_blocks and (not row_blocks or S._Vi[0][0].pattern.n_row_blocks > 0)
    fns, p_fn = _perturbed_tg(dim, nu)
    _set_fields(S, None, fns, p_fn)
    F, x_v, _ = _forms(S)
    m = ScalarLesModel(F, x_v, kappa, sct, model=("smagorinsky", mo.coefficient), source=src)
    m.interpolate(ini)
    S.assemble_first(dt, nu)
    m.assemble(S._UAB.rhost(), dt)
    _check_against(S, m, dt, f"periodic ({dim},{N},{deg})")
    P = _solver(_tg_mesh(dim, N), deg, solver_options=_options(guess=True), options=opts, viscosity_model=mo)
    _set_fields(P, None, fns, p_fn)
    P.assemble_first(dt, nu)
    assert torch.equal(S._A.vals, P._A.vals) and torch.equal(S._BFIRST.rdev(), P._BFIRST.rdev())


# ---- 7. coupled --------------------------------------------------------------------------------------------------------
def test_buoyancy_with_a_model(hip):
    """buoyancy=(0, b) beside Smagorinsky and Sc_t = 0.7 (the coupling of the heated cavity on the perturbed Taylor-Green
    levels, where nut > 0): b_first equals the viscosity model's with the force b M (c* - reference) in b0, to 1e-12
    max|.|; scalar_diffusivity is kappa + eddy_viscosity() / Sc_t, the same two operations, exactly."""
    import torch

    import oasisx_amd as ox
    from tests import viscosity_model as VM
    from tests.buoyancy_model import buoyancy_rows
    from tests.test_gpu_viscosity import _forms, _model_of

    dt, nu, kappa, sct, b = 0.1, 0.5, 0.2, 0.7, (0.0, 3.0)
    clock_c = {"t": 0.0}
    mo = ox.Smagorinsky()
    sc = _scalar(clock_c, kappa, sct, buoyancy=b, reference=0.5)
    S, clock, mesh = _problem(2, 5, 2, mo, [sc], nu, dt)
    F, x_v, x_q = _forms(S, mesh)
    R, rc = VM.tg_step_model(F, x_v, x_q, _model_of(S, mo), nu=nu, dt=dt)
    R.u1[:], R.u2[:] = S._U1.rhost(), S._U2.rhost()
    c1 = S._scalar_groups[0].C1.rhost()[:, 0].copy()
    R.b0 = R.b0 + buoyancy_rows(R.M, np.zeros_like(R.b0), [(c1, c1.copy(), 0.5, b)])
    rc["t"] = dt
    _assemble(S, clock, clock_c, dt, nu)
    R.assemble_first(dt, nu)
    db = np.abs(S._BFIRST.rhost() - R.b_first).max()
    print(f"db_first = {db:.3e} of {np.abs(R.b_first).max():.3e}; max nut = {R.nut.max():.3e}")
    assert R.nut.max() > 0.0 and db <= 1e-12 * np.abs(R.b_first).max()
    m = _les_model(S, mesh, mo, kappa, sct, clock_c)
    m.assemble(S._UAB.rhost(), dt)
    _check_against(S, m, dt, "coupled")
    assert torch.equal(S.scalar_diffusivity("T", nu), kappa + S.eddy_viscosity() / sct)
    assert float(S.scalar_diffusivity("T", nu).max()) > kappa
    with pytest.raises(KeyError):
        S.scalar_diffusivity("no such scalar", nu)
    # an independent figure for scalar_diffusivity: the model's nut per cell, in the mesh's cell order
    lc = S._Vi[0][0].local_cells.cpu().numpy()
    dk = np.abs(S.scalar_diffusivity("T", nu).cpu().numpy()[lc] - (kappa + R.nut / sct)).max()
    assert dk <= 1e-12 * (kappa + R.nut.max() / sct), dk


def test_one_coupled_step(hip):
    """One whole step with buoyancy=(0, b), Smagorinsky and Sc_t = 0.7: c against the model stepped with the device's u_ab
    and nut (relative 1e-8, iterations within 1, as the steps above), and the force moves the velocity: u differs from the
    run with b = 0, whose scalar it leaves bit for bit alone in the first step (the operator of the first step does not
    depend on the force)."""
    import torch

    import oasisx_amd as ox
    from tests.test_gpu_scalar import _options

    dt, nu, kappa, sct = 0.005, 0.01, 0.03, 0.7
    mo = ox.Smagorinsky()
    out = {}
    for b in ((0.0, 3.0), None):
        clock_c = {"t": 0.0}
        sc = _scalar(clock_c, kappa, sct, source=lambda x: 0.5 + x[0], buoyancy=b, reference=0.5)
        S, clock, mesh = _problem(2, 8, 2, mo, [sc], nu, dt, perturb=0.05)
        m = _les_model(S, mesh, mo, kappa, sct, clock_c, options=_options(guess=True)["scalar_transport"],
                       source=lambda x: 0.5 + x[0])
        clock["t"] = clock_c["t"] = dt
        S.solve(dt, nu, max_iter=1)
        m.step(S._UAB.rhost(), dt, nut=S._nut.cpu().numpy())
        c = S._scalar_groups[0].C.rhost()[:, 0]
        rel = np.abs(c - m.c).max() / np.abs(m.c).max()
        its = S.iteration_counts()["scalar_transport"]["T"]
        print(f"b = {b}: rel diff {rel:.3e}, iterations {its} (model {m.its})")
        assert m.reason > 0 and rel < 1e-8 and abs(its - m.its) <= 1
        out[b is None] = (S._U.rdev().clone(), S._scalar_groups[0].C.rdev().clone())
    assert not torch.equal(out[False][0], out[True][0])
    assert torch.equal(out[False][1], out[True][1])


def test_full_stress_form(hip):
    """stress_form="full" beside a scalar: the transposed term touches b_first alone; A_c and b_c against the model."""
    import oasisx_amd as ox

    dt, nu, kappa, sct = 0.1, 0.5, 0.2, 0.7
    clock_c = {"t": 0.0}
    mo = ox.Smagorinsky()
    S, clock, mesh = _problem(3, 3, 2, mo, [_scalar(clock_c, kappa, sct)], nu, dt, stress_form="full")
    m = _les_model(S, mesh, mo, kappa, sct, clock_c)
    _assemble(S, clock, clock_c, dt, nu)
    m.assemble(S._UAB.rhost(), dt)
    _check_against(S, m, dt, "full stress form")


# ---- 8. ScalarFlux -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N,deg", [(2, 4, 2), (3, 3, 1), (3, 3, 3)])
def test_flux_with_a_cell_viscosity(hip, dim, N, deg):
    """flux() facet by facet against -(kappa + nut_c / Sc_t) n . gbar(c) from numpy, to 1e-12 max|.| (the bound of
    tests/test_gpu_buoyancy.py on the flux without a model); the same object on a solver without a model: today's bits."""
    import torch

    import oasisx_amd as ox
    from tests.buoyancy_model import facet_flux
    from tests.test_gpu_viscosity import _forms, _sponge

    dt, nu, kappa, sct = 0.1, 0.4, 0.2, 0.7
    f1 = lambda x: np.cos(2.0 * x[0]) + 0.5 * x[1] + x[0] * x[1] + (x[2] ** 2 if dim == 3 else 0.0)  # noqa: E731
    out = {}
    for key, mo in (("model", ox.CellViscosity(_sponge)), ("plain", None), ("zero", ox.CellViscosity(0.0))):
        clock_c = {"t": 0.0}
        S, clock, mesh = _problem(dim, N, deg, mo, [_scalar(clock_c, kappa, sct, name="a"), _scalar(clock_c, kappa, sct)], nu, dt)
        assert S._scalar_groups[0].nc == 2
        flux = ox.ScalarFlux(S, "T")
        _assemble(S, clock, clock_c, dt, nu)
        S.scalar("T").interpolate(f1)
        flux.sample(0.0, nu, dt=0.5)
        out[key] = (flux.flux().clone(), flux._fq.clone(), flux.facet_mean().clone(), flux.mean_flux().clone())
        if key != "model":
            continue
        F, x_v, _ = _forms(S, mesh)
        fc = S._Vi[0][0].kernel_cell_index(flux.cells)
        c = S.scalar("T")._storage.rhost()[:, 1]
        q1, area, cbar, _ = facet_flux(F, fc, flux.local_facets, c, 1.0)
        nut = S._nut.cpu().numpy()
        q = (kappa + nut[fc] / sct) * q1
        dq = np.abs(flux.flux().cpu().numpy() - q).max()
        dfq = np.abs(flux._fq.cpu().numpy() - area * q).max()
        print(f"{dim}-D P{deg}: dq = {dq:.3e} (max {np.abs(q).max():.3e}), dfq = {dfq:.3e}; nut on the facets' cells "
              f"{nut[fc].min():.3e} .. {nut[fc].max():.3e}")
        assert nut[fc].min() > 0.0
        assert dq <= 1e-12 * np.abs(q).max() and dfq <= 1e-12 * np.abs(area * q).max()
        assert np.abs(flux.flux().cpu().numpy() - kappa * q1).max() > 1e-3 * np.abs(q).max()  # (nut is in it)
    for a, b in zip(out["zero"], out["plain"]):
        assert torch.equal(a, b)


def test_flux_without_a_model_calls_the_plain_entry(hip, monkeypatch):
    import oasisx_amd as ox

    for mo, want in ((None, "ox_scalar_flux"), (ox.CellViscosity(0.1), "ox_scalar_flux_cells")):
        clock_c = {"t": 0.0}
        S, clock, _ = _problem(2, 4, 2, mo, [_scalar(clock_c, 0.2, 0.7)], 0.4, 0.1)
        flux = ox.ScalarFlux(S, "T")
        _assemble(S, clock, clock_c, 0.1, 0.4)
        proxy = _counted(S, monkeypatch)
        flux.sample(0.0, 0.4)
        monkeypatch.undo()
        assert [c for c in proxy.calls if "flux" in c] == [want]


# ---- 9. guards on the device build -------------------------------------------------------------------------------------
def test_guards(hip):
    import oasisx_amd as ox

    clock_c = {"t": 0.0}
    with pytest.raises(NotImplementedError, match="scalars") as e:
        _problem(2, 4, 2, ox.Smagorinsky(), [_scalar(clock_c, 0.1, None)], 0.01, 0.005)
    assert "turbulent_schmidt=" in str(e.value)
    law = ox.CarreauYasuda(nu0=0.16, nu_inf=0.01, lam=3.313, n=0.3568)
    with pytest.raises(ValueError, match="inf"):
        _problem(2, 4, 2, law, [_scalar(clock_c, 0.1, 0.7)], law.base_viscosity, 0.005)
    with pytest.raises(ValueError, match="turbulent_schmidt"):
        _scalar(clock_c, 0.1, 0.0)
    with pytest.raises(NotImplementedError, match="rotational"):
        _problem(2, 4, 2, ox.Smagorinsky(), [_scalar(clock_c, 0.1, 0.7)], 0.01, 0.005, rotational=True)
    S, _, _ = _problem(2, 4, 2, None, [_scalar(clock_c, 0.1, 0.7)], 0.01, 0.005)
    with pytest.raises(RuntimeError, match="viscosity_model"):
        S.scalar_diffusivity("T", 0.01)


def test_kernel_refuses_bad_arguments(hip):
    """The argument checks of ox_scalar_rows_cellvisc, in the style of ox_scalar_rows."""
    import ctypes as C

    import oasisx_amd as ox
    from oasisx_amd import _lib

    clock_c = {"t": 0.0}
    S, clock, _ = _problem(2, 4, 2, ox.CellViscosity(0.1), [_scalar(clock_c, 0.2, 0.7)], 0.5, 0.1)
    _assemble(S, clock, clock_c, 0.1, 0.5)
    g, Vi, lib, st = S._scalar_groups[0], S._Vi[0][0], S._lib, _lib.current_stream()

    def call(Ac=None, nut=True, dt=0.1, ncomp=1, row_blocks=0, A=None):
        return lib.ox_scalar_rows_cellvisc(C.byref(S._cells), C.byref(Vi.assembly_info()), (A or S._A).ref(), S._M.ref(),
                                           S._K.ref(), (Ac or g.Ac).ref(), _lib.ptr(S._nut) if nut else None, 0.1, -0.2, dt,
                                           ncomp, g.C1.rptr(), g.B0.rptr(), g.B.ptr(), None, row_blocks, st)

    assert call() == 0
    for kw, text in ((dict(nut=False), "null argument"), (dict(Ac=S._A), "value array of its own"), (dict(dt=0.0), "dt="),
                     (dict(ncomp=0), "ncomp="), (dict(ncomp=4), "ncomp="), (dict(row_blocks=2), "row_blocks="),
                     (dict(A=S._Ap), "share one sparsity pattern")):
        assert call(**kw) != 0, kw
        assert text in lib.ox_last_error().decode(), (kw, lib.ox_last_error())


# ---- 10. the demo ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_demo(hip, capsys, dim):
    """demo/les_scalar_channel_hip.py at its smallest size: the turbulent part of the scalar diffusivity,
    scalar_diffusivity - kappa, equals the closed form nut(y) / Sc_t to 1e-12 of ITS maximum (the figure
    tests/test_gpu_vandriest.py accepts for nut in demo/les_channel_hip.py, relative to max nut) plus the rounding of the
    sum kappa + nut / Sc_t and of taking kappa off again, 2 eps (kappa + max nut / Sc_t); the diffusivity exceeds kappa in
    every slab, and the two wall fluxes are opposite in sign."""
    from demo.les_scalar_channel_hip import main

    res = main(["-N", "4", "--dim", str(dim), "--A-plus", "2", "--steps", "1"])
    out = capsys.readouterr().out
    assert "closed form" in out and "wall fluxes" in out
    eps = np.finfo(np.float64).eps
    print(f"turbulent part: error {res['error_turbulent']:.3e} of {res['turbulent_max']:.3e}; kappa {res['kappa']:.3e}")
    assert res["error_turbulent"] <= 1e-12 * res["turbulent_max"] + 2.0 * eps * res["diffusivity_max"]
    assert res["error"] <= 1e-12 * res["diffusivity_max"] and res["diffusivity_max"] > res["kappa"]
    rows = res["rows"]
    assert len(rows) == 4 and all(r["diffusivity"] > res["kappa"] for r in rows)
    for lower, upper in (res["flux_first"], res["flux_last"]):
        assert lower > 0.0 > upper, (lower, upper)  # the scalar leaves through the wall held at 0
