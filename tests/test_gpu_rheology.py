"""GPU: the generalised-Newtonian laws (oasisx_amd/viscosity.py, the law branches of csrc/ox_viscosity.hip) and the full
stress form (``stress_form="full"``, k_stress_transpose of csrc/ox_assemble.hip) against the numpy model of
tests/rheology_model.py, which is built on the oracle's forms and pinned by tests/test_rheology_host.py.  Shapes, set-up
and tolerances are those of tests/test_gpu_viscosity.py: the model is fed the device's numbering and velocity blocks."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_viscosity import CASES, _assemble_first, _delaunay, _forms, _model_of, _problem

pytestmark = pytest.mark.gpu

KINDS = ["lattice", "delaunay"]


def _laws():
    import oasisx_amd as ox

    return [ox.CarreauYasuda(nu0=0.16, nu_inf=0.01, lam=3.313, n=0.3568), ox.Cross(nu0=0.16, nu_inf=0.01, lam=1.007, m=1.028),
            ox.PowerLaw(k=0.05, n=0.6, nu_min=0.005, nu_max=0.5)]


def _x2(x):
    return 0.5 * (1.0 + x[0] ** 2)


def _rm_model(S, m):
    """The model tuple of tests/rheology_model.py for a model object."""
    import oasisx_amd as ox

    if isinstance(m, ox.CarreauYasuda):
        return ("carreau_yasuda", m.params)
    if isinstance(m, ox.Cross):
        return ("cross", m.params)
    if isinstance(m, ox.PowerLaw):
        return ("power_law", m.params)
    return _model_of(S, m)


def _transpose(S, uab, nut, b, scale=1.0):
    from oasisx_amd import _lib

    Vi = S._Vi[0][0]
    _lib.check(S._lib.ox_assemble_stress_transpose(Vi.degree, C.byref(S._cells), _lib.ptr(Vi.cell_dofs), C.byref(S._adj_u),
                                                   Vi.n_owned, _lib.ptr(uab), _lib.ptr(nut), float(scale), _lib.ptr(b),
                                                   _lib.current_stream()), "ox_assemble_stress_transpose")


# ---- 1. nut of each law ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_law_nut_per_cell_matches_the_model(hip, dim, N, deg, kind):
    """Carreau-Yasuda (blood: Cho & Kensey's constants in kinematic units), Cross and a power law on Taylor-Green plus the
    non-solenoidal perturbation: max |nut_device - nut_model| <= 1e-12 max nut, with max nut >= base_viscosity (the law
    matters); nut >= 0; effective_viscosity() = base + nut in the mesh's cell order."""
    from tests import rheology_model as RM

    mesh = _delaunay(dim, N) if kind == "delaunay" else None
    for m in _laws():
        nu, dt = m.base_viscosity, 0.1
        S, clock, mesh = _problem(dim, N, deg, m, nu=nu, dt=dt, mesh=mesh, perturb=0.3)
        F, _, _ = _forms(S, mesh)
        _assemble_first(S, clock, dt, nu)
        ref = RM.nut_cells(F, S._UAB.rhost(), _rm_model(S, m))
        dev = S._nut.cpu().numpy()
        d = np.abs(dev - ref).max()
        print(f"{m!r} {kind} ({dim},{N},{deg}): max |d nut| = {d:.3e}, nut in [{ref.min():.3e}, {ref.max():.3e}], "
              f"ratio {d / ref.max():.3e}")
        assert ref.max() >= m.base_viscosity and dev.min() >= 0.0
        assert ref.max() - ref.min() > 1e-2 * ref.max()  # (the shear rate varies over the mesh: the law is exercised)
        assert d <= 1e-12 * ref.max(), (repr(m), d, ref.max())
        lc = S._Vi[0][0].local_cells.cpu().numpy()
        eff = S.effective_viscosity().cpu().numpy()
        assert eff.shape == (int(mesh.num_cells),) and np.array_equal(eff[lc], dev + m.base_viscosity)


def test_power_law_at_rest_takes_the_branches(hip):
    """u = 0: gd == 0 in every cell -- nu_max for n < 1, nu_min for n > 1, the clipped k for n == 1; no NaN."""
    import oasisx_amd as ox

    for n, want in ((0.6, 0.5), (1.4, 0.005), (1.0, 0.05)):
        m = ox.PowerLaw(0.05, n, 0.005, 0.5)
        S, clock, _ = _problem(2, 4, 2, m, nu=m.base_viscosity)
        S._UAB.dev().zero_()
        S.viscosity_assemble()
        assert np.array_equal(S._nut.cpu().numpy(), np.full(S._nut.shape[0], want - 0.005)), n


# ---- 2. the transposed term alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_stress_transpose_matches_the_model(hip, dim, N, deg, kind):
    """ox_assemble_stress_transpose on a zeroed b with scale = 1, with the nut of Smagorinsky and of a non-constant
    CellViscosity: T entry by entry to 1e-12 max |T|; two launches give the same bits; scale and the in/out b are honoured."""
    import torch

    import oasisx_amd as ox
    from tests import rheology_model as RM

    dt, nu = 0.1, 0.5
    mesh = _delaunay(dim, N) if kind == "delaunay" else None
    for m in (ox.Smagorinsky(), ox.CellViscosity(_x2)):
        S, clock, mesh = _problem(dim, N, deg, m, nu=nu, dt=dt, mesh=mesh, perturb=0.3)
        F, _, _ = _forms(S, mesh)
        _assemble_first(S, clock, dt, nu)
        uab, nut = S._UAB.rdev(), S._nut
        ref = RM.transposed_term(F, S._UAB.rhost(), nut.cpu().numpy())
        b1, b2 = torch.zeros_like(uab), torch.zeros_like(uab)
        _transpose(S, uab, nut, b1)
        _transpose(S, uab, nut, b2)
        assert torch.equal(b1, b2)
        d = np.abs(b1.cpu().numpy() - ref).max()
        print(f"{m!r} {kind} ({dim},{N},{deg}): max |dT| = {d:.3e}, max |T| = {np.abs(ref).max():.3e}")
        assert np.abs(ref).max() > 0.0 and d <= 1e-12 * np.abs(ref).max(), (repr(m), d)
        base = torch.full_like(uab, 0.25)
        _transpose(S, uab, nut, base, scale=-2.0)
        assert np.abs(base.cpu().numpy() - (0.25 - 2.0 * ref)).max() <= 1e-12 * max(np.abs(ref).max(), 1.0)


@pytest.mark.parametrize("dim,N,deg", CASES)
def test_rigid_rotation_on_the_device(hip, dim, N, deg):
    """u = omega x x with a random nut per cell in [0.05, 0.1]: the device's T cancels the model's K_nut u to 1e-12
    max |K_nut u| on every row -- the full form exerts no viscous force on a rigid rotation, the Laplacian form does."""
    import torch

    import oasisx_amd as ox
    from tests import rheology_model as RM
    from tests import viscosity_model as VM

    S, clock, mesh = _problem(dim, N, deg, ox.CellViscosity(0.0))
    F, x_v, _ = _forms(S, mesh)
    u = RM.rigid_rotation(x_v)
    nut = np.random.default_rng(7).uniform(0.05, 0.1, F.cells.shape[0])
    Ku = VM.weighted_stiffness(F, nut) @ u
    dev = S._mesh.device
    b = torch.zeros(u.shape, dtype=torch.float64, device=dev)
    _transpose(S, torch.from_numpy(u).to(dev).contiguous(), torch.from_numpy(nut).to(dev), b)
    r = np.abs(Ku + b.cpu().numpy()).max()
    print(f"({dim},{N},{deg}): max |K_nut u| = {np.abs(Ku).max():.3e}, max |K_nut u + T| = {r:.3e}")
    assert np.abs(Ku).max() >= 1e-3
    assert r <= 1e-12 * np.abs(Ku).max()


# ---- 3. b_first with stress_form="full" ---------------------------------------------------------------------------------
@pytest.mark.parametrize("row_blocks", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_full_form_rhs_entry_by_entry(hip, dim, N, deg, kind, row_blocks):
    """assemble_first with stress_form="full" and CellViscosity(0.5 (1 + x^2)): b_first equals the model's to 1e-12
    max |b_first|, by width bins and by row blocks, where the model's T is at least 1e-2 max |b_first| (so the bound
    cannot hide a missing term); A and the A u1 by-product are the bits of the "laplacian" run."""
    import torch

    import oasisx_amd as ox
    from tests import rheology_model as RM
    from tests.helpers import KRYLOV

    dt, nu = 0.005, 0.01
    so = {k: dict(v, ksp_initial_guess_nonzero=True) for k, v in KRYLOV.items()}
    mesh = _delaunay(dim, N) if kind == "delaunay" else None
    out = {}
    for form in ("laplacian", "full"):
        m = ox.CellViscosity(_x2)
        S, clock, mesh = _problem(dim, N, deg, m, nu=nu, dt=dt, mesh=mesh, solver_options=so, stress_form=form,
                                  options={"assemble_row_blocks": row_blocks})
        assert S._row_blocks == row_blocks and (not row_blocks or S._Vi[0][0].pattern.n_row_blocks > 0)
        F, x_v, x_q = _forms(S, mesh)
        R, rc = RM.tg_step_model(F, x_v, x_q, _model_of(S, m), form, nu=nu, dt=dt)
        R.u1[:], R.u2[:] = S._U1.rhost(), S._U2.rhost()
        rc["t"] = dt
        _assemble_first(S, clock, dt, nu)
        R.assemble_first(dt, nu)
        db = np.abs(S._BFIRST.rhost() - R.b_first).max()
        bmax = np.abs(R.b_first).max()
        if form == "full":
            share = np.abs(R.T).max() / bmax
            print(f"{kind} ({dim},{N},{deg}) row_blocks={row_blocks}: max|T| / max|b_first| = {share:.3e}, db = {db:.3e} "
                  f"(max|b| = {bmax:.3e})")
            assert share >= 1e-2
        assert db <= 1e-12 * bmax, (form, db, bmax)
        assert S._AU1_valid
        out[form] = (S._A.vals.clone(), S._B3.rdev()[: S._no_u].clone(), S._BFIRST.rdev().clone())
    assert torch.equal(out["full"][0], out["laplacian"][0]) and torch.equal(out["full"][1], out["laplacian"][1])
    assert not torch.equal(out["full"][2], out["laplacian"][2])


# ---- 4. whole steps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("low_memory", [True, False])
@pytest.mark.parametrize("which", ["carreau_yasuda-laplacian", "smagorinsky-full"])
@pytest.mark.parametrize("dim,N", [(2, 8), (3, 3)])
def test_steps_match_the_model(hip, dim, N, which, low_memory):
    """Three P2-P1 Taylor-Green steps against the model subclass of the oracle: du <= 1e-8, dp <= 1e-7, the bounds of
    tests/test_gpu_viscosity.py::test_steps_match_the_model."""
    import oasisx_amd as ox
    from tests import rheology_model as RM
    from tests.helpers import KRYLOV

    dt = 0.005
    if which == "carreau_yasuda-laplacian":
        m, form = ox.CarreauYasuda(nu0=0.16, nu_inf=0.01, lam=3.313, n=0.3568), "laplacian"
        nu = m.base_viscosity
    else:
        m, form, nu = ox.Smagorinsky(), "full", 0.01
    S, clock, mesh = _problem(dim, N, 2, m, nu=nu, dt=dt, low_memory=low_memory, stress_form=form)
    F, x_v, x_q = _forms(S, mesh)
    R, rc = RM.tg_step_model(F, x_v, x_q, _rm_model(S, m), form, nu=nu, dt=dt, solver_options=KRYLOV, low_memory=low_memory)
    for k in range(3):
        clock["t"] = rc["t"] = (k + 1) * dt
        S.solve(dt, nu, max_iter=1)
        R.solve(dt, nu, max_iter=1)
        du = float(np.abs(S._U.rhost() - R.u1).max())
        dp = float(np.abs(S._P.rhost()[:, 0] - R.p).max())
        dn = float(np.abs(S._nut.cpu().numpy() - R.nut).max())
        print(f"{which} step {k}: du = {du:.3e}, dp = {dp:.3e}, d nut = {dn:.3e} (max nut {R.nut.max():.3e})")
        assert du <= 1e-8 and dp <= 1e-7, (k, du, dp)
    assert R.nut.max() > 0.0
    if form == "full":
        assert np.abs(R.T).max() > 0.0


def test_laplacian_keyword_is_the_default_path(hip):
    """stress_form="laplacian" given explicitly: u and p after two steps are the bits of the solver built without the
    keyword."""
    import torch

    import oasisx_amd as ox

    nu, dt = 0.01, 0.005
    res = []
    for kw in ({}, {"stress_form": "laplacian"}):
        S, clock, _ = _problem(3, 3, 2, ox.Smagorinsky(), nu=nu, dt=dt, **kw)
        for k in range(2):
            clock["t"] = (k + 1) * dt
            S.solve(dt, nu, max_iter=1)
        res.append((S._U.rdev().clone(), S._P.rdev().clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    S0, clock0, _ = _problem(2, 5, 2, None, nu=nu, dt=dt, stress_form="laplacian")  # (and without a model)
    assert S0._stress_form == "laplacian" and S0._nut is None


# ---- 5. wall stress with a law -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N,deg", [(2, 5, 2), (3, 3, 2)])
def test_wall_stress_uses_the_law(hip, dim, N, deg):
    """WallStress.sample on a Carreau-Yasuda solver after one step: the traction equals tests/wall_stress_model.py fed
    nu = base_viscosity and the MODEL's nut of that step, to 1e-12 max |t| (tests/test_gpu_wall_stress.py); it differs from
    the evaluation at the base viscosity alone."""
    import oasisx_amd as ox
    from tests import rheology_model as RM
    from tests.test_gpu_wall_stress import _model

    m = ox.CarreauYasuda(nu0=0.16, nu_inf=0.01, lam=3.313, n=0.3568)
    nu, dt = m.base_viscosity, 0.1
    S, clock, mesh = _problem(dim, N, deg, m, nu=nu, dt=dt, perturb=0.3)
    F, _, _ = _forms(S, mesh)
    clock["t"] = dt
    S.solve(dt, nu, max_iter=1)
    W = ox.WallStress(S)
    W.sample(dt, nu)
    kpos = S._Vi[0][0].kernel_cell_index(W.cells)
    nut = RM.nut_cells(F, S._UAB.rhost(), _rm_model(S, m))[kpos]
    assert nut.min() > 0.0
    t_ref, w_ref = _model(S, W, mesh, nu + nut)
    t_plain, _ = _model(S, W, mesh, nu)
    scale = np.abs(t_ref).max()
    rt = np.abs(W.traction().cpu().numpy() - t_ref).max() / scale
    rw = np.abs(W.wss().cpu().numpy() - w_ref).max() / scale
    print(f"({dim},{N},{deg}): max |dt| / max|t| = {rt:.3e}, max |dwss| / max|t| = {rw:.3e}")
    assert rt <= 1e-12 and rw <= 1e-12
    assert np.abs(t_plain - t_ref).max() > 1e-6 * scale


# ---- 6. the surface and the guards ---------------------------------------------------------------------------------------
def test_surface_and_guards(hip):
    import oasisx_amd as ox
    from oasisx_amd import _lib

    m = ox.CarreauYasuda(nu0=0.16, nu_inf=0.01, lam=3.313, n=0.3568)
    S, clock, _ = _problem(2, 4, 2, m, nu=m.base_viscosity)
    with pytest.raises(ValueError, match="base_viscosity"):
        _assemble_first(S, clock, 0.005, 0.02)
    _assemble_first(S, clock, 0.005, m.base_viscosity)
    assert float(S.effective_viscosity().min()) >= m.base_viscosity
    for other in (ox.Smagorinsky(), ox.CellViscosity(0.1), None):
        S2, clock2, _ = _problem(2, 4, 2, other)
        with pytest.raises(RuntimeError):
            S2.effective_viscosity()
    _assemble_first(S2, clock2, 0.005, 0.37)  # without a law nu is the caller's
    with pytest.raises(RuntimeError):
        S2.stress_transpose_assemble()
    with pytest.raises(ValueError, match="stress_form"):
        _problem(2, 4, 2, None, stress_form="full")
    with pytest.raises(ValueError, match="stress_form"):
        _problem(2, 4, 2, m, stress_form="transposed")
    with pytest.raises(NotImplementedError, match="rotational"):
        _problem(2, 4, 2, m, rotational=True)
    with pytest.raises(NotImplementedError, match="scalars"):
        _problem(2, 4, 2, m, scalars=[ox.ScalarTransport("T", diffusivity=0.1)])
    # the C entry points check their own arguments
    Vi = S._Vi[0][0]
    par = (C.c_double * 4)(0.05, 0.6, 0.5, 0.005)  # nu_min > nu_max
    for model in (4, 2, 0):  # the power law's own check; Carreau-Yasuda takes five parameters; model 0 reads no params
        args = _lib.ox_viscosity_args(model, Vi.degree, _lib.ptr(Vi.cell_dofs), S._UAB.rptr(), _lib.ptr(S._nut), 0.0, par, 4,
                                      None, None, 0, 0, None)
        rc = S._lib.ox_cell_viscosity(C.byref(S._cells), C.byref(args), _lib.current_stream())
        assert rc != 0 and b"ox_cell_viscosity" in S._lib.ox_last_error() and b"param" in S._lib.ox_last_error()


# ---- 7. the demo ---------------------------------------------------------------------------------------------------------
def test_demo_approaches_the_power_law_profile(hip, capsys):
    """demo/non_newtonian_channel_hip.py at N = 8: started from the Newtonian parabola, the profile probed across the
    channel ends closer (L2 over the probes) to the power-law profile than to the parabola."""
    from demo.non_newtonian_channel_hip import main

    rows = main(["-N", "8"])
    out = capsys.readouterr().out
    assert "L2 error" in out and "power-law" in out
    r = rows[0]
    print(out)
    assert np.isfinite(r["u"]).all() and r["nu_min"] >= 0.01 and r["nu_max"] <= 5.0
    assert r["to_power_law"] < r["to_parabola"]
