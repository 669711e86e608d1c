"""GPU: SUPG-stabilised scalars -- ``ScalarTransport(stabilization=SUPG(...))`` (oasisx_amd/scalar.py, ``ox_supg_cells`` of
csrc/ox_scalar.hip, ``ox_scalar_rows_supg`` of csrc/ox_assemble.hip) against the numpy model of
tests/scalar_supg_model.py, which tests/test_scalar_supg_host.py pins.  The model is fed the device's numbering and the
device's own velocity blocks."""
import numpy as np
import pytest

from tests.test_gpu_scalar_les import CASES, INI, SRC, _assemble, _problem, _scalar, _val

pytestmark = pytest.mark.gpu

KAPPA, DT, NU = 1e-3, 0.1, 0.5  # cell Peclet numbers of 10 .. 100 on the O(1) perturbed field
NEW = ("ox_supg_cells", "ox_scalar_rows_supg")


def _supg(**kw):
    import oasisx_amd as ox

    return ox.SUPG(**kw)


def _supg_model(S, mesh, model_obj, kappa, sct, clock_c, dirichlet=True, options=None, source=SRC, initial=INI, forms=None,
                **kw):
    from tests.scalar_supg_model import ScalarSupgModel
    from tests.test_gpu_scalar import _dofs, left
    from tests.test_gpu_viscosity import _forms, _model_of

    F, x_v = forms if forms is not None else _forms(S, mesh)[:2]
    m = ScalarSupgModel(F, x_v, kappa, turbulent_schmidt=None if model_obj is None else sct, model=_model_of(S, model_obj),
                        dofs=_dofs(x_v, left) if dirichlet else None, value=_val(clock_c), source=source, options=options, **kw)
    m.interpolate(initial)
    return m


def _check_against(S, m, dt, what, share=True, ax0=True):
    """A_c, b_c of group 0 against the assembled model: 1e-12 max|.| (tests/test_gpu_scalar.py, test_gpu_parity.py); tau per
    cell to 1e-12 max tau; the stabilising terms are not lost in the bound; the handed A_c c_1 equals the mat-vec bit for
    bit."""
    import torch

    g = S._scalar_groups[0]
    A_ref, b_ref = m.A, m.b
    dA = abs(g.Ac.to_scipy() - A_ref).max()
    db = np.abs(g.B.rhost()[:, 0] - b_ref).max()
    st_share = abs(m.N / dt + 0.5 * m.S).max() / abs(A_ref).max()
    lc = S._Vi[0][0].local_cells.cpu().numpy()
    tau = S.supg_parameter(g.members[0].name).cpu().numpy()[lc]
    dtau = np.abs(tau - m.tau).max()
    rec = g.supg_rec.cpu().numpy()
    dw = np.abs(rec[:-1].T - m.w).max()
    print(f"{what}: dA = {dA:.3e} (max|A_c| = {abs(A_ref).max():.3e}, max|N/dt + S/2| / max|A_c| = {st_share:.2e}), "
          f"db = {db:.3e} (max|b_c| = {np.abs(b_ref).max():.3e}), dtau = {dtau:.3e} (max tau = {m.tau.max():.3e}), "
          f"dw = {dw:.3e}")
    if share:
        assert st_share > 1e-4
    assert dA <= 1e-12 * abs(A_ref).max(), dA
    assert db <= 1e-12 * np.abs(b_ref).max(), db
    assert dtau <= 1e-12 * m.tau.max(), dtau
    assert dw <= 1e-12 * max(np.abs(m.w).max(), 1e-300), dw
    if ax0:
        assert g.ax0_valid
        y = torch.zeros_like(g.C1.rdev())
        g.Ac.mult(g.C1.rdev(), y, 1)
        assert torch.equal(y[: S._no_u], g.AC1.rdev()[: S._no_u])


class Counting:
    """The library with a list of the calls of the scalar row entries and of the per-cell SUPG launch."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        if name in ("ox_scalar_rows", "ox_scalar_rows_cellvisc") + NEW:
            self.calls.append(name)
        return getattr(self._lib, name)


def _counted(S, monkeypatch):
    from oasisx_amd import _lib

    proxy = Counting(_lib.load())
    monkeypatch.setattr(_lib, "_lib", proxy)
    monkeypatch.setattr(S, "_lib", proxy)
    return proxy


def _set_uniform_velocity(S, u):
    for i in range(S._gdim):
        for lvl in (S._u1, S._u2):
            lvl[i].interpolate(lambda x, v=float(u[i]): np.full(x.shape[1], v))


# ---- 1. A_c and b_c, entry by entry ------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_blocks", [False, True])
@pytest.mark.parametrize("mode", ["dictionary", "f64", "delaunay"])
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_operator_and_rhs_entry_by_entry(hip, dim, N, deg, mode, row_blocks):
    """After assemble_first on the perturbed field, kappa = 1e-3, dt = 0.1, a callable source and Dirichlet rows on x = -1,
    without a model and with Smagorinsky at Sc_t = 0.7: A_c, b_c and tau equal the model's to 1e-12 max|.|, with
    max|N/dt + S/2| > 1e-4 max|A_c|; A_c c_1 is the mat-vec's bits, and the velocity's A and b_first are the bits of the same
    solver without scalars."""
    import torch

    import oasisx_amd as ox
    from tests.test_gpu_viscosity import _delaunay

    mesh = _delaunay(dim, N) if mode == "delaunay" else None
    opts = {"value_dictionary": mode != "f64", "assemble_row_blocks": row_blocks}
    for mo, sct in ((None, None), (ox.Smagorinsky(), 0.7)):
        clock_c = {"t": 0.0}
        sc = _scalar(clock_c, KAPPA, sct, stabilization=_supg())
        S, clock, mesh = _problem(dim, N, deg, mo, [sc], NU, DT, mesh=mesh, options=opts)
        assert S._row_blocks == row_blocks and (not row_blocks or S._Vi[0][0].pattern.n_row_blocks > 0)
        if mode == "dictionary" and dim == 2 and deg <= 2:
            assert S._M.vcode is not None and S._K.vcode is not None  # the LDS-dictionary instantiation runs
        elif mode == "f64":
            assert S._M.vcode is None and S._K.vcode is None
        m = _supg_model(S, mesh, mo, KAPPA, sct, clock_c)
        assert np.abs(S._scalar_groups[0].C1.rhost()[:, 0] - m.c1).max() <= 1e-14
        _assemble(S, clock, clock_c, DT, NU)
        m.assemble(S._UAB.rhost(), DT)
        _check_against(S, m, DT, repr(mo))
        P, pclock, _ = _problem(dim, N, deg, mo, None, NU, DT, mesh=mesh, options=opts)
        _assemble(P, pclock, {"t": 0.0}, DT, NU)
        assert torch.equal(S._A.vals, P._A.vals) and torch.equal(S._BFIRST.rdev(), P._BFIRST.rdev())


@pytest.mark.parametrize("kw", [dict(scale=0.5), dict(time_term=False), dict(scale=2.0, time_term=False)])
def test_scale_and_time_term(hip, kw):
    """The two parameters of SUPG reach tau: the check above with another scale and without the time term."""
    clock_c = {"t": 0.0}
    sc = _scalar(clock_c, KAPPA, None, stabilization=_supg(**kw))
    S, clock, mesh = _problem(2, 5, 2, None, [sc], NU, DT)
    m = _supg_model(S, mesh, None, KAPPA, None, clock_c, **kw)
    _assemble(S, clock, clock_c, DT, NU)
    m.assemble(S._UAB.rhost(), DT)
    _check_against(S, m, DT, repr(kw))


# ---- 2. fluid at rest ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_blocks", [False, True])
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_fluid_at_rest(hip, dim, N, deg, row_blocks):
    """u = 0: w_c = 0, tau_c is finite, and A_c.vals and b_c of the stabilised scalar are the BITS of the same scalar
    without stabilisation."""
    import torch

    out = {}
    for stab in (None, _supg()):
        clock_c = {"t": 0.0}
        sc = _scalar(clock_c, KAPPA, None, stabilization=stab)
        S, clock, _ = _problem(dim, N, deg, None, [sc], NU, DT, options={"assemble_row_blocks": row_blocks}, perturb=0.0)
        _set_uniform_velocity(S, [0.0] * dim)
        _assemble(S, clock, clock_c, DT, NU)
        g = S._scalar_groups[0]
        out[stab is None] = (g.Ac.vals.clone(), g.B.rdev().clone())
        if stab is not None:
            tau = S.supg_parameter("T")
            assert bool(torch.isfinite(tau).all()) and float(tau.min()) > 0.0
            assert float(g.supg_rec[:-1].abs().max()) == 0.0
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])


# ---- 3. consistency ------------------------------------------------------------------------------------------------------
def _faces_x(x):
    return np.isclose(np.abs(x[0]), 1.0)


@pytest.mark.parametrize("dim,N,deg", [(2, 6, 1), (2, 5, 2), (2, 4, 3), (3, 3, 1), (3, 3, 2), (3, 2, 3)])
def test_consistency_fixed_point(hip, dim, N, deg):
    """u = (1, 0[, 0]), c = x with Dirichlet values on both x-faces, insulated elsewhere, f = 1, kappa = 0.01: u . grad c = f
    and lap c = 0, so c = x is a fixed point of the stabilised step.  On a DELAUNAY mesh: there tau differs between the cells
    of a patch, so a streamline-diffusion-only scheme -- the model without N f_h in b_c -- moves c = x by about 1e-2 in three
    steps (asserted below on the model: beyond the bound allowed to the device); on the uniform lattice int w . grad phi_i
    over a patch cancels and such a scheme would pass.  Three steps from c = x at ksp_rtol = 1e-11 WITHOUT an initial guess
    (the solves start from 0); the device's drift max|c - x| is allowed 10 x the drift of the numpy model of the same case
    with the same Krylov tolerances (the solves sum in different orders).  Measured on one MI355X, drift of the device / of
    the model: 2-D P1 1.490e-11 / 1.490e-11, P2 5.607e-11 / 5.607e-11, P3 2.407e-11 / 2.407e-11;
    3-D P1 8.551e-11 / 8.550e-11, P2 7.842e-11 / 7.842e-11, P3 7.101e-11 / 7.101e-11; the model without N f_h 8.7e-03 .. 2.7e-02."""
    import oasisx_amd as ox
    from tests.scalar_supg_model import ScalarSupgModel
    from tests.test_gpu_scalar import _dofs, _options
    from tests.test_gpu_viscosity import _delaunay, _forms

    dt, nu, kappa = 0.1, 0.5, 0.01
    lin = lambda x: x[0].copy()  # noqa: E731
    sc = ox.ScalarTransport("T", diffusivity=kappa, source=1.0, initial=lin, stabilization=_supg(),
                            bcs=[ox.DirichletBC(lin, ox.LocatorMethod.GEOMETRICAL, _faces_x)])
    so = _options(guess=False)
    S, clock, mesh = _problem(dim, N, deg, None, [sc], nu, dt, guess=False, solver_options=so, perturb=0.0,
                              mesh=_delaunay(dim, N))
    _set_uniform_velocity(S, [1.0] + [0.0] * (dim - 1))
    F, x_v, _ = _forms(S, mesh)
    models = [ScalarSupgModel(F, x_v, kappa, dofs=_dofs(x_v, _faces_x), value=lin, source=1.0, galerkin_source_only=bad,
                              options=so["scalar_transport"]) for bad in (False, True)]
    for m in models:
        m.interpolate(lin)
    g = S._scalar_groups[0]
    for k in range(3):
        S.assemble_first(dt, nu)
        reasons = S.scalar_solve()
        assert all(r > 0 for r in reasons.values())
        for m in models:
            m.step(S._UAB.rhost(), dt)
            assert m.reason > 0
    tau = models[0].tau
    assert tau.max() > 1.05 * tau.min()  # tau differs from cell to cell
    drift = np.abs(g.C.rhost()[:, 0] - x_v[:, 0]).max()
    drift_model, drift_sd = (np.abs(m.c - x_v[:, 0]).max() for m in models)
    print(f"{dim}-D P{deg}: drift of the device {drift:.3e}, of the model {drift_model:.3e}; of the model without N f_h "
          f"{drift_sd:.3e}; tau {tau.min():.3e} .. {tau.max():.3e}")
    assert drift_sd > 1e3 * 10.0 * drift_model, (drift_sd, drift_model)  # the check rejects streamline diffusion alone
    assert drift <= 10.0 * drift_model, (drift, drift_model)


# ---- 4. whole steps ------------------------------------------------------------------------------------------------------
def _run_steps(dim, N, guess, steps=3, check=True):
    import oasisx_amd as ox

    nu, dt, kappa, sct = 0.01, 0.005, 1e-3, 0.7
    clock_c = {"t": 0.0}
    mo = ox.Smagorinsky()
    src = lambda x: 0.5 + x[0]  # noqa: E731
    ini = lambda x: np.cos(np.pi * x[0]) * np.cos(np.pi * x[1])  # noqa: E731
    sc = _scalar(clock_c, kappa, sct, source=src, initial=ini, stabilization=_supg())
    S, clock, mesh = _problem(dim, N, 2, mo, [sc], nu, dt, guess=guess, perturb=0.05)
    m = None
    if check:
        from tests.test_gpu_scalar import _options

        m = _supg_model(S, mesh, mo, kappa, sct, clock_c, options=_options(guess=guess)["scalar_transport"], source=src,
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
        print(f"step {k}: rel diff {rel:.3e}, iterations {its} (model {m.its}), max nut {m.nut.max():.3e}, "
              f"max tau {m.tau.max():.3e}")
        assert m.reason > 0 and m.nut.max() > 0.0
        assert rel < 1e-8, (k, rel)
        assert its == m.its, (k, its, m.its)
        assert np.array_equal(c, g.C1.rhost()[:, 0])  # c_1 <- c
    return S


@pytest.mark.parametrize("guess", [False, True])
@pytest.mark.parametrize("dim,N", [(2, 8), (3, 4)])
def test_steps_match_the_model(hip, dim, N, guess):
    """Three P2-P1 steps with SUPG, Smagorinsky and Sc_t = 0.7 against the model stepped with the device's u_ab and nut:
    relative max difference in c below 1e-8 (the bound of tests/test_gpu_scalar_les.py::test_steps_match_the_model), equal
    iteration counts, c_1 == c."""
    _run_steps(dim, N, guess)


# ---- 5. overshoot --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg", [1, 2])
def test_overshoot_of_the_skew_step(hip, deg):
    """The skew step of demo/supg_front_hip.py at N = 16, kappa = 1e-6, dt = 0.05, 30 degrees, 10 steps (the case in which
    the numpy model shows the reduction on its own: tests/test_scalar_supg_host.py): on the device max(c) - 1 and -min(c)
    with SUPG are both smaller than the Galerkin run's, and the SUPG field equals the model's to 1e-8 relative."""
    from demo.supg_front_hip import NU as nu_demo, skew_solver
    from tests.scalar_supg_model import run_skew
    from tests.test_gpu_scalar import BCGS
    from tests.test_gpu_viscosity import _forms
    from tests.test_scalar_supg_host import SKEW

    out = {}
    for stab in (False, True):
        S = skew_solver(16, deg, SKEW["kappa"], SKEW["angle_deg"], stab, krylov=BCGS)
        for _ in range(SKEW["steps"]):
            S.assemble_first(SKEW["dt"], nu_demo)
            assert all(r > 0 for r in S.scalar_solve().values())
        c = S._scalar_groups[0].C.rhost()[:, 0].copy()
        out[stab] = (c.max() - 1.0, -c.min())
    print(f"P{deg}: Galerkin over/undershoot {out[False]}, SUPG {out[True]}")
    assert out[True][0] < out[False][0] and out[True][1] < out[False][1]
    F, x_v, _ = _forms(S, S._mesh)
    m = run_skew(F, x_v, stabilize=True, options=BCGS, **SKEW)
    rel = np.abs(c - m.c).max() / np.abs(m.c).max()
    print(f"P{deg}: SUPG field against the model: rel diff {rel:.3e}")
    assert rel < 1e-8, rel


# ---- 6. calls made -------------------------------------------------------------------------------------------------------
def test_calls_made(hip, monkeypatch):
    """Without stabilization= neither new entry is called (no model: ox_scalar_rows; Smagorinsky at Sc_t = 0.7:
    ox_scalar_rows_cellvisc).  With stabilization=, Sc_t = 1 or no model: ox_supg_cells and ox_scalar_rows_supg, none of the
    old entries."""
    import oasisx_amd as ox

    for mo, sct, stab, want in ((None, None, None, ["ox_scalar_rows"]),
                                (ox.Smagorinsky(), 0.7, None, ["ox_scalar_rows_cellvisc"]),
                                (None, None, _supg(), list(NEW)),
                                (ox.Smagorinsky(), 1.0, _supg(), list(NEW)),
                                (ox.Smagorinsky(), 0.7, _supg(), list(NEW))):
        clock_c = {"t": 0.0}
        S, clock, mesh = _problem(2, 5, 2, mo, [_scalar(clock_c, KAPPA, sct, stabilization=stab)], NU, DT)
        proxy = _counted(S, monkeypatch)
        _assemble(S, clock, clock_c, DT, NU)
        monkeypatch.undo()
        assert proxy.calls == want, (mo, sct, stab, proxy.calls)
        if stab is not None:
            m = _supg_model(S, mesh, mo, KAPPA, sct, clock_c)
            m.assemble(S._UAB.rhost(), DT)
            _check_against(S, m, DT, f"{mo!r}, Sc_t = {sct}")
        else:
            with pytest.raises(RuntimeError, match="stabilization"):
                S.supg_parameter("T")
    with pytest.raises(RuntimeError, match="scalar_stabilization_assemble"):
        S.scalar_stabilization_assemble(DT, NU)


# ---- 7. groups -----------------------------------------------------------------------------------------------------------
def test_groups(hip, monkeypatch):
    """Two scalars with equal SUPG share a group (one launch pair per assemble_first, both columns equal the model's); another
    scale, or a scalar without stabilisation, opens a group of its own."""
    clock_c = {"t": 0.0}
    mk = lambda n, st: _scalar(clock_c, KAPPA, None, name=n, stabilization=st)  # noqa: E731
    S, clock, mesh = _problem(2, 5, 2, None, [mk("a", _supg()), mk("T", _supg(scale=1.0, time_term=True))], NU, DT)
    assert len(S._scalar_groups) == 1 and S._scalar_groups[0].nc == 2
    proxy = _counted(S, monkeypatch)
    _assemble(S, clock, clock_c, DT, NU)
    monkeypatch.undo()
    assert proxy.calls == list(NEW)
    m = _supg_model(S, mesh, None, KAPPA, None, clock_c)
    m.assemble(S._UAB.rhost(), DT)
    B = S._scalar_groups[0].B.rhost()
    for j in range(2):
        assert np.abs(B[:, j] - m.b).max() <= 1e-12 * np.abs(m.b).max()
    assert abs(S._scalar_groups[0].Ac.to_scipy() - m.A).max() <= 1e-12 * abs(m.A).max()
    S, _, _ = _problem(2, 5, 2, None, [mk("a", _supg()), mk("b", _supg(scale=0.5)), mk("c", None),
                                       mk("d", _supg(time_term=False)), mk("e", _supg())], NU, DT)
    assert [[x.name for x in g.members] for g in S._scalar_groups] == [["a", "e"], ["b"], ["c"], ["d"]]


# ---- 8. combinations -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_blocks", [False, True])
@pytest.mark.parametrize("dim,N,deg", [(2, 6, 2), (3, 4, 2)])
def test_periodic_box(hip, dim, N, deg, row_blocks):
    """The make_periodic box: check 1 against the model on the reduced space (every face is identified: the wrap-around rows
    gather cells from both sides of the seam), by width bins and by row blocks."""
    import oasisx_amd as ox
    from tests.scalar_supg_model import ScalarSupgModel
    from tests.test_gpu_periodic import _forms, _perturbed_tg, _set_fields, _solver, _tg_mesh
    from tests.test_gpu_scalar import _options

    sct = 0.7
    mo = ox.Smagorinsky()
    src = lambda x: 0.5 + x[0]  # noqa: E731
    ini = lambda x: np.cos(np.pi * x[0]) * np.cos(np.pi * x[1]) + 0.2 * np.sin(np.pi * x[dim - 1])  # noqa: E731
    sc = ox.ScalarTransport("T", diffusivity=KAPPA, source=src, initial=ini, turbulent_schmidt=sct, stabilization=_supg())
    opts = {"assemble_row_blocks": row_blocks}
    S = _solver(_tg_mesh(dim, N), deg, solver_options=_options(guess=True), options=opts, scalars=[sc], viscosity_model=mo)
    assert S._row_blocks == row_blocks and (not row_blocks or S._Vi[0][0].pattern.n_row_blocks > 0)
    fns, p_fn = _perturbed_tg(dim, NU)
    _set_fields(S, None, fns, p_fn)
    F, x_v, _ = _forms(S)
    m = ScalarSupgModel(F, x_v, KAPPA, turbulent_schmidt=sct, model=("smagorinsky", mo.coefficient), source=src)
    m.interpolate(ini)
    S.assemble_first(DT, NU)
    m.assemble(S._UAB.rhost(), DT)
    _check_against(S, m, DT, f"periodic ({dim},{N},{deg})")


def test_robin_open_boundary(hip):
    """RobinBC(h = 0, advective = 1), the open-boundary condition, beside SUPG.  On the face x = 1, where the test field
    only leaves the domain, the pass adds nothing: A_c and b_c are the bits of the run without the condition.  On y = -1,
    with inflow and outflow, it follows the stabilised rows and adds to A_c and b_c what it adds to the Galerkin rows (the
    differences agree to 1e-12 max|.|: the pass reads c_1, u_ab and the facets, not the rows).  A Robin group hands no
    A_c c_1 on."""
    import oasisx_amd as ox
    from tests.helpers import tg_mesh
    from tests.test_gpu_scalar import _dofs, bottom
    from tests.test_gpu_scalar_bc import _facets, right

    mesh = tg_mesh(2, 5)
    faces = {"none": None, "right": _facets(mesh, right), "bottom": _facets(mesh, bottom)}
    out = {}
    for stab in (False, True):
        for key, fr in faces.items():
            clock_c = {"t": 0.0}
            fb = [] if fr is None else [ox.RobinBC(0.0, 0.25, fr, advective=1.0)]
            sc = _scalar(clock_c, KAPPA, None, stabilization=_supg() if stab else None, flux_bcs=fb)
            S, clock, _ = _problem(2, 5, 2, None, [sc], NU, DT, mesh=mesh)
            _assemble(S, clock, clock_c, DT, NU)
            g = S._scalar_groups[0]
            assert g.ax0_valid == (fr is None)
            out[stab, key] = (g.Ac.to_scipy(), g.B.rhost()[:, 0].copy())
    x_v, uab = S._Vi[0][0].x.cpu().numpy(), S._UAB.rhost()
    assert uab[_dofs(x_v, right), 0].min() > 0.05  # outflow alone on x = 1
    un = -uab[_dofs(x_v, bottom), 1]
    assert un.min() < -0.05 and un.max() > 0.05  # inflow and outflow along y = -1
    for stab in (False, True):
        assert abs(out[stab, "right"][0] - out[stab, "none"][0]).max() == 0.0
        assert np.array_equal(out[stab, "right"][1], out[stab, "none"][1])
    dA_s, dA_g = (out[stab, "bottom"][0] - out[stab, "none"][0] for stab in (True, False))
    db_s, db_g = (out[stab, "bottom"][1] - out[stab, "none"][1] for stab in (True, False))
    amax, bmax = abs(out[True, "bottom"][0]).max(), np.abs(out[True, "bottom"][1]).max()
    print(f"|dA| = {abs(dA_g).max():.3e} of {amax:.3e}, |db| = {np.abs(db_g).max():.3e} of {bmax:.3e}; SUPG against "
          f"Galerkin: {abs(dA_s - dA_g).max():.3e}, {np.abs(db_s - db_g).max():.3e}")
    assert abs(dA_g).max() > 1e-4 * amax and np.abs(db_g).max() > 1e-4 * bmax
    assert abs(dA_s - dA_g).max() <= 1e-12 * amax
    assert np.abs(db_s - db_g).max() <= 1e-12 * bmax
    assert abs(out[True, "none"][0] - out[False, "none"][0]).max() > 1e-4 * amax  # (the rows ARE stabilised)


def test_one_coupled_step(hip):
    """One whole step with buoyancy=(0, b) beside SUPG (Smagorinsky, Sc_t = 0.7): c against the model stepped with the
    device's u_ab and nut (relative 1e-8, equal iterations), and the force moves the velocity."""
    import torch

    import oasisx_amd as ox
    from tests.test_gpu_scalar import _options

    dt, nu, kappa, sct = 0.005, 0.01, 1e-3, 0.7
    mo = ox.Smagorinsky()
    out = {}
    for b in ((0.0, 3.0), None):
        clock_c = {"t": 0.0}
        src = lambda x: 0.5 + x[0]  # noqa: E731
        sc = _scalar(clock_c, kappa, sct, source=src, buoyancy=b, reference=0.5, stabilization=_supg())
        S, clock, mesh = _problem(2, 8, 2, mo, [sc], nu, dt, perturb=0.05)
        m = _supg_model(S, mesh, mo, kappa, sct, clock_c, options=_options(guess=True)["scalar_transport"], source=src)
        clock["t"] = clock_c["t"] = dt
        S.solve(dt, nu, max_iter=1)
        m.step(S._UAB.rhost(), dt, nut=S._nut.cpu().numpy())
        c = S._scalar_groups[0].C.rhost()[:, 0]
        rel = np.abs(c - m.c).max() / np.abs(m.c).max()
        its = S.iteration_counts()["scalar_transport"]["T"]
        print(f"b = {b}: rel diff {rel:.3e}, iterations {its} (model {m.its})")
        assert m.reason > 0 and rel < 1e-8 and its == m.its
        out[b is None] = S._U.rdev().clone()
    assert not torch.equal(out[False], out[True])


def test_drag_beside_supg(hip):
    """A drag zone changes A after the scalars' operators were taken from it: A_c and b_c of the stabilised scalar are the
    bits of the run without drag."""
    import torch

    import oasisx_amd as ox

    out = []
    for drag in (False, True):
        clock_c = {"t": 0.0}
        kw = {"drag": ox.DragZone(lambda x: x[0] > 0.0, darcy=3.0, forchheimer=1.5)} if drag else {}
        S, clock, _ = _problem(2, 5, 2, None, [_scalar(clock_c, KAPPA, None, stabilization=_supg())], NU, DT, **kw)
        _assemble(S, clock, clock_c, DT, NU)
        g = S._scalar_groups[0]
        out.append((g.Ac.vals.clone(), g.B.rdev().clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ---- 9. bit-identity and refusals ----------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical(hip):
    import torch

    a, b = (_run_steps(3, 4, True, check=False) for _ in range(2))
    for x, y in ((a._scalar_groups[0].C, b._scalar_groups[0].C), (a._U, b._U), (a._P, b._P)):
        assert torch.equal(x.rdev(), y.rdev())
    assert torch.equal(a._scalar_groups[0].Ac.vals, b._scalar_groups[0].Ac.vals)
    assert torch.equal(a._scalar_groups[0].supg_rec, b._scalar_groups[0].supg_rec)


def test_kernels_refuse_bad_arguments(hip):
    """The argument checks of ox_scalar_rows_supg (those of its sibling) and of ox_supg_cells."""
    import ctypes as C

    import oasisx_amd as ox
    from oasisx_amd import _lib

    clock_c = {"t": 0.0}
    S, clock, _ = _problem(2, 4, 2, ox.CellViscosity(0.1), [_scalar(clock_c, 0.2, 0.7, stabilization=_supg())], 0.5, 0.1)
    _assemble(S, clock, clock_c, 0.1, 0.5)
    g, Vi, lib, st = S._scalar_groups[0], S._Vi[0][0], S._lib, _lib.current_stream()

    def rows(Ac=None, nut=True, rec=True, fh=True, dt=0.1, ncomp=1, row_blocks=0, A=None):
        return lib.ox_scalar_rows_supg(C.byref(S._cells), C.byref(Vi.assembly_info()), (A or S._A).ref(), S._M.ref(),
                                       S._K.ref(), (Ac or g.Ac).ref(), _lib.ptr(S._nut) if nut else None,
                                       _lib.ptr(g.supg_rec) if rec else None, 0.1, -0.2, dt, ncomp, g.C1.rptr(), g.B0.rptr(),
                                       g.FH.rptr() if fh else None, g.B.ptr(), None, row_blocks, st)

    assert rows() == 0 and rows(nut=False) == 0  # (nut is optional: no model, or t = 0)
    for kw, text in ((dict(rec=False), "null argument"), (dict(fh=False), "null argument"),
                     (dict(Ac=S._A), "value array of its own"), (dict(dt=0.0), "dt="), (dict(ncomp=0), "ncomp="),
                     (dict(ncomp=4), "ncomp="), (dict(row_blocks=2), "row_blocks="),
                     (dict(A=S._Ap), "share one sparsity pattern")):
        assert rows(**kw) != 0, kw
        msg = lib.ox_last_error().decode()
        assert text in msg and "ox_scalar_rows_supg" in msg, (kw, msg)

    def cells(uab=True, rec=True, dt=0.1, scale=1.0, kappa=0.2, degree=None):
        return lib.ox_supg_cells(Vi.degree if degree is None else degree, C.byref(S._cells), _lib.ptr(Vi.cell_dofs),
                                 S._UAB.rptr() if uab else None, _lib.ptr(S._nut), kappa, 1.0 / 0.7, dt, scale, 1,
                                 _lib.ptr(g.supg_rec) if rec else None, st)

    assert cells() == 0
    for kw, text in ((dict(uab=False), "null argument"), (dict(rec=False), "null argument"), (dict(dt=0.0), "dt="),
                     (dict(dt=-1.0), "dt="), (dict(scale=0.0), "scale="), (dict(kappa=-1.0), "kappa="),
                     (dict(degree=4), "unsupported")):
        assert cells(**kw) != 0, kw
        msg = lib.ox_last_error().decode()
        assert text in msg and "ox_supg_cells" in msg, (kw, msg)


def test_a_velocity_that_is_not_finite_shows(hip):
    """A NaN in u_ab gives tau = NaN in the cells that hold the dof (shown, not clipped), finite values elsewhere."""
    import torch

    clock_c = {"t": 0.0}
    S, clock, _ = _problem(2, 5, 1, None, [_scalar(clock_c, KAPPA, None, stabilization=_supg())], NU, DT)
    S._U1.dev()[7, 0] = float("nan")
    _assemble(S, clock, clock_c, DT, NU)
    g = S._scalar_groups[0]
    tau = g.supg_rec[-1]
    holds = (S._Vi[0][0].cell_dofs.to(torch.int64) == 7).any(dim=1)
    assert bool(holds.any()) and bool(torch.isnan(tau[holds]).all()) and bool(torch.isfinite(tau[~holds]).all())


def test_expression_source_is_refused(hip):
    import oasisx_amd as ox
    from oasisx_amd.function import Expression

    S, _, _ = _problem(2, 4, 2, None, None, NU, DT)
    e = Expression(lambda x, u: 1.0 + u, S._u1[0])
    with pytest.raises(NotImplementedError, match="Expression"):
        ox.ScalarTransport("T", diffusivity=KAPPA, source=e, stabilization=_supg())
    with pytest.raises(TypeError, match="stabilization"):
        ox.ScalarTransport("T", diffusivity=KAPPA, stabilization="supg")


# ---- 10. the demo --------------------------------------------------------------------------------------------------------
def test_demo(hip, capsys):
    """demo/supg_front_hip.py at its smallest size: finite extrema with and without stabilisation, finite L2 errors of the
    rotating cone and their measured orders."""
    from demo.supg_front_hip import main

    res = main(["-N", "8", "--steps", "4", "--cone-sizes", "4", "8", "--cone-steps", "4"])
    out = capsys.readouterr().out
    assert "Galerkin" in out and "SUPG" in out and "order" in out
    vals = [v for k in ("galerkin", "supg") for v in res["front"][k]] + [r["error"] for r in res["cone"]] + res["orders"]
    assert len(res["cone"]) == 2 and len(res["orders"]) == 1
    assert all(np.isfinite(v) for v in vals), res
