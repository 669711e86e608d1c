"""Host: scalars under a viscosity model (``ScalarTransport(turbulent_schmidt=...)``): the guards,
the grouping and the numpy model of tests/scalar_les_model.py that the GPU tests compare the device with (no GPU)."""
import numpy as np
import pytest

INF = float("inf")


def _cpu_mesh(dim, N=3):
    from tests.helpers import tg_mesh

    return tg_mesh(dim, N, device="cpu")


def _build(mesh, **kw):
    import oasisx_amd as ox
    from tests.helpers import KRYLOV

    dim = mesh.geometry.dim
    return ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_u=[[] for _ in range(dim)], bcs_p=[],
                                   solver_options=KRYLOV, **kw)


def test_guards_raise_before_the_library_is_needed(monkeypatch):
    import oasisx_amd as ox
    from oasisx_amd import _lib

    def no_library():
        raise AssertionError("the guards run before the library is loaded")

    monkeypatch.setattr(_lib, "load", no_library)
    # no default: a model and a scalar without a turbulent Schmidt number
    with pytest.raises(NotImplementedError, match="scalars") as e:
        _build(_cpu_mesh(2), viscosity_model=ox.Smagorinsky(), scalars=[ox.ScalarTransport("T", diffusivity=0.1)])
    assert "turbulent_schmidt=" in str(e.value)
    with pytest.raises(NotImplementedError, match="turbulent_schmidt="):
        _build(_cpu_mesh(2), viscosity_model=ox.CellViscosity(0.1),
               scalars=[ox.ScalarTransport("a", diffusivity=0.1, turbulent_schmidt=0.7), ox.ScalarTransport("b", schmidt=1.0)])
    # a law's nut does not diffuse scalars: only inf
    law = ox.CarreauYasuda(nu0=0.056, nu_inf=0.0035, lam=3.313, n=0.3568)
    for sct in (0.7, 1.0):
        with pytest.raises(ValueError, match="inf"):
            _build(_cpu_mesh(2), viscosity_model=law, scalars=[ox.ScalarTransport("T", diffusivity=0.1, turbulent_schmidt=sct)])
    for law in (ox.Cross(0.05, 0.003, 1.0, 0.8), ox.PowerLaw(0.01, 0.7, 1e-3, 1.0)):
        with pytest.raises(ValueError, match="momentum"):
            _build(_cpu_mesh(2), viscosity_model=law, scalars=[ox.ScalarTransport("T", diffusivity=0.1, turbulent_schmidt=2.0)])
    # with an accepted value the guards pass and the constructor goes on to the library
    for model, sct in ((ox.Smagorinsky(), 0.7), (ox.Smagorinsky(), INF), (ox.CellViscosity(0.1), 1.0),
                       (ox.CarreauYasuda(nu0=0.056, nu_inf=0.0035, lam=3.313, n=0.3568), INF)):
        with pytest.raises(AssertionError, match="before the library"):
            _build(_cpu_mesh(2), viscosity_model=model, scalars=[ox.ScalarTransport("T", diffusivity=0.1, turbulent_schmidt=sct)])
    # rotational=True and partitions stay refused
    with pytest.raises(NotImplementedError, match="rotational"):
        _build(_cpu_mesh(2), viscosity_model=ox.Smagorinsky(), rotational=True,
               scalars=[ox.ScalarTransport("T", diffusivity=0.1, turbulent_schmidt=0.7)])


@pytest.mark.parametrize("bad", [0.0, -0.7, float("nan"), -INF, "x", (1.0, 2.0)])
def test_bad_turbulent_schmidt_values(bad):
    import oasisx_amd as ox

    with pytest.raises(ValueError, match="turbulent_schmidt"):
        ox.ScalarTransport("T", diffusivity=0.1, turbulent_schmidt=bad)


def test_accepted_values_and_the_models_attribute():
    import oasisx_amd as ox

    assert ox.ScalarTransport("T", diffusivity=0.1).turbulent_schmidt is None
    assert ox.ScalarTransport("T", diffusivity=0.1, turbulent_schmidt=0.7).turbulent_schmidt == 0.7
    s = ox.ScalarTransport("T", schmidt=2.0, turbulent_schmidt=INF)
    assert s.turbulent_schmidt == INF and s.inverse_turbulent_schmidt() == 0.0
    assert ox.ScalarTransport("T", diffusivity=0.1, turbulent_schmidt=4).inverse_turbulent_schmidt() == 0.25
    for m in (ox.Smagorinsky(), ox.Smagorinsky(damping=ox.VanDriest()), ox.Wale(), ox.CellViscosity(0.1)):
        assert m.diffuses_scalars is True
    for m in (ox.CarreauYasuda(0.056, 0.0035, 3.313, 0.3568), ox.Cross(0.05, 0.003, 1.0, 0.8), ox.PowerLaw(0.01, 0.7, 1e-3, 1.0)):
        assert m.diffuses_scalars is False


def test_group_key_separates_the_turbulent_schmidt_number():
    import oasisx_amd as ox

    a = ox.ScalarTransport("a", diffusivity=0.1, turbulent_schmidt=0.7)
    b = ox.ScalarTransport("b", diffusivity=0.1, turbulent_schmidt=0.9)
    c = ox.ScalarTransport("c", diffusivity=0.1, turbulent_schmidt=0.7)
    d = ox.ScalarTransport("d", diffusivity=0.1)
    e = ox.ScalarTransport("e", diffusivity=0.1, turbulent_schmidt=INF)
    assert a._spec() == c._spec()
    assert len({a._spec(), b._spec(), d._spec(), e._spec()}) == 4
    assert ox.ScalarTransport("f", schmidt=0.1, turbulent_schmidt=0.7)._spec() != a._spec()


@pytest.mark.parametrize("dim,N,deg", [(2, 4, 2), (3, 2, 1)])
def test_constant_nut_is_a_shifted_diffusivity(dim, N, deg):
    """nut = c in every cell: the model equals ScalarModel at kappa + c / Sc_t, to 1e-13 max|.|."""
    from tests import viscosity_model as VM
    from tests.scalar_les_model import ScalarLesModel
    from tests.scalar_model import ScalarModel, tg_uab

    F = VM.tg_forms(dim, N, deg)
    kappa, c, sct, dt = 0.03, 0.37, 0.7, 0.1
    bd = np.nonzero(np.isclose(F.x_v[:, 0], -1.0))[0]
    kw = dict(dofs=bd, value=lambda x: 1.0 + x[1], source=lambda x: 1.0 + x[0] * x[1])
    ini = lambda x: np.cos(2.0 * x[0]) + 0.5 * x[1]  # noqa: E731
    uab = tg_uab(F.x_v, dt, dt, 0.01)
    les = ScalarLesModel(F, F.x_v, kappa, sct, model=("cell", c), **kw)
    ref = ScalarModel(F, F.x_v, kappa + c / sct, **kw)
    les.interpolate(ini)
    ref.interpolate(ini)
    A, b = les.assemble(uab, dt)
    A0, b0 = ref.assemble(uab, dt)
    assert abs(A - A0).max() <= 1e-13 * abs(A0).max()
    assert np.abs(b - b0).max() <= 1e-13 * np.abs(b0).max()
    # inf: no turbulent part at all
    A, b = ScalarLesModel(F, F.x_v, kappa, INF, model=("cell", c), **kw).assemble(uab, dt)
    A0, b0 = ScalarModel(F, F.x_v, kappa, **kw).assemble(uab, dt)
    assert abs(A - A0).max() == 0.0 and np.abs(b - b0).max() == 0.0


def test_turbulent_diffusivity_lowers_the_scalar_variance():
    """The 3-D Taylor-Green set-up of viscosity_model.DISSIPATION, the scalar advected by the model's own u_ab with the
    Smagorinsky nut of that velocity: c^T M c after the steps is strictly lower with Sc_t = 0.5 than with inf."""
    from tests import viscosity_model as VM
    from tests.scalar_les_model import ScalarLesModel

    D = VM.DISSIPATION
    F = VM.tg_forms(D["dim"], D["N"], D["deg"])
    model = ("smagorinsky", D["Cs"])
    ini = lambda x: np.cos(np.pi * x[0]) * np.cos(np.pi * x[1]) + 0.3 * np.sin(np.pi * x[2])  # noqa: E731
    var = {}
    for sct in (0.5, INF):
        S, clock = VM.tg_step_model(F, F.x_v, F.x_q, model, nu=D["nu"], dt=D["dt"])
        m = ScalarLesModel(F, F.x_v, 0.001, sct, model=model, options={"ksp_rtol": 1e-12, "ksp_atol": 1e-30})
        m.interpolate(ini)
        for k in range(D["steps"]):
            clock["t"] = (k + 1) * D["dt"]
            uab = 1.5 * S.u1 - 0.5 * S.u2
            S.solve(D["dt"], D["nu"], max_iter=1)
            m.step(uab, D["dt"])
            assert m.reason > 0 and m.nut.max() > 0.0
        var[sct] = m.variance()
    print(f"c^T M c: {var[0.5]:.12e} with Sc_t = 0.5, {var[INF]:.12e} with inf")
    assert var[0.5] < var[INF]
