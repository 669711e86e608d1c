"""CPU: the numpy model of the generalised-Newtonian laws and of the full stress form (tests/rheology_model.py) pinned by
identities and closed forms, and the constructor / scope guards, which sit in front of the library load.
tests/test_gpu_rheology.py checks the device against this model."""
import numpy as np
import pytest

from oracle import ipcs_oracle as O
from tests import rheology_model as RM
from tests import viscosity_model as VM

CASES = [(2, 5, 2), (3, 3, 2), (3, 3, 1), (2, 4, 3), (3, 2, 3)]

CY = ("carreau_yasuda", (0.16, 0.01, 3.313, 0.3568, 2.0))
CROSS = ("cross", (0.16, 0.01, 1.007, 1.028))
PL = ("power_law", (0.05, 0.6, 0.005, 0.5))


def _forms(dim, N, deg):
    return VM.tg_forms(dim, N, deg, 2 if deg == 3 else 1)


# ---- the transposed term -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_rigid_rotation_feels_no_viscous_force_in_the_full_form(dim, N, deg):
    """u = omega x x, random nut per cell in [0.05, 0.1]: grad u + grad u^T = 0, so K_w(nut) u + T vanishes on every row,
    while K_w(nut) u alone -- the Laplacian form -- does not: the pin cannot pass with T = 0."""
    F = _forms(dim, N, deg)
    u = RM.rigid_rotation(F.x_v)
    nut = np.random.default_rng(7).uniform(0.05, 0.1, F.cells.shape[0])
    Ku = VM.weighted_stiffness(F, nut) @ u
    T = RM.transposed_term(F, u, nut)
    print(f"({dim},{N},{deg}): max |K_w u| = {np.abs(Ku).max():.3e}, max |K_w u + T| = {np.abs(Ku + T).max():.3e}")
    assert np.abs(Ku + T).max() <= 1e-14
    assert np.abs(Ku).max() >= 1e-3


@pytest.mark.parametrize("dim,N,deg", CASES)
def test_linear_field_with_constant_nut_lives_on_the_boundary(dim, N, deg):
    """u = A x, nut = 0.3: T[r][i] = 0.3 sum_j A[j][i] int d(phi_r)/dx_j, which vanishes for a basis function that is zero
    on the boundary and not for the others."""
    F = _forms(dim, N, deg)
    A = np.array([[0.3, -1.1, 0.4], [0.7, 0.2, -0.5], [-0.6, 0.9, -0.8]])[:dim, :dim]
    u = F.x_v @ A.T
    T = RM.transposed_term(F, u, np.full(F.cells.shape[0], 0.3))
    bd = O.boundary_dofs(F.x_v, F.coords.min(axis=0), F.coords.max(axis=0))
    interior = np.setdiff1d(np.arange(F.nv), bd)
    print(f"({dim},{N},{deg}): {interior.size} interior rows, max |T| there {np.abs(T[interior]).max():.3e}, "
          f"on the boundary {np.abs(T[bd]).max():.3e}")
    assert interior.size >= 8
    assert np.abs(T[interior]).max() <= 1e-14
    assert np.abs(T[bd]).max() >= 1e-2


def test_transposed_term_is_linear_in_nut_and_in_u():
    F = _forms(2, 5, 2)
    rng = np.random.default_rng(1)
    u, v = rng.normal(size=(F.nv, 2)), rng.normal(size=(F.nv, 2))
    a, b = rng.uniform(0.0, 1.0, F.cells.shape[0]), rng.uniform(0.0, 1.0, F.cells.shape[0])
    T = RM.transposed_term
    assert np.abs(T(F, u, a + 2.0 * b) - T(F, u, a) - 2.0 * T(F, u, b)).max() <= 1e-12
    assert np.abs(T(F, u - 3.0 * v, a) - T(F, u, a) + 3.0 * T(F, v, a)).max() <= 1e-12


def test_full_form_only_changes_the_right_hand_side():
    F = _forms(2, 5, 2)
    model = ("cell", 0.5 * (1.0 + F.coords[F.cells].mean(axis=1)[:, 0] ** 2))
    L, _ = RM.tg_step_model(F, F.x_v, F.x_q, model, "laplacian")
    R, _ = RM.tg_step_model(F, F.x_v, F.x_q, model, "full")
    L.assemble_first(0.005, 0.01)
    R.assemble_first(0.005, 0.01)
    assert abs(L.A - R.A).max() == 0.0
    assert np.array_equal(L.b_first - R.T, R.b_first) and np.abs(R.T).max() >= 1e-2 * np.abs(R.b_first).max()


# ---- the laws ----------------------------------------------------------------------------------------------------------
def _shear(F, gamma):
    u = np.zeros((F.nv, F.d))
    u[:, 0] = gamma * F.x_v[:, 1]
    return u


@pytest.mark.parametrize("dim,N,deg", CASES)
def test_laws_in_simple_shear_are_their_closed_forms(dim, N, deg):
    """u = (gamma y, 0[, 0]): S:S = gamma^2 / 2 in every cell, gd = gamma."""
    F = _forms(dim, N, deg)
    g = 1.7
    u = _shear(F, g)
    assert np.abs(RM.shear_rate(F, u) - g).max() <= 1e-13
    ref = {
        "carreau_yasuda": 0.01 + 0.15 * (1.0 + (3.313 * g) ** 2.0) ** ((0.3568 - 1.0) / 2.0) - 0.01,
        "cross": 0.01 + 0.15 / (1.0 + (1.007 * g) ** 1.028) - 0.01,
        "power_law": min(max(0.05 * g ** (0.6 - 1.0), 0.005), 0.5) - 0.005,
    }
    for model in (CY, CROSS, PL):
        nut = RM.nut_cells(F, u, model)
        assert nut.shape == (F.cells.shape[0],) and np.abs(nut - ref[model[0]]).max() <= 1e-13, model


def test_laws_without_a_time_scale_are_newtonian():
    F = _forms(2, 5, 2)
    u = _shear(F, 2.3)
    nc = F.cells.shape[0]
    # (nu_inf + (nu0 - nu_inf) - base: one rounding of 0.16 away from nu0 - base)
    assert np.abs(RM.nut_cells(F, u, ("carreau_yasuda", (0.16, 0.01, 0.0, 0.3568, 2.0))) - 0.15).max() <= 1e-16
    assert np.abs(RM.nut_cells(F, u, ("cross", (0.16, 0.01, 0.0, 1.028))) - 0.15).max() <= 1e-16
    # shear-thickening parameters: the base is nu0
    assert np.abs(RM.nut_cells(F, u, ("cross", (0.01, 0.16, 0.0, 1.0)))).max() <= 1e-16
    # n = 1: k, clipped
    for k, clipped in ((0.05, 0.05), (1.0, 0.5), (0.001, 0.005)):
        nut = RM.nut_cells(F, u, ("power_law", (k, 1.0, 0.005, 0.5)))
        assert np.array_equal(nut, np.full(F.cells.shape[0], clipped - 0.005))


def test_power_law_at_rest():
    F = _forms(3, 3, 1)
    u = np.zeros((F.nv, 3))
    nc = F.cells.shape[0]
    assert np.array_equal(RM.nut_cells(F, u, ("power_law", (0.05, 0.6, 0.005, 0.5))), np.full(nc, 0.5 - 0.005))
    assert np.array_equal(RM.nut_cells(F, u, ("power_law", (0.05, 1.4, 0.005, 0.5))), np.zeros(nc))
    assert np.array_equal(RM.nut_cells(F, u, ("power_law", (0.05, 1.0, 0.005, 0.5))), np.full(nc, 0.05 - 0.005))
    assert np.isfinite(RM.law_viscosity(("power_law", (0.05, 0.6, 0.005, 0.5)), np.array([0.0, 1e-300, 1e300]))).all()


@pytest.mark.parametrize("model", [CY, CROSS, PL])
def test_shear_thinning_is_monotone(model):
    gd = np.concatenate([[0.0], np.logspace(-6, 6, 400)])
    nu = RM.law_viscosity(model, gd)
    assert (np.diff(nu) <= 0.0).all() and nu[0] > nu[-1]
    assert (nu - RM.base_viscosity(model) >= 0.0).all()


# ---- the public classes and the guards (no library call is reached) ----------------------------------------------------
def _cpu_mesh(dim, N=3):
    from tests.helpers import tg_mesh

    return tg_mesh(dim, N, device="cpu")


def _build(mesh, **kw):
    import oasisx_amd as ox
    from tests.helpers import KRYLOV

    dim = mesh.geometry.dim
    return ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_u=[[] for _ in range(dim)], bcs_p=[],
                                   solver_options=KRYLOV, **kw)


def test_laws_are_exported_with_their_base_viscosity():
    import oasisx_amd as ox

    assert {"CarreauYasuda", "Cross", "PowerLaw"} <= set(ox.__all__)
    cy = ox.CarreauYasuda(nu0=0.16, nu_inf=0.01, lam=3.313, n=0.3568)
    assert cy.a == 2.0 and cy.base_viscosity == 0.01 and cy.params == (0.16, 0.01, 3.313, 0.3568, 2.0)
    assert ox.CarreauYasuda(0.01, 0.16, 1.0, 1.5).base_viscosity == 0.01
    assert ox.Cross(0.16, 0.02, 1.0, 1.0).base_viscosity == 0.02
    assert ox.PowerLaw(0.05, 0.6, 0.005, 0.5).base_viscosity == 0.005
    for m, t in ((cy, CY), (ox.Cross(*CROSS[1]), CROSS), (ox.PowerLaw(*PL[1]), PL)):
        assert m.base_viscosity == RM.base_viscosity(t) and tuple(m.params) == t[1]


def test_constructor_guards():
    import oasisx_amd as ox

    nan, inf = float("nan"), float("inf")
    bad = [
        lambda: ox.CarreauYasuda(nan, 0.01, 1.0, 0.5), lambda: ox.CarreauYasuda(0.1, inf, 1.0, 0.5),
        lambda: ox.CarreauYasuda(0.1, 0.01, nan, 0.5), lambda: ox.CarreauYasuda(0.1, 0.01, 1.0, inf),
        lambda: ox.CarreauYasuda(0.1, 0.01, 1.0, 0.5, a=nan),
        lambda: ox.CarreauYasuda(-0.1, 0.01, 1.0, 0.5), lambda: ox.CarreauYasuda(0.1, -0.01, 1.0, 0.5),
        lambda: ox.CarreauYasuda(0.1, 0.01, -1.0, 0.5), lambda: ox.CarreauYasuda(0.1, 0.01, 1.0, 0.0),
        lambda: ox.CarreauYasuda(0.1, 0.01, 1.0, -0.5), lambda: ox.CarreauYasuda(0.1, 0.01, 1.0, 0.5, a=0.0),
        lambda: ox.Cross(nan, 0.01, 1.0, 1.0), lambda: ox.Cross(0.1, 0.01, 1.0, inf),
        lambda: ox.Cross(-0.1, 0.01, 1.0, 1.0), lambda: ox.Cross(0.1, -0.01, 1.0, 1.0),
        lambda: ox.Cross(0.1, 0.01, -1.0, 1.0), lambda: ox.Cross(0.1, 0.01, 1.0, 0.0), lambda: ox.Cross(0.1, 0.01, 1.0, -1.0),
        lambda: ox.PowerLaw(nan, 0.6, 0.005, 0.5), lambda: ox.PowerLaw(0.05, 0.6, 0.005, inf),
        lambda: ox.PowerLaw(-0.05, 0.6, 0.005, 0.5), lambda: ox.PowerLaw(0.05, 0.0, 0.005, 0.5),
        lambda: ox.PowerLaw(0.05, -0.6, 0.005, 0.5), lambda: ox.PowerLaw(0.05, 0.6, 0.5, 0.005),
        lambda: ox.PowerLaw(0.05, 0.6, 0.0, 0.5), lambda: ox.PowerLaw(0.05, 0.6, -0.005, 0.5),
    ]
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"guard {k} did not raise")


def test_guards_raise_before_the_library_is_needed(monkeypatch):
    import oasisx_amd as ox
    from oasisx_amd import _lib
    from oasisx_amd.parallel import Comm

    def no_library():
        raise AssertionError("the guards run before the library is loaded")

    monkeypatch.setattr(_lib, "load", no_library)
    cy = ox.CarreauYasuda(nu0=0.16, nu_inf=0.01, lam=3.313, n=0.3568)
    with pytest.raises(ValueError, match="stress_form"):
        _build(_cpu_mesh(2), stress_form="full")
    with pytest.raises(ValueError, match="stress_form"):
        _build(_cpu_mesh(2), viscosity_model=cy, stress_form="symmetric")
    with pytest.raises(ValueError, match="stress_form"):
        _build(_cpu_mesh(2), stress_form="Full")
    with pytest.raises(NotImplementedError, match="rotational"):
        _build(_cpu_mesh(2), viscosity_model=cy, rotational=True)
    with pytest.raises(NotImplementedError, match="scalars"):
        _build(_cpu_mesh(2), viscosity_model=ox.PowerLaw(0.05, 0.6, 0.005, 0.5),
               scalars=[ox.ScalarTransport("T", diffusivity=0.1)])
    pmesh = _cpu_mesh(2)
    pmesh.comm = Comm(0, 2, None, transport="host")
    with pytest.raises(NotImplementedError, match="partition"):
        _build(pmesh, viscosity_model=ox.Cross(0.16, 0.01, 1.0, 1.0), stress_form="full")
    # the accepted combinations get past every guard, to the library load
    for kw in (dict(viscosity_model=cy), dict(viscosity_model=cy, stress_form="full"),
               dict(viscosity_model=ox.Smagorinsky(), stress_form="full"), dict(stress_form="laplacian")):
        with pytest.raises(AssertionError, match="before the library"):
            _build(_cpu_mesh(2), **kw)
