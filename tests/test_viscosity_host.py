"""CPU: the numpy model of the eddy-viscosity step (tests/viscosity_model.py) pinned by identities and closed forms, and
the scope guards of ``viscosity_model=``, which sit in front of the library load.  tests/test_gpu_viscosity.py checks the
device against this model."""
import numpy as np
import pytest

from oracle import ipcs_oracle as O
from tests import viscosity_model as VM

LU = {k: {"ksp_type": "preonly", "pc_type": "lu"} for k in ("tentative", "pressure", "scalar")}
CASES = [(2, 6, 1), (2, 5, 2), (3, 3, 1), (3, 3, 2), (2, 4, 3), (3, 2, 3)]




@pytest.mark.parametrize("dim,N,deg", CASES)
def test_unit_weights_give_the_stiffness_matrix(dim, N, deg):
    F = VM.tg_forms(dim, N, deg, 2 if deg == 3 else 1)
    K = F.stiffness_v()
    Kw = VM.weighted_stiffness(F, np.ones(F.cells.shape[0]))
    assert abs(Kw - K).max() <= 1e-14 * abs(K).max()


@pytest.mark.parametrize("dim,N,deg", CASES)
def test_weighted_stiffness_is_symmetric_with_zero_row_sums(dim, N, deg):
    F = VM.tg_forms(dim, N, deg, 2 if deg == 3 else 1)
    rng = np.random.default_rng(3)
    Kw = VM.weighted_stiffness(F, rng.uniform(0.0, 2.0, F.cells.shape[0]))
    scale = abs(Kw).max()
    assert abs(Kw - Kw.T).max() <= 1e-14 * scale
    assert np.abs(Kw @ np.ones(F.nv)).max() <= 1e-12 * scale  # a constant has no gradient in any cell


@pytest.mark.parametrize("dim,N,deg", CASES)
def test_smagorinsky_on_a_linear_field_is_the_closed_form(dim, N, deg):
    """u = A x lies in every Lagrange space: grad u = A in every cell, nut_c = (Cs Delta_c)^2 sqrt(2 S:S)."""
    F = VM.tg_forms(dim, N, deg, 2 if deg == 3 else 1)
    A = np.array([[0.3, -1.1, 0.4], [0.7, 0.2, -0.5], [-0.6, 0.9, -0.8]])[:dim, :dim]
    u = F.x_v @ A.T
    g = VM.centroid_gradient(F, u)
    assert np.abs(g - A[None]).max() <= 1e-13
    nut = VM.nut_cells(F, u, ("smagorinsky", 0.17))
    ref = VM.smagorinsky_closed_form(F, A, 0.17)
    assert np.abs(nut - ref).max() <= 1e-13 * ref.max()
    vol = F.adet / (2.0 if dim == 2 else 6.0)
    assert np.abs(VM.delta2(F) - vol ** (2.0 / dim)).max() <= 1e-15


@pytest.mark.parametrize("deg", [1, 2])
def test_wale_vanishes_exactly_in_pure_shear(deg):
    """u = (gamma y, 0, 0): g g = 0, so Sd = 0 and nut = 0 -- exactly: on this mesh (h = 1/2) with gamma = 2 every number
    of the evaluation is a dyadic rational and the centroid derivatives of P1 / P2 tetrahedra are 0 and 1."""
    F = VM.tg_forms(3, 4, deg)
    u = np.zeros((F.nv, 3))
    u[:, 0] = 2.0 * F.x_v[:, 1]
    nut = VM.nut_cells(F, u, ("wale", 0.325))
    assert (nut == 0.0).all()
    assert (VM.nut_cells(F, u, ("smagorinsky", 0.17)) > 0.0).all()  # (the shear itself is there)
    assert (VM.nut_cells(F, np.zeros((F.nv, 3)), ("wale", 0.325)) == 0.0).all()  # 0 / 0 -> 0


@pytest.mark.parametrize("deg", [1, 2, 3])
def test_wale_in_solid_body_rotation_is_the_closed_form(deg):
    """u = omega e_z x r: S = 0, g g = diag(-omega^2, -omega^2, 0), Sd:Sd = 2 omega^4 / 3 and
    nut = (Cw Delta)^2 (Sd:Sd)^(3/2 - 5/4) = (Cw Delta)^2 (2/3)^(1/4) omega."""
    F = VM.tg_forms(3, 3, deg, 2 if deg == 3 else 1)
    om, Cw = 1.7, 0.325
    u = np.zeros((F.nv, 3))
    u[:, 0], u[:, 1] = -om * F.x_v[:, 1], om * F.x_v[:, 0]
    nut = VM.nut_cells(F, u, ("wale", Cw))
    ref = Cw ** 2 * VM.delta2(F) * (2.0 / 3.0) ** 0.25 * om
    assert np.abs(nut - ref).max() <= 1e-12 * ref.max()


def test_wale_is_three_dimensional_in_the_model():
    F = VM.tg_forms(2, 3, 1)
    with pytest.raises(ValueError):
        VM.nut_cells(F, np.zeros((F.nv, 2)), ("wale", 0.3))


@pytest.mark.parametrize("dim,N,deg", [(2, 6, 2), (3, 3, 2), (2, 4, 1)])
def test_constant_cell_viscosity_is_a_shift_of_nu(dim, N, deg):
    """K_w(c) = c K: the model step with CellViscosity(c) at nu is the plain oracle step at nu + c."""
    F = VM.tg_forms(dim, N, deg)
    nu, c, dt = 0.01, 0.035, 0.005
    A, _ = VM.tg_step_model(F, F.x_v, F.x_q, ("cell", c), nu=nu, dt=dt, solver_options=LU)
    B, _ = VM.tg_step_model(F, F.x_v, F.x_q, None, nu=nu, dt=dt, solver_options=LU)
    # (the boundary data of both is the Taylor-Green field at nu: only the operator differs)
    for k in range(2):
        A.solve(dt, nu, max_iter=1)
        B.solve(dt, nu + c, max_iter=1)
        assert abs(A.A - B.A).max() <= 1e-13 * abs(B.A).max()
        assert np.abs(A.b_first - B.b_first).max() <= 1e-12 * np.abs(B.b_first).max()
        assert np.abs(A.u1 - B.u1).max() <= 1e-11 and np.abs(A.p - B.p).max() <= 1e-10
    assert np.array_equal(A.nut, np.full(F.cells.shape[0], c))


def test_model_without_a_model_is_the_oracle():
    F = VM.tg_forms(2, 5, 2)
    A, ca = VM.tg_step_model(F, F.x_v, F.x_q, None, solver_options=LU)
    B, cb = O.taylor_green_problem(5, 2, solver_options=LU)
    for k in range(2):
        ca["t"] = cb["t"] = (k + 1) * 0.005
        A.solve(0.005, 0.01, max_iter=1)
        B.solve(0.005, 0.01, max_iter=1)
    assert np.array_equal(A.u1, B.u1) and np.array_equal(A.p, B.p)


def test_smagorinsky_dissipates_in_the_model():
    """3-D Taylor-Green, five steps: (1/2) u^T M u with Smagorinsky is strictly below the run without a model (the GPU
    test asserts the same inequality on the same mesh)."""
    d = VM.DISSIPATION
    F = VM.tg_forms(d["dim"], d["N"], d["deg"])
    e0, _ = VM.run_energy(F, F.x_v, F.x_q, None, d["steps"], d["nu"], d["dt"], LU)
    e1, S = VM.run_energy(F, F.x_v, F.x_q, ("smagorinsky", d["Cs"]), d["steps"], d["nu"], d["dt"], LU)
    print(f"kinetic energy after {d['steps']} steps: {e0:.12e} without, {e1:.12e} with Smagorinsky; "
          f"nut in [{S.nut.min():.3e}, {S.nut.max():.3e}]")
    assert S.nut.min() >= 0.0 and S.nut.max() > 0.0
    assert e1 < e0


# ---- the public classes and the scope guards (no library call is reached) ---------------------------------------------
def _cpu_mesh(dim, N=3):
    from tests.helpers import tg_mesh

    return tg_mesh(dim, N, device="cpu")


def _build(mesh, **kw):
    import oasisx_amd as ox
    from tests.helpers import KRYLOV

    dim = mesh.geometry.dim
    return ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_u=[[] for _ in range(dim)], bcs_p=[],
                                   solver_options=KRYLOV, **kw)


def test_models_are_exported_with_their_defaults():
    import oasisx_amd as ox

    assert ox.Smagorinsky().coefficient == 0.1677 and ox.Wale().coefficient == 0.325
    assert {"Smagorinsky", "Wale", "CellViscosity"} <= set(ox.__all__)
    with pytest.raises(ValueError):
        ox.Smagorinsky(Cs=-0.1)


def test_guards_raise_before_the_library_is_needed(monkeypatch):
    import oasisx_amd as ox
    from oasisx_amd import _lib
    from oasisx_amd.parallel import Comm

    def no_library():
        raise AssertionError("the guards run before the library is loaded")

    monkeypatch.setattr(_lib, "load", no_library)
    with pytest.raises(NotImplementedError, match="rotational"):
        _build(_cpu_mesh(2), viscosity_model=ox.Smagorinsky(), rotational=True)
    with pytest.raises(NotImplementedError, match="scalars"):
        _build(_cpu_mesh(2), viscosity_model=ox.Smagorinsky(), scalars=[ox.ScalarTransport("T", diffusivity=0.1)])
    pmesh = _cpu_mesh(2)
    pmesh.comm = Comm(0, 2, None, transport="host")
    with pytest.raises(NotImplementedError, match="partition"):
        _build(pmesh, viscosity_model=ox.Smagorinsky())
    with pytest.raises(ValueError, match="three-dimensional"):
        _build(_cpu_mesh(2), viscosity_model=ox.Wale())
    with pytest.raises(TypeError):
        _build(_cpu_mesh(2), viscosity_model="smagorinsky")


def test_cell_viscosity_values_and_negative_values():
    import oasisx_amd as ox

    mesh = _cpu_mesh(3, 2)
    nc = int(mesh.num_cells)
    cen = mesh.coords[mesh.cells.long()].mean(dim=1).numpy()
    assert np.array_equal(ox.CellViscosity(0.25).values(mesh), np.full(nc, 0.25))
    v = ox.CellViscosity(lambda x: 4.0 + x[0] + 2.0 * x[2]).values(mesh)
    assert np.abs(v - (4.0 + cen[:, 0] + 2.0 * cen[:, 2])).max() <= 1e-15
    arr = np.linspace(0.0, 1.0, nc)
    assert np.array_equal(ox.CellViscosity(arr).values(mesh), arr)
    with pytest.raises(ValueError):
        ox.CellViscosity(-1e-3)
    with pytest.raises(ValueError):
        ox.CellViscosity(-arr)
    with pytest.raises(ValueError):
        ox.CellViscosity(arr[:-1]).values(mesh)
    with pytest.raises(ValueError, match=">= 0"):  # a callable is evaluated when the solver is built: still before the library
        _build(mesh, viscosity_model=ox.CellViscosity(lambda x: x[0]))
