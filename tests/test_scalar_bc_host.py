"""No GPU: the numpy model of the scalars' flux and Robin conditions (tests/scalar_bc_model.py) pinned by closed forms and
by tests/outlet_model.backflow_matrix, the construction errors and the grouping rule of ``flux_bcs=``
(oasisx_amd/scalar.py), and the model's own fixed-point drift and conservation defect at the tolerances of the two
physical tests of tests/test_gpu_scalar_bc.py."""
import numpy as np
import pytest

from oracle import ipcs_oracle as O
from tests import outlet_model as OM
from tests import scalar_bc_model as BM

CASES = [(2, 6, 1), (2, 5, 2), (3, 3, 1), (3, 3, 2), (2, 4, 3)]
TIGHT = {"ksp_type": "bcgs", "pc_type": "jacobi", "ksp_rtol": 1e-12, "ksp_atol": 1e-30}


def _forms(dim, N, deg):
    if dim == 2:
        coords, cells = O.create_rectangle_mesh([-1, -1], [1, 1], [N, N])
    else:
        coords, cells = O.create_box_mesh([-1, -1, -1], [1, 1, 1], [N, N, N])
    return O.Forms(coords, cells, deg, 2 if deg == 3 else 1)


def _side(F, axis, sign):
    """(cell, opposite vertex) of the exterior facets on the side x_axis = sign of [-1, 1]^d."""
    fc, fa = F.exterior_facets()
    mid = F.facet_midpoints(fc, fa)
    sel = np.isclose(mid[:, axis], float(sign))
    order = np.lexsort((fa[sel], fc[sel]))
    return fc[sel][order], fa[sel][order]


def _tg_uab(F):
    X = np.zeros((3, F.x_v.shape[0]))
    X[: F.d] = F.x_v.T
    return np.stack([f(X, 0.0, 0.01) for f in [O.tg_u, O.tg_v, O.tg_w][: F.d]], axis=1)


# ---- the model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_model_closed_forms(dim, N, deg):
    """H is symmetric; 1^T H 1 = sum_f |f| h for a constant h; the load of a constant q sums to q |Gamma|; a polynomial
    q of the element's degree is integrated exactly."""
    F = _forms(dim, N, deg)
    fc, fa = _side(F, 0, 1)
    area = 2.0 ** (dim - 1)
    uab = _tg_uab(F)
    rob = BM.Robin(fc, fa, lambda x: 1.0 + x[1] ** 2, lambda x: 0.5 - x[1], beta=0.7)
    H, _, _ = BM.surface_terms(F, F.x_v, rob, uab)
    assert abs(H - H.T).max() <= 1e-15 * abs(H).max()
    H, load, Hadv = BM.surface_terms(F, F.x_v, BM.Robin(fc, fa, 0.3, 2.0), uab)
    assert abs(Hadv).max() == 0.0
    one = np.ones(F.nv)
    assert abs(one @ (H @ one) - 0.3 * area) <= 1e-13 * area
    assert abs(load.sum() - 0.3 * 2.0 * area) <= 1e-13 * area  # hq c_inf
    assert abs(BM.boundary_measure(F, rob) - area) <= 1e-13 * area
    _, load, _ = BM.surface_terms(F, F.x_v, BM.Flux(fc, fa, -1.7), uab)
    assert abs(load.sum() + 1.7 * area) <= 1e-13 * area
    q = (lambda x: 1.0 + 3.0 * x[1] ** deg)  # int over the side: area (1 + 3 mean(y^deg))
    _, load, _ = BM.surface_terms(F, F.x_v, BM.Flux(fc, fa, q), uab)
    mean = 0.0 if deg % 2 else 1.0 / (deg + 1)
    assert abs(load.sum() - area * (1.0 + 3.0 * mean)) <= 1e-13 * area


@pytest.mark.parametrize("dim,N,deg", CASES)
def test_open_boundary_on_a_uniform_outflow_is_exactly_zero(dim, N, deg):
    F = _forms(dim, N, deg)
    fc, fa = _side(F, 0, 1)
    uab = np.zeros((F.nv, dim))
    uab[:, 0] = 1.0  # leaves through x = 1
    H, load = BM.boundary_terms(F, F.x_v, [BM.Robin(fc, fa, 0.0, 3.0, beta=1.0)], uab)
    assert abs(H).max() == 0.0 and np.abs(load).max() == 0.0
    H, load = BM.boundary_terms(F, F.x_v, [BM.Robin(fc, fa, 0.0, 3.0, beta=1.0)], -uab)  # inflow carries c_inf
    area = 2.0 ** (dim - 1)
    assert abs(load.sum() - 3.0 * area) <= 1e-13 * area


@pytest.mark.parametrize("dim,N,deg", CASES)
def test_advective_part_is_the_backflow_matrix(dim, N, deg):
    """The Crank-Nicolson share H_adv / 2 of the model equals (beta / 2) B of tests/outlet_model.py."""
    F = _forms(dim, N, deg)
    fc, fa = _side(F, 1, -1)
    uab = _tg_uab(F)
    beta = 0.7
    _, _, Hadv = BM.surface_terms(F, F.x_v, BM.Robin(fc, fa, 0.4, 1.0, beta=beta), uab)
    B = OM.backflow_matrix(F.coords, F.cells, fc, fa, F.vd, uab, deg, 1.0, F.nv)
    assert abs(B).max() > 0.0
    assert abs(0.5 * Hadv - (0.5 * beta) * B).max() <= 1e-14 * abs(B).max()


def test_conditions_on_one_facet_add():
    F = _forms(2, 4, 2)
    fc, fa = _side(F, 0, 1)
    uab = _tg_uab(F)
    a, b = BM.Robin(fc, fa, 0.3, 1.0, beta=0.2), BM.Robin(fc[:2], fa[:2], 0.5, -2.0)
    H, load = BM.boundary_terms(F, F.x_v, [a, BM.Flux(fc, fa, 0.25), b], uab)
    Ha, la, _ = BM.surface_terms(F, F.x_v, a, uab)
    Hb, lb, _ = BM.surface_terms(F, F.x_v, b, uab)
    _, lq, _ = BM.surface_terms(F, F.x_v, BM.Flux(fc, fa, 0.25), uab)
    assert abs(H - (Ha + Hb)).max() <= 1e-15 and np.abs(load - (la + lb + lq)).max() <= 1e-15


# ---- construction errors -------------------------------------------------------------------------------------------------
def test_construction_errors():
    import oasisx_amd as ox
    from oasisx_amd import mesh as M
    from oasisx_amd.scalar import _nodal
    from tests.helpers import tg_mesh

    mesh = tg_mesh(2, 4, device="cpu")
    ext = np.asarray(mesh.exterior_facets(), dtype=np.int64)
    with pytest.raises(ValueError, match=">= 0"):
        ox.RobinBC(-0.1, 0.0, ext)
    for beta in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="advective"):
            ox.RobinBC(1.0, 0.0, ext, advective=beta)
    with pytest.raises(ValueError, match="finite"):
        ox.FluxBC(float("nan"), ext)
    with pytest.raises(ValueError, match="finite"):
        ox.RobinBC(float("inf"), 0.0, ext)
    with pytest.raises(ValueError, match="finite"):
        ox.RobinBC(1.0, float("inf"), ext)
    X = np.zeros((3, 5))
    X[0] = np.linspace(-1.0, 1.0, 5)
    with pytest.raises(ValueError, match="not finite"):  # a callable: at evaluation
        _nodal("FluxBC", "q", lambda x: np.where(x[0] == 0.0, np.inf, x[0]), X)
    with pytest.raises(ValueError, match=">= 0"):
        _nodal("RobinBC", "h", lambda x: x[0], X, nonneg=True)
    assert np.array_equal(_nodal("RobinBC", "h", 2.0, X, nonneg=True), np.full(5, 2.0))
    interior = np.setdiff1d(np.arange(mesh._entities(1)[0].shape[0]), ext)[:1]
    with pytest.raises(ValueError, match="interior"):
        ox.FluxBC(1.0, np.hstack([ext[:2], interior])).facet_ids(mesh)
    with pytest.raises(ValueError, match="interior"):
        ox.RobinBC(1.0, 0.0, interior).facet_ids(mesh)
    assert np.array_equal(ox.FluxBC(1.0, ext[::-1].copy()).facet_ids(mesh), np.sort(ext))
    per = M.make_periodic(tg_mesh(2, 4, device="cpu"), (0,))
    seam = per.periodic_facets()
    assert seam.shape[0] == 8
    with pytest.raises(ValueError, match="identified"):
        ox.FluxBC(1.0, seam[:2]).facet_ids(per)
    tags = M.meshtags(per, 1, seam, np.full(seam.shape[0], 3, dtype=np.int32))
    with pytest.raises(ValueError, match="identified"):
        ox.RobinBC(1.0, 0.0, (tags, 3)).facet_ids(per)
    with pytest.raises(TypeError, match="FluxBC and RobinBC"):
        ox.ScalarTransport("T", diffusivity=0.1, flux_bcs=[ox.DirichletBC(0.0, ox.LocatorMethod.GEOMETRICAL, lambda x: x[0] < 0)])
    with pytest.raises(TypeError, match="DirichletBC"):  # bcs= stays Dirichlet-only
        ox.ScalarTransport("T", diffusivity=0.1, bcs=[ox.FluxBC(1.0, ext)])
    assert ox.ScalarTransport("T", diffusivity=0.1).flux_bcs == []


# ---- grouping ------------------------------------------------------------------------------------------------------------
def test_grouping_rule():
    """The key gains the matrix-changing part of the conditions: facets, h (a float or the callable's identity) and
    advective.  Equal h / facets with different c_inf: one group; different h: two; FluxBC-only scalars group with plain
    ones."""
    import oasisx_amd as ox
    from oasisx_amd import mesh as M
    from oasisx_amd.scalar import group_key, group_scalars
    from tests.helpers import tg_mesh

    mesh = tg_mesh(2, 4, device="cpu")
    right = M.locate_entities_boundary(mesh, 1, lambda x: np.isclose(x[0], 1.0))
    top = M.locate_entities_boundary(mesh, 1, lambda x: np.isclose(x[1], 1.0))
    hfun = lambda x: 1.0 + x[1] ** 2  # noqa: E731
    T = lambda name, fb: ox.ScalarTransport(name, diffusivity=0.1, flux_bcs=fb)  # noqa: E731

    def groups(scalars):
        rows = np.zeros(0, np.int64)
        keyed = [(group_key(s, rows, mesh)[0], rows, s) for s in scalars]
        return [[m.name for m in members] for _, members in group_scalars(keyed)]

    assert groups([T("a", [ox.RobinBC(0.5, 1.0, right)]), T("b", [ox.RobinBC(0.5, lambda x: x[1], right)])]) == [["a", "b"]]
    assert groups([T("a", [ox.RobinBC(0.5, 1.0, right)]), T("b", [ox.RobinBC(0.6, 1.0, right)])]) == [["a"], ["b"]]
    assert groups([T("a", [ox.RobinBC(hfun, 1.0, right)]), T("b", [ox.RobinBC(hfun, 2.0, right)])]) == [["a", "b"]]
    assert groups([T("a", [ox.RobinBC(hfun, 1.0, right)]),
                   T("b", [ox.RobinBC(lambda x: 1.0 + x[1] ** 2, 1.0, right)])]) == [["a"], ["b"]]
    assert groups([T("a", [ox.RobinBC(0.5, 1.0, right)]), T("b", [ox.RobinBC(0.5, 1.0, top)])]) == [["a"], ["b"]]
    assert groups([T("a", [ox.RobinBC(0.5, 1.0, right)]), T("b", [ox.RobinBC(0.5, 1.0, right, advective=0.5)])]) == [["a"], ["b"]]
    assert groups([T("a", []), T("b", [ox.FluxBC(1.0, right)]), T("c", [ox.FluxBC(lambda x: x[1], top), ox.FluxBC(2.0, right)])]) \
        == [["a", "b", "c"]]
    assert groups([T("a", [ox.FluxBC(1.0, top), ox.RobinBC(0.5, 1.0, right)]), T("b", [ox.RobinBC(0.5, 0.0, right)]),
                   T("c", [])]) == [["a", "b"], ["c"]]
    assert groups([T(f"s{i}", [ox.RobinBC(0.5, float(i), right)]) for i in range(4)]) == [["s0", "s1", "s2"], ["s3"]]


# ---- the two physical tests, on the model ---------------------------------------------------------------------------------
def robin_profile(kappa, h, c_inf):
    """c = 1 + a (x + 1) / 2 on [-1, 1] with c(-1) = 1 and -kappa c' = h (c - c_inf) at x = 1."""
    a = h * (c_inf - 1.0) / (h + 0.5 * kappa)
    return lambda x: 1.0 + a * (x[0] + 1.0) / 2.0


@pytest.mark.parametrize("dim,N,deg", [(2, 8, 1), (2, 8, 2), (2, 4, 3), (3, 4, 2)])
def test_fixed_point_drift_of_the_model(dim, N, deg):
    """Fluid at rest, c = 1 on x = -1, RobinBC on x = 1, nothing elsewhere: the linear profile is a fixed point of the
    discrete step; after three steps at ksp_rtol 1e-12 the model stays within 1e-8 relative (the device test's bound)."""
    kappa, h, c_inf, dt = 0.3, 2.0, -0.5, 0.05
    F = _forms(dim, N, deg)
    fc, fa = _side(F, 0, 1)
    left = np.nonzero(np.isclose(F.x_v[:, 0], -1.0))[0]
    m = BM.ScalarBCModel(F, F.x_v, kappa, dofs=left, value=1.0, options=TIGHT, conditions=[BM.Robin(fc, fa, h, c_inf)])
    prof = robin_profile(kappa, h, c_inf)
    m.interpolate(prof)
    ref = m.c1.copy()
    uab = np.zeros((F.nv, dim))
    for _ in range(3):
        m.step(uab, dt)
        assert m.reason > 0
    drift = np.abs(m.c - ref).max() / np.abs(ref).max()
    print(f"({dim},{N},P{deg}): drift {drift:.3e}")
    assert drift < 1e-8
    # a wrong factor moves it at first order
    bad = BM.ScalarBCModel(F, F.x_v, kappa, dofs=left, value=1.0, options=TIGHT, conditions=[BM.Robin(fc, fa, 0.5 * h, c_inf)])
    bad.interpolate(prof)
    bad.step(uab, dt)
    assert np.abs(bad.c - ref).max() / np.abs(ref).max() > 1e-4


@pytest.mark.parametrize("dim,N,deg", [(2, 8, 1), (2, 8, 2), (2, 4, 3), (3, 4, 2)])
def test_conservation_defect_of_the_model(dim, N, deg):
    """Fluid at rest, FluxBC(q) with a non-constant q on one side, no Dirichlet row, no source, c(0) = 0:
    1^T M (c^n - c^0) = n dt sum_f int_f q_I ds to 1e-8 relative (the device test's bound)."""
    kappa, dt, n = 0.3, 0.05, 3
    F = _forms(dim, N, deg)
    fc, fa = _side(F, 1, -1)
    q = lambda x: 1.0 + 0.5 * x[0] + x[0] ** 2  # noqa: E731
    cond = BM.Flux(fc, fa, q)
    m = BM.ScalarBCModel(F, F.x_v, kappa, options=TIGHT, conditions=[cond])
    uab = np.zeros((F.nv, dim))
    _, load, _ = BM.surface_terms(F, F.x_v, cond, uab)
    total = load.sum()
    assert total > 0.5
    for _ in range(n):
        m.step(uab, dt)
        assert m.reason > 0
    one = np.ones(F.nv)
    gained = one @ (m.M @ m.c)
    defect = abs(gained - n * dt * total) / abs(n * dt * total)
    print(f"({dim},{N},P{deg}): gained {gained:.12e}, expected {n * dt * total:.12e}, defect {defect:.3e}")
    assert defect < 1e-8
