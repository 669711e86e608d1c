"""No GPU: the numpy model of SUPG-stabilised scalar transport (tests/scalar_supg_model.py) pinned against closed forms, and
the argument guards and the grouping key of ``oasisx_amd.SUPG`` / ``ScalarTransport(stabilization=...)``."""
import numpy as np
import pytest

from oracle import ipcs_oracle as O
from tests import scalar_supg_model as SM


def _forms(dim, N, deg, jiggle=0.0):
    """The lattice on [-1, 1]^dim; ``jiggle``: the interior vertices moved by up to that share of the mesh width (cells of
    different shapes, so tau differs from cell to cell also in a uniform flow)."""
    if dim == 2:
        coords, cells = O.create_rectangle_mesh([-1, -1], [1, 1], [N, N])
    else:
        coords, cells = O.create_box_mesh([-1, -1, -1], [1, 1, 1], [N, N, N])
    if jiggle:
        inner = np.all(np.abs(coords) < 1.0 - 1e-9, axis=1)
        coords = coords.copy()
        coords[inner] += jiggle * (2.0 / N) * np.random.default_rng(11).uniform(-1.0, 1.0, (int(inner.sum()), dim))
    return O.Forms(coords, cells, deg, 1)


# ---- tau -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("time_term", [True, False])
def test_tau_against_the_1d_closed_form(time_term):
    """A uniform 1-D P1 mesh of width h: grad lambda = -1/h, +1/h, so q = 2|w|/h, g = 2/h^2 and
    tau = ((2/dt)^2 + (2|w|/h)^2 + (4 kappa/h^2)^2)^(-1/2)."""
    h, dt, kappa = 0.125, 0.05, 3e-3
    w = np.array([[-2.0], [0.0], [0.7], [11.0]])
    G = np.tile(np.array([[[-1.0 / h], [1.0 / h]]]), (w.shape[0], 1, 1))
    ref = ((2.0 / dt) ** 2 * time_term + (2.0 * np.abs(w[:, 0]) / h) ** 2 + (4.0 * kappa / h ** 2) ** 2) ** -0.5
    tau = SM.tau_cells(w, G, kappa, dt, 1, time_term=time_term)
    assert np.abs(tau - ref).max() <= 4.0 * np.finfo(float).eps * ref.max()
    assert np.array_equal(SM.tau_cells(w, G, kappa, dt, 1, scale=0.5, time_term=time_term), 0.5 * tau)
    # the convective limit on the lattice: flow along x on right triangles of leg h has q = 2|w|/h as in 1-D
    F = _forms(2, 8, 1)
    hh = 2.0 / 8
    uab = np.zeros((F.nv, 2))
    uab[:, 0] = 1.5
    t2 = SM.tau_cells(SM.centroid_velocity(F, uab), F.G, 0.0, dt, 1, time_term=time_term)
    ref2 = ((2.0 / dt) ** 2 * time_term + (2.0 * 1.5 / hh) ** 2) ** -0.5
    assert np.abs(t2 - ref2).max() <= 1e-14 * ref2


def test_tau_at_rest_and_with_a_velocity_that_is_not_finite():
    F = _forms(2, 4, 2)
    w = np.zeros((F.cells.shape[0], 2))
    tau = SM.tau_cells(w, F.G, 1e-3, 0.1, 2)
    assert np.isfinite(tau).all() and (tau > 0.0).all()
    assert np.array_equal(SM.tau_cells(w, F.G, 0.0, 0.1, 2, time_term=False), np.zeros_like(tau))
    w[3, 1] = np.inf
    w[5, 0] = np.nan
    tau = SM.tau_cells(w, F.G, 1e-3, 0.1, 2)
    assert np.isnan(tau[[3, 5]]).all() and np.isfinite(np.delete(tau, [3, 5])).all()


# ---- N and S of one element ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_one_p1_element_against_hand_formulas(dim):
    """P1: grad phi_i = G[i] is constant and int phi_j = |T| / (d + 1), so
    N_ij = tau (w . G[i]) |T| / (d + 1) and S_ij = tau (w . G[i]) (w . G[j]) |T|."""
    rng = np.random.default_rng(3)
    coords = np.vstack([np.zeros(dim), np.eye(dim)]) @ (np.eye(dim) + 0.3 * rng.standard_normal((dim, dim))) + 0.2
    cells = np.arange(dim + 1)[None]
    F = O.Forms(coords, cells, 1, 1)
    vol = F.adet[0] / (2.0 if dim == 2 else 6.0)
    w, tau = rng.standard_normal((1, dim)), np.array([0.37])
    Ne, Se = SM.supg_element_matrices(F, w, tau)
    wg = F.G[0] @ w[0]
    # the local dofs of Forms are the vertices in the cell's order
    loc = np.argsort(F.vd[0])
    assert np.array_equal(F.vd[0][loc], np.arange(dim + 1))
    N_ref = tau[0] * np.outer(wg, np.ones(dim + 1)) * vol / (dim + 1)
    S_ref = tau[0] * np.outer(wg, wg) * vol
    assert np.abs(Ne[0] - N_ref).max() <= 1e-14 * np.abs(N_ref).max()
    assert np.abs(Se[0] - S_ref).max() <= 1e-14 * np.abs(S_ref).max()


@pytest.mark.parametrize("dim,N,deg", [(2, 4, 1), (2, 3, 2), (2, 2, 3), (3, 2, 1), (3, 2, 2), (3, 1, 3)])
def test_row_and_column_sums(dim, N, deg):
    """sum_j phi_j = 1: sum_j S_ij = sum_c tau int (w . grad phi_i)(w . grad 1) = 0, and sum_i N_ij = int (w . grad 1)
    phi_j = 0."""
    F = _forms(dim, N, deg)
    rng = np.random.default_rng(5)
    uab = rng.standard_normal((F.nv, dim))
    w = SM.centroid_velocity(F, uab)
    tau = SM.tau_cells(w, F.G, 1e-3, 0.1, deg)
    Nm, Sm = SM.supg_matrices(F, w, tau)
    assert np.abs(np.asarray(Sm.sum(axis=1))).max() <= 1e-13 * abs(Sm).max()
    assert np.abs(np.asarray(Nm.sum(axis=0))).max() <= 1e-13 * abs(Nm).max()
    assert abs(Sm - Sm.T).max() <= 1e-14 * abs(Sm).max()


# ---- consistency -----------------------------------------------------------------------------------------------------------
def _fixed_point_model(dim, N, deg, jiggle=0.0, **kw):
    F = _forms(dim, N, deg, jiggle)
    x = F.x_v
    bd = np.nonzero(np.isclose(np.abs(x[:, 0]), 1.0))[0]
    m = SM.ScalarSupgModel(F, x, 0.01, dofs=bd, value=lambda X: X[0], source=1.0, **kw)
    m.interpolate(lambda X: X[0])
    uab = np.zeros((F.nv, dim))
    uab[:, 0] = 1.0
    return m, uab


@pytest.mark.parametrize("dim,N,deg", [(2, 6, 1), (2, 4, 2), (2, 3, 3), (3, 3, 1), (3, 2, 2)])
def test_the_fixed_point(dim, N, deg):
    """u = (1, 0), f = 1, c = x between Dirichlet faces, insulated elsewhere: u . grad c = f and lap c = 0, so c = x solves
    the stabilised system exactly -- A_c x = b_c to rounding -- because the test function meets the WHOLE residual, on the
    lattice and on a mesh with moved vertices.  Without N f_h in b_c (streamline diffusion alone) c = x is no solution
    once tau differs between the cells of a patch (on the uniform lattice int w . grad phi_i over a patch cancels)."""
    for jiggle in (0.0, 0.25):
        m, uab = _fixed_point_model(dim, N, deg, jiggle)
        A, b = m.assemble(uab, 0.1)
        r = np.abs(A @ m.c1 - b).max()
        assert r <= 1e-12 * np.abs(b).max(), (jiggle, r)
    m2, _ = _fixed_point_model(dim, N, deg, 0.25, galerkin_source_only=True)
    A2, b2 = m2.assemble(uab, 0.1)
    assert np.abs(A2 @ m2.c1 - b2).max() > 1e-4 * np.abs(b2).max()
    m, uab = _fixed_point_model(dim, N, deg)
    # and three steps leave it there
    m.rtol, m.atol = 1e-11, 1e-30
    for _ in range(3):
        m.step(uab, 0.1)
        assert m.reason > 0
    assert np.abs(m.c - m.x_v[:, 0]).max() <= 1e-9


# ---- overshoot -------------------------------------------------------------------------------------------------------------
SKEW = dict(kappa=1e-6, dt=0.05, steps=10, angle_deg=30.0)


@pytest.mark.parametrize("deg", [1, 2])
def test_supg_reduces_the_overshoot_of_the_skew_step(deg):
    """The skew step of demo/supg_front_hip.py at N = 16, kappa = 1e-6 (cell Peclet number ~ 1e5), 10 steps: max(c) - 1
    and -min(c) are both smaller with SUPG than with plain Galerkin.  (SUPG has no discontinuity capturing: the layer
    across the streamlines keeps an overshoot.)"""
    F = _forms(2, 16, deg)
    out = {}
    for stab in (False, True):
        m = SM.run_skew(F, F.x_v, stabilize=stab, **SKEW)
        out[stab] = (m.c.max() - 1.0, -m.c.min())
    print(f"P{deg}: Galerkin over/undershoot {out[False]}, SUPG {out[True]}")
    assert out[False][0] > 0.05 and out[False][1] > 0.05
    assert out[True][0] < out[False][0] and out[True][1] < out[False][1]


def test_at_rest_the_model_is_the_plain_one():
    from tests.scalar_model import ScalarModel

    F = _forms(2, 4, 2)
    src = lambda x: 1.0 + x[0]  # noqa: E731
    a, b = SM.ScalarSupgModel(F, F.x_v, 0.1, source=src), ScalarModel(F, F.x_v, 0.1, source=src)
    for m in (a, b):
        m.interpolate(lambda x: np.cos(x[0]) + x[1])
    uab = np.zeros((F.nv, 2))
    Aa, ba = a.assemble(uab, 0.1)
    Ab, bb = b.assemble(uab, 0.1)
    assert abs(Aa - Ab).max() == 0.0 and np.array_equal(ba, bb)


# ---- the public surface ----------------------------------------------------------------------------------------------------
def test_supg_argument_guards():
    import oasisx_amd as ox
    from oasisx_amd.function import Expression

    s = ox.SUPG()
    assert s.scale == 1.0 and s.time_term is True
    assert ox.SUPG(scale=2, time_term=False).key() == (2.0, False)
    for bad in (0.0, -1.0, float("inf"), float("nan"), "x", None):
        with pytest.raises(ValueError, match="scale"):
            ox.SUPG(scale=bad)
    for bad in (1, "yes", None):
        with pytest.raises(TypeError, match="time_term"):
            ox.SUPG(time_term=bad)
    assert ox.ScalarTransport("c", diffusivity=0.1).stabilization is None
    assert ox.ScalarTransport("c", diffusivity=0.1, stabilization=s).stabilization is s
    for bad in ("supg", 1.0, True, ox.SUPG):
        with pytest.raises(TypeError, match="stabilization"):
            ox.ScalarTransport("c", diffusivity=0.1, stabilization=bad)
    e = Expression.__new__(Expression)  # (the guard looks at the type alone)
    with pytest.raises(NotImplementedError, match="Expression"):
        ox.ScalarTransport("c", diffusivity=0.1, source=e, stabilization=s)
    ox.ScalarTransport("c", diffusivity=0.1, source=e)  # without stabilisation an Expression source stays accepted


def test_grouping_key():
    import oasisx_amd as ox
    from oasisx_amd.scalar import group_key, group_scalars

    rows = np.array([1, 2, 3])
    mk = lambda n, st, **kw: ox.ScalarTransport(n, diffusivity=0.1, stabilization=st, **kw)  # noqa: E731
    plain, a, b = mk("p", None), mk("a", ox.SUPG()), mk("b", ox.SUPG(1.0, True))
    c, d = mk("c", ox.SUPG(scale=0.5)), mk("d", ox.SUPG(time_term=False))
    keys = {s.name: group_key(s, rows, None)[0] for s in (plain, a, b, c, d)}
    assert keys["a"] == keys["b"]
    assert len({keys[k] for k in "pacd"}) == 4
    # a scalar without stabilisation keeps the key it had
    assert keys["p"] == (("kappa", 0.1, ("turbulent_schmidt", None)), rows.astype(np.int64).tobytes())
    assert keys["a"] == (("kappa", 0.1, ("turbulent_schmidt", None), ("supg", 1.0, True)), rows.astype(np.int64).tobytes())
    groups = group_scalars([(keys[s.name], rows, s) for s in (plain, a, b, c, d)])
    assert [[m.name for m in members] for _, members in groups] == [["p"], ["a", "b"], ["c"], ["d"]]
