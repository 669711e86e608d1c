"""CPU: the numpy model of the drag zones (tests/drag_model.py) pinned on its own -- the weighted mass matrix against the
oracle's, the coefficient against its closed form, the discrete Brinkman channel against the analytic profile -- and the
scope guards of ``drag=``, which need neither the library nor a GPU."""
import numpy as np
import pytest

CASES = [(2, 6, 1), (2, 5, 2), (3, 3, 1), (3, 3, 2), (2, 4, 3), (3, 2, 3)]


def _forms(dim, N, deg):
    from tests import viscosity_model as VM

    return VM.tg_forms(dim, N, deg, 2 if deg == 3 else 1)


def _two_zones(F, rng=None):
    """The zones of the GPU tests on the oracle's own mesh: a half space x < 0.1 and a small box with a target."""
    from tests import drag_model as DM

    cen = F.coords[F.cells].mean(axis=1)
    half = np.nonzero(cen[:, 0] < 0.1)[0]
    box = np.nonzero((cen[:, 0] > 0.3) & (np.abs(cen[:, 1]) < 0.5))[0]
    assert half.size and box.size and not np.intersect1d(half, box).size
    ut = np.zeros((F.nv, F.d))
    ut[:, 0], ut[:, 1] = 0.4, -0.2
    return [DM.Zone(half, alpha=3.0 + cen[half, 1] ** 2), DM.Zone(box, alpha=0.5, beta=2.0, ut=ut)]


@pytest.mark.parametrize("dim,N,deg", CASES)
def test_weighted_mass_of_one_is_the_mass_matrix(dim, N, deg):
    """weighted_mass(F, 1) = Forms.mass_v() to rounding (the same element matrices through the same _csr)."""
    from tests import drag_model as DM

    F = _forms(dim, N, deg)
    M = F.mass_v()
    d = abs(DM.weighted_mass(F, 1.0) - M).max()
    assert d <= 4 * np.finfo(float).eps * abs(M).max(), d


@pytest.mark.parametrize("dim,N,deg", CASES)
def test_drag_matrix_is_symmetric_with_the_load_as_row_sums(dim, N, deg):
    """D = sum_c sigma_c M_c: symmetric; its row sums are sum_c sigma_c int_c phi_i (the basis sums to one); zero on the
    rows no zone cell touches."""
    from tests import drag_model as DM

    F = _forms(dim, N, deg)
    zones = _two_zones(F)
    uab = np.stack([np.sin(1.3 * F.x_v[:, 0] + k) for k in range(dim)], axis=1)
    sig = DM.sigma_field(F, uab, zones)
    assert sig.min() >= 0.0 and (sig > 0).sum() == sum(z.cells.size for z in zones)
    D = DM.weighted_mass(F, sig)
    scale = abs(D).max()
    assert abs(D - D.T).max() <= 1e-14 * scale
    rows = np.asarray(D.sum(axis=1)).ravel()
    assert np.abs(rows - DM.weighted_load(F, sig)).max() <= 1e-13 * scale
    touched = np.zeros(F.nv, dtype=bool)
    touched[np.unique(F.vd[sig > 0])] = True
    assert not touched.all() and abs(D[~touched]).max() == 0.0


@pytest.mark.parametrize("dim,N,deg", CASES)
def test_sigma_of_a_uniform_field(dim, N, deg):
    """u_ab = c, u_t = t constant: sigma_c = alpha_c + beta_c |c - t| in every cell of the zone (the basis sums to one at
    the centroid, also where single basis functions are negative there)."""
    from tests import drag_model as DM

    F = _forms(dim, N, deg)
    c = np.array([0.7, -1.1, 0.4])[:dim]
    t = np.array([0.2, 0.3, -0.5])[:dim]
    cells = np.arange(0, F.cells.shape[0], 2)
    alpha = 0.1 + 0.01 * np.arange(cells.size)
    beta = 2.0 + 0.02 * np.arange(cells.size)
    uab = np.tile(c, (F.nv, 1))
    z = DM.Zone(cells, alpha=alpha, beta=beta, ut=np.tile(t, (F.nv, 1)))
    ref = alpha + beta * np.linalg.norm(c - t)
    assert np.abs(DM.sigma_cells(F, uab, z) - ref).max() <= 1e-14 * ref.max()
    z0 = DM.Zone(cells, alpha=alpha, beta=beta)
    ref0 = alpha + beta * np.linalg.norm(c)
    assert np.abs(DM.sigma_cells(F, uab, z0) - ref0).max() <= 1e-14 * ref0.max()
    full = DM.sigma_field(F, uab, [z0])
    assert np.array_equal(full[cells], DM.sigma_cells(F, uab, z0)) and np.count_nonzero(full) == cells.size


@pytest.mark.parametrize("deg,N", [(1, 8), (2, 4), (2, 8), (3, 4)])
def test_brinkman_channel_against_the_closed_form(deg, N):
    """[-1, 1]^2, nu = 0.5, sigma = 2 everywhere, f = 1 along x, exact Dirichlet data: the discrete steady state (one
    solve with nu K + sigma M) against u = (f / sigma)(1 - cosh(m y) / cosh(m)), m = sqrt(sigma / nu).  Measured on the
    CPU as max error over the centreline value: P1 N = 8 6.1e-3, P2 N = 4 1.0e-3, P2 N = 8 7.5e-5, P3 N = 4 2.8e-4; the bound is
    1.5 x these (it pins the model; the margin covers another numbering only)."""
    from tests import drag_model as DM

    err, u, F = DM.brinkman_direct(deg, N)
    print(f"P{deg} N = {N}: max |u_h - u| / u(0) = {err:.3e} (recorded {DM.BRINKMAN_MEASURED[(deg, N)]:.1e})")
    assert err <= 1.5 * DM.BRINKMAN_MEASURED[(deg, N)], err
    assert err >= 0.1 * DM.BRINKMAN_MEASURED[(deg, N)]  # (the closed form is not reproduced by accident of a zero field)


def test_model_step_without_zones_is_the_oracle_step():
    """DragOracleStep restates the oracle's assemble_first: without zones, A and b_first are the oracle's bits."""
    from oracle import ipcs_oracle as O
    from tests import drag_model as DM
    from tests import viscosity_model as VM

    F = _forms(2, 4, 2)
    R, clock = VM.tg_step_model(F, F.x_v, F.x_q, None)
    bd = O.boundary_dofs(F.x_v, F.coords.min(axis=0), F.coords.max(axis=0))
    bcs = [[O.DirichletData(bd, 0.0)] for _ in range(2)]
    P = DM.DragOracleStep(F, F.x_v, F.x_q, bcs)
    P.u1[:], P.u2[:] = R.u1, R.u2
    R.assemble_first(0.005, 0.01)
    P.assemble_first(0.005, 0.01)
    assert abs(P.A - R.A).max() == 0.0 and np.array_equal(P.b_first, R.b_first)
    # with zones: A - A0 = theta D off the identity rows, b - b0 = D u_t - (1 - theta) D u1
    zones = _two_zones(F)
    Z = DM.DragOracleStep(F, F.x_v, F.x_q, bcs, zones=zones, theta=0.5)
    Z.u1[:], Z.u2[:] = R.u1, R.u2
    Z.assemble_first(0.005, 0.01)
    free = np.setdiff1d(np.arange(F.nv), bd)
    assert abs((Z.A - R.A)[free] - 0.5 * Z.drag_matrix[free]).max() <= 1e-13 * abs(Z.A).max()
    ut = DM.merged_target(F, zones)
    rhs = Z.drag_matrix @ ut - 0.5 * (Z.drag_matrix @ Z.u1)
    assert np.abs(Z.b_first - R.b_first - rhs).max() <= 1e-13 * np.abs(Z.b_first).max()
    f, mag = DM.zone_force(F, Z.u1, Z.sigma, zones[1])
    assert f.shape == (2,) and (mag >= np.abs(f)).all()


# ---- guards ------------------------------------------------------------------------------------------------------------
def _cpu_mesh(dim=2, N=4):
    from tests.helpers import tg_mesh

    return tg_mesh(dim, N, device="cpu")


def _build(mesh, **kw):
    import oasisx_amd as ox
    from tests.helpers import KRYLOV

    dim = mesh.geometry.dim
    return ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_u=[[] for _ in range(dim)], bcs_p=[],
                                   solver_options=KRYLOV, **kw)


def test_drag_zone_is_exported():
    import oasisx_amd as ox

    assert "DragZone" in ox.__all__ and ox.DragZone is ox.drag.DragZone


def test_guards_raise_before_the_library_is_needed(monkeypatch):
    import oasisx_amd as ox
    from oasisx_amd import _lib
    from oasisx_amd.parallel import Comm

    def no_library():
        raise AssertionError("the guards run before the library is loaded")

    monkeypatch.setattr(_lib, "load", no_library)
    left = lambda x: x[0] < 0.0  # noqa: E731
    with pytest.raises(NotImplementedError, match="rotational"):
        _build(_cpu_mesh(), drag=ox.DragZone(left, darcy=1.0), rotational=True)
    pmesh = _cpu_mesh()
    pmesh.comm = Comm(0, 2, None, transport="host")
    with pytest.raises(NotImplementedError, match="partition"):
        _build(pmesh, drag=ox.DragZone(left, darcy=1.0))
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="darcy"):
            ox.DragZone(left, darcy=bad)
        with pytest.raises(ValueError, match="forchheimer"):
            ox.DragZone(left, forchheimer=bad)
    with pytest.raises(ValueError, match="darcy"):  # a callable or an array is checked when the mesh is known
        _build(_cpu_mesh(), drag=ox.DragZone(left, darcy=lambda x: x[1]))
    with pytest.raises(ValueError, match="forchheimer"):
        _build(_cpu_mesh(), drag=ox.DragZone(np.array([0, 1, 2]), forchheimer=np.array([1.0, -1.0, 0.0])))
    with pytest.raises(ValueError, match="values"):
        _build(_cpu_mesh(), drag=ox.DragZone(np.array([0, 1, 2]), darcy=np.array([1.0, 1.0])))
    for theta in (0.49, 1.01, float("nan")):
        with pytest.raises(ValueError, match="drag_theta"):
            _build(_cpu_mesh(), drag=ox.DragZone(left, darcy=1.0), drag_theta=theta)
    with pytest.raises(ValueError, match="no cell"):
        _build(_cpu_mesh(), drag=ox.DragZone(lambda x: x[0] > 5.0, darcy=1.0))
    with pytest.raises(ValueError, match="two zones"):
        _build(_cpu_mesh(), drag=[ox.DragZone(left, darcy=1.0), ox.DragZone(lambda x: x[0] < 0.6, darcy=1.0)])
    with pytest.raises(ValueError, match="cell id"):
        _build(_cpu_mesh(), drag=ox.DragZone(np.array([0, 10 ** 6]), darcy=1.0))
    with pytest.raises(TypeError, match="DragZone"):
        _build(_cpu_mesh(), drag=["sponge"])
    with pytest.raises(RuntimeError, match="not the drag="):
        ox.DragZone(left, darcy=1.0).sample(0.0)


def test_zone_selection_and_coefficients_on_the_host():
    """select: by tag, then by cell id, for meshtags, ids and a marker; coefficients: float, callable on the zone's
    centroids, array over the zone's cells."""
    import oasisx_amd as ox
    from oasisx_amd import mesh as M

    mesh = _cpu_mesh(2, 4)
    nc = int(mesh.num_cells)
    cen = mesh.coords[mesh.cells.long()].mean(dim=1).numpy()
    vals = np.where(cen[:, 0] < 0.0, 7, 9).astype(np.int32)
    mt = M.meshtags(mesh, 2, np.arange(nc), vals)
    z = ox.DragZone((mt, (9, 7)), darcy=lambda x: 1.0 + x[0] ** 2, forchheimer=0.5)
    ids, tag_of, tags = z.select(mesh)
    assert list(tags) == [9, 7] and ids.shape[0] == nc
    n9 = int((vals == 9).sum())
    assert np.array_equal(ids[:n9], np.nonzero(vals == 9)[0]) and np.array_equal(ids[n9:], np.nonzero(vals == 7)[0])
    assert np.array_equal(tag_of, np.repeat([0, 1], [n9, nc - n9]))
    a, b = z.coefficients(mesh, ids)
    assert np.allclose(a, 1.0 + cen[ids, 0] ** 2, rtol=1e-15) and np.array_equal(b, np.full(nc, 0.5))
    zm = ox.DragZone(lambda x: x[1] > 0.0)
    im, tm, _ = zm.select(mesh)
    assert np.array_equal(im, np.nonzero(cen[:, 1] > 0.0)[0]) and not tm.any()
    with pytest.raises(ValueError, match="twice"):
        ox.DragZone(np.array([3, 3])).select(mesh)
