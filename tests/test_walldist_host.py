"""No GPU: the numpy model of the wall distance and of the van Driest damping (tests/walldist_model.py) pinned by closed
forms, and the guards of WallDistance / VanDriest that hold before the HIP library is loaded."""
import numpy as np
import pytest

from tests import walldist_model as WD

EPS = np.finfo(np.float64).eps


def _mesh(dim, n, lo=None, hi=None):
    from oasisx_amd import mesh as M

    lo = [0.0] * dim if lo is None else lo
    hi = [2.0, 1.0, 1.5][:dim] if hi is None else hi
    make = M.create_rectangle if dim == 2 else M.create_box
    return make(None, [lo, hi], list(n), device="cpu")


def _facets_on(mesh, axis, values):
    """Ids and vertex coordinates (nf, d, d) of the exterior facets that lie on x_axis = one of ``values``."""
    d = mesh.gdim
    fv, _ = mesh._entities(d - 1)
    X = mesh.coords.numpy()
    ext = np.asarray(mesh.exterior_facets(), dtype=np.int64)
    on = np.zeros(ext.shape[0], dtype=bool)
    for v in values:
        on |= np.isclose(X[fv[ext]][:, :, axis], v).all(axis=1)
    return ext[on], X[fv[ext[on]]]


@pytest.mark.parametrize("dim,n", [(2, (7, 5)), (3, (4, 3, 2))])
def test_two_opposite_walls_give_the_channel_distance(dim, n):
    """A box with the faces y = 0 and y = 1 as walls: d = min(y, 1 - y) for every point inside (and on) the box."""
    mesh = _mesh(dim, n)
    _, xyz = _facets_on(mesh, 1, (0.0, 1.0))
    rng = np.random.default_rng(5)
    x = rng.uniform(0.0, 1.0, size=(257, dim)) * np.array([2.0, 1.0, 1.5][:dim])
    x = np.concatenate([x, mesh.coords.numpy()])
    dist, near, D = WD.nearest(xyz, x)
    ref = np.minimum(x[:, 1], 1.0 - x[:, 1])
    assert np.abs(dist - ref).max() <= 8 * EPS
    assert (D[np.arange(x.shape[0]), near] == dist).all()
    ids, _ = _facets_on(mesh, 1, (0.0, 1.0))
    assert ids.shape[0] == 2 * (n[0] if dim == 2 else 2 * n[0] * n[2])


def test_points_beyond_a_triangles_vertex_edge_and_face():
    """The seven regions of the triangle (0,0,0), (2,0,0), (0,1,0): closed forms."""
    tri = np.array([[[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 1.0, 0.0]]])
    pts = np.array([
        [-1.0, -2.0, 2.0],   # vertex a: |x - a| = 3
        [3.0, -0.5, 0.5],    # vertex b
        [-0.5, 2.0, -1.0],   # vertex c
        [1.0, -3.0, 4.0],    # edge ab: sqrt(9 + 16) = 5
        [-3.0, 0.5, 4.0],    # edge ac: 5
        [2.0, 1.5, 0.0],     # edge bc: the line x + 2 y = 2, distance (2 + 3 - 2) / sqrt(5)
        [0.5, 0.25, -7.0],   # face: 7
        [0.5, 0.25, 0.0],    # on the face: 0
        [2.0, 0.0, 0.0],     # a vertex: exactly 0
    ])
    ref = np.array([3.0, np.sqrt(1.0 + 0.25 + 0.25), np.sqrt(0.25 + 1.0 + 1.0), 5.0, 5.0, 3.0 / np.sqrt(5.0), 7.0, 0.0, 0.0])
    dist, near, _ = WD.nearest(tri, pts)
    assert np.abs(dist - ref).max() <= 8 * EPS * 7.0
    assert dist[-1] == 0.0 and dist[-2] == 0.0 and (near == 0).all()
    q = WD.closest_points(tri, pts)[:, 0]
    assert np.allclose(q[5], [1.4, 0.3, 0.0], atol=1e-15) and np.allclose(q[6], [0.5, 0.25, 0.0], atol=1e-15)


def test_segment_regions_and_exact_zeros_on_vertices():
    seg = np.array([[[0.1, 0.2], [0.3, 0.7]], [[0.3, 0.7], [1.1, 0.7]]])
    pts = np.array([[0.1, 0.2], [0.3, 0.7], [1.1, 0.7], [0.0, 0.0], [0.7, 1.7], [2.1, 0.7]])
    dist, near, _ = WD.nearest(seg, pts)
    assert (dist[:3] == 0.0).all() and list(near[:3]) == [0, 0, 1]  # (ties go to the lower facet)
    assert np.abs(dist[3:] - [np.hypot(0.1, 0.2), 1.0, 1.0]).max() <= 4 * EPS


def test_image_minimum_reaches_across_the_seam():
    """Walls: a patch of y = 0 at x in [1.5, 2] of a domain periodic in x with period 2.  A point at x = 0.1 is 0.1 from
    the patch's image, 1.4 from the patch itself."""
    seg = np.array([[[1.5, 0.0], [1.75, 0.0]], [[1.75, 0.0], [2.0, 0.0]]])
    x = np.array([[0.1, 0.0], [0.1, 0.3], [1.0, 0.2]])
    plain, _, _ = WD.nearest(seg, x)
    shifts = WD.image_shifts(np.array([2.0, 0.0, 0.0]), (0,))
    assert len(shifts) == 2 and len(WD.image_shifts(np.array([2.0, 1.0, 0.0]), (0, 1))) == 8
    dist, near, _ = WD.nearest(seg, x, shifts)
    assert np.abs(plain - [1.4, np.hypot(1.4, 0.3), np.hypot(0.5, 0.2)]).max() <= 4 * EPS
    assert np.abs(dist - [0.1, np.hypot(0.1, 0.3), np.hypot(0.5, 0.2)]).max() <= 4 * EPS
    assert list(near) == [1, 1, 0]


def test_distance_bound_constants():
    seg = np.array([[[0.0, 0.0], [1.0, 0.0]]])
    C, L = WD.distance_bound(seg, np.array([[0.0, 1.0], [np.nan, 0.0]]))
    assert C == 22.0 and L == np.sqrt(2.0)
    tri = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]])
    kappa, lmin = WD.shape_factor(tri)
    assert abs(kappa - 2.0) < 1e-15 and abs(lmin - np.sqrt(2.0)) < 1e-15


def test_van_driest_formula():
    yp, D = WD.damping([0.0, 0.05, 1.0], 2.0, 0.01, 26.0)
    assert np.array_equal(yp, [0.0, 10.0, 200.0]) and D[0] == 0.0
    assert abs(D[1] - (1.0 - np.exp(-10.0 / 26.0))) <= 2 * EPS and abs(D[2] - (1.0 - np.exp(-200.0 / 26.0))) <= 2 * EPS
    assert np.all(np.diff(D) > 0.0) and D[2] < 1.0
    _, D0 = WD.damping([0.3, 0.7], 0.0, 0.01, 26.0)  # fluid at rest: D = 0, not NaN
    assert np.array_equal(D0, [0.0, 0.0])
    assert np.allclose(WD.friction_velocity(np.array([[3.0, 4.0], [0.0, 0.0]])), [np.sqrt(5.0), 0.0], rtol=4 * EPS)
    # Poiseuille: the closed form vanishes at the walls and on the centre line
    nut = WD.poiseuille_nut(0.17, 0.01, np.array([0.0, 0.25, 0.5, 1.0]), 1.0, 2.0, 0.01, 2.0)
    assert nut[0] == 0.0 and nut[2] == 0.0 and nut[3] == 0.0 and nut[1] > 0.0


def test_guards_before_the_library_is_loaded():
    import oasisx_amd as ox
    from oasisx_amd import geometry
    from oasisx_amd.parallel import Comm

    assert ox.WallDistance is geometry.WallDistance
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="A_plus"):
            ox.VanDriest(A_plus=bad)
    with pytest.raises(ValueError, match="u_tau"):
        ox.VanDriest(u_tau=-0.1)
    with pytest.raises(ValueError, match="Wale"):
        ox.Wale(damping=ox.VanDriest())
    with pytest.raises(TypeError, match="VanDriest"):
        ox.Smagorinsky(0.1, damping=26.0)
    assert ox.Smagorinsky(0.1, damping=None).damping is None and "damping" not in repr(ox.Smagorinsky(0.1))
    assert "VanDriest(A_plus=2.0" in repr(ox.Smagorinsky(0.1, damping=ox.VanDriest(A_plus=2.0)))
    mesh = _mesh(2, (4, 3))
    with pytest.raises(ValueError, match="no facet"):
        ox.WallDistance(mesh, facets=np.zeros(0, dtype=np.int64))
    with pytest.raises(ValueError, match="bins"):
        ox.WallDistance(mesh, bins=(0, 1))
    pmesh = _mesh(2, (4, 3))
    pmesh.comm = Comm(0, 2, None, transport="host")
    with pytest.raises(NotImplementedError, match="partition"):
        ox.WallDistance(pmesh)
    # a solver with an empty wall selection is refused by the scope guards, before anything is built
    with pytest.raises(ValueError, match="no facet"):
        ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_u=[[], []], bcs_p=[],
                                viscosity_model=ox.Smagorinsky(0.1, damping=ox.VanDriest(np.zeros(0, dtype=np.int64))))
