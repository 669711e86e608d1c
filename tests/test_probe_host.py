"""Point evaluation without a GPU: the numpy model (tests/probe_model.py) against polynomials, the argument validation of
``oasisx_amd.geometry`` / ``Probes`` / ``Function.eval`` that needs no device, and the ownership rule of points on CPU
mesh partitions."""
import numpy as np
import pytest
import torch

from oasisx_amd import fem, geometry
from oasisx_amd import mesh as M
from tests import probe_model as PM


def _mesh(kind):
    if kind == "box":
        return M.create_box(None, [[-1.0] * 3, [1.0] * 3], [8, 8, 8], device="cpu")
    if kind == "square":
        return M.create_unit_square(None, 16, 16, device="cpu")
    return M.create_delaunay_box(None, [[-1.0] * 3, [1.0] * 3], 6, seed=4, device="cpu")


def _poly(degree, d):
    """A polynomial of exactly that degree in d variables, x of shape (3, n) -> (n,)."""
    if degree == 1:
        return lambda x: 0.3 + 0.7 * x[0] - 0.4 * x[1] + (0.2 * x[2] if d == 3 else 0.0)
    return lambda x: 0.3 + 0.7 * x[0] - 0.4 * x[1] + 0.9 * x[0] * x[1] - 0.5 * x[1] ** 2 + (
        0.2 * x[2] + 0.6 * x[2] * x[0] - 0.8 * x[2] ** 2 if d == 3 else 0.0)


@pytest.mark.parametrize("kind", ["box", "square", "delaunay"])
@pytest.mark.parametrize("degree", [1, 2])
def test_model_locates_every_point_and_reproduces_polynomials(kind, degree):
    mesh = _mesh(kind)
    d = mesh.gdim
    V = fem.FunctionSpace(mesh, degree, window=64)
    u = fem.Function(V)
    f = _poly(degree, d)
    u.interpolate(f)
    x = PM.sample_points(mesh, 400, 50, 50, seed=11)
    coords, cells = mesh.coords.numpy(), mesh.cells.numpy()
    cell, bary = PM.locate(coords, cells, x)
    print("unlocated:", int((cell < 0).sum()), "of", x.shape[0])
    assert int((cell < 0).sum()) == 0  # the cap on points left out is zero
    assert bary.min() >= -1e-10 and np.abs(bary.sum(axis=1) - 1.0).max() < 1e-13
    vals = PM.evaluate(V, u.x.array, x, cell, bary)[:, 0]
    X3 = np.zeros((3, x.shape[0]))
    X3[:d] = x.T
    exact = f(X3)
    err = float(np.abs(vals - exact).max())
    print("max deviation from the polynomial:", err)
    assert err <= 1e-12 * max(1.0, float(np.abs(exact).max()))
    # a point outside the mesh: -1, NaN values
    far = np.full((1, d), 7.0)
    c, _ = PM.locate(coords, cells, far)
    assert c[0] == -1 and np.isnan(PM.evaluate(V, u.x.array, far, c)).all()


def test_model_takes_the_lowest_cell_on_a_shared_vertex():
    mesh = _mesh("square")
    coords, cells = mesh.coords.numpy(), mesh.cells.numpy()
    v = 5 * 17 + 7  # an interior vertex: six cells meet there
    around = np.nonzero((cells == v).any(axis=1))[0]
    assert around.size == 6
    c, bary = PM.locate(coords, cells, coords[v:v + 1])
    assert c[0] == around.min()
    c2, _ = PM.locate(coords, cells, coords[v:v + 1], cell_ids=around[1:])
    assert c2[0] == np.sort(around)[1]


# ---- validation that needs no device -----------------------------------------------------------------------------------
def test_bb_tree_arguments():
    mesh = _mesh("square")
    with pytest.raises(NotImplementedError):
        geometry.bb_tree(mesh, 1)
    with pytest.raises(ValueError):
        geometry.bb_tree(mesh, 2, tol=0.5)
    with pytest.raises(ValueError):
        geometry.bb_tree(mesh, 2, padding=-1.0)
    with pytest.raises(ValueError):
        geometry.bb_tree(mesh, 2, entities=np.zeros(0, dtype=np.int32))
    with pytest.raises(ValueError):
        geometry.bb_tree(mesh, 2, entities=[0, mesh.num_cells])
    from oasisx_amd import _lib

    with pytest.raises(_lib.OasisxHipError):  # no CPU fallback: the locator is a device object
        geometry.bb_tree(mesh, 2)
    with pytest.raises(TypeError):
        geometry.compute_collisions_points(object(), np.zeros((1, 3)))
    with pytest.raises(TypeError):
        geometry.compute_colliding_cells(mesh, object(), np.zeros((1, 3)))


def test_point_shapes():
    assert tuple(geometry.as_points(np.zeros((4, 3)), 2, "cpu").shape) == (4, 2)
    assert tuple(geometry.as_points(np.zeros((4, 2)), 2, "cpu").shape) == (4, 2)
    assert tuple(geometry.as_points(torch.zeros(5, 3), 3, "cpu").shape) == (5, 3)
    assert tuple(geometry.as_points([0.1, 0.2, 0.0], 2, "cpu").shape) == (1, 2)
    for bad in (np.zeros((4, 4)), np.zeros((2, 2, 3)), np.zeros((3, 2))):
        with pytest.raises(ValueError):
            geometry.as_points(bad, 3, "cpu")


def test_adjacency_has_zero_or_one_link_per_point():
    adj = geometry.AdjacencyList.from_cells(torch.tensor([4, -1, 0, 9]))
    assert adj.num_nodes == 4 and adj.offsets.tolist() == [0, 1, 1, 2, 3] and adj.array.tolist() == [4, 0, 9]
    assert adj.links(0).tolist() == [4] and adj.links(1).tolist() == [] and adj.links(3)[0] == 9
    mesh = _mesh("square")
    assert geometry.compute_colliding_cells(mesh, adj, np.zeros((4, 3))) is adj
    with pytest.raises(ValueError):
        geometry.compute_colliding_cells(mesh, adj, np.zeros((3, 3)))


def test_eval_and_probes_refuse_what_they_do_not_cover():
    import oasisx_amd as ox

    assert ox.Probes is geometry.Probes and ox.geometry is geometry
    mesh = _mesh("square")
    x = np.array([[0.5, 0.5, 0.0]])
    dg = fem.Function(fem.functionspace(mesh, ("DG", 1)))
    with pytest.raises(NotImplementedError, match="DGSpace"):
        dg.eval(x)
    hi = fem.Function(fem.functionspace(mesh, ("Lagrange", 4)))
    with pytest.raises(NotImplementedError, match="HighOrderLagrangeSpace"):
        hi.eval(x, [0])
    with pytest.raises(NotImplementedError):
        geometry.Probes(x, dg)
    u = fem.Function(fem.FunctionSpace(mesh, 1, window=64))
    with pytest.raises(ValueError):
        u.eval(np.zeros((2, 3)), [0])  # two points, one cell
    with pytest.raises(ValueError):
        u.eval(x, [mesh.num_cells])
    with pytest.raises(ValueError):
        u.eval(np.zeros((1, 5)))
    with pytest.raises(TypeError):
        geometry.Probes(x, [])
    with pytest.raises(TypeError):
        geometry.Probes(x, [u, "p"])
    with pytest.raises(ValueError):
        geometry.Probes(x, u, capacity=0)
    other = fem.Function(fem.FunctionSpace(_mesh("square"), 1, window=64))
    with pytest.raises(ValueError, match="same mesh"):
        geometry.Probes(x, [u, other])


def test_interpolate_between_functions_on_one_space_still_copies():
    mesh = _mesh("square")
    V = fem.FunctionSpace(mesh, 2, window=64)
    a, b = fem.Function(V), fem.Function(V)
    a.interpolate(lambda x: np.sin(3.0 * x[0]) + x[1])
    b.interpolate(a)
    assert np.array_equal(a.x.array, b.x.array)
    W = fem.FunctionSpace(mesh, 2, window=64)  # another object, the same mesh and degree: the copy of today
    c = fem.Function(W)
    c.interpolate(a)
    assert np.array_equal(a.x.array, c.x.array)


# ---- the ownership rule on CPU partitions ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["box", "delaunay"])
@pytest.mark.parametrize("nparts", [2, 3, 8])
def test_every_point_has_one_owner_that_holds_its_cell(kind, nparts):
    from oasisx_amd.parallel import MeshPartition

    mesh = _mesh(kind)
    coords, cells = mesh.coords.numpy(), mesh.cells.numpy()
    x = PM.sample_points(mesh, 300, 150, 150, seed=5, n_centroids=150, n_faces=150)
    assert x.shape[0] == 900
    glob, _ = PM.locate(coords, cells, x)
    assert (glob >= 0).all()
    parts = [MeshPartition(mesh, r, nparts) for r in range(nparts)]
    res = PM.owners(mesh, parts, x)
    count = np.zeros(x.shape[0], dtype=np.int64)
    for (rank, mine, c), part in zip(res, parts):
        count += mine
        assert np.array_equal(c[mine], glob[mine])  # the owner's c* is the lowest containing cell of the WHOLE mesh
        assert np.isin(c[mine], part.local_cells.numpy()).all()  # and the owner can evaluate there
    assert (count == 1).all(), np.unique(count, return_counts=True)
