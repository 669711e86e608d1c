"""GPU: the nearest-wall-facet query (oasisx_amd.geometry.WallDistance, ox_walldist_* of csrc/ox_probe.hip) against the
brute-force numpy model of tests/walldist_model.py, which tests/test_walldist_host.py pins by closed forms."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
MESHES = ["rectangle", "box", "delaunay2", "delaunay3"]
WALLS = ["all", "one_face", "opposite", "adjacent", "single"]


def _mesh(kind):
    from oasisx_amd import mesh as M

    if kind == "rectangle":
        return M.create_rectangle(None, [[0.0, 0.0], [2.0, 1.0]], [7, 5])
    if kind == "box":
        return M.create_box(None, [[0.0, 0.0, 0.0], [2.0, 1.0, 1.5]], [4, 3, 2])
    dim, N = (2, 6) if kind == "delaunay2" else (3, 3)
    return M.create_delaunay_box(None, [[-1.0] * dim, [1.0] * dim], N, seed=2)


def _wall_ids(mesh, which):
    """Facet ids of a wall set: faces of the mesh's bounding box (axis, side)."""
    d = mesh.gdim
    ext = np.asarray(mesh.exterior_facets(), dtype=np.int64)
    if which == "all":
        return None, ext
    fv, _ = mesh._entities(d - 1)
    X = mesh.coords.cpu().numpy()
    lo, hi = X.min(axis=0), X.max(axis=0)
    faces = {"one_face": [(1, 0)], "opposite": [(1, 0), (1, 1)], "adjacent": [(0, 0), (1, 0)], "single": [(1, 0)]}[which]
    on = np.zeros(ext.shape[0], dtype=bool)
    for axis, side in faces:
        on |= np.isclose(X[fv[ext]][:, :, axis], (lo, hi)[side][axis]).all(axis=1)
    ids = ext[on]
    if which == "single":
        ids = ids[len(ids) // 2: len(ids) // 2 + 1]
    assert ids.size
    return ids, ids


def _facet_xyz(mesh, ids):
    fv, _ = mesh._entities(mesh.gdim - 1)
    return mesh.coords.cpu().numpy()[fv[ids]]


def _queries(mesh, xyz):
    """name -> (n, d) points: centroids, P2 dof coordinates, random points in a box 1.5 times the mesh's, the facets'
    vertices and midpoints, one point."""
    import torch

    from oasisx_amd import fem

    d = mesh.gdim
    X = mesh.coords.cpu().numpy()
    lo, hi = X.min(axis=0), X.max(axis=0)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    rng = np.random.default_rng(1031)
    V2 = fem.FunctionSpace(mesh, 2, window=128)
    return {
        "centroids": mesh.coords[mesh.cells.to(torch.int64)].mean(dim=1).cpu().numpy(),
        "p2_dofs": V2.x.cpu().numpy() if torch.is_tensor(V2.x) else np.asarray(V2.x),
        "random": mid + 1.5 * half * rng.uniform(-1.0, 1.0, size=(1031, d)),
        "vertices": xyz.reshape(-1, d),
        "midpoints": xyz.mean(axis=1),
        "one": (mid + 0.3 * half)[None, :],
    }, V2


def _check(name, wd, xyz, x, shifts=None, worst=None):
    """(a) and (b) for one set of points; returns the device's (dist, nearest) tensors."""
    from tests import walldist_model as WD

    dist_t, near_t = wd.query(x)
    dist, near = dist_t.cpu().numpy(), near_t.cpu().numpy()
    assert dist.shape == (x.shape[0],) and near.dtype == np.int32
    ref, _, D = WD.nearest(xyz, x, shifts)
    C, L = WD.distance_bound(xyz, x)
    err = np.abs(dist - ref).max()
    assert near.min() >= 0 and near.max() < xyz.shape[0]
    err_b = np.abs(D[np.arange(x.shape[0]), near] - ref).max()  # nearest is A minimiser of the model's distances
    print(f"{name}: max |d_dev - d_model| = {err:.3e} = {err / (EPS * L):.2f} eps L, minimiser gap {err_b / (EPS * L):.2f} "
          f"eps L (bound C = {C:.0f})")
    if worst is not None:
        worst.append(max(err, err_b) / (EPS * L))
    assert err <= C * EPS * L, (name, err, C * EPS * L)
    assert err_b <= C * EPS * L, (name, err_b, C * EPS * L)
    return dist_t, near_t


@pytest.mark.parametrize("walls", WALLS)
@pytest.mark.parametrize("kind", MESHES)
def test_distance_and_nearest_match_the_model(hip, kind, walls):
    """(a) |d_dev - d_model| <= C eps L with C, L of walldist_model.distance_bound (its docstring derives C from the
    operation count of the closest-point formulas: 22 in 2-D, 2 (42 kappa^2 L / l_min + 8) in 3-D); (b) the model's
    distance to facet nearest[i] equals the model's minimum within the same bound; (c) d == 0 exactly on the facets'
    vertices; (d) dist AND nearest are the same bits with bins = (1, ..), the default grid and 4 times the default per
    axis, and on a second run; (e) non-finite points give NaN and -1; a query of no point launches nothing.

    Observed on one MI355X, maximum over all cases of max(|d_dev - d_model|, minimiser gap): 0.71 eps L (the bounds: 22 eps L
    in 2-D, 3.5e2 to 6.9e3 eps L in 3-D)."""
    import torch

    import oasisx_amd as ox
    from tests import walldist_model as WD

    mesh = _mesh(kind)
    d = mesh.gdim
    sel, ids = _wall_ids(mesh, walls)
    wd = ox.WallDistance(mesh, sel)
    assert np.array_equal(wd.facets, np.sort(ids)) and wd.n_facets == ids.shape[0]
    xyz = _facet_xyz(mesh, wd.facets)
    info = wd.info()
    assert info["facets"] == wd.n_facets and info["bins"] == int(np.prod(info["bins_per_axis"])) and info["list"] >= wd.n_facets
    if walls in ("one_face", "single"):  # a bounding box without thickness along y: one bin there
        assert info["bins_per_axis"][1] == 1
    brute = ox.WallDistance(mesh, sel, bins=(1,) * d)
    fine = ox.WallDistance(mesh, sel, bins=tuple(4 * b for b in info["bins_per_axis"]))
    assert brute.info()["bins"] == 1 and brute.info()["list"] == wd.n_facets
    for k, (b, b4) in enumerate(zip(info["bins_per_axis"], fine.info()["bins_per_axis"])):  # (a flat axis keeps its one bin)
        assert b4 == (4 * b if np.ptp(xyz[..., k]) > 0.0 else 1), (k, b, b4)
    Q, V2 = _queries(mesh, xyz)
    worst = []
    for name, x in Q.items():
        dist, near = _check(f"{kind}/{walls}/{name}", wd, xyz, x, worst=worst)
        for other in (brute, fine, wd):  # (d)
            d2, n2 = other.query(x)
            assert torch.equal(dist, d2) and torch.equal(near, n2), name
        if name == "vertices":  # (c)
            assert bool((dist == 0.0).all())
        if name == "midpoints":
            C, L = WD.distance_bound(xyz, x)
            assert float(dist.max()) <= C * EPS * L
    print(f"{kind}/{walls}: worst {max(worst):.2f} eps L, bins {info['bins_per_axis']}, list {info['list']}")
    # (e)
    bad = Q["random"][:7].copy()
    bad[1, 0], bad[3, d - 1], bad[5, 1] = np.nan, np.inf, -np.inf
    dist, near = wd.query(bad)
    dist, near = dist.cpu().numpy(), near.cpu().numpy()
    assert np.isnan(dist[[1, 3, 5]]).all() and (near[[1, 3, 5]] == -1).all()
    assert np.isfinite(dist[[0, 2, 4, 6]]).all() and (near[[0, 2, 4, 6]] >= 0).all()
    dist, near = wd.query(np.zeros((0, d)))
    assert tuple(dist.shape) == (0,) and tuple(near.shape) == (0,) and near.dtype == torch.int32
    # cells(): the centroids in the mesh's cell order
    dc, nc = wd.cells()
    d0, n0 = wd.query(Q["centroids"])
    assert torch.equal(dc, d0) and torch.equal(nc, n0)
    # (g) function(V) holds query(V.x), is evaluated by eval at the dofs' points and is sampled by Probes
    f = wd.function(V2)
    dv, _ = wd.query(V2.x)
    assert torch.equal(f._storage.rdev()[: int(dv.shape[0]), 0], dv)
    pts = Q["p2_dofs"][:: max(1, Q["p2_dofs"].shape[0] // 16)]
    vals = f.eval(pts)[:, 0]
    ref = wd.query(pts)[0].cpu().numpy()
    assert np.abs(np.asarray(vals) - ref).max() <= 1e-12 * max(1.0, ref.max())


def test_tagged_walls_are_ordered_by_tag_then_id(hip):
    """(meshtags, ids): the facets of the listed tags in that order, each by facet id; nearest is a position in it."""
    import oasisx_amd as ox
    from oasisx_amd import mesh as M
    from tests import walldist_model as WD

    mesh = _mesh("box")
    _, bottom = _wall_ids(mesh, "one_face")
    _, both = _wall_ids(mesh, "opposite")
    top = np.setdiff1d(both, bottom)
    ent = np.concatenate([bottom, top])
    val = np.concatenate([np.full(bottom.shape[0], 7), np.full(top.shape[0], 3)])
    order = np.argsort(ent)
    tags = M.meshtags(mesh, 2, ent[order].astype(np.int32), val[order].astype(np.int32))
    wd = ox.WallDistance(mesh, (tags, (7, 3)))
    assert np.array_equal(wd.facets, np.concatenate([np.sort(bottom), np.sort(top)]))
    x = np.array([[0.4, 0.1, 0.3], [1.7, 0.8, 1.2]])
    dist, near = wd.query(x)
    assert np.abs(dist.cpu().numpy() - [0.1, 0.2]).max() <= 22 * EPS * 3.0
    near = near.cpu().numpy()
    assert near[0] < bottom.shape[0] <= near[1]
    D = WD.distances(_facet_xyz(mesh, wd.facets), x)
    assert np.abs(D[[0, 1], near] - [0.1, 0.2]).max() <= 22 * EPS * 3.0


def test_periodic_images(hip):
    """(f) A 6 x 4 rectangle, periodic in x.  Wall: the facets of y = 0 whose midpoint has x > 1.5; queries at x < 0.3
    reach it across the seam: the model's minimum over the images x + s * period.  On the full walls (facets=None: the
    exterior facets without the seam) the closed form min(y, 1 - y)."""
    import oasisx_amd as ox
    from oasisx_amd import mesh as M
    from tests import walldist_model as WD

    mesh = M.make_periodic(M.create_rectangle(None, [[0.0, 0.0], [2.0, 1.0]], [6, 4]), (0,))
    fv, _ = mesh._entities(1)
    X = mesh.coords.cpu().numpy()
    ext = np.asarray(mesh.exterior_facets(), dtype=np.int64)
    mid = X[fv[ext]].mean(axis=1)
    patch = ext[np.isclose(mid[:, 1], 0.0) & (mid[:, 0] > 1.5)]
    assert patch.shape[0] == 1 or patch.shape[0] == 2
    wd = ox.WallDistance(mesh, patch)
    xyz = _facet_xyz(mesh, wd.facets)
    rng = np.random.default_rng(3)
    x = np.stack([rng.uniform(0.0, 0.3, 64), rng.uniform(0.0, 1.0, 64)], axis=1)
    shifts = WD.image_shifts(np.asarray(mesh.periodic.period, dtype=np.float64), mesh.periodic.axes)
    dist, _ = _check("periodic patch", wd, xyz, x, shifts)
    plain = WD.nearest(xyz, x)[0]
    assert (dist.cpu().numpy() < plain - 0.5).all()  # (every one of them is nearer across the seam)
    full = ox.WallDistance(mesh)
    assert np.array_equal(full.facets, np.sort(ext)) and not np.isin(mesh.periodic_facets(), full.facets).any()
    x = np.stack([rng.uniform(-0.5, 2.5, 200), rng.uniform(0.0, 1.0, 200)], axis=1)
    dist, _ = full.query(x)
    assert np.abs(dist.cpu().numpy() - np.minimum(x[:, 1], 1.0 - x[:, 1])).max() <= 22 * EPS * 4.0
