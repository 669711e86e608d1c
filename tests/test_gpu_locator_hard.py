"""GPU: the cell locator, ``Function.eval`` and ``Probes`` (csrc/ox_probe.hip) on the meshes of tests/hard_meshes.py --
the 254-wide fan and spindle, slivers of aspect 1e4, flat tetrahedra, millimetre cells a kilometre from the origin, cells
of both orientations -- against the extended-precision model of tests/locator_model.py.

Location: only DECIDED points are fed (every comparison of the device has a margin above the counted bound on its
barycentric coordinates; asserted on the host), so ``find`` must return the model's lowest containing cell for every
point, and ``bary`` must lie within the counted bound of lambda*.  Evaluation: the model's sum over the device's own
``bary`` under ``assembly_model.check`` (|dev - value| <= (n + 2) 2^-53 B).  Grid economy: at most four bins per cell on
every mesh, at least a quarter of a bin per cell on the lattice-derived ones; the grids of the isotropic meshes of
tests/test_gpu_probes.py are the ones the single-length rule gave."""
import numpy as np
import pytest
import torch

from tests import assembly_model as AM
from tests import hard_meshes as H
from tests import locator_model as LM
from tests import probe_model as PM

pytestmark = pytest.mark.gpu

ZOO = [(d, name) for d in (2, 3) for name in H.zoo(d, 1)]
LATTICE = ("stretched", "squashed", "tiny_far", "flipped")
_CACHE = {}


def _case(d, name, degree=1):
    """The mesh on the device and the decided point classes of the model, computed once per mesh and left unchanged."""
    key = (d, name, degree)
    if key not in _CACHE:
        from oasisx_amd import mesh as M

        mesh = M.from_arrays(*H.zoo(d, degree)[name])
        coords, cells = mesh.coords.cpu().numpy(), mesh.cells.cpu().numpy()
        P = LM.point_classes(coords, cells, seed=d, corners=name in ("fan254", "spindle254"))
        _CACHE[key] = (mesh, coords, cells, P)
    return _CACHE[key]


def _check_classes(d, name, P):
    """The split of the candidates is as the model's host test states it: nothing dropped, no class empty -- but
    ``within_tol`` on tiny_far, where float64 near 1e3 moves lambda in steps of about 1.7e-10."""
    for cls, v in P.items():
        if cls == "within_tol" and name == "tiny_far":
            continue
        assert v["dropped"] == 0 and v["x"].shape[0] > 0, (d, name, cls, v["dropped"], v["x"].shape)


def _bary_ratio(coords, cells, x, cell, dev):
    """max |dev - lambda*| / bound over the points (cell >= 0 everywhere), and the largest bound."""
    lam, bnd = LM.bary_in_cells(coords, cells, x, cell)
    return float(LM.bary_ratio(dev, lam, bnd).max()), float(bnd.max())


# ---- 1. location ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,name", ZOO)
def test_location_on_the_zoo_equals_the_model(hip, d, name):
    from oasisx_amd import geometry as G

    mesh, coords, cells, P = _case(d, name)
    _check_classes(d, name, P)
    x = np.concatenate([v["x"] for v in P.values()])
    want = np.concatenate([v["cell"] for v in P.values()])
    inside = want >= 0
    n_out = {c: int(P[c]["x"].shape[0]) for c in LM.OUTSIDE if c in P}
    assert all((P[c]["cell"] == -1).all() for c in n_out) and all((P[c]["cell"] >= 0).all() for c in LM.INSIDE if c in P)
    tree = G.bb_tree(mesh, d)
    c1, b1 = tree.find(x)
    got = c1.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (name, bad[:10], got[bad[:10]], want[bad[:10]], x[bad[:10]])
    bary = b1.cpu().numpy()
    assert np.isnan(bary[~inside]).all() and not np.isnan(bary[inside]).any()
    ratio, worst = _bary_ratio(coords, cells, x[inside], want[inside], bary[inside])
    print(f"RATIO location {d}-D {name}: worst |bary - lambda*| / bound = {ratio:.3f} (allowance 1; the largest bound {worst:.2e}, "
          f"{int(inside.sum())} points inside, {int((~inside).sum())} outside)")
    assert ratio <= 1.0, (name, ratio)
    assert worst < 0.1 * tree.tol  # the relation the decisions rest on: the bound stays well under the tolerance
    # the same bits from the cells given, and from a second call
    b3 = tree.bary(x, c1)
    assert torch.equal(b3[inside], b1[inside]) and bool(torch.isnan(b3[~inside]).all())
    c2, b2 = tree.find(torch.from_numpy(x).cuda())
    assert torch.equal(c1, c2) and torch.equal(b1[inside], b2[inside])
    # every third cell, handed over in descending order: the model restricted to them (the same points: a point decided
    # in every cell is decided in every third)
    sub = np.arange(1, mesh.num_cells, 3)
    R = LM.locate(coords, cells, x, cell_ids=sub)
    assert R["decided"].all()
    csub, bsub = G.bb_tree(mesh, d, entities=sub[::-1].copy()).find(x)
    assert np.array_equal(csub.cpu().numpy(), R["cell"]) and (R["cell"] >= 0).sum() > 50 and (R["cell"][inside] < 0).sum() > 50
    hit = R["cell"] >= 0
    rs, _ = _bary_ratio(coords, cells, x[hit], R["cell"][hit], bsub.cpu().numpy()[hit])
    assert rs <= 1.0, (name, rs)


# ---- 2. grid economy -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,name", ZOO)
def test_the_grid_has_about_one_bin_per_cell(hip, d, name):
    from oasisx_amd import geometry as G

    mesh, coords, cells, _ = _case(d, name)
    info = G.bb_tree(mesh, d).info()
    model = LM.grid_sizing(coords, cells, rule="axis")
    old = LM.grid_sizing(coords, cells, rule="isotropic")
    print(f"GRID {d}-D {name}: cells {info['cells']}, bins per axis {info['bins_per_axis']}, bins {info['bins']}, list {info['list']} "
          f"(the single-length rule, emulated: {old['nb']}, bins {old['bins']}, list {old['list']}, widest cell {old['span']} bins)")
    assert info["cells"] == mesh.num_cells and int(np.prod(info["bins_per_axis"])) == info["bins"]
    assert info["bins"] <= 4 * mesh.num_cells, info
    if name in LATTICE:
        assert info["bins"] >= 0.25 * mesh.num_cells, info
    assert model["frac"] > 1e-6 and info["bins_per_axis"] == model["nb"] and info["list"] == model["list"], (info, model)


@pytest.mark.parametrize("kind,nb", [("box2", [23, 23]), ("box3", [15, 15, 15]), ("delaunay", [12, 12, 12])])
def test_isotropic_meshes_keep_their_grids(hip, kind, nb):
    from oasisx_amd import geometry as G
    from tests.test_gpu_probes import _mesh

    mesh = _mesh(kind)
    coords, cells = mesh.coords.cpu().numpy(), mesh.cells.cpu().numpy()
    old = LM.grid_sizing(coords, cells, rule="isotropic")
    info = G.bb_tree(mesh, mesh.gdim).info()
    assert old["nb"] == nb and old["frac"] > 1e-6  # what the single-length rule gave (3 375 bins on box3)
    assert info["bins_per_axis"] == nb and info["list"] == old["list"], (info, old)


# ---- 3. the tile offsets of the bin scan -----------------------------------------------------------------------------------
def test_scan_over_five_tiles(hip):
    from oasisx_amd import geometry as G
    from oasisx_amd import mesh as M

    tile = 2048  # OX_LOC_SCAN_TILE
    mesh = M.create_rectangle(None, [[-1.0, -1.0], [1.0, 1.0]], [64, 64])
    coords, cells = mesh.coords.cpu().numpy(), mesh.cells.cpu().numpy()
    tree = G.bb_tree(mesh, 2)
    info = tree.info()
    S = LM.grid_sizing(coords, cells)
    nbins = info["bins"]
    assert mesh.num_cells == 8192 and info["bins_per_axis"] == S["nb"] and info["list"] == S["list"]
    assert nbins >= 4 * tile and nbins % tile != 0 and nbins <= 4 * mesh.num_cells, info  # >= 4 tiles, the last not full
    ends = sorted({b for t in range((nbins + tile - 1) // tile) for b in (t * tile, min((t + 1) * tile, nbins) - 1)})
    ix, iy = np.array(ends) % S["nb"][0], np.array(ends) // S["nb"][0]
    centres = S["lo"] + (np.stack([ix, iy], axis=1) + 0.5) / S["inv_h"]
    x = np.concatenate([PM.sample_points(mesh, 300, 80, 80, seed=5, n_centroids=40), centres])
    want, wbary = PM.locate(coords, cells, x)
    # (float64 model: every comparison of it has a margin of 1e-12 or more -- the bound on these cells is below 1e-14)
    margin = min(float(np.abs(PM.barycentric(coords, cells, np.arange(mesh.num_cells), x[p:p + 64]).min(axis=2) + tree.tol).min())
                 for p in range(0, x.shape[0], 64))
    assert margin > 1e-12 and (want >= 0).all(), margin
    got, bary = tree.find(x)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.abs(bary.cpu().numpy() - wbary).max() < 1e-12
    print(f"scan: {nbins} bins in {(nbins + tile - 1) // tile} tiles, list {info['list']}, {x.shape[0]} points, margin {margin:.2e}")


# ---- 4. evaluation ---------------------------------------------------------------------------------------------------------
def _space(d, name, degree):
    from oasisx_amd import fem

    mesh, coords, cells, P = _case(d, name, degree)
    key = ("space", d, name, degree)
    if key not in _CACHE:
        V = fem.FunctionSpace(mesh, degree, window=256)
        W = fem.VectorFunctionSpace(V, d)
        w = fem.Function(W)
        rng = np.random.default_rng(100 * d + degree)
        dofs = rng.standard_normal((V.num_dofs, d))
        dofs[:, 1] += 1e6  # far from well-scaled data: the second right-hand side
        w._storage.host()[:, :] = dofs
        w._storage.rdev()  # (the host check-out goes back)
        _CACHE[key] = (V, w, dofs)
    return (mesh, coords, cells, P) + _CACHE[key]


def _inside_points(P):
    x = np.concatenate([P[c]["x"] for c in LM.INSIDE if c in P])
    cell = np.concatenate([P[c]["cell"] for c in LM.INSIDE if c in P])
    return x, cell


def _model_values(V, d, degree, dofs, cell, bary):
    cd = V.cell_dofs.cpu().numpy()[V.kernel_cell_index(cell)]
    return LM.evaluate(d, degree, bary, dofs[cd])


EVAL = [(d, name, degree) for d in (2, 3) for degree in (1, 2, 3) for name in H.zoo(d, degree)]


@pytest.mark.parametrize("d,name,degree", EVAL)
def test_eval_on_the_zoo_is_within_the_counted_bound(hip, d, name, degree):
    from oasisx_amd import fem
    from oasisx_amd import geometry as G

    mesh, coords, cells, P, V, w, dofs = _space(d, name, degree)
    _check_classes(d, name, P)
    x, cell = _inside_points(P)
    bary = G.space_tree(V).bary(x, cell).cpu().numpy()  # the device's own coordinates, as eval forms them
    val, B, n = _model_values(V, d, degree, dofs, cell, bary)
    gen = w._storage.generation
    given, located = w.eval(x, cell), w.eval(x)
    ok, r, allow = AM.check(given, val, B, n)
    print(f"RATIO eval {d}-D P{degree} {name}: worst |eval - value| / (u B) = {r:.2f} (allowance {allow:.0f}), {x.shape[0]} points, "
          f"max |value| = {float(np.abs(given).max()):.3e}")
    assert ok, (name, degree, r, allow)
    assert np.array_equal(given, located)  # decided points: the search finds the model's cell, and forms the same bary
    comp = fem.Function(V, "w1", w._storage, 1)  # one column of the block: the same sums
    assert np.array_equal(comp.eval(x, cell)[:, 0], given[:, 1])
    assert np.array_equal(w.eval(x, cell), given) and w._storage.generation == gen  # twice the same bits; evaluation reads


@pytest.mark.parametrize("d,name", [(3, "stretched"), (2, "tiny_far")])
def test_probes_on_the_zoo_sample_the_same_values(hip, d, name):
    import oasisx_amd as ox
    from oasisx_amd import geometry as G

    mesh, coords, cells, P, V, w, dofs = _space(d, name, 2)
    x, cell = _inside_points(P)
    pr = ox.Probes(x, w, capacity=1)
    pr.sample(0.0)
    pr.sample(1.0)
    A = pr.array()
    assert A.shape == (2, x.shape[0], d) and np.array_equal(pr.cells, cell) and np.array_equal(A[0], A[1])
    assert np.array_equal(A[0], w.eval(x, cell))
    bary = G.space_tree(V).bary(x, cell).cpu().numpy()
    val, B, n = _model_values(V, d, 2, dofs, cell, bary)
    ok, r, allow = AM.check(A[0], val, B, n)
    print(f"RATIO probes {d}-D P2 {name}: worst |sample - value| / (u B) = {r:.2f} (allowance {allow:.0f})")
    assert ok, (name, r, allow)
