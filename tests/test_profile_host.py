"""CPU: the reference of the slab-averaged statistics (tests/profile_model.py) against closed forms, its merge recurrence
against the space-time two-pass moments, the seeded recurrence on a mean of 1e6, ``oasisx_amd.slab_bins``, and the set-up
tables and argument checks of ``oasisx_amd.ProfileStatistics`` (built on the host: nothing is launched)."""
import math
import types

import numpy as np
import pytest

from tests import assembly_model as AM
from tests import diagnostics_model as DM
from tests import profile_model as PM
from tests import viscosity_model as VM


def _mesh_of(F):
    from oasisx_amd import mesh as M

    return M.from_arrays(F.coords, F.cells, device="cpu")


def _slabs(dim, N, deg, axis=1):
    """The oracle's lattice mesh on [-1, 1]^dim with the bins of ``oasisx_amd.slab_bins`` along ``axis``."""
    import oasisx_amd as ox

    F = VM.tg_forms(dim, N, deg, 2 if deg == 3 else 1)
    bins, edges = ox.slab_bins(_mesh_of(F), axis)
    assert edges.shape == (N + 1,) and np.allclose(edges, np.linspace(-1.0, 1.0, N + 1), atol=1e-14)
    assert np.array_equal(np.bincount(bins), np.full(N, F.cells.shape[0] // N))
    return F, PM.Slabs(DM.geometry_of_forms(F), F.vd, deg, bins), edges


def _one_sample(slabs, q):
    r = PM.recurrence(slabs, [q], [1.0])
    return AM.to_f64(r["mean"]), AM.to_f64(r["m2"]), r


# ---- 1. closed forms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N", [(2, 5), (3, 3)])
def test_linear_field_on_p1(dim, N):
    """q = (slope y + c, 2 x): the slab means of the first component are its values at the slab midpoints, its slab
    variance (slope h)^2 / 12; the second has mean 0 and variance 4/3 in every slab; the volumes add up to the box."""
    F, slabs, edges = _slabs(dim, N, 1)
    slope, c, h = 0.7, 0.2, 2.0 / N
    q = np.stack([slope * F.x_v[:, 1] + c, 2.0 * F.x_v[:, 0]], axis=1)
    mean, m2, r = _one_sample(slabs, q)
    mid = 0.5 * (edges[:-1] + edges[1:])
    assert np.abs(mean[:, 0] - (slope * mid + c)).max() < 1e-14 and np.abs(mean[:, 1]).max() < 1e-14
    assert np.abs(m2[:, 0] - (slope * h) ** 2 / 12.0).max() < 1e-15
    assert np.abs(m2[:, 2] - 4.0 / 3.0).max() < 1e-14 and np.abs(m2[:, 1]).max() < 1e-14  # (x and y are uncorrelated)
    assert abs(float(r["vol"].sum()) - 2.0 ** dim) < 1e-14
    assert r["n_mean"] <= AM.N_MAX and r["n_cov"] <= AM.N_MAX


@pytest.mark.parametrize("dim,N", [(2, 4), (3, 3)])
def test_quadratic_field_on_p2(dim, N):
    """q = y^2 is in P2 and the mass matrix integrates its square: slab mean (y1^3 - y0^3) / (3 h), slab variance
    (y1^5 - y0^5) / (5 h) - mean^2."""
    F, slabs, edges = _slabs(dim, N, 2)
    mean, m2, _ = _one_sample(slabs, F.x_v[:, 1:2] ** 2)
    y0, y1 = edges[:-1], edges[1:]
    want = (y1 ** 3 - y0 ** 3) / (3.0 * (y1 - y0))
    assert np.abs(mean[:, 0] - want).max() < 1e-14
    assert np.abs(m2[:, 0] - ((y1 ** 5 - y0 ** 5) / (5.0 * (y1 - y0)) - want ** 2)).max() < 1e-14


@pytest.mark.parametrize("dim,N", [(2, 4), (3, 3)])
def test_the_mean_is_not_a_nodal_average(dim, N):
    """A P2 field that is 1 on the vertex dofs and 0 on the edge dofs: the slab mean is the sum of the vertex functions'
    means, 0 on triangles and -1/5 on tetrahedra -- far from any average of the nodal values (all in [0, 1])."""
    F, slabs, _ = _slabs(dim, N, 2)
    q = np.zeros((F.x_v.shape[0], 1))
    q[np.unique(F.vd[:, : dim + 1]), 0] = 1.0
    assert 0 < int(q.sum()) < q.shape[0]
    mean, _, _ = _one_sample(slabs, q)
    w = AM.to_f64(AM.ref("weights", dim, 2)) * math.factorial(dim)
    rows = AM.to_f64(PM.mean_mass(dim, 2)).sum(axis=1)
    assert np.abs(rows - w).max() < 1e-16  # the row sums of the mean mass matrix are the means of the basis functions
    want = w[: dim + 1].sum()
    assert abs(want - (0.0 if dim == 2 else -0.2)) < 1e-15
    assert np.abs(mean[:, 0] - want).max() < 1e-14


# ---- 2. the recurrence -------------------------------------------------------------------------------------------------
def _levels(F, nq, offset=0.0):
    X = np.zeros((3, F.x_v.shape[0]))
    X[: F.x_v.shape[1]] = F.x_v.T
    return DM.stat_levels(X, nq, offset=offset)


@pytest.mark.parametrize("dim,N,deg,nq", [(2, 4, 2, 3), (3, 2, 1, 3), (2, 3, 3, 1)])
def test_recurrence_equals_two_pass(dim, N, deg, nq):
    """Twelve unequal weights: the merge recurrence in the extended type gives the space-time two-pass moments (both are
    exact up to a few hundred roundings of 2^-64: 1e-15 of the largest entry), the bounds dominate the values, and the
    same recurrence in float64 meets its counted bound."""
    F, slabs, _ = _slabs(dim, N, deg)
    ws = DM.STAT_WEIGHTS
    xs = _levels(F, nq)
    r = PM.recurrence(slabs, xs, ws)
    mean, m2 = PM.two_pass(slabs, xs, ws)
    assert np.abs(AM.to_f64(r["mean"] - mean)).max() <= 1e-15 * np.abs(AM.to_f64(mean)).max()
    assert np.abs(AM.to_f64(r["m2"] - m2)).max() <= 1e-15 * np.abs(AM.to_f64(m2)).max()
    assert r["W"] == sum(ws) and (r["Bm"] >= np.abs(AM.to_f64(mean))).all() and (r["Bc"] >= np.abs(AM.to_f64(m2))).all()
    r64 = PM.recurrence(slabs, xs, ws, dtype=np.float64)
    for name, B, n in (("mean", r["Bm"], r["n_mean"]), ("m2", r["Bc"], r["n_cov"])):
        ok, ratio, allow = AM.check(r64[name], r[name], B, np.full(B.shape, n))
        print(f"({dim},{N},{deg}) nq {nq} {name}: float64 against extended {ratio:.2f} of {allow:.0f}")
        assert ok, (name, ratio, allow)


@pytest.mark.parametrize("nq", [1, 3])
def test_seeding_keeps_the_variance_under_a_large_mean(nq):
    """On a mean of 1e6 the seeded recurrence in float64 stays within 1e-8 (relative to the largest entry) of the
    extended two-pass second moments -- the bound of test_stats_kernel_against_the_extended_recurrence --, while the first
    sample taken about 0, a raw second moment, does not."""
    F, slabs, _ = _slabs(2, 4, 2)
    ws = DM.STAT_WEIGHTS
    xs = _levels(F, nq, offset=1.0e6)
    ref = AM.to_f64(PM.two_pass(slabs, xs, ws)[1])
    scale = np.abs(ref).max(axis=0)
    seeded = (np.abs(PM.recurrence(slabs, xs, ws, dtype=np.float64)["m2"] - ref).max(axis=0) / scale).max()
    raw = (np.abs(PM.recurrence(slabs, xs, ws, dtype=np.float64, seed=False)["m2"] - ref).max(axis=0) / scale).max()
    print(f"nq {nq}: seeded {seeded:.2e}, first sample about 0 {raw:.2e}")
    assert seeded <= 1e-8 < raw


# ---- 3. slab_bins ------------------------------------------------------------------------------------------------------
def test_slab_bins_on_lattices():
    import oasisx_amd as ox
    from oasisx_amd import mesh as M

    m2 = M.create_rectangle(None, [[0.0, -1.0], [3.0, 1.0]], [4, 6], device="cpu")
    b, e = ox.slab_bins(m2, 1)
    assert b.dtype == np.int64 and b.shape == (48,) and np.array_equal(np.bincount(b), np.full(6, 8))
    cen = m2.coords[m2.cells].mean(dim=1).numpy()
    assert np.array_equal(b, np.searchsorted(e, cen[:, 1], side="right") - 1)
    b0, e0 = ox.slab_bins(m2, 0)
    assert e0.shape == (5,) and np.array_equal(np.bincount(b0), np.full(4, 12))
    m3 = M.create_box(None, [[0.0, -1.0, 0.0], [3.0, 1.0, 2.0]], [3, 4, 5], device="cpu")
    b3, e3 = ox.slab_bins(m3, 1)
    assert e3.shape == (5,) and np.array_equal(np.bincount(b3), np.full(4, 3 * 5 * 6))
    # a stretched, non-uniform set of planes (a wall-refined channel)
    x = m3.coords.numpy().copy()
    x[:, 1] = np.tanh(1.5 * x[:, 1]) / np.tanh(1.5)
    stretched = M.from_arrays(x, m3.cells.numpy(), device="cpu")
    bs, es = ox.slab_bins(stretched, 1)
    assert np.array_equal(bs, b3) and np.allclose(es, np.tanh(1.5 * e3) / np.tanh(1.5)) and np.ptp(np.diff(es)) > 0.1
    with pytest.raises(ValueError, match="axis"):
        ox.slab_bins(m2, 2)


def test_slab_bins_on_a_delaunay_box():
    import oasisx_amd as ox
    from oasisx_amd import mesh as M

    m = M.create_delaunay_box(None, [[-1.0] * 3, [1.0] * 3], 3, seed=2, device="cpu")
    with pytest.raises(ValueError, match=r"cell \d+ .*edges="):
        ox.slab_bins(m, 1)
    edges = np.linspace(-1.0, 1.0, 4)
    b, e = ox.slab_bins(m, 1, edges=edges)
    cen = m.coords[m.cells].mean(dim=1).numpy()[:, 1]
    assert np.array_equal(e, edges) and b.min() == 0 and b.max() == 2
    assert ((edges[b] <= cen) & (cen < edges[b + 1])).all()
    # outside the range: -1
    b, _ = ox.slab_bins(m, 1, edges=[-0.5, 0.0, 0.5])
    assert (b == -1).any() and np.array_equal(b == -1, (cen < -0.5) | (cen >= 0.5)) and set(np.unique(b)) == {-1, 0, 1}
    # a bin without a cell
    with pytest.raises(ValueError, match="bin 1 .*no cell"):
        ox.slab_bins(m, 1, edges=[-1.0, 0.3, 0.3 + 1e-9, 1.0])
    for bad in ([0.0], [0.0, 0.0, 1.0], [1.0, 0.0]):
        with pytest.raises(ValueError, match="strictly increasing"):
            ox.slab_bins(m, 1, edges=bad)


def test_slab_bins_of_a_periodic_mesh():
    import oasisx_amd as ox
    from oasisx_amd import mesh as M

    m = M.create_box(None, [[0.0, -1.0, 0.0], [3.0, 1.0, 2.0]], [4, 4, 4], device="cpu")
    p = M.make_periodic(m, (0, 2))
    assert p.periodic is not None
    for axis in (0, 1, 2):
        (b, e), (bp, ep) = ox.slab_bins(m, axis), ox.slab_bins(p, axis)
        assert np.array_equal(b, bp) and np.array_equal(e, ep)


# ---- 4. the set-up of ProfileStatistics ----------------------------------------------------------------------------------
def _stub_solver(m, comm=None):
    """What the constructor of ProfileStatistics reads of a solver, on the host (P2-P1): the mesh, the geometry records,
    the two spaces, the blocks of u and p, and the scalar lookup."""
    from oasisx_amd import fem

    if comm is not None:
        m.comm = comm
    Vi, Q = fem.FunctionSpace(m, 2, window=64), fem.FunctionSpace(m, 1, window=64)

    def scalar(name):
        raise KeyError(f"no scalar named {name!r} (have: [])")

    return types.SimpleNamespace(_mesh=m, _geom=fem.cell_geometry(m, Vi.local_cells), _Vi=[(Vi, None)], _Q=Q,
                                 _U=fem.FieldStorage(Vi.n_local, m.gdim, "cpu"), _P=fem.FieldStorage(Q.n_local, 1, "cpu"),
                                 scalar=scalar)


def test_chunk_tables_on_the_host():
    """The set-up tables on a 40 x 40 lattice (3200 cells): slabs along y (40 bins of 80 cells, one chunk each); bins of 1,
    255, 256, 257 cells, 300 cells left out and the rest (2131 cells, 9 chunks) in a fifth bin."""
    import oasisx_amd as ox
    from oasisx_amd import mesh as M

    m = M.create_rectangle(None, [[-1.0, -1.0], [1.0, 1.0]], [40, 40], device="cpu")
    S = _stub_solver(m)
    lc = S._Vi[0][0].local_cells.numpy()
    P = ox.ProfileStatistics(S, axis=1)
    assert (P.n_bins, P.n_chunks, P.n_sampled) == (40, 40, 3200) and P.names == ("u", "p") and [g.nq for g in P._groups] == [2, 1]
    lab = PM.chunk_labels(P._order.numpy(), P._chunks.numpy(), P._bin_chunk_ptr.numpy(), 3200)
    assert np.array_equal(lab, P._bins[lc])  # one chunk per bin: the chunk IS the bin
    assert P._partials.shape == (40, 1 + 2 + 3) and np.allclose(P.coordinates(), -1.0 + 0.05 * (np.arange(40) + 0.5))
    rng = np.random.default_rng(11)
    perm = rng.permutation(3200)
    cb = np.full(3200, 4, dtype=np.int64)
    at = 0
    for k, size in enumerate((1, 255, 256, 257)):
        cb[perm[at:at + size]] = k
        at += size
    cb[perm[at:at + 300]] = -1
    P = ox.ProfileStatistics(S, cell_bins=cb, fields=("p",))
    assert np.diff(P._bin_chunk_ptr.numpy()).tolist() == [1, 1, 1, 2, 9] and P.n_sampled == 2900 and P.coordinates() is None
    lab = PM.chunk_labels(P._order.numpy(), P._chunks.numpy(), P._bin_chunk_ptr.numpy(), 3200)
    assert np.array_equal(lab >= 0, cb[lc] >= 0) and np.array_equal(P._chunks.numpy()[lab[lab >= 0], 2], cb[lc][lab >= 0])
    assert P._partials.shape == (14, 1 + 2 + 3)  # (room for slab_mean of a velocity whatever is averaged)


def test_argument_validation():
    import oasisx_amd as ox
    from oasisx_amd import mesh as M
    from oasisx_amd.parallel import Comm

    m = M.create_unit_square(None, 3, 3, device="cpu")
    S = _stub_solver(m)
    for kw in ({}, dict(axis=1, cell_bins=np.zeros(18, dtype=np.int64))):
        with pytest.raises(ValueError, match="ProfileStatistics.*exactly one"):
            ox.ProfileStatistics(S, **kw)
    with pytest.raises(ValueError, match="ProfileStatistics: unknown field 'w'"):
        ox.ProfileStatistics(S, axis=1, fields=("w",))
    with pytest.raises(ValueError, match="ProfileStatistics: 3 scalars"):
        ox.ProfileStatistics(S, axis=1, scalars=("A", "B", "C"))
    with pytest.raises(ValueError, match="ProfileStatistics: no scalar named"):
        ox.ProfileStatistics(S, axis=1, scalars=("T",))
    with pytest.raises(ValueError, match="ProfileStatistics: cell_bins"):
        ox.ProfileStatistics(S, cell_bins=np.zeros(18))
    with pytest.raises(ValueError, match="ProfileStatistics: bin 0 holds no cell"):
        ox.ProfileStatistics(S, cell_bins=np.ones(18, dtype=np.int64))
    with pytest.raises(ValueError, match="no field"):
        ox.ProfileStatistics(S, axis=1, fields=())
    P = ox.ProfileStatistics(S, axis=0)
    for dt in (0.0, -1.0, float("inf")):
        with pytest.raises(ValueError, match="dt"):
            P.sample(dt)
    with pytest.raises(RuntimeError, match="ProfileStatistics"):
        P.mean("u")
    with pytest.raises(ValueError, match="no statistics"):
        P._get("T")
    with pytest.raises(NotImplementedError, match=r"ProfileStatistics.*comm.size > 1"):
        ox.ProfileStatistics(_stub_solver(M.create_unit_square(None, 3, 3, device="cpu"), Comm(0, 2, None, transport="host")), axis=1)
