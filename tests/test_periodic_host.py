"""CPU: periodic meshes (oasisx_amd.mesh.make_periodic) and the spaces numbered on them, through the torch twin of the
set-up (CPU meshes): vertex maps, refusals, dof counts and coordinates, the oracle's operators on the merged tables,
boundary-condition lookups on both images of a face."""
import numpy as np
import pytest

from oracle import ipcs_oracle as O


def _mesh(dim, n, p0=None, p1=None):
    from oasisx_amd import mesh as M

    p0 = [0.0, -1.0, 0.5][:dim] if p0 is None else p0
    p1 = [3.0, 1.0, 2.0][:dim] if p1 is None else p1
    if dim == 2:
        return M.create_rectangle(None, [p0, p1], list(n), device="cpu")
    return M.create_box(None, [p0, p1], list(n), device="cpu")


CASES = [(2, (4, 5), (0,)), (2, (4, 5), (0, 1)), (3, (3, 4, 5), (0, 2)), (3, (3, 4, 3), (0, 1, 2))]


@pytest.mark.parametrize("dim,n,axes", CASES)
def test_maps(dim, n, axes):
    from oasisx_amd import mesh as M

    m = _mesh(dim, n)
    pm = M.make_periodic(m, axes)
    per = pm.periodic
    assert per.axes == axes
    x = m.coords.numpy()
    lo, hi = x.min(axis=0), x.max(axis=0)
    exp_period = np.array([hi[k] - lo[k] if k in axes else 0.0 for k in range(dim)])
    assert np.allclose(per.period, exp_period, rtol=0, atol=1e-15)
    vm = per.vertex_master
    assert vm.dtype == np.int64 and vm.shape == (m.num_vertices,)
    assert (vm[vm] == vm).all()  # idempotent
    # a master lies at lo -- never at hi -- on every periodic axis, and differs from its slaves by whole periods only
    for k in range(dim):
        if k in axes:
            assert (x[vm, k] < hi[k] - 1e-9).all()
            shift = (x[:, k] - x[vm, k]) / per.period[k]
            assert np.abs(shift - np.round(shift)).max() < 1e-12
        else:
            assert np.abs(x[:, k] - x[vm, k]).max() < 1e-12
    sizes = np.bincount(vm, minlength=m.num_vertices)
    on_hi = np.stack([np.isclose(x[:, k], hi[k]) | np.isclose(x[:, k], lo[k]) for k in axes], axis=1).sum(axis=1)
    masters = np.nonzero(sizes)[0]
    assert (sizes[masters] == 2 ** on_hi[masters]).all()  # corner classes: 2^k members
    assert sizes.max() == 2 ** len(axes)
    expect_free = int(np.prod([n[k] if k in axes else n[k] + 1 for k in range(dim)]))
    assert per.n_free_vertices == expect_free == masters.shape[0]
    # exterior facets shrink by exactly the identified ones
    ext0, ext1, idf = m.exterior_facets(), pm.exterior_facets(), pm.periodic_facets()
    assert np.intersect1d(ext1, idf).size == 0
    assert np.array_equal(np.sort(np.concatenate([ext1, idf])), ext0)
    per_face = {2: lambda k: n[1 - k], 3: lambda k: 2 * int(np.prod([n[j] for j in range(3) if j != k]))}[dim]
    assert idf.shape[0] == sum(2 * per_face(k) for k in axes)
    assert m.periodic is None and m.periodic_facets().size == 0
    assert np.array_equal(pm.coords.numpy(), x) and np.array_equal(pm.cells.numpy(), m.cells.numpy())


def test_value_errors():
    from oasisx_amd import mesh as M

    # fewer than three cells across
    with pytest.raises(ValueError, match="axis 0.*three cells"):
        M.make_periodic(_mesh(2, (2, 4)), (0,))
    with pytest.raises(ValueError, match="axis 2.*three cells"):
        M.make_periodic(_mesh(3, (3, 3, 2)), (0, 2))
    # one vertex of the hi face moved along the face by 1e-3
    m = _mesh(3, (3, 3, 3))
    x = m.coords.numpy().copy()
    v = int(np.nonzero(np.isclose(x[:, 0], 3.0) & np.isclose(x[:, 1], -1.0 + 2.0 / 3.0) & np.isclose(x[:, 2], 1.0))[0][0])
    x[v, 1] += 1e-3
    with pytest.raises(ValueError, match="axis 0.*vertices"):
        M.make_periodic(M.from_arrays(x, m.cells.numpy(), device="cpu"), (0,))
    # ... and off the face
    x = m.coords.numpy().copy()
    x[v, 0] -= 1e-3
    with pytest.raises(ValueError, match="axis 0.*vertices"):
        M.make_periodic(M.from_arrays(x, m.cells.numpy(), device="cpu"), (0,))
    # the hi face re-triangulated: flip the diagonal of one pair of facets (the two tetrahedra behind them re-cut)
    cells = m.cells.numpy().copy()
    xs = m.coords.numpy()
    fv, cf = m._entities(2)
    on_hi = np.isclose(xs[:, 0], 3.0)
    hi_f = np.nonzero(on_hi[fv].all(axis=1))[0]
    done = False
    for i, fa in enumerate(hi_f):
        for fb in hi_f[i + 1:]:
            shared = np.intersect1d(fv[fa], fv[fb])
            if shared.shape[0] != 2:
                continue
            a, b = int(np.setdiff1d(fv[fa], shared)[0]), int(np.setdiff1d(fv[fb], shared)[0])
            ca, cb = int(np.nonzero((cf == fa).any(axis=1))[0][0]), int(np.nonzero((cf == fb).any(axis=1))[0][0])
            pa, pb = np.setdiff1d(cells[ca], fv[fa]), np.setdiff1d(cells[cb], fv[fb])
            if ca == cb or pa[0] != pb[0]:
                continue  # (flip only a pair whose two tetrahedra share their fourth vertex: the result is conforming)
            s0, s1, apex = int(shared[0]), int(shared[1]), int(pa[0])
            cells[ca] = [a, b, s0, apex]
            cells[cb] = [a, b, s1, apex]
            done = True
            break
        if done:
            break
    assert done
    with pytest.raises(ValueError, match="axis 0.*facets"):
        M.make_periodic(M.from_arrays(xs, cells, device="cpu"), (0,))
    with pytest.raises(ValueError, match="axes"):
        M.make_periodic(_mesh(2, (4, 4)), (2,))


def test_faces_with_round_off_match():
    """Matching vertices that differ by round-off below the tolerance are paired wherever they lie (an imported mesh):
    the vertices of the identified faces moved along them by up to 0.45 of the tolerance, 20 draws."""
    from oasisx_amd import mesh as M

    for dim, n, axes in ((2, (5, 4), (0, 1)), (3, (4, 5, 4), (0, 1, 2))):
        # the unit box with 4 or 5 cells a side: every lattice coordinate is a whole multiple of 2 atol, the width of the
        # search grid's cells, so about half of the moved vertices leave the cell of their image
        m = _mesh(dim, n, p0=[0.0] * dim, p1=[1.0] * dim)
        x = m.coords.numpy().copy()
        lo, hi = x.min(axis=0), x.max(axis=0)
        atol = 1e-8 * (hi - lo)
        rng = np.random.default_rng(11)
        for _ in range(20):
            # every vertex of an identified face moves by up to 0.45 atol along the faces it lies in (never across one):
            # two images then differ by up to 0.9 atol
            on_face = np.stack([np.isclose(x[:, j], lo[j]) | np.isclose(x[:, j], hi[j]) for j in range(dim)], axis=1)
            move = (rng.random(x.shape) - 0.5) * 0.9 * atol
            move[on_face] = 0.0
            move[~on_face[:, list(axes)].any(axis=1)] = 0.0
            y = x + move
            pm = M.make_periodic(M.from_arrays(y, m.cells.numpy(), device="cpu"), axes)
            ref = M.make_periodic(m, axes)
            assert np.array_equal(pm.periodic.vertex_master, ref.periodic.vertex_master)


def test_delaunay_box_faces_do_not_match():
    """The Delaunay-box generator jitters the points of opposite faces independently: refused, naming the axis."""
    from oasisx_amd import mesh as M

    m = M.create_delaunay_box(None, [[0.0, 0.0], [1.0, 1.0]], 5, seed=1, device="cpu")
    with pytest.raises(ValueError, match="axis 0"):
        M.make_periodic(m, (0,))


@pytest.fixture(scope="module")
def spaces():
    """(mesh, periodic mesh, {degree: space}) per case, built once."""
    from oasisx_amd import fem
    from oasisx_amd import mesh as M

    out = {}
    for dim, n, axes in CASES:
        m = _mesh(dim, n)
        pm = M.make_periodic(m, axes)
        out[(dim, n, axes)] = (m, pm, {deg: fem.FunctionSpace(pm, deg, window=128) for deg in (1, 2)})
    return out


@pytest.mark.parametrize("dim,n,axes", CASES)
@pytest.mark.parametrize("deg", [1, 2])
def test_dof_counts_and_coordinates(spaces, dim, n, axes, deg):
    m, pm, Vs = spaces[(dim, n, axes)]
    V = Vs[deg]
    # lattice argument: deg * n_k points along a periodic axis, deg * n_k + 1 along a wall axis
    expect = int(np.prod([deg * n[k] if k in axes else deg * n[k] + 1 for k in range(dim)]))
    assert V.num_dofs == expect == V.n_owned == V.num_dofs_global
    assert V.pattern.n_rows == expect
    x = V.x.numpy()
    assert x.shape == (expect, dim) and np.isfinite(x).all()
    lo, hi = m.coords.numpy().min(axis=0), m.coords.numpy().max(axis=0)
    for k in axes:
        assert (x[:, k] >= lo[k]).all() and (x[:, k] < hi[k]).all()
    # every (cell, local node): the dof's coordinates differ from the geometric node by whole periods, periodic axes only
    cells = V.cells_in_kernel_order()
    X = m.coords.numpy()[cells]
    if deg == 2:
        X = np.concatenate([X] + [0.5 * (X[:, [a]] + X[:, [b]]) for a, b in O.local_edges(dim)], axis=1)
    diff = x[V.cell_dofs.numpy().astype(np.int64)] - X
    for k in range(dim):
        if k in axes:
            q = diff[:, :, k] / pm.periodic.period[k]
            assert np.abs(q - np.round(q)).max() < 1e-12
            assert set(np.unique(np.round(q)).astype(int)) <= {-1, 0}
        else:
            assert np.abs(diff[:, :, k]).max() < 1e-14
    assert len(np.unique(np.round(x, 9), axis=0)) == expect  # one dof per point


@pytest.mark.parametrize("dim,n,axes", CASES)
@pytest.mark.parametrize("deg", [1, 2])
def test_operators_on_merged_tables(spaces, dim, n, axes, deg):
    m, pm, Vs = spaces[(dim, n, axes)]
    V, Q = Vs[deg], Vs[1]
    F = O.Forms(m.coords.numpy(), V.cells_in_kernel_order(), deg, 1, vd=V.cell_dofs.numpy(), qd=Q.cell_dofs.numpy(),
                nv_dofs=V.num_dofs, nq_dofs=Q.num_dofs)
    Mm, K = F.mass_v(), F.stiffness_v()
    vol = float(np.prod(m.coords.numpy().max(axis=0) - m.coords.numpy().min(axis=0)))
    assert abs(Mm.sum() - vol) < 1e-13 * max(1.0, vol)  # (test_oracle_pins.test_exactness_identities: 1e-13 at vol ~ 1)
    assert np.abs(K @ np.ones(F.nv)).max() < 1e-12
    assert abs(Mm - Mm.T).max() < 1e-15 and abs(K - K.T).max() < 1e-13
    rng = np.random.default_rng(0)
    C = F.convection(rng.standard_normal((F.nv, dim)))
    assert np.abs(C @ np.ones(F.nv)).max() < 1e-13 * 10
    # the product's pattern holds exactly these entries
    P = V.pattern
    csr = P.to_csr(P.new_values() + 1.0)
    Mm.eliminate_zeros()
    assert csr.nnz == P.nnz and set(zip(*Mm.nonzero())) <= set(zip(*csr.nonzero()))
    if deg == 1 and len(axes) == dim:
        lens = np.unique(P.row_len.numpy())
        assert lens.tolist() == [7 if dim == 2 else 15]  # one row length on the fully periodic P1 box


@pytest.mark.parametrize("dim,n,axes", CASES)
@pytest.mark.parametrize("deg", [1, 2])
def test_bc_lookups_on_both_images(spaces, dim, n, axes, deg):
    from oasisx_amd import fem
    from oasisx_amd import mesh as M

    m, pm, Vs = spaces[(dim, n, axes)]
    V = Vs[deg]
    x = m.coords.numpy()
    fv, _ = pm._entities(dim - 1)
    per = pm.periodic
    k = axes[0]
    lo, hi = x.min(axis=0), x.max(axis=0)
    hi_f = np.nonzero(np.isclose(x[fv][:, :, k], hi[k]).all(axis=1))[0]
    lo_f = np.nonzero(np.isclose(x[fv][:, :, k], lo[k]).all(axis=1))[0]
    assert set(hi_f) | set(lo_f) <= set(per.facets)
    mid = x[fv].mean(axis=1)
    for f in hi_f[:: max(1, len(hi_f) // 4)]:
        target = mid[f].copy()
        target[k] = lo[k]
        g = lo_f[np.argmin(np.abs(mid[lo_f] - target).sum(axis=1))]
        assert np.abs(mid[g] - target).max() < 1e-12
        a = fem.locate_dofs_topological(V, dim - 1, np.array([f]))
        b = fem.locate_dofs_topological(V, dim - 1, np.array([g]))
        assert np.array_equal(a, b) and a.shape[0] == (dim if deg == 1 else (3 if dim == 2 else 6))
        # the dofs are the ones at the lo image's points
        xa = V.x.numpy()[a]
        assert np.abs(xa[:, k] - lo[k]).max() < 1e-12
    # vertex ids of both images give the master's dof
    vm = per.vertex_master
    import torch

    ids = torch.arange(m.num_vertices)
    loc = V.global_to_local(ids).numpy()
    assert np.array_equal(loc, loc[vm]) and len(np.unique(loc)) == per.n_free_vertices
    xm = x[vm]
    assert np.abs(V.x.numpy()[loc] - xm).max() < 1e-14
    # geometric and topological location of a wall agree, and exterior facets exclude the seam
    wall_axes = [j for j in range(dim) if j not in axes]
    if wall_axes:
        j = wall_axes[0]
        facets = M.locate_entities_boundary(pm, dim - 1, lambda X: np.isclose(X[j], hi[j]))
        assert facets.size and not per.is_periodic_facet(facets).any()
        topo = fem.locate_dofs_topological(V, dim - 1, facets)
        geo = fem.locate_dofs_geometrical(V, lambda X: np.isclose(X[j], hi[j]))
        assert np.array_equal(np.sort(topo), np.sort(geo))
    else:
        assert pm.exterior_facets().size == 0
        assert M.locate_entities_boundary(pm, dim - 1, lambda X: np.full(X.shape[1], True)).size == 0


def test_interpolate_uses_dof_coordinates(spaces):
    from oasisx_amd.fem import Function

    m, pm, Vs = spaces[CASES[1]]
    V = Vs[2]
    f = Function(V)
    f.interpolate(lambda X: np.sin(2 * np.pi * X[0] / 3.0) + X[1])
    x = V.x.numpy()
    assert np.array_equal(f.x.array, np.sin(2 * np.pi * x[:, 0] / 3.0) + x[:, 1])


class _RaisingComm:
    """A communicator of two ranks whose collectives raise: a refusal must come before any of them."""

    rank, size = 0, 2

    def allreduce(self, *a, **k):
        raise AssertionError("collective before the refusal")

    Barrier = _all_ok = allreduce


def test_refusals():
    import oasisx_amd as ox
    from oasisx_amd import fem
    from oasisx_amd import mesh as M

    pm = M.make_periodic(_mesh(2, (4, 4)), (0,))
    with pytest.raises(NotImplementedError, match="degree 3"):
        fem.FunctionSpace(pm, 3)
    with pytest.raises(NotImplementedError, match="degree 3"):
        fem.functionspace(pm, ("Lagrange", 3))  # (the boundary-condition-only high-order space numbers geometric entities)
    assert fem.functionspace(pm, ("Lagrange", 2)).num_dofs == 4 * 2 * (4 * 2 + 1)
    with pytest.raises(NotImplementedError, match="P3-P2"):
        ox.FractionalStep_AB_CN(pm, ("Lagrange", 3), ("Lagrange", 2), bcs_u=[[], []], bcs_p=[])
    base = _mesh(2, (4, 4))
    base.comm = _RaisingComm()
    pc = M.make_periodic(base, (0,))
    assert pc.comm is base.comm
    with pytest.raises(NotImplementedError, match="periodic"):
        fem.FunctionSpace(pc, 2)
    with pytest.raises(NotImplementedError, match="periodic"):
        ox.FractionalStep_AB_CN(pc, ("Lagrange", 2), ("Lagrange", 1), bcs_u=[[], []], bcs_p=[])


def test_facet_addons_refuse_identified_facets():
    from oasisx_amd import mesh as M
    from oasisx_amd.wall import facet_table

    pm = M.make_periodic(_mesh(2, (4, 4)), (0,))
    seam = pm.periodic_facets()
    with pytest.raises(ValueError, match="identified"):
        facet_table(pm, seam[:2])
    cell, opp = facet_table(pm, pm.exterior_facets())
    assert cell.shape[0] == pm.exterior_facets().shape[0] == 8
