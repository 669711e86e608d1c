"""GPU: periodic boundaries (oasisx_amd.mesh.make_periodic) from the library's set-up to output.  Identified dofs are one
dof, so a row of a wrap-around pattern has columns at both ends of the numbering: the storage forms of the mat-vecs (16-bit
column stream, value dictionaries, pair slots, LDS windows) and the row kernels of the assembly run on such rows here, on
the smallest meshes that have a seam in every form (N = 3, 4 in 3-D, N = 4 .. 6 in 2-D; windows of 128 rows), against the
CPU oracle fed the product's own tables."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAT, VEC = 1e-12, 1e-11  # tests/test_gpu_partitioned_bcs.py
WINDOW = 128


def _periodic(mesh, axes):
    from oasisx_amd import mesh as M

    return M.make_periodic(mesh, axes)


def _tg_mesh(dim, N):
    from tests.helpers import tg_mesh

    return _periodic(tg_mesh(dim, N), tuple(range(dim)))


def _solver(mesh, deg, bcs_u=None, solver_options=None, options=None, **kw):
    import oasisx_amd as ox
    from tests.helpers import KRYLOV

    d = mesh.gdim
    opts = {"sell_window": WINDOW, "low_memory_version": True}
    opts.update(options or {})
    return ox.FractionalStep_AB_CN(mesh, ("Lagrange", deg), ("Lagrange", 1), bcs_u=bcs_u or [[] for _ in range(d)], bcs_p=[],
                                   solver_options=solver_options or KRYLOV, options=opts, **kw)


def _forms(S):
    from oracle import ipcs_oracle as O

    Vi, Q, mesh = S._Vi[0][0], S._Q, S._mesh
    F = O.Forms(mesh.coords.cpu().numpy(), Vi.cells_in_kernel_order(), Vi.degree, Q.degree, vd=Vi.cell_dofs.cpu().numpy(),
                qd=Q.cell_dofs.cpu().numpy(), nv_dofs=Vi.num_dofs, nq_dofs=Q.num_dofs)
    return F, Vi.x.cpu().numpy(), Q.x.cpu().numpy()


def _twin(S, dofs=None, cls=None, **kw):
    """The oracle on the product's tables: no Dirichlet condition at all, or zero on ``dofs`` in every component."""
    from oracle import ipcs_oracle as O
    from tests.helpers import KRYLOV

    F, x_v, x_q = _forms(S)
    bcs = [[] if dofs is None else [O.DirichletData(dofs, 0.0)] for _ in range(F.d)]
    kw.setdefault("solver_options", KRYLOV)
    return (cls or O.OracleFractionalStep)(F, x_v, x_q, bcs, **kw)


def _X(x):
    X = np.zeros((3, x.shape[0]))
    X[: x.shape[1]] = x.T
    return X


def _set_fields(S, R, fns, p_fn):
    """u1 = u2 = the callables ``fns`` and p = ``p_fn`` on both sides (the product through ``interpolate``: V.x)."""
    for i, f in enumerate(fns):
        S._u1[i].interpolate(f)
        S._u2[i].interpolate(f)
    S._p.interpolate(p_fn)
    if R is not None:
        for i, f in enumerate(fns):
            R.u1[:, i] = R.u2[:, i] = f(_X(R.x_v))
        R.p[:] = p_fn(_X(R.x_q))


def _tg(dim, nu, shift=0.0, t=0.0):
    from oracle import ipcs_oracle as O

    def moved(f):
        def g(x):
            y = np.array(x, dtype=np.float64, copy=True)
            y[0] = y[0] + shift
            return f(y, t, nu)
        return g
    return [moved(f) for f in [O.tg_u, O.tg_v, O.tg_w][:dim]], moved(O.tg_p)


# ---- 1. native set-up -------------------------------------------------------------------------------------------------
SETUP = [("rect", (5, 7), (0,), 1), ("rect", (6, 5), (0, 1), 2), ("box", (3, 4, 3), (0, 1, 2), 2), ("box", (4, 3, 5), (0, 2), 1),
         ("box", (3, 4, 3), (1,), 2)]


def _setup_mesh(kind, n):
    from oasisx_amd import mesh as M

    if kind == "rect":
        return M.create_rectangle(None, [[0.0, -1.0], [3.0, 1.0]], list(n))
    return M.create_box(None, [[0.0, -1.0, 0.5], [3.0, 1.0, 2.0]], list(n))


@pytest.mark.parametrize("kind,n,axes,deg", SETUP)
def test_native_space_matches_the_torch_twin(hip, kind, n, axes, deg):
    """As tests/test_gpu_native_setup.py for plain meshes: the same dof count and operator pattern through the dof
    coordinates, V.x of every native dof equal to the twin's BITS (both write the master image), in [lo, hi) on periodic
    axes; identical arrays where the numbering coincides; adjacency positions pointing at the right columns."""
    import torch

    from oasisx_amd import fem

    mesh = _periodic(_setup_mesh(kind, n), axes)
    os.environ["OX_SETUP"] = "torch"
    try:
        Vt = fem.FunctionSpace(mesh, deg, window=WINDOW)
    finally:
        os.environ.pop("OX_SETUP")
    Vn = fem.FunctionSpace(mesh, deg, window=WINDOW)
    assert Vt.native is None and Vn.native is not None
    d = mesh.gdim
    expect = int(np.prod([deg * n[k] if k in axes else deg * n[k] + 1 for k in range(d)]))
    assert Vn.num_dofs == Vt.num_dofs == expect and Vn.pattern.nnz == Vt.pattern.nnz
    assert sorted(Vn._rank_initial.cpu().tolist()) == list(range(expect))
    x, xt = Vn.x.cpu().numpy(), Vt.x.cpu().numpy()
    assert np.isfinite(x).all()
    per = mesh.periodic
    for k in axes:
        assert (x[:, k] >= per.lo[k]).all() and (x[:, k] < per.hi[k]).all()

    def key(xx):
        return [tuple(np.round(r * 1e9).astype(np.int64)) for r in xx]
    kt = {k: i for i, k in enumerate(key(xt))}
    assert len(kt) == expect
    perm = np.array([kt[k] for k in key(x)])  # torch index of native dof i
    assert np.array_equal(x, xt[perm])
    assert np.array_equal(perm[Vn.cell_dofs.cpu().numpy()], Vt.cell_dofs.cpu().numpy()[
        Vt.kernel_cell_index(Vn.local_cells.cpu().numpy())])
    P = Vn.pattern
    ones_n = P.to_csr(torch.ones(P.size, dtype=torch.float64, device="cuda"))
    ones_t = Vt.pattern.to_csr(torch.ones(Vt.pattern.size, dtype=torch.float64, device="cuda"))
    assert abs(ones_n - ones_t[perm][:, perm]).max() == 0
    # every (cell, node): the dof's point is the geometric node up to whole periods
    cd = Vn.cell_dofs.cpu().numpy()
    Xc = mesh.coords.cpu().numpy()[Vn.cells_in_kernel_order()]
    if deg == 2:
        Xc = np.concatenate([Xc] + [0.5 * (Xc[:, [a]] + Xc[:, [b]]) for a, b in fem.local_edges(d)], axis=1)
    diff = x[cd] - Xc
    for k in range(d):
        q = diff[:, :, k] / per.period[k] if k in axes else diff[:, :, k]
        assert np.abs(q - np.round(q)).max() < 1e-12 and (k in axes or np.abs(q).max() == 0.0)
    # adjacency of the wrap-around rows: positions point at the right columns
    adj_cell, adj_loc = Vn.adj.adj_cell.cpu().numpy(), Vn.adj.adj_loc.cpu().numpy()
    adj_pos, ap = Vn.adj.adj_pos.cpu().numpy(), Vn.adj.adj_ptr.cpu().numpy()
    cols, sp = P.cols.cpu().numpy(), P.slice_ptr.cpu().numpy()
    seen = 0
    for s in range(min(P.n_slices, 6)):
        T = (ap[s + 1] - ap[s]) // 64
        for lane in range(64):
            r = s * 64 + lane
            if r >= expect:
                continue
            for t in range(T):
                e = adj_cell[ap[s] + t * 64 + lane]
                if e < 0:
                    continue
                seen += 1
                assert cd[e, adj_loc[ap[s] + t * 64 + lane]] == r
                for j in range(Vn.nd):
                    kk = int(adj_pos[ap[s] + t * 64 + lane, j])
                    assert cols[sp[s] + (kk // 2) * 128 + lane * 2 + (kk % 2)] == cd[e, j]
    assert seen > 0 and int(Vn.adj_count.sum().item()) == mesh.num_cells * Vn.nd
    if torch.equal(Vn.cell_dofs, Vt.cell_dofs):
        assert torch.equal(Vn.x, Vt.x) and torch.equal(P.cols, Vt.pattern.cols)
        assert torch.equal(Vn.adj.adj_pos, Vt.adj.adj_pos) and torch.equal(Vn.local_cells, Vt.local_cells)


def test_c_abi_alone(hip):
    """ox_mesh_create_periodic + ox_space_create through ctypes with host numpy arrays, nothing of the Python set-up but
    the vertex classes: the reduced count, x in [lo, hi) and the same space FunctionSpace wraps."""
    from oasisx_amd import _lib, fem

    lib = _lib.load()
    n, axes, deg = (3, 4, 3), (0, 2), 2
    mesh = _periodic(_setup_mesh("box", n), axes)
    per = mesh.periodic
    coords = np.ascontiguousarray(mesh.coords.cpu().numpy())
    cells = np.ascontiguousarray(mesh.cells.cpu().numpy().astype(np.int32))
    topo = np.ascontiguousarray(per.vertex_topo[mesh.cells.cpu().numpy()].astype(np.int32))
    cut = (C.c_double * 3)(per.hi[0] - per.atol[0], float("inf"), per.hi[2] - per.atol[2])
    M_, V_ = C.c_void_p(), C.c_void_p()
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    _lib.check(lib.ox_mesh_create_periodic(vp(coords), coords.shape[0], vp(cells), vp(topo), per.n_free_vertices, cells.shape[0],
                                           3, 0, -1, cut, C.byref(M_)), "ox_mesh_create_periodic")
    try:
        assert per.n_free_vertices == 3 * 5 * 3
        _lib.check(lib.ox_space_create(M_, deg, WINDOW, C.byref(V_)), "ox_space_create")
        try:
            v = _lib.ox_space_info()
            _lib.check(lib.ox_space_view(V_, C.byref(v)), "ox_space_view")
            nd_, ndofs = int(v.nd), int(v.n_dofs)
            assert ndofs == 6 * 9 * 6 and nd_ == 10
            cd = np.empty((cells.shape[0], nd_), dtype=np.int32)
            x = np.empty((ndofs, 3))
            _lib.check(lib.ox_memcpy(vp(cd), v.cell_dofs, cd.nbytes, 0, None), "ox_memcpy")
            _lib.check(lib.ox_memcpy(vp(x), v.x, x.nbytes, 0, None), "ox_memcpy")
            assert cd.min() == 0 and cd.max() == ndofs - 1
            for k in axes:
                assert (x[:, k] >= per.lo[k]).all() and (x[:, k] < per.hi[k]).all()
            Vn = fem.FunctionSpace(mesh, deg, window=WINDOW)
            assert np.array_equal(cd, Vn.cell_dofs.cpu().numpy()) and np.array_equal(x, Vn.x.cpu().numpy())
            # refusals of the library itself
            bad = C.c_void_p()
            assert lib.ox_space_create(M_, 3, WINDOW, C.byref(bad)) != 0
            # a hi_cut below the lo face leaves the dofs without any image to take coordinates from: the space is refused
            # by the library itself, not ordered from NaN keys
            low = (C.c_double * 3)(per.lo[0] - 1.0, float("inf"), per.hi[2] - per.atol[2])
            M2 = C.c_void_p()
            _lib.check(lib.ox_mesh_create_periodic(vp(coords), coords.shape[0], vp(cells), vp(topo), per.n_free_vertices,
                                                   cells.shape[0], 3, 0, -1, low, C.byref(M2)), "ox_mesh_create_periodic")
            try:
                assert lib.ox_space_create(M2, deg, WINDOW, C.byref(bad)) != 0
                assert b"no image below hi_cut" in lib.ox_last_error()
            finally:
                lib.ox_mesh_destroy(M2)
            topo_bad = topo.copy()
            topo_bad[0, 0] = per.n_free_vertices
            assert lib.ox_mesh_create_periodic(vp(coords), coords.shape[0], vp(cells), vp(topo_bad), per.n_free_vertices,
                                               cells.shape[0], 3, 0, -1, cut, C.byref(bad)) != 0
        finally:
            lib.ox_space_destroy(V_)
    finally:
        lib.ox_mesh_destroy(M_)


# ---- 2. operators -----------------------------------------------------------------------------------------------------
TG_CASES = [(2, 4, 1), (2, 6, 2), (3, 3, 2), (3, 4, 1)]


@pytest.fixture(scope="module")
def tg_solvers():
    """One periodic Taylor-Green solver and its oracle twin per case, shared by the operator and mat-vec tests (both
    leave the fields as they found them or set them anew)."""
    cache = {}

    def get(dim, N, deg, windows=False):
        key = (dim, N, deg, windows)
        if key not in cache:
            S = _solver(_tg_mesh(dim, N), deg, options={"spmv_windows": True} if windows else None)
            cache[key] = (S, None if windows else _twin(S))
        return cache[key]
    return get


@pytest.mark.parametrize("dim,N,deg", TG_CASES)
def test_operators_entry_by_entry(hip, tg_solvers, dim, N, deg):
    """M, K, Ap and, after one assemble_first on random velocity levels, A entry by entry (1e-12 max|.|) and b_first
    (1e-11 max|.|) against the oracle's matrices on the same tables; no row is an identity row."""
    S, R = tg_solvers(dim, N, deg)
    for name, mine, ref in (("M", S._M, R.M), ("K", S._K, R.K), ("Ap", S._Ap, R.Ap)):
        dA = abs(mine.to_scipy() - ref).max()
        print(f"({dim},{N},{deg}) {name}: max |d| = {dA:.3e}, max |ref| = {abs(ref).max():.3e}")
        assert dA <= MAT * abs(ref).max(), (name, dA)
    assert abs(S._vol - 2.0 ** dim) < 1e-12 and abs(R.vol - 2.0 ** dim) < 1e-12
    rng = np.random.default_rng(5)
    dt, nu = 0.1, 0.5
    u1, u2 = rng.standard_normal((S._n_u, dim)), rng.standard_normal((S._n_u, dim))
    for i in range(dim):
        S._u1[i].x.array[:] = u1[:, i]
        S._u2[i].x.array[:] = u2[:, i]
    ps = rng.standard_normal(S._n_q)
    S._ps.x.array[:] = ps
    R.u1[:], R.u2[:], R.ps[:] = u1, u2, ps
    S.assemble_first(dt, nu)
    R.assemble_first(dt, nu)
    A = S._A.to_scipy()
    dA = abs(A - R.A).max()
    bf = S._BFIRST.rhost()
    db = np.abs(bf - R.b_first).max()
    print(f"({dim},{N},{deg}) A: {dA:.3e} of {abs(R.A).max():.3e}; b_first: {db:.3e} of {np.abs(R.b_first).max():.3e}")
    assert dA <= MAT * abs(R.A).max() and db <= VEC * np.abs(R.b_first).max()
    assert np.abs(S._UAB.rhost() - (1.5 * u1 - 0.5 * u2)).max() < 1e-14


@pytest.mark.parametrize("dim,N,deg,windows", [c + (False,) for c in TG_CASES] + [c + (True,) for c in TG_CASES if c[2] == 2])
def test_matvecs_on_wrap_around_rows(hip, tg_solvers, dim, N, deg, windows):
    """y = A x for M, K (dictionary matrices), Ap and the assembled A, one and gdim columns, under every storage level the
    matrix carries (None = all; 1 plain stream; 3 + 16-bit columns; 7 + value codes; 15 + pair slots; 31 + LDS windows)
    against the CSR product of to_csr(): 1e-12 max|ref|, the bound of test_gpu_parity.test_spmv_matches_scipy; the
    LDS-window stream (options={"spmv_windows": True}) is built for P2 velocity patterns, so it runs on those.  Rows
    with columns at both ends of the numbering exist in every pattern, and every form exists on the matrices multiplied
    (both asserted): the 16-bit stream on both patterns; value codes on M, Ap and K (but K on P2 tetrahedra); and, since
    freeze() builds no pair slots on these patterns by itself, copies of M and Ap frozen with pairs="always", P1 and P2."""
    import torch

    from oasisx_amd.la import SellMatrix

    S, _ = tg_solvers(dim, N, deg, windows)
    rng = np.random.default_rng(9)
    _set_fields(S, None, *_tg(dim, 0.5))
    S.assemble_first(0.1, 0.5)
    Vi, Q = S._Vi[0][0], S._Q
    if windows:
        assert getattr(Vi.pattern, "wcode", None) is not None and S._spmv_windows
    for V in (Vi, Q):
        csr = V.pattern.to_csr(V.pattern.new_values() + 1.0)
        rows, cols = csr.nonzero()
        span = np.zeros(V.num_dofs)
        np.maximum.at(span, rows, np.abs(cols - rows))
        assert span.max() > 0.5 * V.num_dofs  # a row that reaches across more than half of the numbering: a seam row
        assert V.pattern.cols16 is not None and 0.0 < V.pattern.frac16 <= 1.0
    # (the stiffness matrix of P2 tetrahedra takes more than 256 distinct values: no dictionary is built, f64 is read --
    # as tests/test_gpu_viscosity.py notes for plain meshes)
    for A in (S._M, S._Ap) + (() if (dim, deg) == (3, 2) else (S._K,)):
        assert A.vcode is not None and A.vdict is not None, A.name

    def with_pair_slots(A):
        B = SellMatrix(A.pattern, symmetric=True, name=A.name + " pairs")
        B.vals.copy_(A.vals)
        B.version += 1
        assert B.freeze(pairs="always") and B.vcode is not None and B.ps_code is not None and B.ps_code.numel() > 0
        return B
    worst = 0.0
    for name, A in (("M", S._M), ("K", S._K), ("A", S._A), ("Ap", S._Ap), ("M pairs", with_pair_slots(S._M)),
                    ("Ap pairs", with_pair_slots(S._Ap))):
        ref_m = A.to_scipy()
        n = A.pattern.n_cols
        for ncomp in (1, dim):
            x = rng.standard_normal((n, ncomp))
            xd = torch.from_numpy(x).cuda()
            ref = ref_m @ x
            first = None
            for levels in (None, 1, 3, 7, 15, 31):
                A.set_levels(levels)
                yd = torch.full_like(xd, 3.0)
                A.mult(xd, yd, ncomp)
                y = yd.cpu().numpy()
                err = np.abs(y - ref).max() / np.abs(ref).max()
                worst = max(worst, err)
                assert err <= 1e-12, (name, ncomp, levels, err)
                first = y if first is None else first
                assert np.array_equal(y, first), (name, ncomp, levels)  # storage levels never change the bits
            A.set_levels(None)
    print(f"({dim},{N},{deg}) windows={windows}: worst |y - ref| / max|ref| = {worst:.3e}; pair slots built by "
          f"freeze() itself on M: {S._M.ps_code is not None}, Ap: {S._Ap.ps_code is not None}; 16-bit share "
          f"{Vi.pattern.frac16}, {Q.pattern.frac16}")


# ---- 3. periodic Taylor-Green against the oracle --------------------------------------------------------------------------
def _run_pair(dim, N, deg, steps=2, nu=0.01, dt=0.005, low_memory=True, rotational=False, solver_options=None):
    S = _solver(_tg_mesh(dim, N), deg, options={"low_memory_version": low_memory}, rotational=rotational,
                solver_options=solver_options)
    R = _twin(S, low_memory=low_memory, rotational=rotational)
    fns, p_fn = _tg(dim, nu)
    _set_fields(S, R, fns, p_fn)
    for _ in range(steps):
        S.solve(dt, nu, max_iter=1)
        R.solve(dt, nu, max_iter=1)
    du = float(np.abs(S._U.rhost() - R.u1).max())
    dp = float(np.abs(S._P.rhost()[:, 0] - R.p).max())
    return S, R, du, dp


@pytest.mark.parametrize("dim,N,deg,low_memory,rotational", [c + (True, False) for c in TG_CASES] + [
    (2, 6, 2, False, False), (2, 6, 2, True, True)])
def test_taylor_green_against_the_oracle(hip, dim, N, deg, low_memory, rotational):
    """Two steps with no Dirichlet condition at all: du < 1e-8, dp < 1e-7 (tests/test_gpu_parity.py)."""
    S, R, du, dp = _run_pair(dim, N, deg, low_memory=low_memory, rotational=rotational)
    print(f"({dim},{N},{deg}) low_memory={low_memory} rotational={rotational}: du = {du:.3e}, dp = {dp:.3e}, "
          f"max|u| = {np.abs(R.u1).max():.3f}, iterations {S.iteration_counts()}")
    assert np.abs(R.u1).max() > 0.5
    assert du < 1e-8 and dp < 1e-7


# ---- 4. shift equivariance: the seam test ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N", [(2, 6), (3, 3)])
def test_shift_by_one_cell(hip, dim, N):
    """The same P2-P1 problem with the initial data shifted by one cell along x: after 3 steps u and p of the shifted run
    equal the unshifted run read at x + h (dofs matched by coordinates modulo the period), to du < 1e-8, dp < 1e-7.  A
    cell column next to the seam does in one run what an interior column does in the other."""
    nu, dt, h = 0.01, 0.005, 2.0 / N
    mesh = _tg_mesh(dim, N)
    out = []
    for shift in (0.0, h):
        S = _solver(mesh, 2)
        fns, p_fn = _tg(dim, nu, shift=shift)
        _set_fields(S, None, fns, p_fn)
        for _ in range(3):
            S.solve(dt, nu, max_iter=1)
        out.append((S._Vi[0][0].x.cpu().numpy(), S._Q.x.cpu().numpy(), S._U.rhost(), S._P.rhost()[:, 0]))

    def match(x):
        """Index j of the dof at x_i + h e_x (modulo 2 in x) for every dof i."""
        key = lambda a: [tuple(r) for r in np.round(a * 1e6).astype(np.int64)]  # noqa: E731
        y = x.copy()
        y[:, 0] = (y[:, 0] + h + 1.0) % 2.0 - 1.0
        y[np.abs(y[:, 0] - 1.0) < 1e-9, 0] = -1.0
        where = {k: j for j, k in enumerate(key(x))}
        return np.array([where[k] for k in key(y)])
    (xv, xq, u0, p0), (xv1, xq1, u1, p1) = out
    assert np.array_equal(xv, xv1) and np.array_equal(xq, xq1)
    ju, jp = match(xv), match(xq)
    assert sorted(ju) == list(range(xv.shape[0])) and not np.array_equal(ju, np.arange(xv.shape[0]))
    du, dp = float(np.abs(u1 - u0[ju]).max()), float(np.abs(p1 - p0[jp]).max())
    print(f"({dim},{N}): shifted against unshifted at x + h: du = {du:.3e}, dp = {dp:.3e} (max|u| = {np.abs(u0).max():.3f}, "
          f"not shifted: {np.abs(u1 - u0).max():.3e})")
    assert np.abs(u1 - u0).max() > 1e-3  # (the shift is visible)
    assert du < 1e-8 and dp < 1e-7


# ---- 5. the body-force channel --------------------------------------------------------------------------------------------
def _channel_mesh(dim):
    from oasisx_amd import mesh as M

    if dim == 2:
        return _periodic(M.create_rectangle(None, [[0.0, -1.0], [3.0, 1.0]], [3, 4]), (0,))
    return _periodic(M.create_box(None, [[0.0, -1.0, 0.0], [3.0, 1.0, 2.0]], [3, 4, 3]), (0, 2))


def _walls(x):
    return np.isclose(np.abs(x[1]), 1.0)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("locate", ["geometrical", "topological"])
def test_poiseuille_channel(hip, dim, locate):
    """P2-P1 Poiseuille flow under the body force (2 nu, 0[, 0]), periodic in x (and z), no-slip walls located
    geometrically or through tagged facets: 3 steps from 1 - y^2 stay at 1 - y^2 to 1e-8 and match the oracle (du < 1e-8,
    dp < 1e-7).  WallStress(facets=None) lists the wall facets only, and the force on the walls balances body force x
    volume to 1e-12 rho sum |t_f| |f|, the bound tests/test_gpu_wall_stress.py puts on its force sums -- on the exact
    profile and after the steps.  The velocity solves run at ksp_rtol = 1e-13 on both sides: the start is the exact
    discrete steady state, so what a step adds is the error of its solves, and at the 1e-11 of tests.helpers.KRYLOV that
    error alone (1.1e-11 in u, in the oracle just as in the product) exceeds the bound of the force sum (measured: 6.4e-12
    against 1.2e-12 in 2-D, 2.0e-11 against 2.4e-12 in 3-D)."""
    import oasisx_amd as ox
    from oasisx_amd import mesh as M
    from tests.helpers import KRYLOV

    nu, dt = 0.1, 0.05
    so = {k: dict(v, ksp_rtol=1e-13) if k != "pressure" else dict(v) for k, v in KRYLOV.items()}
    mesh = _channel_mesh(dim)
    if locate == "geometrical":
        bc = lambda: ox.DirichletBC(0.0, ox.LocatorMethod.GEOMETRICAL, _walls)  # noqa: E731
    else:
        facets = M.locate_entities_boundary(mesh, dim - 1, _walls)
        assert np.array_equal(facets, mesh.exterior_facets())
        tags = M.meshtags(mesh, dim - 1, facets, np.full(facets.shape[0], 7, dtype=np.int32))
        bc = lambda: ox.DirichletBC(0.0, ox.LocatorMethod.TOPOLOGICAL, (tags, 7))  # noqa: E731
    force = (2.0 * nu,) + (0.0,) * (dim - 1)
    S = _solver(mesh, 2, bcs_u=[[bc()] for _ in range(dim)], body_force=force, solver_options=so)
    x_v = S._Vi[0][0].x.cpu().numpy()
    wall_dofs = np.nonzero(_walls(_X(x_v)))[0]
    assert np.array_equal(np.sort(S._bcs_u[0][0]._dofs), wall_dofs)
    R = _twin(S, dofs=wall_dofs, body_force=force, solver_options=so)
    zero = lambda x: 0.0 * x[0]  # noqa: E731
    fns = [lambda x: 1.0 - x[1] ** 2] + [zero] * (dim - 1)
    _set_fields(S, R, fns, zero)
    for i, f in enumerate(fns):
        S._u[i].interpolate(f)
    W = ox.WallStress(S)
    mid = W.midpoints
    n_wall = 2 * 3 if dim == 2 else 2 * 2 * 3 * 3
    assert W.n_facets == n_wall == mesh.exterior_facets().shape[0] and np.isclose(np.abs(mid[:, 1]), 1.0).all()
    W.sample(0.0, nu)
    for _ in range(3):
        S.solve(dt, nu, max_iter=1)
        R.solve(dt, nu, max_iter=1)
    W.sample(1.0, nu)
    u, p = S._U.rhost(), S._P.rhost()[:, 0]
    du, dp = float(np.abs(u - R.u1).max()), float(np.abs(p - R.p).max())
    exact = np.stack([f(_X(x_v)) for f in fns], axis=1)
    de, de_oracle = float(np.abs(u - exact).max()), float(np.abs(R.u1 - exact).max())
    print(f"dim {dim} {locate}: du = {du:.3e}, dp = {dp:.3e}, |u - (1 - y^2)| = {de:.3e} (oracle {de_oracle:.3e})")
    assert du < 1e-8 and dp < 1e-7
    assert de < 1e-8
    vol = 3.0 * 2.0 * (1.0 if dim == 2 else 2.0)
    F = W.forces()  # (samples, tags, dim)
    want = np.zeros(dim)
    want[0] = 2.0 * nu * vol
    t = np.linalg.norm(W.traction().cpu().numpy(), axis=1)
    size = float((t * W.areas).sum())
    for k in range(2):
        err = np.abs(F[k].sum(axis=0) - want).max()
        print(f"  sample {k}: |sum F - f |Omega|| = {err:.3e}, bound {1e-12 * size:.3e}")
    assert np.abs(F[0].sum(axis=0) - want).max() <= 1e-12 * size
    assert np.abs(F[1].sum(axis=0) - want).max() <= 1e-12 * size


def test_facet_addons_refuse_identified_facets(hip):
    import oasisx_amd as ox
    from oasisx_amd import mesh as M

    mesh = _channel_mesh(2)
    S = _solver(mesh, 2, bcs_u=[[ox.DirichletBC(0.0, ox.LocatorMethod.GEOMETRICAL, _walls)] for _ in range(2)])
    seam = mesh.periodic_facets()
    assert seam.shape[0] == 8
    with pytest.raises(ValueError, match="identified"):
        ox.WallStress(S, facets=seam[:2])
    tags = M.meshtags(mesh, 1, seam, np.full(seam.shape[0], 3, dtype=np.int32))
    with pytest.raises(ValueError, match="identified"):
        ox.FlowRate(S, (tags, 3))
    with pytest.raises(ValueError, match="identified"):
        ox.ScalarFlux(_solver(mesh, 2, bcs_u=[[ox.DirichletBC(0.0, ox.LocatorMethod.GEOMETRICAL, _walls)] for _ in range(2)],
                              scalars=[ox.ScalarTransport("T", diffusivity=0.1)]), "T", (tags, 3))
    with pytest.raises(ValueError, match="identified"):
        ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_u=[[], []], bcs_p=[ox.PressureBC(0.0, (tags, 3))],
                                options={"sell_window": WINDOW})


# ---- 6. add-ons on the periodic box ---------------------------------------------------------------------------------------
def _perturbed_tg(dim, nu, amp=0.3):
    """Taylor-Green plus a 2-periodic perturbation with a divergence (every entry of grad u is exercised)."""
    fns, p_fn = _tg(dim, nu)
    return [lambda x, f=f, i=i: f(x) + amp * np.sin(np.pi * (x[0] + 2.0 * x[1] - x[2]) + 1.1 * i) for i, f in enumerate(fns)], p_fn


@pytest.mark.parametrize("dim,N,deg", [(2, 5, 2), (3, 3, 2), (3, 4, 1)])
def test_flow_diagnostics_cell_integrals(hip, dim, N, deg):
    """FlowDiagnostics.sample on the periodic box against tests/diagnostics_model.cell_integrals under its own criterion
    (|dev - value| <= (n + 2) 2^-53 B per cell and column), and the volume column of the ring = the box."""
    import oasisx_amd as ox
    from tests import assembly_model as AM
    from tests import diagnostics_model as DM

    nu = 0.5
    S = _solver(_tg_mesh(dim, N), deg)
    fns, p_fn = _perturbed_tg(dim, nu)
    _set_fields(S, None, fns, p_fn)
    for i, f in enumerate(fns):
        S._u[i].interpolate(f)
    D = ox.FlowDiagnostics(S, cell_integrals=True)
    D.sample(0.0, 0.1, nu)
    geo = AM.geometry_from_records(S._geom.cpu().numpy())
    val, B, n = DM.cell_integrals(geo, S._Vi[0][0].cell_dofs.cpu().numpy(), deg, S._U.rhost(), nu)
    dev = D._cint.cpu().numpy()
    for k, name in enumerate(DM.COLUMNS):
        ok, r, allow = AM.check(dev[:, k], val[:, k], B[:, k], np.full(dev.shape[0], n[k]))
        print(f"({dim},{N},{deg}) {name}: |dev - value| / (u B) = {r:.2f} of {allow:.0f}")
        assert ok, (name, r, allow)
    row = D.latest().cpu().numpy()
    assert abs(row[0] - 2.0 ** dim) < 1e-12 and row[1] > 0.0


@pytest.mark.parametrize("dim,N", [(2, 6), (3, 3)])
def test_smagorinsky_step(hip, dim, N):
    """One P2-P1 step with Smagorinsky against tests/viscosity_model.py: nut per cell to 1e-12 max nut, A and b_first to
    1e-12 max|.|, the fields after the step to du < 1e-8, dp < 1e-7 (tests/test_gpu_viscosity.py)."""
    import oasisx_amd as ox
    from tests import viscosity_model as VM

    nu, dt = 0.01, 0.005
    m = ox.Smagorinsky()
    S = _solver(_tg_mesh(dim, N), 2, viscosity_model=m)
    R = _twin(S, cls=VM.ViscosityOracleStep, model=("smagorinsky", m.coefficient))
    fns, p_fn = _perturbed_tg(dim, nu, amp=0.05)
    _set_fields(S, R, fns, p_fn)
    S.solve(dt, nu, max_iter=1)
    R.solve(dt, nu, max_iter=1)
    dn = float(np.abs(S._nut.cpu().numpy() - R.nut).max())
    dA = abs(S._A.to_scipy() - R.A).max()
    db = np.abs(S._BFIRST.rhost() - R.b_first).max()
    du, dp = float(np.abs(S._U.rhost() - R.u1).max()), float(np.abs(S._P.rhost()[:, 0] - R.p).max())
    print(f"({dim},{N}): d nut = {dn:.3e} of {R.nut.max():.3e}, dA = {dA:.3e} of {abs(R.A).max():.3e}, db = {db:.3e} of "
          f"{np.abs(R.b_first).max():.3e}, du = {du:.3e}, dp = {dp:.3e}")
    assert R.nut.max() > 0.0 and dn <= 1e-12 * R.nut.max()
    assert dA <= 1e-12 * abs(R.A).max() and db <= 1e-12 * np.abs(R.b_first).max()
    assert du < 1e-8 and dp < 1e-7


@pytest.mark.parametrize("dim,N", [(2, 6), (3, 3)])
def test_scalar_transport_step(hip, dim, N):
    """One step of a scalar with a source and no Dirichlet condition against tests/scalar_model.py: relative max
    difference below 1e-8, iteration count within 1 (tests/test_gpu_scalar.test_steps_match_the_model)."""
    import oasisx_amd as ox
    from tests.scalar_model import ScalarModel
    from tests.test_gpu_scalar import _c, _options

    nu, dt, kappa = 0.01, 0.005, 0.03
    src = lambda x: 0.5 + x[0]  # noqa: E731  (linear, as in tests/test_gpu_scalar.py: no quadrature rule enters the comparison)
    ini = lambda x: np.cos(np.pi * x[0]) * np.cos(np.pi * x[1]) + 0.2 * np.sin(np.pi * x[dim - 1])  # noqa: E731
    so = _options()
    S = _solver(_tg_mesh(dim, N), 2, solver_options=so, scalars=[ox.ScalarTransport("T", diffusivity=kappa, source=src, initial=ini)])
    fns, p_fn = _tg(dim, nu)
    _set_fields(S, None, fns, p_fn)
    F, x_v, _ = _forms(S)
    m = ScalarModel(F, x_v, kappa, source=src, options=so["scalar_transport"])
    m.interpolate(ini)
    assert np.abs(_c(S, "T", 1) - m.c1).max() <= 1e-14
    S.solve(dt, nu, max_iter=1)
    m.step(S._UAB.rhost(), dt)
    c = _c(S, "T")
    rel = np.abs(c - m.c).max() / np.abs(m.c).max()
    its = S.iteration_counts()["scalar_transport"]["T"]
    print(f"({dim},{N}): rel diff {rel:.3e}, iterations {its} (model {m.its})")
    assert m.reason > 0 and rel < 1e-8 and abs(its - m.its) <= 1


@pytest.mark.parametrize("dim,N,deg", [(2, 6, 2), (3, 4, 1)])
def test_gamg_on_the_periodic_pressure_operator(hip, dim, N, deg):
    """pc_type gamg on the singular periodic pressure Laplacian: positive reasons, and with both runs at ksp_rtol = 1e-12
    its fields match the Jacobi run to du < 1e-8, dp < 1e-7."""
    tight = {k: {"ksp_type": t, "pc_type": "jacobi", "ksp_rtol": 1e-12, "ksp_atol": 1e-30}
             for k, t in (("tentative", "bcgs"), ("pressure", "cg"), ("scalar", "cg"))}
    gamg = dict(tight, pressure=dict(tight["pressure"], pc_type="gamg"))
    out = {}
    for name, so in (("jacobi", tight), ("gamg", gamg)):
        S = _solver(_tg_mesh(dim, N), deg, solver_options=so)
        _set_fields(S, None, *_tg(dim, 0.01))
        reasons = []
        for _ in range(2):
            S.solve(0.005, 0.01, max_iter=1)
            reasons.append(int(S._solver_p.last_result.reason[0]))
        out[name] = (S._U.rhost(), S._P.rhost()[:, 0], reasons, S.iteration_counts()["pressure"])
    du = float(np.abs(out["gamg"][0] - out["jacobi"][0]).max())
    dp = float(np.abs(out["gamg"][1] - out["jacobi"][1]).max())
    print(f"({dim},{N},{deg}): gamg against jacobi du = {du:.3e}, dp = {dp:.3e}; reasons {out['gamg'][2]}, "
          f"iterations gamg {out['gamg'][3]} jacobi {out['jacobi'][3]}")
    assert all(r > 0 for r in out["gamg"][2]) and all(r > 0 for r in out["jacobi"][2])
    assert du < 1e-8 and dp < 1e-7


# ---- 7. output -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N,deg", [(2, 4, 1), (2, 5, 2), (3, 3, 2)])
def test_vtx_writer_writes_the_unfolded_field(hip, tmp_path, dim, N, deg):
    """A piece read back: the points are the geometric nodes (vertices, and edge midpoints for P2) of EVERY image, every
    cell's points are its geometric nodes, and the values on a hi-face point equal those on its lo-face image bit for bit
    (and the dof's value: the gather through the image table runs on the device)."""
    import oasisx_amd as ox
    from oasisx_amd import fem, io

    S = _solver(_tg_mesh(dim, N), deg)
    fns, p_fn = _perturbed_tg(dim, 0.01)
    for i, f in enumerate(fns):
        S._u[i].interpolate(f)
    S._p.interpolate(p_fn)
    mesh = S._mesh
    for fn, V, stem in ((S.u, S._Vi[0][0], "u"), (S._p, S._Q, "p")):
        w = io.VTXWriter(None, str(tmp_path / f"{stem}.bp"), [fn])
        w.write(0.25)
        w.close()
        back = io.read_vtu(str(tmp_path / f"{stem}_000000.vtu"))
        pts = back["points"][:, :dim]
        nv = mesh.num_vertices
        vdeg = V.degree
        n_edges = mesh._entities(1)[0].shape[0]
        assert pts.shape[0] == nv + (n_edges if vdeg == 2 else 0)  # the geometric count
        xc = mesh.coords.cpu().numpy()
        assert np.array_equal(pts[:nv], xc)
        nper = {(2, 1): 3, (3, 1): 4, (2, 2): 6, (3, 2): 10}[(dim, vdeg)]
        conn = back["connectivity"].reshape(-1, nper)
        cells_k = V.cells_in_kernel_order()
        assert np.array_equal(conn[:, : dim + 1], cells_k)  # every cell's corner points are its own vertices
        if vdeg == 2:
            inv = np.argsort(io._VTK_PERM[(dim, 2)])  # VTK node order -> local dof order
            mine = conn[:, inv]
            for e, (a, b) in enumerate(fem.local_edges(dim)):
                assert np.array_equal(pts[mine[:, dim + 1 + e]], 0.5 * (xc[cells_k[:, a]] + xc[cells_k[:, b]]))
        # values: every point carries its dof's value; images of one dof carry the same bits
        vals = back["point_data"][fn.name]
        host = fn._storage.rhost()
        vals = vals[:, : host.shape[1]] if host.shape[1] > 1 else vals.reshape(-1, 1)
        if host.shape[1] == 1 or fn._comp is None:
            src = host
        else:
            src = host[:, [fn._comp]]
        per = mesh.periodic
        wrapped = pts.copy()
        for k in per.axes:
            wrapped[np.abs(wrapped[:, k] - per.hi[k]) < 1e-9, k] = per.lo[k]
        key = lambda a: [tuple(r) for r in np.round(a * 1e6).astype(np.int64)]  # noqa: E731
        dof_at = {k: i for i, k in enumerate(key(V.x.cpu().numpy()))}
        img = np.array([dof_at[k] for k in key(wrapped)])
        assert np.array_equal(vals, src[img])
        on_hi = np.nonzero((np.abs(pts[:, 0] - per.hi[0]) < 1e-9))[0]
        assert on_hi.size > 0
        first = {k: i for i, k in reversed(list(enumerate(key(pts))))}
        lo_img = np.array([first[k] for k in key(wrapped[on_hi])])
        assert (np.abs(pts[lo_img, 0] - per.lo[0]) < 1e-9).all() and np.array_equal(vals[on_hi], vals[lo_img])


def test_eval_and_probes_across_the_seam(hip):
    """Function.eval and Probes read cell_dofs: a point in a cell next to the hi face is interpolated from dofs whose
    coordinates lie at the lo face.  Against the P1 interpolation done on the host from the geometric cell that holds the
    point (1e-12); a point on the hi face and its image on the lo face give the same value."""
    import oasisx_amd as ox

    dim, N = 2, 4
    S = _solver(_tg_mesh(dim, N), 2)
    f = lambda x: np.sin(np.pi * x[0]) + 0.5 * np.cos(np.pi * x[1])  # noqa: E731
    S._p.interpolate(f)
    pts = np.array([[0.93, 0.31, 0.0], [-0.93, 0.31, 0.0], [0.77, -0.91, 0.0], [0.77, 0.91, 0.0], [1.0, 0.3, 0.0], [-1.0, 0.3, 0.0],
                    [0.2, 1.0, 0.0], [0.2, -1.0, 0.0]])
    v = S._p.eval(pts)[:, 0]
    Q = S._Q
    xc = S._mesh.coords.cpu().numpy()[Q.cells_in_kernel_order()]  # (nc, 3, 2)
    cd, vals = Q.cell_dofs.cpu().numpy(), S._P.rhost()[:, 0]
    ref = np.zeros(pts.shape[0])
    for i, pt in enumerate(pts[:, :2]):
        T = np.stack([xc[:, 1] - xc[:, 0], xc[:, 2] - xc[:, 0]], axis=2)  # (nc, 2, 2)
        lam = np.linalg.solve(T, (pt[None, :] - xc[:, 0])[:, :, None])[:, :, 0]
        bary = np.concatenate([1.0 - lam.sum(axis=1, keepdims=True), lam], axis=1)
        c = int(np.argmax(bary.min(axis=1)))
        assert bary[c].min() > -1e-12
        ref[i] = bary[c] @ vals[cd[c]]
    print(f"eval against the host interpolation: {np.abs(v - ref).max():.3e}; across the seam: {abs(v[4] - v[5]):.3e}, "
          f"{abs(v[6] - v[7]):.3e}")
    assert np.abs(v - ref).max() < 1e-12
    assert abs(v[4] - v[5]) < 1e-12 and abs(v[6] - v[7]) < 1e-12
    probes = ox.Probes(pts, S._p)
    probes.sample(0.0)
    assert np.abs(probes.array()[0, :, 0] - v).max() < 1e-12


# ---- 8. demos --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_channel_demo(hip, capsys, dim):
    """demo/periodic_channel_hip.py: start-up from rest follows the series solution (the P2 error of a coarse channel) and
    the drag grows towards G |Omega|."""
    from demo.periodic_channel_hip import main

    rows = main(["-N", "4", "--dim", str(dim), "--steps", "4"])
    out = capsys.readouterr().out
    assert "identified facets" in out and len(rows) == 4
    assert all(r["error"] < 0.05 * rows[-1]["series"] for r in rows)
    assert all(0.0 < a["drag"] < b["drag"] < b["balance"] for a, b in zip(rows, rows[1:]))


def test_les_demo_periodic_switch(hip, capsys):
    """demo/les_taylor_green_hip.py --periodic: the energies decay and the model's run ends below the other."""
    from demo.les_taylor_green_hip import main

    out = main(["-N", "4", "--steps", "3", "--periodic"])
    assert "periodic" in capsys.readouterr().out
    e0, e1 = [r["energy"] for r in out["none"]], [r["energy"] for r in out["smagorinsky"]]
    assert all(b < a for a, b in zip(e0, e0[1:])) and e1[-1] < e0[-1] and out["smagorinsky"][-1]["nut_max"] > 0.0
