"""GPU: wall shear stress, traction, forces and TAWSS / OSI / RRT on exterior facets (oasisx_amd/wall.py,
csrc/ox_wall.hip) against the numpy model of tests/wall_stress_model.py, which uses a facet quadrature and coordinates
only and is pinned by tests/test_wall_stress_host.py.  The model is fed the device's dof numbering."""
import logging

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [(2, 6, 1), (2, 5, 2), (3, 3, 1), (3, 3, 2), (2, 4, 3), (3, 2, 3)]
KINDS = ["lattice", "delaunay"]


def _side_tags(mesh):
    """Meshtags of all exterior facets of the box [-1, 1]^dim: tag 2 axis + (1 on the upper side), tags 10, 11, ..."""
    from oasisx_amd import mesh as M

    d = mesh.gdim
    ext = np.asarray(mesh.exterior_facets(), dtype=np.int32)
    fv, _ = mesh._entities(d - 1)
    mid = mesh.coords.cpu().numpy()[fv[ext]].mean(axis=1)
    axis = np.argmax(np.abs(mid), axis=1)
    val = (10 + 2 * axis + (mid[np.arange(mid.shape[0]), axis] > 0)).astype(np.int32)
    return M.meshtags(mesh, d - 1, ext, val), tuple(int(v) for v in np.unique(val))


def _solver(dim, N, deg, kind, model=None, **kw):
    from tests.test_gpu_viscosity import _delaunay, _problem

    mesh = _delaunay(dim, N) if kind in ("delaunay", "rolled") else None
    if kind == "rolled":  # the Delaunay mesh with the vertices of cell c rotated c times: every local facet index occurs
        from oasisx_amd import mesh as M

        cells = mesh.cells.cpu().numpy()
        idx = (np.arange(dim + 1)[None, :] + np.arange(cells.shape[0])[:, None]) % (dim + 1)
        mesh = M.from_arrays(mesh.coords.cpu().numpy(), np.take_along_axis(cells, idx, axis=1))
    return _problem(dim, N, deg, model, mesh=mesh, **kw)


def _tables(S, mesh):
    """The device's velocity and pressure dof tables indexed by MESH cell id."""
    Vi, Q = S._Vi[0][0], S._Q
    lc = Vi.local_cells.cpu().numpy()
    vd = np.zeros((int(mesh.num_cells), Vi.cell_dofs.shape[1]), dtype=np.int64)
    qd = np.zeros((int(mesh.num_cells), Q.cell_dofs.shape[1]), dtype=np.int64)
    vd[lc], qd[lc] = Vi.cell_dofs.cpu().numpy(), Q.cell_dofs.cpu().numpy()
    return vd, qd


def _model(S, W, mesh, nu_eff):
    """(t, wss) of the numpy model for the solver's current u and p on W's facets."""
    from tests import wall_stress_model as WM

    vd, qd = _tables(S, mesh)
    Vi, Q = S._Vi[0][0], S._Q
    return WM.wall_stress(mesh.coords.cpu().numpy(), mesh.cells.cpu().numpy(), W.cells, W.local_facets, vd, qd,
                          S._U.rhost(), S._P.rhost()[:, 0], Vi.degree, Q.degree, nu_eff)


def _set_tg(S, dim, nu, amp=0.3, t=0.0):
    """u = Taylor-Green plus the non-solenoidal perturbation of the viscosity tests, p = Taylor-Green."""
    from oracle import ipcs_oracle as O
    from tests.test_gpu_viscosity import _perturbed

    for i, f in enumerate([O.tg_u, O.tg_v, O.tg_w][:dim]):
        S._u[i].interpolate(_perturbed(f, i, t, nu, amp))
    S._p.interpolate(lambda x: O.tg_p(x, t, nu))


def _set_poly(S, dim, deg, seed=5, sign=1.0):
    from tests.test_wall_stress_host import _fields

    p_deg = S._Q.degree
    u, gu, p = _fields(dim, deg, p_deg, seed)
    for i in range(dim):
        S._u[i].interpolate(lambda x, i=i: sign * u(x[:dim].T)[:, i])
    S._p.interpolate(lambda x: sign * p(x[:dim].T))
    return u, gu, p


# ---- 1. device = model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS + ["rolled"])
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_device_equals_the_model(hip, dim, N, deg, kind):
    """Taylor-Green plus a smooth non-solenoidal perturbation, all exterior facets in 2 dim tags: max |t_dev - t_model|
    <= 1e-12 max |t_model| and the same for wss -- the bound tests/test_gpu_viscosity.py and tests/test_gpu_parity.py put
    on assembled quantities; normals, areas and midpoints equal the model's (from coordinates alone) to the same bound;
    the facets are ordered by tag, then by id; without a model the nut pointer is null.

    Observed on one MI355X, maximum over the cases of max |d| / max |t_model|: 1.3e-14 for t, 7.4e-15 for wss (both on
    the P3 tetrahedra of the lattice; at most 2.1e-15 for P1 and P2)."""
    import oasisx_amd as ox
    from tests import wall_stress_model as WM

    nu = 0.5
    S, clock, mesh = _solver(dim, N, deg, kind, nu=nu, perturb=0.3)
    assert S._nut is None
    _set_tg(S, dim, nu)
    tags, ids = _side_tags(mesh)
    W = ox.WallStress(S, facets=(tags, ids), rho=1.3)
    assert W.n_tags == 2 * dim and W.n_facets == mesh.exterior_facets().shape[0]
    assert np.array_equal(W.tags, np.asarray(ids))
    key = W.facet_tags.astype(np.int64) * (int(W.facets.max()) + 1) + W.facets
    assert (np.diff(key) > 0).all()  # by tag, then by facet id
    if kind == "rolled":
        assert set(W.local_facets.tolist()) == set(range(dim + 1))
    W.sample(0.0, nu)
    t_ref, w_ref = _model(S, W, mesh, nu)
    t_dev, w_dev = W.traction().cpu().numpy(), W.wss().cpu().numpy()
    scale = np.abs(t_ref).max()
    rt, rw = np.abs(t_dev - t_ref).max() / scale, np.abs(w_dev - w_ref).max() / scale
    print(f"{kind} ({dim},{N},{deg}): max |dt| / max|t| = {rt:.3e}, max |dwss| / max|t| = {rw:.3e}")
    assert scale > 0.0 and np.abs(w_ref).max() > 1e-3 * scale
    assert rt <= 1e-12 and rw <= 1e-12
    n_ref, a_ref, m_ref = WM.facet_geometry(mesh.coords.cpu().numpy(), mesh.cells.cpu().numpy(), W.cells, W.local_facets)
    assert np.abs(W.normals - n_ref).max() <= 1e-12
    assert np.abs(W.areas - a_ref).max() <= 1e-12 * a_ref.max()
    assert np.abs(W.midpoints - m_ref).max() <= 1e-12
    F_ref = WM.forces(t_ref, a_ref, W.facet_tags, W.tags, rho=1.3)
    F = W.forces()
    assert F.shape == (1, 2 * dim, dim)
    assert np.abs(F[0] - F_ref).max() <= 1e-12 * 1.3 * (a_ref * np.linalg.norm(t_ref, axis=1)).sum()


# ---- 2. exactness --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_polynomial_fields_give_the_closed_forms(hip, dim, N, deg, kind):
    """u linear (degree 1) / quadratic (degree >= 2), p linear (P1) / quadratic (P2), interpolated into the solver's u and
    p: traction and shear equal the closed forms -- grad u at the facet midpoint, the exact facet mean of p from the
    facet's vertices, the sides' normals -- to 1e-12 max |t|.

    Observed on one MI355X, maximum over the cases: 2.1e-15 for t, 7.3e-16 for wss."""
    import oasisx_amd as ox
    from tests.test_wall_stress_host import _facet_vertices, _mean_of_quadratic

    nu = 0.37
    S, clock, mesh = _solver(dim, N, deg, kind, nu=nu)
    u, gu, p = _set_poly(S, dim, deg)
    W = ox.WallStress(S)  # all exterior facets, one tag
    assert W.n_tags == 1 and np.array_equal(W.facets, np.sort(mesh.exterior_facets()))
    W.sample(0.0, nu)
    mid = W.midpoints
    side = np.argmax(np.abs(mid), axis=1)
    n = np.zeros_like(mid)
    n[np.arange(mid.shape[0]), side] = np.sign(mid[np.arange(mid.shape[0]), side])
    g = gu(mid)
    xf = _facet_vertices(mesh.coords.cpu().numpy(), mesh.cells.cpu().numpy(), W.cells, W.local_facets)
    pbar = _mean_of_quadratic(p, xf)
    t_ref = -pbar[:, None] * n + nu * np.einsum("nik,nk->ni", g + np.swapaxes(g, 1, 2), n)
    w_ref = t_ref - np.einsum("ni,ni->n", t_ref, n)[:, None] * n
    scale = np.abs(t_ref).max()
    rt = np.abs(W.traction().cpu().numpy() - t_ref).max() / scale
    rw = np.abs(W.wss().cpu().numpy() - w_ref).max() / scale
    print(f"{kind} ({dim},{N},{deg}): max |dt| / max|t| = {rt:.3e}, max |dwss| / max|t| = {rw:.3e}")
    assert rt <= 1e-12 and rw <= 1e-12


# ---- 3. Gauss identities -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_gauss_identities_on_the_closed_boundary(hip, dim, N, deg, kind):
    """All exterior facets in 2 dim tags, the tags summed: u = 0, p = a . x + c gives sum F = rho a |Omega|; for degree >=
    2, u = (y^2, 0[, 0]), p = 0 gives -rho nu (2 |Omega|, 0[, 0]).  The sums cancel: 1e-12 relative to rho sum |f| |t_f|.

    Observed on one MI355X, maximum over the cases: 8.7e-16."""
    import oasisx_amd as ox

    rho, nu, vol = 1.3, 0.2, 2.0 ** dim
    S, clock, mesh = _solver(dim, N, deg, kind, nu=nu)
    tags, ids = _side_tags(mesh)
    W = ox.WallStress(S, facets=(tags, ids), rho=rho)
    a = np.array([0.7, -1.1, 0.4])[:dim]
    for i in range(dim):
        S._u[i].interpolate(lambda x: 0.0 * x[0])
    S._p.interpolate(lambda x: 0.25 + sum(a[k] * x[k] for k in range(dim)))
    W.sample(0.0, nu)
    cases = [np.asarray(rho * a * vol)]
    if deg >= 2:
        S._u[0].interpolate(lambda x: x[1] ** 2)
        S._p.interpolate(lambda x: 0.0 * x[0])
        W.sample(1.0, nu)
        want = np.zeros(dim)
        want[0] = -rho * nu * 2.0 * vol
        cases.append(want)
        size1 = rho * float((_row_norms(W.traction()) * W.areas).sum())
    F = W.forces()
    # (the scale of the first sample: |t| = |p| on every facet)
    xq_mid = W.midpoints
    size0 = rho * float((np.abs(0.25 + xq_mid @ a) * W.areas).sum())
    sizes = [size0] + ([size1] if deg >= 2 else [])
    for k, (want, size) in enumerate(zip(cases, sizes)):
        tot = F[k].sum(axis=0)
        print(f"{kind} ({dim},{N},{deg}) identity {k}: |sum F - exact| / size = {np.abs(tot - want).max() / size:.3e}")
        assert np.abs(tot - want).max() <= 1e-12 * size


def _row_norms(t):
    return np.linalg.norm(t.cpu().numpy(), axis=1)


# ---- 4. with a viscosity model ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_with_a_cell_viscosity(hip, dim, N, deg, kind):
    """CellViscosity(_sponge) of the viscosity tests: after one solve, sample uses nu + nut[c] and equals the model fed
    S._nut, to the bound of the first test; it differs from the constant-viscosity evaluation.

    Observed on one MI355X, maximum over the cases: 1.7e-15 for t, 7.9e-16 for wss."""
    import oasisx_amd as ox
    from tests.test_gpu_viscosity import _sponge

    nu, dt = 0.5, 0.1
    S, clock, mesh = _solver(dim, N, deg, kind, model=ox.CellViscosity(_sponge), nu=nu, dt=dt, perturb=0.3)
    clock["t"] = dt
    S.solve(dt, nu, max_iter=1)
    W = ox.WallStress(S)
    W.sample(dt, nu)
    kpos = S._Vi[0][0].kernel_cell_index(W.cells)
    nut = S._nut.cpu().numpy()[kpos]
    assert nut.min() > 0.0
    t_ref, w_ref = _model(S, W, mesh, nu + nut)
    t_plain, _ = _model(S, W, mesh, nu)
    scale = np.abs(t_ref).max()
    rt = np.abs(W.traction().cpu().numpy() - t_ref).max() / scale
    rw = np.abs(W.wss().cpu().numpy() - w_ref).max() / scale
    print(f"{kind} ({dim},{N},{deg}): max |dt| / max|t| = {rt:.3e}, max |dwss| / max|t| = {rw:.3e}")
    assert rt <= 1e-12 and rw <= 1e-12
    assert np.abs(t_plain - t_ref).max() > 1e-6 * scale  # (the term under test is not lost in the bound)


# ---- 5. time loop --------------------------------------------------------------------------------------------------------
def _tg_loop(steps, with_wall, capacity=2):
    import oasisx_amd as ox
    from tests.helpers import KRYLOV, make_hip_problem

    nu, dt = 0.01, 0.005
    opts = {k: dict(v, ksp_initial_guess_nonzero=True) for k, v in KRYLOV.items()}
    S, clock, mesh = make_hip_problem(3, 8, 2, nu=nu, dt=dt, solver_options=opts, window=128)
    W = None
    if with_wall:
        tags, ids = _side_tags(mesh)
        W = ox.WallStress(S, facets=(tags, ids), capacity=capacity)
    return S, W, clock, nu, dt


def test_sampling_in_a_time_loop_is_read_only_and_loses_nothing(hip, caplog):
    """Five Taylor-Green steps (N = 8, P2-P1) with a sample after every step, capacity 2: sampling never makes the solver
    log "u was handed out writable"; u, p and the iteration counts are bit-equal to a run without WallStress; the ring
    grows and forces() has five rows; two identical runs give bit-identical forces."""
    import torch

    caplog.set_level(logging.INFO, logger="oasisx")
    note = "u was handed out writable"
    steps = 5
    runs = []
    for rep in range(2):
        S, W, clock, nu, dt = _tg_loop(steps, True)
        tokens = []
        for k in range(steps):
            clock["t"] += dt
            S.solve(dt, nu, max_iter=1)
            W.sample(clock["t"], nu, dt=dt)
            if k == 0:  # the first step always says it (u1 was written by interpolate): start listening after it
                assert S._shortcut_note
                S._shortcut_note = False
                caplog.clear()
            tokens.append(S._u_is_u1 == (S._U.generation, S._U1.generation))
        assert tokens == [True] * steps
        assert not any(note in r.getMessage() for r in caplog.records)
        F = W.forces()
        assert F.shape == (steps, 6, 3) and W.capacity >= steps and W.n_samples == steps
        assert np.allclose(W.times, dt * np.arange(1, steps + 1)) and abs(W.total_weight - steps * dt) < 1e-15
        assert np.isfinite(F).all() and np.abs(F[-1] - F[0]).max() > 0.0
        runs.append((S, F))
    assert np.array_equal(runs[0][1], runs[1][1])
    S0, _, clock0, nu, dt = _tg_loop(steps, False)
    for _ in range(steps):
        clock0["t"] += dt
        S0.solve(dt, nu, max_iter=1)
    S = runs[0][0]
    assert torch.equal(S._U.rdev(), S0._U.rdev()) and torch.equal(S._P.rdev(), S0._P.rdev())
    assert {k: list(v) for k, v in S.iteration_counts().items()} == {k: list(v) for k, v in S0.iteration_counts().items()}


# ---- 6. statistics -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N,deg", [(2, 5, 2), (3, 3, 2)])
def test_statistics(hip, dim, N, deg):
    """Three samples with unequal dt, the fields set by hand between them -- a field, its exact reversal, another field:
    tawss, mean_wss, osi and rrt equal numpy on the three wss() arrays to 1e-14 relative.  The kernel rounds every product
    and sum of the accumulation on its own (no fma), in sample order: the same sums in the same order as numpy's.  An
    equal-weight reversal gives OSI = 0.5 exactly (the accumulated vector is exactly 0); a steady field gives OSI = 0 up
    to the rounding of |sum w x| against sum w |x| (two samples, each norm and each sum rounded once: <= 4 eps, and the
    ratio is clamped at 1); facets without shear give OSI 0 and RRT inf; reset_statistics() clears.

    Observed on one MI355X: at most 2.4e-16 relative (mean_wss: 0)."""
    import torch

    import oasisx_amd as ox

    nu = 0.37
    S, clock, mesh = _solver(dim, N, deg, "delaunay", nu=nu)
    W = ox.WallStress(S)
    with pytest.raises(RuntimeError):
        W.tawss()
    dts = [0.5, 0.2, 0.3]
    samples = []
    for k, dt in enumerate(dts):
        if k < 2:
            _set_poly(S, dim, deg, seed=5, sign=1.0 if k == 0 else -1.0)
        else:
            _set_poly(S, dim, deg, seed=11)
        W.sample(float(k), nu, dt=dt)
        samples.append(W.wss().cpu().numpy().copy())
    assert np.array_equal(samples[1], -samples[0])
    T = (dts[0] + dts[1]) + dts[2]
    acc_vec = dts[0] * samples[0] + dts[1] * samples[1] + dts[2] * samples[2]
    mags = [np.sqrt((s * s).sum(axis=1)) for s in samples]
    acc_mag = dts[0] * mags[0] + dts[1] * mags[1] + dts[2] * mags[2]
    tawss, mean = acc_mag / T, acc_vec / T
    osi = 0.5 * (1.0 - np.minimum(np.sqrt((acc_vec * acc_vec).sum(axis=1)) / acc_mag, 1.0))
    rrt = 1.0 / ((1.0 - 2.0 * osi) * tawss)
    for name, got, ref in (("tawss", W.tawss(), tawss), ("mean_wss", W.mean_wss(), mean), ("osi", W.osi(), osi),
                           ("rrt", W.rrt(), rrt)):
        got = got.cpu().numpy()
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"({dim},{N},{deg}) {name}: max rel err {err:.3e}")
        assert err <= 1e-14, (name, err)
    assert osi.min() >= 0.0 and osi.max() <= 0.5 and osi.max() > 0.05
    # equal-weight reversal
    W.reset_statistics()
    assert W.total_weight == 0.0 and float(W._acc_mag.abs().max()) == 0.0 and float(W._acc_vec.abs().max()) == 0.0
    for sign in (1.0, -1.0):
        _set_poly(S, dim, deg, seed=5, sign=sign)
        W.sample(0.0, nu, dt=0.25)
    assert torch.equal(W.osi(), torch.full_like(W.osi(), 0.5))
    assert bool(torch.isinf(W.rrt()).all())
    # steady
    W.reset_statistics()
    for _ in range(2):
        W.sample(0.0, nu, dt=0.25)
    assert float(W.osi().max()) <= 4.0 * np.finfo(np.float64).eps and float(W.osi().min()) >= 0.0
    # no shear at all: u = 0, p = 1
    W.reset_statistics()
    for i in range(dim):
        S._u[i].interpolate(lambda x: 0.0 * x[0])
    S._p.interpolate(lambda x: 1.0 + 0.0 * x[0])
    W.sample(0.0, nu, dt=0.5)
    assert float(W.wss().abs().max()) <= 1e-15  # -p n has no tangential part beyond rounding
    S._p.interpolate(lambda x: 0.0 * x[0])
    W.reset_statistics()
    W.sample(0.0, nu, dt=0.5)
    assert float(W.tawss().abs().max()) == 0.0
    assert float(W.osi().abs().max()) == 0.0 and bool(torch.isinf(W.rrt()).all())


# ---- 7. scope guards -------------------------------------------------------------------------------------------------------
def test_scope_guards(hip):
    import oasisx_amd as ox
    from oasisx_amd.parallel import Comm

    S, clock, mesh = _solver(2, 4, 2, "lattice")
    _, cf = mesh._entities(1)
    counts = np.bincount(cf.ravel())
    interior = int(np.nonzero(counts == 2)[0][0])
    with pytest.raises(ValueError, match="interior"):
        ox.WallStress(S, facets=np.array([int(mesh.exterior_facets()[0]), interior]))
    with pytest.raises(ValueError):
        ox.WallStress(S, capacity=0)
    old = mesh.comm
    try:
        mesh.comm = Comm(0, 2, None, transport="host")
        with pytest.raises(NotImplementedError, match="partition"):
            ox.WallStress(S)
    finally:
        mesh.comm = old
    W = ox.WallStress(S, facets=mesh.exterior_facets()[:3])
    assert W.n_facets == 3 and W.n_tags == 1
    with pytest.raises(ValueError):
        W.sample(0.0, 0.1, dt=-1.0)


# ---- 8. output -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N", [(2, 5), (3, 3)])
def test_facet_vtu_round_trip(hip, tmp_path, dim, N):
    import oasisx_amd as ox

    nu = 0.37
    S, clock, mesh = _solver(dim, N, 2, "delaunay", nu=nu)
    _set_poly(S, dim, 2)
    W = ox.WallStress(S)
    W.sample(0.5, nu, dt=0.1)
    path = tmp_path / "out" / "wall.vtu"
    ox.io.write_facet_vtu(path, mesh, W.facets, {"wss": W.wss(), "tawss": W.tawss()}, time=0.5)
    d = ox.io.read_vtu(str(path))
    assert d["time"] == 0.5 and d["types"].shape[0] == W.n_facets and set(d["types"].tolist()) == {3 if dim == 2 else 5}
    assert np.array_equal(d["cell_data"]["wss"][:, :dim], W.wss().cpu().numpy())
    assert np.array_equal(d["cell_data"]["tawss"], W.tawss().cpu().numpy())
    # the cells are the facets: their vertices' mean is the facet midpoint
    conn = d["connectivity"].reshape(-1, dim)
    assert np.abs(d["points"][conn].mean(axis=1)[:, :dim] - W.midpoints).max() <= 1e-15
    W.save(tmp_path / "wall.npz")
    z = np.load(tmp_path / "wall.npz")
    assert np.array_equal(z["forces"], W.forces()) and np.array_equal(z["facets"], W.facets)
    assert np.array_equal(z["tawss"], W.tawss().cpu().numpy())


def test_demo_and_exact_poiseuille(hip, capsys):
    """demo/wall_shear_hip.py at -N 8 --steps 3 runs and prints; with the flow set to the exact Poiseuille profile the
    wall |wss| equals nu |dU/dy| = G / 2 and the drag G L to 1e-12 max |t|."""
    import oasisx_amd as ox
    from demo.wall_shear_hip import WALLS, build_channel, main

    rows = main(["-N", "8", "--steps", "3"])
    out = capsys.readouterr().out
    assert "wall facets" in out and "drag" in out and len(rows) == 3
    # (the run starts 5 % below the steady profile; three coarse steps: the printed values have the size of the exact
    # ones -- the exact values are asserted below, on the exact profile)
    assert all(0.25 < r["wss_max"] < 1.0 and 1.0 < r["drag"] < 3.0 for r in rows)
    nu, G, L = 0.1, 1.0, 2.0
    mesh, tags, S = build_channel(8, nu, G, L)
    W = ox.WallStress(S, facets=(tags, WALLS))
    W.sample(0.0, nu)
    t = W.traction().cpu().numpy()
    scale = np.abs(t).max()
    mag = np.linalg.norm(W.wss().cpu().numpy(), axis=1)
    print(f"Poiseuille: max ||wss| - G/2| / max|t| = {np.abs(mag - G / 2).max() / scale:.3e}")
    assert np.abs(mag - G / 2).max() <= 1e-12 * scale
    assert abs(W.forces()[0, 0, 0] - G * L) <= 1e-12 * scale * W.areas.sum()
