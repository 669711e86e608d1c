"""GPU: drag zones in FractionalStep_AB_CN (oasisx_amd/drag.py, csrc/ox_drag.hip) against the numpy model of
tests/drag_model.py, which is built on the oracle's forms and pinned by tests/test_drag_host.py.  The model is fed the
device's numbering (fields and matrices compare index by index) and the device's own velocity blocks.

In every case there are two zones: a half space along the slowest direction of the numbering, which cuts through the
neighbourhoods of cells (rows that mix zone and non-zone cells) and reaches the Dirichlet boundary (zone rows that become
identity rows), with a Darcy coefficient that varies from cell to cell; and a small box with a Forchheimer part and a target
velocity that is not zero."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [(2, 6, 1), (2, 5, 2), (3, 3, 1), (3, 3, 2), (2, 4, 3), (3, 2, 3)]
MAT = 1e-12  # the project's bound on assembled entries (tests/test_gpu_parity.py)


def _X(x):
    X = np.zeros((3, x.shape[0]))
    X[: x.shape[1]] = x.T
    return X


def _half(dim):
    return lambda x: x[dim - 1] < -0.2


def _box(dim):
    return lambda x: (x[0] > 0.3) & (np.abs(x[1]) < 0.6) & (x[dim - 1] >= -0.2) & (x[dim - 1] < 0.3)


def _alpha(x):
    return 40.0 * (1.0 + x[0] ** 2)


def _target(dim):
    return lambda x: np.stack([0.3 + 0.1 * x[1], -0.2 + 0.05 * x[0], 0.1 - 0.1 * x[0] * x[1]][:dim])


def _zones(dim, rho=1.0):
    import oasisx_amd as ox

    return [ox.DragZone(_half(dim), darcy=_alpha), ox.DragZone(_box(dim), darcy=5.0, forchheimer=2.0, target=_target(dim), rho=rho)]


def _model_zones(S, mesh, zones, x_v):
    """The model's description of bound zones: kernel cell positions, coefficients from the zone's own evaluation on the
    host, the target evaluated here at the dof coordinates."""
    from tests import drag_model as DM

    Vi = S._Vi[0][0]
    out = []
    for z in zones:
        a, b = z.coefficients(mesh, z.cells)
        t = z._target
        ut = None if t is None else np.ascontiguousarray(np.asarray(t(_X(x_v)), dtype=np.float64).T)
        out.append(DM.Zone(Vi.kernel_cell_index(z.cells), a, b, ut, rho=z.rho))
    return out


def _model(S, mesh, zones, theta, nu, dt, model=None, solver_options=None, low_memory=True):
    """DragOracleStep on the device's tables with the Taylor-Green boundary data of tests/viscosity_model.tg_step_model."""
    from oracle import ipcs_oracle as O
    from tests import drag_model as DM
    from tests.test_gpu_viscosity import _forms, _model_of

    F, x_v, x_q = _forms(S, mesh)
    d = F.d
    clock = {"t": 0.0}
    fns = [O.tg_u, O.tg_v, O.tg_w][:d]
    bd = O.boundary_dofs(x_v, F.coords.min(axis=0), F.coords.max(axis=0))
    bcs_u = [[O.DirichletData(bd, (lambda x, f=f: f(x, clock["t"], nu)))] for f in fns]
    R = DM.DragOracleStep(F, x_v, x_q, bcs_u, solver_options=solver_options, low_memory=low_memory,
                          model=_model_of(S, model), zones=_model_zones(S, mesh, zones, x_v), theta=theta)
    R.u1[:], R.u2[:], R.p[:] = S._U1.rhost(), S._U2.rhost(), S._P.rhost()[:, 0]
    return R, clock, F


def _problem(dim, N, deg, zones, **kw):
    from tests.test_gpu_viscosity import _problem as vp

    model = kw.pop("model", None)
    kw.setdefault("perturb", 0.3)
    if zones is not None:
        kw["drag"] = zones
    return vp(dim, N, deg, model, **kw)


def _assemble_first(S, clock, dt, nu):
    from tests.test_gpu_viscosity import _assemble_first as af

    af(S, clock, dt, nu)


# ---- 1. sigma per cell -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lattice", "delaunay"])
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_sigma_per_cell_matches_the_model(hip, dim, N, deg, kind):
    """sigma after assemble_first on perturbed Taylor-Green levels: max |sigma_device - sigma_model| <= 1e-12 max sigma;
    zero outside the zones; drag_coefficient() is the same array in the mesh's cell order.  On the (3,3,2) lattice the
    touched rows span more than one 64-row slice and one slice holds no row next to a zone cell (4 of 6 touched).

    Observed on one MI355X, maximum of max |d sigma| / max sigma over the twelve cases: 2.8e-17 (P3 tetrahedra)."""
    from tests import drag_model as DM
    from tests.test_gpu_viscosity import _delaunay

    dt, nu = 0.1, 0.5
    mesh = _delaunay(dim, N) if kind == "delaunay" else None
    zones = _zones(dim)
    S, clock, mesh = _problem(dim, N, deg, zones, nu=nu, dt=dt, mesh=mesh)
    assert all(z.n_cells > 0 for z in zones) and not S._drag.static
    R, _, F = _model(S, mesh, zones, 1.0, nu, dt)
    _assemble_first(S, clock, dt, nu)
    ref = DM.sigma_field(F, S._UAB.rhost(), R.zones)
    dev = S._drag._sigma.cpu().numpy()
    d = np.abs(dev - ref).max()
    G = S._drag
    print(f"{kind} ({dim},{N},{deg}): max |d sigma| = {d:.3e}, max sigma = {ref.max():.3e}, ratio {d / ref.max():.3e}; "
          f"{G.n_slices_touched} of {G.n_slices} slices touched, {G.n_zone_cells} of {dev.shape[0]} cells in zones")
    assert d <= 1e-12 * ref.max(), (d, ref.max())
    outside = np.ones(dev.shape[0], dtype=bool)
    outside[np.concatenate([z.cells for z in R.zones])] = False
    assert outside.any() and not dev[outside].any() and (dev[~outside] > 0).all()
    lc = S._Vi[0][0].local_cells.cpu().numpy()
    mo = S.drag_coefficient().cpu().numpy()
    assert mo.shape == (int(mesh.num_cells),) and np.array_equal(mo[lc], dev)
    if (dim, N, deg, kind) == (3, 3, 2, "lattice"):
        assert 1 < G.n_slices_touched < G.n_slices, (G.n_slices_touched, G.n_slices)


# ---- 2. A and b_first, entry by entry ----------------------------------------------------------------------------------
@pytest.mark.parametrize("row_blocks", [False, True])
@pytest.mark.parametrize("mode", ["dictionary", "f64", "delaunay"])
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_operator_and_rhs_entry_by_entry(hip, dim, N, deg, mode, row_blocks):
    """After assemble_first with the two zones, theta = 0.5 and 1: A (identity rows on the first component's Dirichlet
    dofs) and b_first equal the model's to 1e-12 max|.| -- with value dictionaries, with f64 values and on a Delaunay mesh,
    by the width bins and by the row blocks of the fused kernel.  theta D is at least 1 % of max|A|: a missing term cannot
    hide under the bound.  The A u1 by-product is not handed to the tentative solve.

    Observed on one MI355X over all cases: dA / max|A| <= 3.9e-15, db / max|b| <= 8.0e-15; theta D between 20 % and 71 % of
    max|A|."""
    from tests.helpers import KRYLOV
    from tests.test_gpu_viscosity import _delaunay

    dt, nu = 0.1, 0.5
    so = {k: dict(v, ksp_initial_guess_nonzero=True) for k, v in KRYLOV.items()}
    mesh = _delaunay(dim, N) if mode == "delaunay" else None
    for theta in (0.5, 1.0):
        zones = _zones(dim)
        S, clock, mesh = _problem(dim, N, deg, zones, nu=nu, dt=dt, mesh=mesh, solver_options=so, drag_theta=theta,
                                  options={"value_dictionary": mode != "f64", "assemble_row_blocks": row_blocks})
        assert S._row_blocks == row_blocks and (not row_blocks or S._Vi[0][0].pattern.n_row_blocks > 0)
        if mode == "f64":
            assert S._M.vcode is None and S._K.vcode is None
        R, rc, F = _model(S, mesh, zones, theta, nu, dt)
        rc["t"] = dt
        _assemble_first(S, clock, dt, nu)
        R.assemble_first(dt, nu)
        dA = abs(S._A.to_scipy() - R.A).max()
        db = np.abs(S._BFIRST.rhost() - R.b_first).max()
        share = theta * abs(R.drag_matrix).max() / abs(R.A).max()
        print(f"theta = {theta}: dA = {dA:.3e} (max|A| = {abs(R.A).max():.3e}, max|theta D| / max|A| = {share:.2e}), "
              f"db = {db:.3e} (max|b| = {np.abs(R.b_first).max():.3e})")
        assert share >= 1e-2
        assert dA <= MAT * abs(R.A).max(), dA
        assert db <= MAT * np.abs(R.b_first).max(), db
        assert not S._AU1_valid


def test_periodic_zone_across_the_seam(hip):
    """A make_periodic box, P2-P1: the zone |x| > 0.6 lies on both sides of the seam x = +-1, where the adjacency and the
    cell dofs wrap; sigma, A and b_first against the model on the reduced space, theta = 0.5, to 1e-12 max|.|."""
    import oasisx_amd as ox
    from tests import drag_model as DM
    from tests.test_gpu_periodic import _perturbed_tg, _set_fields, _solver, _tg_mesh, _twin

    dim, N, deg, dt, nu, theta = 2, 6, 2, 0.1, 0.5, 0.5
    tgt = _target(dim)
    z = ox.DragZone(lambda x: np.abs(x[0]) > 0.6, darcy=_alpha, forchheimer=1.5, target=tgt)
    S = _solver(_tg_mesh(dim, N), deg, drag=z, drag_theta=theta)
    fns, p_fn = _perturbed_tg(dim, nu)
    x_v = S._Vi[0][0].x.cpu().numpy()
    R = _twin(S, cls=DM.DragOracleStep, zones=_model_zones(S, S._mesh, [z], x_v), theta=theta)
    _set_fields(S, R, fns, p_fn)
    R.u1[:], R.u2[:] = S._U1.rhost(), S._U2.rhost()
    cen = S._mesh.coords[S._mesh.cells.long()].mean(dim=1).cpu().numpy()[z.cells]
    assert (cen[:, 0] > 0.6).any() and (cen[:, 0] < -0.6).any()
    S.assemble_first(dt, nu)
    R.assemble_first(dt, nu)
    ds = np.abs(S._drag._sigma.cpu().numpy() - R.sigma).max()
    dA = abs(S._A.to_scipy() - R.A).max()
    db = np.abs(S._BFIRST.rhost() - R.b_first).max()
    print(f"periodic: d sigma = {ds:.3e} of {R.sigma.max():.3e}, dA = {dA:.3e} of {abs(R.A).max():.3e}, "
          f"db = {db:.3e} of {np.abs(R.b_first).max():.3e}")
    assert theta * abs(R.drag_matrix).max() >= 1e-2 * abs(R.A).max()
    assert ds <= 1e-12 * R.sigma.max() and dA <= MAT * abs(R.A).max() and db <= MAT * np.abs(R.b_first).max()


# ---- 3. pins that need no model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta", [0.5, 1.0])
@pytest.mark.parametrize("dim,N,deg", [(2, 5, 2), (3, 3, 1), (2, 4, 3)])
def test_zero_coefficients_leave_the_bits(hip, dim, N, deg, theta):
    """darcy = forchheimer = 0 (the rows kernel runs and skips every cell): A.vals and b_first are torch.equal to those
    of a solver without zones, and so are u and p after a whole step."""
    import torch

    import oasisx_amd as ox

    dt, nu = 0.1, 0.5
    out = {}
    for key in ("plain", "zero"):
        zones = None if key == "plain" else [ox.DragZone(_half(dim)), ox.DragZone(_box(dim), target=_target(dim))]
        kw = {} if zones is None else {"drag_theta": theta}
        S, clock, _ = _problem(dim, N, deg, zones, nu=nu, dt=dt, **kw)
        _assemble_first(S, clock, dt, nu)
        out[key] = [S._A.vals.clone(), S._BFIRST.rdev().clone()]
        clock["t"] = dt
        S.solve(dt, nu, max_iter=1)
        out[key] += [S._U.rdev().clone(), S._P.rdev().clone()]
        if zones is not None:
            assert S._drag.static and not bool(S._drag._sigma.any())
    for a, b in zip(out["plain"], out["zero"]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dim,N,deg", CASES)
def test_uniform_darcy_adds_a_times_the_mass_matrix(hip, dim, N, deg):
    """darcy = a on every cell, theta = 1, no target: A = A_plain + a M (the solver's own M) off the identity rows, to
    1e-12 max|A|; b_first keeps its bits (nothing is added to it)."""
    import torch

    import oasisx_amd as ox

    dt, nu, a = 0.1, 0.5, 7.0
    P, clock, _ = _problem(dim, N, deg, None, nu=nu, dt=dt)
    _assemble_first(P, clock, dt, nu)
    S, clock, _ = _problem(dim, N, deg, ox.DragZone(lambda x: x[0] > -5.0, darcy=a), nu=nu, dt=dt)
    _assemble_first(S, clock, dt, nu)
    assert S._drag.static and S._drag.n_slices_touched == S._drag.n_slices
    rows = torch.cat([b._rows_dev for b in S._bcs_u[0]]).cpu().numpy()
    free = np.setdiff1d(np.arange(S._no_u), rows)
    A, A0, M = S._A.to_scipy().tocsr(), P._A.to_scipy().tocsr(), S._M.to_scipy().tocsr()
    d = abs(A[free] - (A0[free] + a * M[free])).max()
    print(f"({dim},{N},{deg}): max |A - (A0 + a M)| = {d:.3e}, max|A| = {abs(A).max():.3e}, a max|M| / max|A| = "
          f"{a * abs(M).max() / abs(A).max():.2e}")
    assert a * abs(M).max() >= 1e-2 * abs(A).max()
    assert d <= MAT * abs(A).max()
    assert abs(A[rows] - A0[rows]).max() == 0.0  # identity rows win
    assert torch.equal(S._BFIRST.rdev(), P._BFIRST.rdev())


@pytest.mark.parametrize("dim,N,deg", [(2, 5, 2), (3, 3, 2)])
def test_two_launches_give_equal_bits(hip, dim, N, deg):
    """ox_drag_rows twice on equal inputs (A.vals and b_first restored in between): torch.equal, and not a no-op."""
    import torch

    dt, nu = 0.1, 0.5
    S, clock, _ = _problem(dim, N, deg, _zones(dim), nu=nu, dt=dt, drag_theta=0.5)
    _assemble_first(S, clock, dt, nu)
    A0, b0 = S._A.vals.clone(), S._BFIRST.rdev().clone()
    res = []
    for _ in range(2):
        S._A.vals.copy_(A0)
        S._BFIRST.dev().copy_(b0)
        S._drag.launch_rows()
        res.append((S._A.vals.clone(), S._BFIRST.rdev().clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert not torch.equal(res[0][0], A0) and not torch.equal(res[0][1], b0)


def test_scalars_do_not_see_the_drag(hip):
    """With a scalar present, its A_c and b_c are torch.equal to those of the same solver without zones: the drag pass
    runs after scalar_assemble took its operator from A."""
    import torch

    import oasisx_amd as ox
    from tests.test_gpu_scalar import _options

    dim, N, deg, dt, nu = 2, 5, 2, 0.1, 0.5
    out = {}
    for key in ("plain", "drag"):
        sc = ox.ScalarTransport("T", diffusivity=0.2, source=lambda x: 0.5 + x[0],
                                initial=lambda x: np.cos(np.pi * x[0]) * np.cos(np.pi * x[1]))
        S, clock, _ = _problem(dim, N, deg, _zones(dim) if key == "drag" else None, nu=nu, dt=dt, scalars=[sc],
                               solver_options=_options(guess=True))
        _assemble_first(S, clock, dt, nu)
        g = S._scalar_groups[0]
        out[key] = (g.Ac.vals.clone(), g.B.rdev().clone(), S._A.vals.clone())
    assert torch.equal(out["plain"][0], out["drag"][0]) and torch.equal(out["plain"][1], out["drag"][1])
    assert not torch.equal(out["plain"][2], out["drag"][2])


# ---- 4. whole steps ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N,low_memory,les", [(2, 8, True, False), (2, 8, False, False), (3, 3, True, False),
                                                  (3, 3, False, False), (3, 3, True, True)])
def test_steps_match_the_model(hip, dim, N, low_memory, les):
    """Three P2-P1 Taylor-Green steps with the two zones (theta = 1; one case with Smagorinsky()) against the model loop:
    du <= 1e-8, dp <= 1e-7, the bounds of the viscosity tests, with equal iteration counts.

    Observed on one MI355X, maxima over the three steps: 2-D du = 2.7e-15, dp = 3.4e-14 (both settings); 3-D du = 1.3e-11,
    dp = 2.7e-10; 3-D with Smagorinsky() du = 6.0e-12, dp = 1.4e-10; iteration counts equal in every step (2-D: tentative 14-15,
    pressure 36, update 25-26; 3-D: 17-19, 26-27, 41-44)."""
    import oasisx_amd as ox
    from tests.helpers import KRYLOV

    nu, dt = 0.01, 0.005
    mo = ox.Smagorinsky() if les else None
    zones = _zones(dim)
    S, clock, mesh = _problem(dim, N, 2, zones, nu=nu, dt=dt, low_memory=low_memory, model=mo, perturb=0.0)
    R, rc, _ = _model(S, mesh, zones, 1.0, nu, dt, model=mo, solver_options=KRYLOV, low_memory=low_memory)
    for k in range(3):
        clock["t"] = rc["t"] = (k + 1) * dt
        S.solve(dt, nu, max_iter=1)
        R.solve(dt, nu, max_iter=1)
        du = float(np.abs(S._U.rhost() - R.u1).max())
        dp = float(np.abs(S._P.rhost()[:, 0] - R.p).max())
        ds = float(np.abs(S._drag._sigma.cpu().numpy() - R.sigma).max())
        its, its_o = S.iteration_counts(), R.its
        print(f"step {k}: du = {du:.3e}, dp = {dp:.3e}, d sigma = {ds:.3e} (max sigma {R.sigma.max():.3e}), "
              f"iterations {its} / {its_o}")
        assert du <= 1e-8 and dp <= 1e-7, (k, du, dp)
        assert list(its["tentative"][:dim]) == list(its_o["tentative"]), (its, its_o)
        assert list(its["update"][:dim]) == list(its_o["update"]), (its, its_o)
        assert int(np.atleast_1d(its["pressure"])[0]) == int(np.atleast_1d(its_o["pressure"])[0]), (its, its_o)


# ---- 5. forces ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N,deg", [(2, 5, 2), (3, 3, 2), (2, 4, 3), (3, 3, 1)])
def test_forces_match_the_model_and_leave_the_step_alone(hip, dim, N, deg):
    """sample() after a step: the force on every zone equals the model's rho sum_c sigma_c int_c (u - u_t) to 1e-12 of the
    sum of the magnitudes of its terms (u_t is one field: on the dofs the two adjacent zones share it is the box's target);
    the next solve gives the bits of a run that did not sample."""
    import torch

    from tests import drag_model as DM

    nu, dt, rho = 0.01, 0.005, 1.7
    runs = {}
    for key in ("sampled", "plain"):
        zones = _zones(dim, rho=rho)
        S, clock, mesh = _problem(dim, N, deg, zones, nu=nu, dt=dt)
        clock["t"] = dt
        S.solve(dt, nu, max_iter=1)
        if key == "sampled":
            R, _, F = _model(S, mesh, zones, 1.0, nu, dt)
            sig = np.zeros(F.cells.shape[0])
            sig[:] = S._drag._sigma.cpu().numpy()
            u = S._U.rhost()
            for z, mz in zip(zones, R.zones):
                z.sample(dt)
                f_ref, mag = DM.zone_force(F, u, sig, mz, DM.merged_target(F, R.zones))
                f = z.forces()
                assert f.shape == (1, 1, dim) and np.array_equal(z.times(), [dt])
                d = np.abs(f[0, 0] - f_ref)
                print(f"({dim},{N},{deg}) rho = {z.rho}: force {f[0, 0]}, |d| = {d}, sum of magnitudes {mag}")
                assert (d <= 1e-12 * mag).all(), (d, mag)
                assert mag.min() > 0.0
                vol = z.volume()
                assert vol.shape == (1,) and abs(vol[0] - F.adet[mz.cells].sum() / (2 if dim == 2 else 6)) <= 1e-13 * vol[0]
        clock["t"] = 2 * dt
        S.solve(dt, nu, max_iter=1)
        runs[key] = (S._U.rdev().clone(), S._P.rdev().clone())
    assert torch.equal(runs["sampled"][0], runs["plain"][0]) and torch.equal(runs["sampled"][1], runs["plain"][1])


def test_ring_grows_and_coefficients_and_target_can_be_reset(hip, tmp_path):
    """capacity = 1 and three samples: the ring doubles and keeps its entries.  set_coefficients / set_target between
    steps: sigma and A follow (a ramped sponge, a moving target) without a rebuild -- against the model again."""
    import oasisx_amd as ox

    dim, N, deg, dt, nu = 2, 5, 2, 0.1, 0.5
    z = ox.DragZone(_half(dim), darcy=3.0, capacity=1)
    S, clock, mesh = _problem(dim, N, deg, z, nu=nu, dt=dt)
    _assemble_first(S, clock, dt, nu)
    assert S._drag.static and S._drag._ut is None
    for k in range(3):
        z.sample(0.1 * k)
    f = z.forces()
    assert f.shape == (3, 1, dim) and z.capacity == 4 and np.array_equal(f[0], f[1]) and np.array_equal(f[1], f[2])
    z.save(tmp_path / "zone.npz")
    saved = np.load(tmp_path / "zone.npz")
    assert np.array_equal(saved["forces"], f) and np.array_equal(saved["cells"], z.cells)
    z.set_coefficients(darcy=_alpha, forchheimer=0.7)
    z.set_target((0.25, -0.5))
    assert not S._drag.static
    z._target = lambda x: np.stack([np.full(x.shape[1], 0.25), np.full(x.shape[1], -0.5)])  # (the model's description)
    R, rc, F = _model(S, mesh, [z], 1.0, nu, dt)
    rc["t"] = dt
    _assemble_first(S, clock, dt, nu)
    R.assemble_first(dt, nu)
    ds = np.abs(S._drag._sigma.cpu().numpy() - R.sigma).max()
    dA = abs(S._A.to_scipy() - R.A).max()
    db = np.abs(S._BFIRST.rhost() - R.b_first).max()
    print(f"after set_coefficients / set_target: d sigma = {ds:.3e}, dA = {dA:.3e}, db = {db:.3e}")
    assert ds <= 1e-12 * R.sigma.max() and dA <= MAT * abs(R.A).max() and db <= MAT * np.abs(R.b_first).max()
    with pytest.raises(ValueError, match="darcy"):
        z.set_coefficients(darcy=-1.0)


# ---- 6. a velocity that is not finite ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N,deg", [(2, 5, 2), (2, 4, 3), (3, 3, 1)])
def test_nan_in_uab_reaches_sigma(hip, dim, N, deg):
    """A NaN planted in u_ab at a dof of one cell of the Forchheimer zone: sigma of that cell is NaN, not clipped; cells
    that do not hold the dof keep their finite values."""
    dt, nu = 0.1, 0.5
    zones = _zones(dim)
    S, clock, _ = _problem(dim, N, deg, zones, nu=nu, dt=dt)
    _assemble_first(S, clock, dt, nu)
    G = S._drag
    before = G._sigma.cpu().numpy().copy()
    e = int(G._zc[zones[1]._off].item())
    cd = S._Vi[0][0].cell_dofs.cpu().numpy()
    dof = int(cd[e, -1])  # (P3: the last dof is interior, the only one with a weight at the centroid of a triangle)
    S._UAB.dev()[dof, 0] = float("nan")
    G.launch_sigma()
    after = G._sigma.cpu().numpy()
    holds = (cd == dof).any(axis=1)
    assert np.isnan(after[e])
    assert np.array_equal(after[~holds], before[~holds]) and np.isfinite(after[~holds]).all()


# ---- 7. what is called -------------------------------------------------------------------------------------------------
class _Spy:
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        if name.startswith("ox_drag_"):
            self.calls.append(name)
        return getattr(self._lib, name)


def test_no_drag_call_without_zones_and_no_au1_with_them(hip, monkeypatch):
    """Spying on the library: a solver without drag= calls none of ox_drag_* during assemble_first (and asks for its
    A u1 by-product as before); a solver with zones calls ox_drag_sigma once, then ox_drag_rows (per width bin of the
    pattern), and hands no a_u1 buffer to the fused kernel."""
    from oasisx_amd import _lib
    from tests.helpers import KRYLOV

    dim, N, deg, dt, nu = 2, 5, 2, 0.1, 0.5
    so = {k: dict(v, ksp_initial_guess_nonzero=True) for k, v in KRYLOV.items()}
    for zones in (None, _zones(dim)):
        S, clock, _ = _problem(dim, N, deg, zones, nu=nu, dt=dt, solver_options=so)
        spy = _Spy(_lib.load())
        handed = []
        real = _lib.ox_first_args

        def recording(*a, _real=real, _handed=handed):
            _handed.append(a[6])
            return _real(*a)

        with monkeypatch.context() as m:
            m.setattr(_lib, "_lib", spy)
            m.setattr(S, "_lib", spy)
            m.setattr(_lib, "ox_first_args", recording)
            _assemble_first(S, clock, dt, nu)
        assert len(handed) == 1
        if zones is None:
            assert spy.calls == [] and handed[0] is not None and S._AU1_valid
            with pytest.raises(RuntimeError, match="drag"):
                S.drag_assemble()
            with pytest.raises(RuntimeError, match="drag"):
                S.drag_coefficient()
        else:
            assert spy.calls[0] == "ox_drag_sigma" and len(spy.calls) > 1 and set(spy.calls[1:]) == {"ox_drag_rows"}
            assert handed[0] is None and not S._AU1_valid


# ---- 8. guards ---------------------------------------------------------------------------------------------------------
def test_guards(hip):
    """The refusals on the GPU host: a communicator of two ranks whose collectives would raise (no peer exists) is
    refused before any is entered."""
    import oasisx_amd as ox
    from oasisx_amd.parallel import Comm
    from tests.helpers import tg_mesh

    left = lambda x: x[0] < 0.0  # noqa: E731
    pmesh = tg_mesh(2, 4)
    pmesh.comm = Comm(0, 2, None, transport="host")
    with pytest.raises(NotImplementedError, match="partition"):
        _problem(2, 4, 2, ox.DragZone(left, darcy=1.0), mesh=pmesh)
    with pytest.raises(NotImplementedError, match="rotational"):
        _problem(2, 4, 2, ox.DragZone(left, darcy=1.0), rotational=True)
    with pytest.raises(ValueError, match="drag_theta"):
        _problem(2, 4, 2, ox.DragZone(left, darcy=1.0), drag_theta=0.3)
    with pytest.raises(ValueError, match="no cell"):
        _problem(2, 4, 2, ox.DragZone(lambda x: x[0] > 5.0, darcy=1.0))
    with pytest.raises(ValueError, match="two zones"):
        _problem(2, 4, 2, [ox.DragZone(left, darcy=1.0), ox.DragZone(lambda x: x[0] < 0.6)])
    with pytest.raises(ValueError, match="darcy"):
        _problem(2, 4, 2, ox.DragZone(left, darcy=lambda x: x[0]))
    z = ox.DragZone(left, darcy=1.0)
    _problem(2, 4, 2, z)
    with pytest.raises(ValueError, match="one solver"):
        _problem(2, 4, 2, z)
