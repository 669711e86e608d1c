"""GPU: Smagorinsky with van Driest wall damping (oasisx_amd.VanDriest, the damping of ox_cell_viscosity,
csrc/ox_viscosity.hip) against the numpy models of tests/walldist_model.py, tests/wall_stress_model.py and
tests/viscosity_model.py, on the cases and the perturbed Taylor-Green levels of tests/test_gpu_viscosity.py.

The model is fed the device's ``nearest`` table -- validated first as a minimiser of the model's own distances, as
tests/test_gpu_walldist.py does: a tie broken one ulp differently would otherwise change u_tau -- and the model's own
distances, wall shear and damping."""
import numpy as np
import pytest

from tests.test_gpu_viscosity import CASES, _assemble_first, _delaunay, _forms, _problem

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
NU, DT, A_PLUS, CS = 0.01, 0.1, 2.0, 0.1677


def _damped(u_tau=None, facets=None):
    import oasisx_amd as ox

    return ox.Smagorinsky(CS, damping=ox.VanDriest(facets, A_plus=A_PLUS, u_tau=u_tau))


class _Walls:
    """The model's view of a bound VanDriest object: facet vertices, the centroids in kernel cell order, the model's
    distances there and the device's nearest table checked against them."""

    def __init__(self, S, mesh):
        from tests import walldist_model as WD

        vd = S._viscosity_model.damping
        Vi = S._Vi[0][0]
        fv, _ = mesh._entities(mesh.gdim - 1)
        X = mesh.coords.cpu().numpy()
        self.vd, self.xyz = vd, X[fv[vd.facets]]
        self.lc = Vi.local_cells.cpu().numpy()
        self.cen = X[mesh.cells.cpu().numpy()[self.lc]].mean(axis=1)
        per = mesh.periodic
        shifts = None if per is None else WD.image_shifts(np.asarray(per.period, dtype=np.float64), per.axes)
        self.dist, _, D = WD.nearest(self.xyz, self.cen, shifts)
        self.near = vd._nearest.cpu().numpy().astype(np.int64)
        C, L = WD.distance_bound(self.xyz, self.cen)
        assert self.near.min() >= 0 and self.near.max() < self.xyz.shape[0]
        assert np.abs(D[np.arange(self.cen.shape[0]), self.near] - self.dist).max() <= C * EPS * L
        assert np.abs(vd._dist.cpu().numpy() - self.dist).max() <= C * EPS * L

    def u_tau(self, S, mesh, uab, nu):
        """sqrt(|wss|) per wall facet: the wall-stress model on u_ab with the molecular nu."""
        from tests import wall_stress_model as WM
        from tests import walldist_model as WD
        from tests.test_gpu_wall_stress import _tables

        vdofs, qdofs = _tables(S, mesh)
        Vi, Q = S._Vi[0][0], S._Q
        _, wss = WM.wall_stress(mesh.coords.cpu().numpy(), mesh.cells.cpu().numpy(), self.vd.cells, self.vd.local_facets, vdofs,
                                qdofs, uab, S._P.rhost()[:, 0], Vi.degree, Q.degree, nu)
        return WD.friction_velocity(wss)

    def nut(self, S, mesh, F, uab, nu, u_tau=None):
        """(nut, y+, D) per cell in kernel cell order."""
        from tests import walldist_model as WD

        ut = self.u_tau(S, mesh, uab, nu)[self.near] if u_tau is None else u_tau
        yp, D = WD.damping(self.dist, ut, nu, A_PLUS)
        return WD.damped_smagorinsky(F, uab, CS, D), yp, D


# ---- (h) nut per cell --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lattice", "delaunay"])
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_damped_nut_per_cell_matches_the_model(hip, dim, N, deg, kind):
    """All exterior facets as walls, nu = 0.01, dt = 0.1, A+ = 2: max |nut_device - nut_model| <= 1e-12 max nut (the bound
    of tests/test_gpu_viscosity.py), with u_tau from the wall shear and with u_tau = 0.1; wall_units() equals the
    model's (y+, D) to 1e-12 of their maxima; at rest nut == 0, finite.  On the lattice cases the MODEL's D spans at
    most 0.3 to at least 0.9: a damping that does nothing cannot pass.

    Observed on one MI355X, maximum over the cases of max |d nut| / max nut: 2.0e-14 (wall shear; the P3 Delaunay triangles),
    1.9e-15 (u_tau = 0.1)."""
    import torch

    mesh = _delaunay(dim, N) if kind == "delaunay" else None
    S, clock, mesh = _problem(dim, N, deg, _damped(), nu=NU, dt=DT, mesh=mesh, perturb=0.3)
    F, _, _ = _forms(S, mesh)
    W = _Walls(S, mesh)
    _assemble_first(S, clock, DT, NU)
    uab = S._UAB.rhost()
    ref, yp, D = W.nut(S, mesh, F, uab, NU)
    dev = S._nut.cpu().numpy()
    d = np.abs(dev - ref).max()
    print(f"{kind} ({dim},{N},{deg}): max |d nut| = {d:.3e}, max nut = {ref.max():.3e}, ratio {d / ref.max():.3e}, "
          f"D in [{D.min():.3f}, {D.max():.3f}], y+ up to {yp.max():.2f}")
    if kind == "lattice":
        assert D.min() <= 0.3 and D.max() >= 0.9, (D.min(), D.max())
    assert ref.max() > 0.0 and np.isfinite(dev).all() and dev.min() >= 0.0
    assert d <= 1e-12 * ref.max(), (d, ref.max())
    yp_dev, D_dev = (t.cpu().numpy() for t in S.wall_units())
    assert yp_dev.shape == (int(mesh.num_cells),)
    assert np.abs(yp_dev[W.lc] - yp).max() <= 1e-12 * yp.max() and np.abs(D_dev[W.lc] - D).max() <= 1e-12
    # a constant friction velocity: no wall-stress launch
    S2, clock2, _ = _problem(dim, N, deg, _damped(u_tau=0.1), nu=NU, dt=DT, mesh=mesh, perturb=0.3)
    _assemble_first(S2, clock2, DT, NU)
    ref2, _, _ = _Walls(S2, mesh).nut(S2, mesh, F, S2._UAB.rhost(), NU, u_tau=0.1)
    d2 = np.abs(S2._nut.cpu().numpy() - ref2).max()
    print(f"   u_tau = 0.1: max |d nut| = {d2:.3e}, ratio {d2 / ref2.max():.3e}")
    assert d2 <= 1e-12 * ref2.max(), (d2, ref2.max())
    assert not np.array_equal(ref, ref2)
    # fluid at rest (u = 0, p = 0): wss = 0, D = 0, nut = 0 -- not NaN.  (With a pressure field the facet shear keeps the
    # rounding residue of -pbar n + (pbar n.n) n, about eps |p|: D is then tiny, not zero; nut is zero through |S|.)
    S._U1.dev().zero_()
    S._U2.dev().zero_()
    S._P.dev().zero_()
    S.assemble_first(DT, NU)
    assert bool(torch.isfinite(S._nut).all()) and float(S._nut.abs().max()) == 0.0
    assert float(S.wall_units()[1].abs().max()) == 0.0


# ---- (i) Poiseuille ----------------------------------------------------------------------------------------------------
def test_poiseuille_closed_form(hip):
    """P2 on the rectangle [0, 2] x [0, 1], walls y = 0 and y = 1, u_x = G y (H - y) / (2 nu): |wss| = G H / 2 on both
    walls and nut_c = Cs^2 |cell| D(y_c)^2 G |H - 2 y_c| / (2 nu), to 1e-12 max nut.  Observed: 1.9e-15 max nut."""
    from oasisx_amd import mesh as M
    from tests import walldist_model as WD

    G, Hh = 0.03, 1.0
    mesh = M.create_rectangle(None, [[0.0, 0.0], [2.0, Hh]], [7, 5])
    fv, _ = mesh._entities(1)
    X = mesh.coords.cpu().numpy()
    ext = np.asarray(mesh.exterior_facets(), dtype=np.int64)
    mid = X[fv[ext]].mean(axis=1)
    wall_ids = ext[np.isclose(mid[:, 1], 0.0) | np.isclose(mid[:, 1], Hh)]
    S, clock, _ = _problem(2, 5, 2, _damped(facets=wall_ids), nu=NU, dt=DT, mesh=mesh)
    for u in (S._u1[0], S._u2[0]):
        u.interpolate(lambda x: G * x[1] * (Hh - x[1]) / (2.0 * NU))
    for u in (S._u1[1], S._u2[1]):
        u.interpolate(lambda x: 0.0 * x[0])
    S.assemble_first(DT, NU)
    ut = S._viscosity_model.damping.friction_velocity().cpu().numpy()
    assert np.abs(ut - np.sqrt(G * Hh / 2.0)).max() <= 1e-13
    tri = X[mesh.cells.cpu().numpy()]
    e = tri[:, 1:] - tri[:, :1]
    area = 0.5 * np.abs(np.linalg.det(e))
    ref = WD.poiseuille_nut(CS, area, tri.mean(axis=1)[:, 1], Hh, G, NU, A_PLUS)
    dev = S.eddy_viscosity().cpu().numpy()
    d = np.abs(dev - ref).max()
    print(f"Poiseuille: max |nut - closed form| = {d:.3e}, max nut = {ref.max():.3e}, ratio {d / ref.max():.3e}")
    assert ref.max() > 0.0 and d <= 1e-12 * ref.max()


# ---- (j), (k) steps and operators against the oracle with the damped nut ---------------------------------------------
def _damped_oracle(S, mesh, F, x_v, x_q, W, solver_options=None, low_memory=True):
    """tests.viscosity_model's step model with nut replaced by the damped model's (u_ab -> wss -> u_tau -> D -> nut)."""
    from oracle import ipcs_oracle as O
    from tests import viscosity_model as VM

    class _Forms(VM._FormsWithNut):
        def convection(self, uab):
            nut = W.nut(S, mesh, self._F, uab, NU)[0]
            self._owner.nut = nut
            return self._F.convection(uab) + VM.weighted_stiffness(self._F, nut)

    class DampedOracleStep(VM.ViscosityOracleStep):
        def assemble_first(self, dt, nu):
            plain = self.F
            self.F = _Forms(plain, self)
            try:
                O.OracleFractionalStep.assemble_first(self, dt, nu)
            finally:
                self.F = plain

    R, rc = VM.tg_step_model(F, x_v, x_q, ("smagorinsky", CS), nu=NU, dt=DT, solver_options=solver_options,
                             low_memory=low_memory)
    R.__class__ = DampedOracleStep
    return R, rc


@pytest.mark.parametrize("dim,N", [(2, 8), (3, 3)])
def test_steps_match_the_damped_model(hip, dim, N):
    """(j) Three P2-P1 steps against the ViscosityOracleStep subclass with the damped nut: du < 1e-8, dp < 1e-7."""
    from tests.helpers import KRYLOV

    dt = 0.005
    S, clock, mesh = _problem(dim, N, 2, _damped(), nu=NU, dt=dt)
    F, x_v, x_q = _forms(S, mesh)
    W = _Walls(S, mesh)
    R, rc = _damped_oracle(S, mesh, F, x_v, x_q, W, solver_options=KRYLOV)
    R.u1[:], R.u2[:], R.p[:] = S._U1.rhost(), S._U2.rhost(), S._P.rhost()[:, 0]
    for k in range(3):
        clock["t"] = rc["t"] = (k + 1) * dt
        S.solve(dt, NU, max_iter=1)
        R.solve(dt, NU, max_iter=1)
        du = float(np.abs(S._U.rhost() - R.u1).max())
        dp = float(np.abs(S._P.rhost()[:, 0] - R.p).max())
        dn = float(np.abs(S._nut.cpu().numpy() - R.nut).max())
        print(f"step {k}: du = {du:.3e}, dp = {dp:.3e}, d nut = {dn:.3e} (max nut {R.nut.max():.3e})")
        assert du < 1e-8 and dp < 1e-7, (k, du, dp)
    assert R.nut.max() > 0.0


@pytest.mark.parametrize("kind", ["lattice", "delaunay"])
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_operator_and_rhs_with_damping(hip, dim, N, deg, kind):
    """(k) A and b_first after assemble_first with damping equal the model's entry by entry to 1e-12 max|.|."""
    mesh = _delaunay(dim, N) if kind == "delaunay" else None
    S, clock, mesh = _problem(dim, N, deg, _damped(), nu=NU, dt=DT, mesh=mesh, perturb=0.3)
    F, x_v, x_q = _forms(S, mesh)
    W = _Walls(S, mesh)
    R, rc = _damped_oracle(S, mesh, F, x_v, x_q, W)
    R.u1[:], R.u2[:], R.p[:] = S._U1.rhost(), S._U2.rhost(), S._P.rhost()[:, 0]
    rc["t"] = DT
    _assemble_first(S, clock, DT, NU)
    R.assemble_first(DT, NU)
    dA = abs(S._A.to_scipy() - R.A).max()
    db = np.abs(S._BFIRST.rhost() - R.b_first).max()
    print(f"{kind} ({dim},{N},{deg}): dA = {dA:.3e} (max|A| = {abs(R.A).max():.3e}), db = {db:.3e} "
          f"(max|b| = {np.abs(R.b_first).max():.3e}), max nut {R.nut.max():.3e}")
    assert R.nut.max() > 0.0
    assert dA <= 1e-12 * abs(R.A).max(), dA
    assert db <= 1e-12 * np.abs(R.b_first).max(), db


# ---- (l) damping=None is the undamped model, bit for bit ---------------------------------------------------------------
@pytest.mark.parametrize("dim,N,deg", [(2, 5, 2), (3, 3, 2)])
def test_no_damping_is_the_plain_model(hip, dim, N, deg):
    import torch

    import oasisx_amd as ox

    out = []
    for m in (ox.Smagorinsky(CS), ox.Smagorinsky(CS, damping=None)):
        S, clock, _ = _problem(dim, N, deg, m, nu=NU, dt=DT, perturb=0.3)
        _assemble_first(S, clock, DT, NU)
        out.append((S._nut.clone(), S._A.vals.clone(), S._BFIRST.rdev().clone()))
        with pytest.raises(RuntimeError, match="wall damping"):
            S.wall_units()
    for a, b in zip(*out):
        assert torch.equal(a, b)
    S, clock, _ = _problem(dim, N, deg, _damped(), nu=NU, dt=DT, perturb=0.3)
    _assemble_first(S, clock, DT, NU)
    assert not torch.equal(S._nut, out[0][0]) and bool((S._nut <= out[0][0]).all())  # (D <= 1)


# ---- (m) guards --------------------------------------------------------------------------------------------------------
def test_guards(hip):
    import oasisx_amd as ox
    from oasisx_amd.parallel import Comm
    from tests.helpers import tg_mesh

    with pytest.raises(ValueError, match="Wale"):
        ox.Wale(damping=ox.VanDriest())
    mesh = tg_mesh(2, 4)
    fv, cf = mesh._entities(1)
    interior = np.nonzero(np.bincount(cf.ravel()) == 2)[0][:3]
    with pytest.raises(ValueError, match="interior"):
        _problem(2, 4, 2, _damped(facets=interior), mesh=mesh)
    with pytest.raises(ValueError, match="no facet"):
        _problem(2, 4, 2, _damped(facets=np.zeros(0, dtype=np.int64)))
    with pytest.raises(NotImplementedError, match="rotational"):
        _problem(2, 4, 2, _damped(), rotational=True)
    with pytest.raises(NotImplementedError, match="scalars"):
        _problem(2, 4, 2, _damped(), scalars=[ox.ScalarTransport("T", diffusivity=0.1)])
    pmesh = tg_mesh(2, 4)
    pmesh.comm = Comm(0, 2, None, transport="host")
    with pytest.raises(NotImplementedError, match="partition"):
        _problem(2, 4, 2, _damped(), mesh=pmesh)
    S, _, _ = _problem(2, 4, 2, _damped())
    with pytest.raises(ValueError, match="molecular viscosity"):
        S.viscosity_assemble()
    with pytest.raises(RuntimeError, match="assemble_first"):
        S.wall_units()
    # a table entry outside the wall set writes NaN and reads nothing
    S.assemble_first(DT, NU)
    S._viscosity_model.damping._nearest[:2] = torch_int32([-1, 10 ** 6], S._nut.device)
    S.viscosity_assemble(NU)
    nut = S._nut.cpu().numpy()
    assert np.isnan(nut[:2]).all() and np.isfinite(nut[2:]).all()


def torch_int32(values, device):
    import torch

    return torch.tensor(values, dtype=torch.int32, device=device)


# ---- (n) the demo ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_demo_prints_the_closed_form(hip, capsys, dim):
    """demo/les_channel_hip.py at its smallest size: nut per slab equals the closed form, vanishes towards the wall where
    the undamped model peaks, and y+ of the wall-adjacent cells is printed."""
    from demo.les_channel_hip import main

    res = main(["-N", "4", "--dim", str(dim), "--A-plus", "2"])
    out = capsys.readouterr().out
    assert "y+ of the wall-adjacent cells" in out and "closed form" in out
    assert res["nut_max"] > 0.0 and res["error"] <= 1e-12 * res["nut_max"]
    rows = res["rows"]
    assert len(rows) == 4 and all(r["nut"] < r["nut_plain"] for r in rows)
    assert rows[0]["nut_plain"] > rows[1]["nut_plain"] and rows[0]["damping"] < rows[1]["damping"]
