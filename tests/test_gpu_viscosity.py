"""GPU: eddy-viscosity models in FractionalStep_AB_CN (oasisx_amd/viscosity.py, csrc/ox_viscosity.hip and the NUT
instantiations of csrc/ox_assemble.hip) against the numpy model of tests/viscosity_model.py, which is built on the
oracle's forms and pinned by tests/test_viscosity_host.py.  The model is fed the device's numbering (fields and matrices
compare index by index) and the device's own velocity blocks."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [(2, 6, 1), (2, 5, 2), (3, 3, 1), (3, 3, 2), (2, 4, 3), (3, 2, 3)]


def _perturbed(f, i, t, nu, amp):
    """Taylor-Green plus a smooth perturbation with a divergence (every entry of grad u is exercised)."""
    return lambda x: f(x, t, nu) + amp * np.sin(1.3 * x[0] + 0.7 * x[1] - 0.9 * x[2] + 1.1 * i + 40.0 * t)


def _problem(dim, N, deg, model, nu=0.01, dt=0.005, solver_options=None, options=None, mesh=None, low_memory=True,
             perturb=0.0, **kw):
    """The Taylor-Green set-up of tests.helpers.make_hip_problem with ``viscosity_model=`` (and P3-P2, a mesh handed in
    and, with ``perturb``, velocity levels that are neither solenoidal nor symmetric)."""
    import oasisx_amd as ox
    from oracle import ipcs_oracle as O
    from tests.helpers import KRYLOV, on_boundary, on_boundary3, tg_mesh

    mesh = tg_mesh(dim, N) if mesh is None else mesh
    clock = {"t": 0.0}
    marker = on_boundary if dim == 2 else on_boundary3
    fns = [O.tg_u, O.tg_v, O.tg_w][:dim]
    bcs_u = [[ox.DirichletBC(lambda x, f=f: f(x, clock["t"], nu), ox.LocatorMethod.GEOMETRICAL, marker)] for f in fns]
    opts = {"sell_window": 256, "low_memory_version": low_memory}
    opts.update(options or {})
    if model is not None:
        kw["viscosity_model"] = model
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", deg), ("Lagrange", 2 if deg == 3 else 1), bcs_u=bcs_u, bcs_p=[],
                                solver_options=solver_options or KRYLOV, options=opts, **kw)
    for i, f in enumerate(fns):
        S._u2[i].interpolate(_perturbed(f, i, -dt, nu, perturb))
        S._u1[i].interpolate(_perturbed(f, i, 0.0, nu, perturb))
    S._p.interpolate(lambda x: O.tg_p(x, -dt / 2.0, nu))
    return S, clock, mesh


def _delaunay(dim, N):
    from oasisx_amd import mesh as M

    return M.create_delaunay_box(None, [[-1.0] * dim, [1.0] * dim], N, seed=2)


def _forms(S, mesh):
    """The oracle's forms on the device's mesh arrays, cell order and dof numbering."""
    from oracle import ipcs_oracle as O

    Vi, Q = S._Vi[0][0], S._Q
    F = O.Forms(mesh.coords.cpu().numpy(), Vi.cells_in_kernel_order(), Vi.degree, Q.degree, vd=Vi.cell_dofs.cpu().numpy(),
                qd=Q.cell_dofs.cpu().numpy(), nv_dofs=Vi.num_dofs, nq_dofs=Q.num_dofs)
    return F, Vi.x.cpu().numpy(), Q.x.cpu().numpy()


def _model_of(S, m):
    """The numpy model's description of an oasisx_amd model object, per cell values in the KERNEL's cell order."""
    import oasisx_amd as ox

    if m is None:
        return None
    if isinstance(m, ox.Smagorinsky):
        return ("smagorinsky", m.coefficient)
    if isinstance(m, ox.Wale):
        return ("wale", m.coefficient)
    lc = S._Vi[0][0].local_cells.cpu().numpy()
    return ("cell", m.values(S._mesh)[lc])


def _assemble_first(S, clock, dt, nu):
    clock["t"] = dt
    for bcl in S._bcs_u:
        for bc in bcl:
            bc.update_bc()
    S.assemble_first(dt, nu)


def _sponge(x):
    return 0.02 + 0.05 * (1.0 + x[0]) ** 2 + 0.03 * np.abs(x[1])


# ---- 1. nut per cell ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lattice", "delaunay"])
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_nut_per_cell_matches_the_model(hip, dim, N, deg, kind):
    """Smagorinsky (and, in 3-D, WALE) on Taylor-Green plus a smooth non-solenoidal perturbation: max |nut_device -
    nut_model| <= 1e-12 max nut, the bound tests/test_gpu_parity.py puts on assembled quantities.  S.eddy_viscosity() is
    the same array in the mesh's cell order.

    Observed on one MI355X, maximum of max |d nut| / max nut over the cases: 3.0e-15 for Smagorinsky, 6.4e-15 for WALE
    (both on the P3 tetrahedra)."""
    import oasisx_amd as ox
    from tests import viscosity_model as VM

    dt, nu = 0.1, 0.5
    models = [ox.Smagorinsky()] + ([ox.Wale()] if dim == 3 else [])
    mesh = _delaunay(dim, N) if kind == "delaunay" else None
    for m in models:
        S, clock, mesh = _problem(dim, N, deg, m, nu=nu, dt=dt, mesh=mesh, perturb=0.3)
        F, _, _ = _forms(S, mesh)
        _assemble_first(S, clock, dt, nu)
        ref = VM.nut_cells(F, S._UAB.rhost(), _model_of(S, m))
        dev = S._nut.cpu().numpy()
        d = np.abs(dev - ref).max()
        print(f"{m!r} {kind} ({dim},{N},{deg}): max |d nut| = {d:.3e}, max nut = {ref.max():.3e}, ratio {d / ref.max():.3e}")
        assert ref.max() > 0.0 and dev.min() >= 0.0
        assert d <= 1e-12 * ref.max(), (repr(m), d, ref.max())
        lc = S._Vi[0][0].local_cells.cpu().numpy()
        mesh_order = S.eddy_viscosity().cpu().numpy()
        assert mesh_order.shape == (int(mesh.num_cells),) and np.array_equal(mesh_order[lc], dev)


@pytest.mark.parametrize("dim,N", [(2, 5), (3, 3)])
def test_eddy_viscosity_is_in_mesh_cell_order(hip, dim, N):
    """A CellViscosity given as a function of the centroid: eddy_viscosity() equals it at the centroids of mesh.cells,
    in that order, whatever order the kernels keep their cells in; an array in mesh order comes back as it went in."""
    import oasisx_amd as ox

    f = lambda x: 8.0 + x[0] + 2.0 * x[1] + 4.0 * x[2]  # noqa: E731
    S, clock, mesh = _problem(dim, N, 2, ox.CellViscosity(f))
    _assemble_first(S, clock, 0.005, 0.01)
    cen = mesh.coords[mesh.cells.long()].mean(dim=1).cpu().numpy()
    X = np.zeros((3, cen.shape[0]))
    X[:dim] = cen.T
    assert np.array_equal(S.eddy_viscosity().cpu().numpy(), f(X))
    lc = S._Vi[0][0].local_cells.cpu().numpy()
    assert not np.array_equal(lc, np.arange(lc.shape[0]))  # (the kernel order IS another order here)
    arr = np.arange(cen.shape[0], dtype=np.float64)
    S2, clock2, _ = _problem(dim, N, 2, ox.CellViscosity(arr))
    _assemble_first(S2, clock2, 0.005, 0.01)
    assert np.array_equal(S2.eddy_viscosity().cpu().numpy(), arr)
    with pytest.raises(RuntimeError):
        _problem(dim, N, 2, None)[0].eddy_viscosity()


# ---- 2. A and b_first, entry by entry ----------------------------------------------------------------------------------
@pytest.mark.parametrize("row_blocks", [False, True])
@pytest.mark.parametrize("mode", ["dictionary", "f64", "delaunay"])
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_operator_and_rhs_entry_by_entry(hip, dim, N, deg, mode, row_blocks):
    """After assemble_first with Smagorinsky and with a non-constant CellViscosity: A (identity rows on the first
    component's Dirichlet dofs) and b_first equal the model's to 1e-12 max|.| (tests/test_gpu_parity.py:81-83) -- with
    value dictionaries, with f64 values and on a Delaunay mesh, by width bins and by row blocks.  With a nonzero initial
    guess the A u1 block handed to the tentative solve equals A.mult(u1) bit for bit."""
    import torch

    import oasisx_amd as ox
    from tests import viscosity_model as VM
    from tests.helpers import KRYLOV

    dt, nu = 0.1, 0.5
    so = {k: dict(v, ksp_initial_guess_nonzero=True) for k, v in KRYLOV.items()}
    mesh = _delaunay(dim, N) if mode == "delaunay" else None
    for m in (ox.Smagorinsky(), ox.CellViscosity(_sponge)):
        S, clock, mesh = _problem(dim, N, deg, m, nu=nu, dt=dt, mesh=mesh, solver_options=so, perturb=0.3,
                                  options={"value_dictionary": mode != "f64", "assemble_row_blocks": row_blocks})
        assert S._row_blocks == row_blocks and (not row_blocks or S._Vi[0][0].pattern.n_row_blocks > 0)
        if mode == "dictionary" and dim == 2 and deg <= 2:  # (elsewhere K may exceed 256 distinct values: then f64 is read)
            assert S._M.vcode is not None and S._K.vcode is not None  # the LDS-dictionary instantiation runs
        elif mode == "f64":
            assert S._M.vcode is None and S._K.vcode is None
        F, x_v, x_q = _forms(S, mesh)
        R, rc = VM.tg_step_model(F, x_v, x_q, _model_of(S, m), nu=nu, dt=dt)
        R.u1[:], R.u2[:] = S._U1.rhost(), S._U2.rhost()
        rc["t"] = dt
        _assemble_first(S, clock, dt, nu)
        R.assemble_first(dt, nu)
        dA = abs(S._A.to_scipy() - R.A).max()
        bfirst = S._BFIRST.rhost()
        db = np.abs(bfirst - R.b_first).max()
        kw_share = abs(VM.weighted_stiffness(F, R.nut)).max() / abs(R.A).max()
        print(f"{m!r}: dA = {dA:.3e} (max|A| = {abs(R.A).max():.3e}, max|K_nut| / max|A| = {kw_share:.2e}), "
              f"db = {db:.3e} (max|b| = {np.abs(R.b_first).max():.3e})")
        assert kw_share > 1e-4  # (the term under test is not lost in the bound)
        assert dA <= 1e-12 * abs(R.A).max(), dA
        assert db <= 1e-12 * np.abs(R.b_first).max(), db
        assert S._AU1_valid
        y = torch.zeros_like(S._U1.rdev())
        S._A.mult(S._U1.rdev(), y, dim)
        assert torch.equal(y[: S._no_u], S._B3.rdev()[: S._no_u])


# ---- 3. two pins that need no model ------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_blocks", [False, True])
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_zero_and_constant_cell_viscosity(hip, dim, N, deg, row_blocks):
    """CellViscosity(0.0): A.vals and b_first are the BITS of the run without a model.  CellViscosity(c) at nu: A and
    b_first of the run without a model at nu + c, to 1e-12 max|.|."""
    import torch

    import oasisx_amd as ox

    dt, nu, c = 0.1, 0.5, 0.37
    out = {}
    for key, model, nu_run in (("plain", None, nu), ("zero", ox.CellViscosity(0.0), nu), ("const", ox.CellViscosity(c), nu),
                               ("shifted", None, nu + c)):
        S, clock, _ = _problem(dim, N, deg, model, nu=nu, dt=dt, perturb=0.3, options={"assemble_row_blocks": row_blocks})
        _assemble_first(S, clock, dt, nu_run)
        out[key] = (S._A.vals.clone(), S._BFIRST.rdev().clone())
    assert torch.equal(out["zero"][0], out["plain"][0]) and torch.equal(out["zero"][1], out["plain"][1])
    for k in (0, 1):
        ref = out["shifted"][k]
        d = float((out["const"][k] - ref).abs().max())
        print(f"{'A' if k == 0 else 'b_first'}: max diff {d:.3e}, max|.| {float(ref.abs().max()):.3e}")
        assert d <= 1e-12 * float(ref.abs().max()), (k, d)
    assert not torch.equal(out["const"][0], out["plain"][0])


# ---- 4. whole steps ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("low_memory", [True, False])
@pytest.mark.parametrize("dim,N", [(2, 8), (3, 3)])
def test_steps_match_the_model(hip, dim, N, low_memory):
    """Three P2-P1 Taylor-Green steps with Smagorinsky against the model subclass of the oracle: du < 1e-8, dp < 1e-7,
    the bounds of test_full_steps_match_oracle_krylov."""
    import oasisx_amd as ox
    from tests import viscosity_model as VM
    from tests.helpers import KRYLOV

    nu, dt = 0.01, 0.005
    m = ox.Smagorinsky()
    S, clock, mesh = _problem(dim, N, 2, m, nu=nu, dt=dt, low_memory=low_memory)
    F, x_v, x_q = _forms(S, mesh)
    R, rc = VM.tg_step_model(F, x_v, x_q, _model_of(S, m), nu=nu, dt=dt, solver_options=KRYLOV, low_memory=low_memory)
    for k in range(3):
        clock["t"] = rc["t"] = (k + 1) * dt
        S.solve(dt, nu, max_iter=1)
        R.solve(dt, nu, max_iter=1)
        du = float(np.abs(S._U.rhost() - R.u1).max())
        dp = float(np.abs(S._P.rhost()[:, 0] - R.p).max())
        dn = float(np.abs(S._nut.cpu().numpy() - R.nut).max())
        print(f"step {k}: du = {du:.3e}, dp = {dp:.3e}, d nut = {dn:.3e} (max nut {R.nut.max():.3e})")
        assert du < 1e-8 and dp < 1e-7, (k, du, dp)
    assert R.nut.max() > 0.0


# ---- 5. dissipation ----------------------------------------------------------------------------------------------------
def test_smagorinsky_dissipates(hip):
    """3-D Taylor-Green, five steps: (1/2) u^T M u with Smagorinsky is strictly below the run without a model -- the
    inequality tests/test_viscosity_host.py asserts in the numpy model on the same mesh."""
    import oasisx_amd as ox
    from tests.viscosity_model import DISSIPATION as D

    e = []
    for m in (None, ox.Smagorinsky(Cs=D["Cs"])):
        S, clock, _ = _problem(D["dim"], D["N"], D["deg"], m, nu=D["nu"], dt=D["dt"])
        for k in range(D["steps"]):
            clock["t"] = (k + 1) * D["dt"]
            S.solve(D["dt"], D["nu"], max_iter=1)
        u = S._U.rhost()
        M = S._M.to_scipy()
        e.append(0.5 * float(sum(u[:, i] @ (M @ u[:, i]) for i in range(D["dim"]))))
    print(f"kinetic energy: {e[0]:.12e} without, {e[1]:.12e} with Smagorinsky")
    assert e[1] < e[0]


# ---- 6. guards ---------------------------------------------------------------------------------------------------------
def test_guards(hip):
    import oasisx_amd as ox
    from oasisx_amd.parallel import Comm
    from tests.helpers import tg_mesh

    with pytest.raises(NotImplementedError, match="rotational"):
        _problem(2, 4, 2, ox.Smagorinsky(), rotational=True)
    with pytest.raises(NotImplementedError, match="scalars"):
        _problem(2, 4, 2, ox.Smagorinsky(), scalars=[ox.ScalarTransport("T", diffusivity=0.1)])
    pmesh = tg_mesh(2, 4)
    pmesh.comm = Comm(0, 2, None, transport="host")
    with pytest.raises(NotImplementedError, match="partition"):
        _problem(2, 4, 2, ox.Smagorinsky(), mesh=pmesh)
    with pytest.raises(ValueError, match="three-dimensional"):
        _problem(2, 4, 2, ox.Wale())
    with pytest.raises(ValueError):
        ox.CellViscosity(-0.1)
    with pytest.raises(ValueError):
        _problem(2, 4, 2, ox.CellViscosity(lambda x: x[0]))
    S, _, _ = _problem(2, 4, 2, None)
    with pytest.raises(RuntimeError):
        S.viscosity_assemble()


# ---- 7. the demo -------------------------------------------------------------------------------------------------------
def test_demo_prints_a_decreasing_energy(hip, capsys):
    """demo/les_taylor_green_hip.py at a small N: the printed kinetic energy decreases step by step, with and without
    the model, and the model's run ends below the other."""
    from demo.les_taylor_green_hip import main

    rows = main(["-N", "4", "--steps", "4"])
    out = capsys.readouterr().out
    assert "kinetic energy" in out and "nut" in out
    for key in ("none", "smagorinsky"):
        e = [r["energy"] for r in rows[key]]
        assert len(e) == 4 and all(b < a for a, b in zip(e, e[1:])), (key, e)
    assert all(r["nut_max"] >= r["nut_mean"] >= r["nut_min"] >= 0.0 for r in rows["smagorinsky"])
    assert rows["smagorinsky"][-1]["energy"] < rows["none"][-1]["energy"]
