"""GPU: the Lagrangian average of the dynamic Smagorinsky model (oasisx_amd.DynamicSmagorinsky(average="lagrangian"),
ox_dynamic_lagrangian in csrc/ox_probe.hip) against the numpy model of tests/lagrangian_model.py, which is pinned by
tests/test_lagrangian_host.py.  The model is fed the device's numbering (kernel cell order, mesh cell ids, vertex classes),
so every vertex compares index by index; interpolated values are compared, never cell ids."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [(2, 6, 1), (2, 5, 2), (3, 3, 1), (3, 3, 2), (2, 4, 3), (3, 2, 3)]
PERIODIC = [(2, 6, (0, 1)), (3, 4, (0, 1, 2)), (2, 6, (0,))]
TINY = np.finfo(np.float64).tiny
REL = 1e-12


def _mesh(dim, N, kind="lattice", axes=None):
    from oasisx_amd import mesh as M
    from tests.helpers import tg_mesh

    if kind == "delaunay":
        return M.create_delaunay_box(None, [[-1.0] * dim, [1.0] * dim], N, seed=2)
    mesh = tg_mesh(dim, N)
    return mesh if axes is None else M.make_periodic(mesh, axes)


def _field_fn(dim, axes=None):
    from tests import lagrangian_model as LM

    if axes is None:
        return lambda x: LM.input_field(x, dim)
    return (lambda x: LM.periodic_field(x, dim)) if len(axes) == dim else (lambda x: LM.channel_field(x, dim))


def _problem(dim, N, deg, model, mesh=None, axes=None, nu=0.01, low_memory=True, **kw):
    """A solver on [-1, 1]^dim with both velocity levels set to the test's input field, which is held on the faces that
    are not periodic."""
    import oasisx_amd as ox
    from tests.helpers import KRYLOV

    mesh = _mesh(dim, N, axes=axes) if mesh is None else mesh
    fld = _field_fn(dim, axes)
    free = [k for k in range(dim) if axes is None or k not in axes]

    def marker(x):
        on = np.zeros(x.shape[1], dtype=bool)
        for k in free:
            on |= np.isclose(np.abs(x[k]), 1.0)
        return on

    bcs_u = [[ox.DirichletBC(lambda x, i=i: fld(np.asarray(x)[:dim].T)[:, i], ox.LocatorMethod.GEOMETRICAL, marker)] if free
             else [] for i in range(dim)]
    if model is not None:
        kw["viscosity_model"] = model
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", deg), ("Lagrange", 2 if deg == 3 else 1), bcs_u=bcs_u, bcs_p=[],
                                solver_options=KRYLOV, options={"sell_window": 256, "low_memory_version": low_memory}, **kw)
    for i in range(dim):
        for u in (S._u1[i], S._u2[i]):
            u.interpolate(lambda x, i=i: fld(np.asarray(x)[:dim].T)[:, i])
    return S, mesh


def _forms(S, mesh):
    from oracle import ipcs_oracle as O

    Vi, Q = S._Vi[0][0], S._Q
    F = O.Forms(mesh.coords.cpu().numpy(), Vi.cells_in_kernel_order(), Vi.degree, Q.degree, vd=Vi.cell_dofs.cpu().numpy(),
                qd=Q.cell_dofs.cpu().numpy(), nv_dofs=Vi.num_dofs, nq_dofs=Q.num_dofs)
    return F, Vi.x.cpu().numpy(), Q.x.cpu().numpy()


def _geometry(S, mesh):
    """The model's geometry in the device's numbering: cells in kernel order, their mesh ids, the vertex classes."""
    from tests import lagrangian_model as LM

    Vi = S._Vi[0][0]
    geo, _ = LM.mesh_geometry(mesh, cells=Vi.cells_in_kernel_order(), cell_ids=Vi.local_cells.cpu().numpy())
    m = S._viscosity_model
    if m is not None and getattr(m, "_patches", None) is not None:
        assert geo.n == m._patches.n_vertices and np.array_equal(geo.P.verts, m._patches.cell_verts.cpu().numpy())
    return geo


def _params(m):
    return dict(cs2_max=m.cs2_max, cs2_initial=m.cs2_initial, time_scale=m.time_scale, cs2_floor=m.cs2_floor)


def _dev_fields(m):
    import torch

    return torch.stack(m.lagrangian_fields(), dim=1).cpu().numpy()


def _close(dev, ref, bound, what):
    """|dev - ref| <= bound entry by entry, NaN exactly where the model has NaN; returns max diff / bound."""
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(dev), nan), what
    d = np.abs(np.where(nan, 0.0, dev - ref))
    assert (d <= np.where(nan, 0.0, bound)).all(), (what, float(d.max()), float((d / np.maximum(bound, TINY)).max()))
    return float((d / np.maximum(np.where(nan, np.inf, bound), TINY)).max())


def _compare_update(S, m, F, geo, h, f_old, first, label, out):
    """One evaluated update against the model, stage by stage; the model's update is fed the device's own sources, patch
    mean velocity and old fields, so the per-vertex bounds apply.  Returns the device's new fields."""
    from tests import dynamic_model as DM
    from tests import lagrangian_model as LM

    d = geo.d
    uab = S._UAB.rhost()
    s_lm, s_mm, u_v = LM.sources(F, uab, geo.P, m.filter_ratio)
    src, mom = m._src.cpu().numpy(), m._mom.cpu().numpy()
    for key, dev, ref in (("s_LM", -2.0 * src[:, 0], s_lm), ("s_MM", 4.0 * src[:, 1], s_mm), ("u_v", mom[:, :d], u_v)):
        r = np.abs(dev - ref).max() / np.abs(ref).max()
        out[key] = max(out.get(key, 0.0), float(r))
        assert r <= REL, (label, key, r)
    assert np.abs(m._delta_v.cpu().numpy() - geo.delta).max() <= REL * geo.delta.max()
    res = LM.update(geo, -2.0 * src[:, 0], 4.0 * src[:, 1], mom[:, :d], h, f_old, first, **_params(m))
    dev = _dev_fields(m)
    for k, key in ((0, "F_LM"), (1, "F_MM")):
        out[key] = max(out.get(key, 0.0), _close(dev[:, k], res["F"][:, k], REL * res["mag"][:, k], (label, key)))
    status = m.backtrace_status().cpu().numpy()
    assert status.dtype == np.int32 and np.array_equal(status, res["status"]), (label, status, res["status"])
    if not first:
        ml = res["minlam"][res["status"] != 2]
        assert (np.abs(ml) > 1e-10).all() and (np.abs(ml + geo.tol) > 1e-10).all(), label
    cb = np.nan_to_num(LM.cs2_bound(res, REL), nan=0.0, posinf=0.0)
    near = LM.near_floor(res, m.cs2_floor, REL)
    assert near.mean() <= 0.05, (label, near.mean())
    cs2v = m.vertex_coefficients().cpu().numpy()
    keep = ~near
    out["Cs2_v"] = max(out.get("Cs2_v", 0.0), _close(cs2v[keep], res["cs2v"][keep], cb[keep] + TINY, (label, "Cs2_v")))
    # Cs2 per cell: the mean of the device's own vertex values, to rounding; nut with the coefficient's bound times D s
    cs2c = m._cs2.cpu().numpy()
    ref_c = geo.P.to_cells(cs2v)
    assert np.array_equal(np.isnan(cs2c), np.isnan(ref_c))
    assert np.abs(np.nan_to_num(cs2c - ref_c)).max() <= 4 * np.finfo(float).eps * m.cs2_max
    ds = DM.record_array(F, uab)[:, -2]
    nut, nut_ref = S._nut.cpu().numpy(), geo.P.to_cells(res["cs2v"]) * ds
    cbc = geo.P.to_cells(np.where(near, m.cs2_max, cb))  # (a vertex on the floor's edge: its whole range)
    ok = ~np.isnan(nut_ref)
    out["nut"] = max(out.get("nut", 0.0), _close(nut, nut_ref, REL * nut_ref[ok].max() + np.nan_to_num(cbc) * ds, (label, "nut")))
    assert nut_ref[ok].max() > 0.0 and nut[ok].min() >= 0.0
    lc = S._Vi[0][0].local_cells.cpu().numpy()
    assert np.array_equal(S.smagorinsky_coefficient().cpu().numpy()[lc], cs2c, equal_nan=True)
    assert np.array_equal(S.eddy_viscosity().cpu().numpy()[lc], nut, equal_nan=True)
    return dev, res


def _run_stages(S, m, mesh, dt, nu, label, n=3):
    from tests import lagrangian_model as LM

    F, _, _ = _forms(S, mesh)
    geo = _geometry(S, mesh)
    out = {}
    f_old = np.zeros((geo.n, 2))
    own = LM.Lagrangian(geo, **_params(m))  # the model with its own memory and its own sources
    for k in range(n):
        S.assemble_first(dt, nu)
        assert (m.n_evaluations, m.n_updates) == (k + 1, k + 1)
        f_old, res = _compare_update(S, m, F, geo, dt, f_old, k == 0, f"{label} update {k}", out)
        own.evaluate(F, S._UAB.rhost(), dt)
        # the independent chain: the sources agree to 1e-12 of their maxima and every update is a convex combination
        # (0 <= eps <= 1, sum |lambda| ~ 1), so k + 1 updates differ by at most (k + 1) 1e-12 (max |s| + max |F|)
        scale = np.abs(own.res["mag"]).max(axis=0) + np.abs(own.res["F"]).max(axis=0)
        dd = np.abs(f_old - own.res["F"]).max(axis=0)
        out["chain"] = max(out.get("chain", 0.0), float((dd / scale).max()))
        assert (dd <= (k + 1) * REL * scale).all(), (label, k, dd, scale)
        assert np.array_equal(res["status"], own.res["status"])
    print(f"  {label}: " + ", ".join(f"{k} {v:.2e}" for k, v in out.items()) + f"; status {np.bincount(res['status'], minlength=3).tolist()}")
    return out, geo, F


def _walled_dt(S, mesh):
    from tests import lagrangian_model as LM

    F, _, _ = _forms(S, mesh)
    geo = _geometry(S, mesh)
    return LM.walled_dt(geo, LM.sources(F, S._U1.rhost(), geo.P)[2])


# ---- 1. stage by stage -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lattice", "delaunay"])
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_stages_match_the_model(hip, dim, N, deg, kind):
    """Three assemble_first calls (three updates with memory) on the drifted wave / shear field, dt at 0.45 of the smallest
    altitude over max |u_v|: the sources and u_v within 1e-12 of their maxima; F_LM, F_MM per vertex within 1e-12 of the
    model's magnitude sums; Cs2_v within the bound that follows; Cs2 per cell the mean of the vertex values; nut within
    1e-12 max nut plus the coefficient's bound times D s; status equal on every vertex.

    Observed on one MI355X: see the periodic test's docstring (the maxima are taken over both)."""
    import oasisx_amd as ox

    m = ox.DynamicSmagorinsky(average="lagrangian")
    S, mesh = _problem(dim, N, deg, m, mesh=_mesh(dim, N, kind), nu=0.5)
    dt = _walled_dt(S, mesh)
    out, geo, _ = _run_stages(S, m, mesh, dt, 0.5, f"{kind} ({dim},{N},{deg})")
    assert (m.backtrace_status() == 1).any()  # walls: some path lines leave


@pytest.mark.parametrize("dim,N,axes", PERIODIC)
@pytest.mark.parametrize("deg", [1, 2])
def test_stages_on_periodic_meshes(hip, dim, N, axes, deg):
    """make_periodic lattices, all axes (dt = 0.3 carries departure points across the seam: no status 1) and a channel
    periodic in x (only wall classes leave): the stages as above on the vertex classes.

    Observed on one MI355X, maxima over this and the walled test: s_LM 1.1e-14, s_MM 4.5e-15, u_v 1.2e-15 of max|.|
    (bound 1e-12); F_LM 3.0e-3 and F_MM 3.2e-3 of the bound 1e-12 x the magnitude sum, that is 3.2e-15 of the sums; Cs2_v
    3.9e-4 of its bound; nut 2.1e-3 of its bound; the independent chain 4.9e-15 of (max|s| + max|F|) after three updates
    (bound 3e-12); no vertex near the floor's edge."""
    import oasisx_amd as ox

    m = ox.DynamicSmagorinsky(average="lagrangian")
    S, mesh = _problem(dim, N, deg, m, axes=axes, nu=0.5)
    full = len(axes) == dim
    dt = 0.3 if full else _walled_dt(S, mesh)
    _run_stages(S, m, mesh, dt, 0.5, f"periodic {axes} ({dim},{N},{deg})")
    st = m.backtrace_status().cpu().numpy()
    assert (st == 0).all() if full else ((st == 1).any() and (st != 2).all())


# ---- 2. the kernel through the C ABI -----------------------------------------------------------------------------------
def _launch(S, m, h, first, u, src, f_old):
    """ox_dynamic_lagrangian on given device inputs; returns (F (n, 2), cs2v, status) as numpy."""
    import ctypes as C

    import torch

    from oasisx_amd import _lib

    dev = m._cs2.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
    u, src, f_old = t(u), t(src), t(f_old)
    n = int(f_old.shape[0])
    f_new = torch.full((n, 2), -7.0, dtype=torch.float64, device=dev)
    cs2v = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    status = torch.full((n,), -7, dtype=torch.int32, device=dev)
    args = m.lagrangian_args(h, first, u, int(u.shape[1]), src, f_old, f_new, cs2v, status)
    _lib.check(S._lib.ox_dynamic_lagrangian(C.byref(args), _lib.current_stream()), "ox_dynamic_lagrangian")
    torch.cuda.synchronize()
    return f_new.cpu().numpy(), cs2v.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("kind", ["lattice", "delaunay"])
@pytest.mark.parametrize("dim,N", [(2, 6), (3, 3)])
def test_kernel_on_given_fields_and_sources(hip, dim, N, kind):
    """The kernel alone on random old fields (positive), random sources of both signs and random velocities, with
    cs2_floor = 1e-3 so that the floor is met: fields within 1e-12 of the magnitude sums, status equal, Cs2_v within its
    bound away from the floor's edge; the first-update branch is exact.

    Observed on one MI355X: F_LM 4.0e-4, F_MM 2.2e-4 of the bound; 35 to 38 % of the vertices on the floor, none on its edge."""
    import oasisx_amd as ox
    from tests import lagrangian_model as LM

    m = ox.DynamicSmagorinsky(average="lagrangian", cs2_floor=1e-3, time_scale=0.05)  # (eps ~ 0.5: the sources count)
    S, mesh = _problem(dim, N, 1, m, mesh=_mesh(dim, N, kind))
    geo = _geometry(S, mesh)
    rng = np.random.default_rng(5)
    n = geo.n
    f_old = np.stack([rng.uniform(0.01, 0.05, n), rng.uniform(0.5, 2.0, n)], axis=1)
    s = np.stack([rng.uniform(-0.05, 0.08, n), rng.uniform(0.5, 2.0, n)], axis=1)
    u = rng.standard_normal((n, dim + 2))  # a row stride that is not gdim
    h = 0.6 * 2.0 / N / np.abs(u[:, :dim]).max()
    src = np.stack([-0.5 * s[:, 0], 0.25 * s[:, 1]], axis=1)
    res = LM.update(geo, s[:, 0], s[:, 1], u[:, :dim], h, f_old, False, **_params(m))
    ml = res["minlam"]
    assert (np.abs(ml) > 1e-10).all() and (np.abs(ml + geo.tol) > 1e-10).all()
    F, cs2v, status = _launch(S, m, h, False, u, src, f_old)
    assert np.array_equal(status, res["status"]) and (status == 0).any() and (status == 1).any()
    r = [_close(F[:, k], res["F"][:, k], REL * res["mag"][:, k], k) for k in range(2)]
    floored = res["F"][:, 0] == m.cs2_floor * res["F"][:, 1]
    near = LM.near_floor(res, m.cs2_floor, REL)
    print(f"  {kind} {dim}-D: F_LM {r[0]:.2e}, F_MM {r[1]:.2e} of the bound; floored {floored.mean():.2f}, near {near.mean():.3f}")
    assert floored.any() and not floored.all() and near.mean() <= 0.05
    _close(cs2v[~near], res["cs2v"][~near], LM.cs2_bound(res, REL)[~near] + TINY, "Cs2_v")
    # the first update: no back-trace, exact products
    F1, c1, st1 = _launch(S, m, h, True, np.full_like(u, np.nan), src, f_old)
    ref = LM.update(geo, s[:, 0], s[:, 1], u[:, :dim], h, f_old, True, **_params(m))
    assert np.array_equal(F1, ref["F"]) and (st1 == 0).all()
    assert np.abs(c1 - ref["cs2v"]).max() <= 4 * np.finfo(float).eps * m.cs2_max


@pytest.mark.parametrize("kind", ["lattice", "delaunay"])
@pytest.mark.parametrize("dim,N", [(2, 6), (3, 3)])
def test_backtrace_in_isolation(hip, dim, N, kind):
    """Sources equal to the old fields.  A constant comes back as the constant; with F_LM > 0 > F_MM the product is not
    positive, eps = 0 exactly, and the kernel returns the interpolant alone: a linear field gives a.(x_v - h U) + b at
    every status-0 vertex within 1e-13 max|F|, at 0.4 and at 2.5 cell widths (off the hint, through the grid); h = 0 gives
    the old field within 1e-14.

    Observed on one MI355X: constant within 2.5e-16; linear within 1.3e-16 of max|F| at 0.4 and at 2.5 widths; h = 0 within
    2.3e-16."""
    import oasisx_amd as ox

    m = ox.DynamicSmagorinsky(average="lagrangian", cs2_floor=0.0)
    S, mesh = _problem(dim, N, 1, m, mesh=_mesh(dim, N, kind))
    geo = _geometry(S, mesh)
    n, x = geo.n, geo.x_v
    as_src = lambda f: np.stack([-0.5 * f[:, 0], 0.25 * f[:, 1]], axis=1)  # noqa: E731
    U = np.array([0.8, -0.5, 0.33])[:dim] / np.linalg.norm(np.array([0.8, -0.5, 0.33])[:dim])
    u = np.tile(U, (n, 1))
    const = np.tile([0.03, 1.75], (n, 1))
    F, cs2v, status = _launch(S, m, 0.4 * 2.0 / N, False, u, as_src(const), const)
    dc = np.abs(F - const).max() / 1.75
    assert dc <= 4 * np.finfo(float).eps and np.abs(cs2v - 0.03 / 1.75).max() <= 1e-15
    a, b = np.array([[0.7, -1.3, 0.4], [1.1, 0.6, -0.9]])[:, :dim], np.array([5.0, -5.0])
    lin = x @ a.T + b
    assert (lin[:, 0] > 0).all() and (lin[:, 1] < 0).all()
    seen = []
    for widths in (0.4, 2.5):
        h = widths * 2.0 / N
        F, cs2v, status = _launch(S, m, h, False, u, as_src(lin), lin)
        ok = status == 0
        assert ok.any() and (status == 1).any() and (status != 2).all()
        ref = (x - h * U) @ a.T + b
        seen.append(np.abs(F[ok] - ref[ok]).max() / np.abs(lin).max())
        assert seen[-1] <= 1e-13
        assert np.array_equal(F[~ok], lin[~ok]) and (cs2v == 0.0).all()  # F_MM < 0: the coefficient is 0
        # inside the box the point has a cell, outside it has none
        inside = (np.abs(x - h * U) < 1.0 - 1e-9).all(axis=1)
        outside = (np.abs(x - h * U) > 1.0 + 1e-9).any(axis=1)
        assert ok[inside].all() and not ok[outside].any()
    F, _, status = _launch(S, m, 0.0, False, u, as_src(lin), lin)
    d0 = np.abs(F - lin).max() / np.abs(lin).max()
    assert (status == 0).all() and d0 <= 1e-14
    print(f"  {kind} {dim}-D: constant {dc:.2e}, linear {seen[0]:.2e} / {seen[1]:.2e} of max|F|, h = 0 {d0:.2e}")


@pytest.mark.parametrize("dim,N,axes", [(2, 6, (0, 1)), (3, 4, (0, 1, 2))])
def test_backtrace_across_the_seam(hip, dim, N, axes):
    """On the periodic lattice a velocity that carries every vertex class across the seam along x (1.8 of the period 2;
    the masters lie in [-1, 1 - 2/N]) gives status 0 everywhere and the model's values; a periodic old field
    sin(pi x + 1) comes back as the P1 interpolant of the shifted field.

    Observed on one MI355X: F within 2.2e-4 of 1e-12 x the magnitude sums (2-D), bit-equal (3-D)."""
    import oasisx_amd as ox
    from tests import lagrangian_model as LM

    m = ox.DynamicSmagorinsky(average="lagrangian", cs2_floor=0.0)
    S, mesh = _problem(dim, N, 1, m, axes=axes)
    geo = _geometry(S, mesh)
    n, x = geo.n, geo.x_v
    U = np.array([1.8, 0.37, -0.23])[:dim]
    u = np.tile(U, (n, 1))
    raw = x - U
    assert (raw[:, 0] < -1.0).all() and (geo.fold(raw) >= -1.0).all() and (geo.fold(raw) < 1.0).all()
    f_old = np.stack([2.0 + np.sin(np.pi * x[:, 0] + 1.0), -3.0 + np.cos(np.pi * x[:, 1])], axis=1)  # product < 0: eps = 0
    src = np.stack([-0.5 * f_old[:, 0], 0.25 * f_old[:, 1]], axis=1)
    res = LM.update(geo, f_old[:, 0], f_old[:, 1], u, 1.0, f_old, False, **_params(m))
    assert (res["eps"] == 0.0).all()
    ml = res["minlam"]
    assert (np.abs(ml) > 1e-10).all() and (np.abs(ml + geo.tol) > 1e-10).all()
    F, _, status = _launch(S, m, 1.0, False, u, src, f_old)
    assert (status == 0).all() and (res["status"] == 0).all()
    r = [_close(F[:, k], res["F"][:, k], REL * res["mag"][:, k], k) for k in range(2)]
    print(f"  seam {dim}-D: F within {max(r):.2e} of the bound")
    assert np.abs(F - f_old).max() > 0.1  # (the field did move)


# ---- 3. whole steps ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("update_every", [1, 2])
@pytest.mark.parametrize("dim,N", [(2, 8), (3, 3)])
def test_steps_match_the_model(hip, dim, N, update_every):
    """Three P2-P1 steps against LagrangianOracleStep: du < 1e-8, dp < 1e-7 with equal iteration counts, the bounds of
    test_gpu_dynamic.test_steps_match_the_model; with update_every = 2 the fields are updated in steps 0 and 2 and the
    nut of step 1 comes from the stored Cs2 (nut = Cs2 D s of the new u_ab, Cs2 bit-equal to step 0's).

    Observed on one MI355X: du <= 1.5e-11, dp <= 5.2e-10, d nut <= 6.4e-14 (max nut 1.7e-2), the iteration counts equal."""
    import torch

    import oasisx_amd as ox
    from tests import lagrangian_model as LM
    from tests.helpers import KRYLOV

    nu, dt = 0.01, 0.005
    m = ox.DynamicSmagorinsky(average="lagrangian", update_every=update_every)
    S, mesh = _problem(dim, N, 2, m, nu=nu)
    F, x_v, x_q = _forms(S, mesh)
    geo = _geometry(S, mesh)
    R = LM.step_model(F, x_v, x_q, geo, update_every=update_every, nu=nu, dt=dt, solver_options=KRYLOV)
    R.u1[:], R.u2[:] = S._U1.rhost(), S._U2.rhost()
    cs2_prev = None
    for k in range(3):
        S.solve(dt, nu, max_iter=1)
        R.solve(dt, nu, max_iter=1)
        du = float(np.abs(S._U.rhost() - R.u1).max())
        dp = float(np.abs(S._P.rhost()[:, 0] - R.p).max())
        dn = float(np.abs(S._nut.cpu().numpy() - R.nut).max())
        its, rits = S.iteration_counts(), dict(R.its)
        print(f"step {k}: du = {du:.3e}, dp = {dp:.3e}, d nut = {dn:.3e} (max nut {R.nut.max():.3e}), its {its} / {rits}")
        assert du < 1e-8 and dp < 1e-7, (k, du, dp)
        for key in ("tentative", "pressure", "update"):  # (the device pads its lists with zeros to four solves)
            dev_its, ref_its = np.ravel(its[key]), np.ravel(rits[key])
            assert np.array_equal(dev_its[: ref_its.shape[0]], ref_its) and not dev_its[ref_its.shape[0]:].any(), (k, key, its, rits)
        assert (m.n_evaluations, m.n_updates) == (R.n_evaluations, R.n_updates) == (k + 1, k // update_every + 1)
        cs2 = m._cs2.clone()
        if update_every == 2 and k == 1:
            assert torch.equal(cs2, cs2_prev)  # between updates: the stored Cs2 ...
            assert dn <= 1e-12 * R.nut.max()   # ... with the D s of this step's u_ab, as the model does
        cs2_prev = cs2
    assert R.nut.max() > 0.0


# ---- 4. reproducibility and restart ------------------------------------------------------------------------------------
def _three_steps(dim, N, update_every, tmp_path=None, restart_after=None):
    import torch

    import oasisx_amd as ox

    nu, dt = 0.01, 0.005
    m = ox.DynamicSmagorinsky(average="lagrangian", update_every=update_every)
    S, mesh = _problem(dim, N, 2, m, nu=nu)
    for k in range(3):
        if restart_after is not None and k == restart_after:
            path = str(tmp_path / "lagrangian.npz")
            m.save(path)
            state = [t.rdev().clone() for t in (S._U1, S._U2, S._P)]
            m = ox.DynamicSmagorinsky(average="lagrangian", update_every=update_every)
            S, mesh = _problem(dim, N, 2, m, mesh=mesh, nu=nu)
            for t, s in zip((S._U1, S._U2, S._P), state):
                t.dev().copy_(s)
            S._U.dev().copy_(state[0])
            m.load(path)
        S.solve(dt, nu, max_iter=1)
    torch.cuda.synchronize()
    return S, m


@pytest.mark.parametrize("update_every", [1, 2])
def test_reproducible_and_restart_bit_for_bit(hip, tmp_path, update_every):
    """Two runs of three steps are torch.equal in u, p, nut and the fields; save after step 2, load into a fresh solver and
    model, and step 3 gives the same bits."""
    import torch

    S1, m1 = _three_steps(2, 8, update_every)
    S2, m2 = _three_steps(2, 8, update_every)
    S3, m3 = _three_steps(2, 8, update_every, tmp_path, restart_after=2)
    for S, m in ((S2, m2), (S3, m3)):
        assert torch.equal(S._U.rdev(), S1._U.rdev()) and torch.equal(S._P.rdev(), S1._P.rdev())
        assert torch.equal(S._nut, S1._nut)
        for a, b in zip(m.lagrangian_fields(), m1.lagrangian_fields()):
            assert torch.equal(a, b)
        assert torch.equal(m.vertex_coefficients(), m1.vertex_coefficients())
        assert torch.equal(m.backtrace_status(), m1.backtrace_status())
        assert (m.n_evaluations, m.n_updates) == (m1.n_evaluations, m1.n_updates)
    assert float(S1._nut.max()) > 0.0


# ---- 5. NaN ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N,deg", [(2, 6, 1), (3, 8, 1)])  # (the NaN reaches three rings of cells: 3-D needs room)
def test_nan_stays_in_its_neighbourhood(hip, dim, N, deg):
    """After a clean first update, a NaN in one dof of u_ab: in the next update the vertices whose patch mean velocity is
    NaN get status 2 and NaN fields, nut is NaN exactly where the model's is, and finite everywhere else.

    Observed on one MI355X: (2,6,1): status 2 at 4 of 49 vertices, NaN nut in 18 of 72 cells; (3,8,1): 8 of 729 vertices,
    162 of 3072 cells."""
    import torch

    import oasisx_amd as ox
    from tests import lagrangian_model as LM

    m = ox.DynamicSmagorinsky(average="lagrangian")
    S, mesh = _problem(dim, N, deg, m, nu=0.5)
    dt = _walled_dt(S, mesh)
    geo = _geometry(S, mesh)
    S.assemble_first(dt, 0.5)
    f_old = _dev_fields(m)
    S._UAB.dev()[int(S._Vi[0][0].cell_dofs[0, 0]), 0] = float("nan")
    S.viscosity_assemble(0.5, dt)
    # the model's update on the device's own sources and patch mean velocity (as in the stage test: where a NaN dof meets
    # a coefficient that is exactly 0, the cell kernels of section 26 and numpy need not agree on the product)
    src, mom = m._src.cpu().numpy(), m._mom.cpu().numpy()
    u_v = mom[:, :dim]
    res = LM.update(geo, -2.0 * src[:, 0], 4.0 * src[:, 1], u_v, dt, f_old, False, **_params(m))
    status = m.backtrace_status().cpu().numpy()
    assert np.array_equal(status, res["status"]) and (status == 2).any() and (status != 2).any()
    assert np.array_equal(status == 2, np.isnan(u_v).any(axis=1))
    dev = _dev_fields(m)
    assert np.array_equal(np.isnan(dev), np.isnan(res["F"])) and np.isnan(dev[status == 2]).all()
    cs2v = m.vertex_coefficients().cpu().numpy()
    assert np.array_equal(np.isnan(cs2v), np.isnan(res["cs2v"])) and np.isnan(cs2v[status == 2]).all()
    ds = m._rec.cpu().numpy()[:, -2]
    nut = S._nut.cpu().numpy()
    nan_ref = np.isnan(geo.P.to_cells(res["cs2v"])) | np.isnan(ds)  # a cell with a NaN vertex coefficient, or a NaN D s
    assert np.array_equal(np.isnan(nut), nan_ref)
    assert np.isnan(nut).any() and not np.isnan(nut).all() and bool(torch.isnan(S._nut[0]))
    near_nan = np.isnan(cs2v)[geo.P.verts].any(axis=1)
    assert np.isfinite(nut[~near_nan & ~np.isnan(ds)]).all()
    print(f"  ({dim},{N},{deg}): status 2 at {int((status == 2).sum())} of {status.shape[0]} vertices, NaN nut in "
          f"{int(np.isnan(nut).sum())} of {nut.shape[0]} cells")


# ---- 6. combinations ---------------------------------------------------------------------------------------------------
def test_scalars_full_stress_and_storage_modes(hip):
    """turbulent_schmidt= runs with scalar_diffusivity == kappa + nut / Sc_t; stress_form="full" and low_memory_version
    False take steps whose nut agrees with the model's update from the device's own sources, as the stage test asks; a
    solver without this model makes none of the new calls."""
    import torch

    import oasisx_amd as ox
    from oasisx_amd import _lib

    nu, dt, kappa, sct = 0.01, 0.005, 0.2, 0.7
    sc = ox.ScalarTransport("T", diffusivity=kappa, turbulent_schmidt=sct)
    S, mesh = _problem(2, 5, 2, ox.DynamicSmagorinsky(average="lagrangian"), nu=nu, scalars=[sc])
    S.scalar("T").interpolate(lambda x: np.sin(x[0]) * np.cos(x[1]))
    S.solve(dt, nu, max_iter=1)
    assert torch.equal(S.scalar_diffusivity("T", nu), kappa + S.eddy_viscosity() / sct)
    assert float(S.scalar_diffusivity("T", nu).max()) > kappa and bool(torch.isfinite(S._U.rdev()).all())
    for kw in ({"stress_form": "full"}, {"low_memory": False}):
        m = ox.DynamicSmagorinsky(average="lagrangian")
        S, mesh = _problem(3, 3, 2, m, nu=nu, **kw)
        F, _, _ = _forms(S, mesh)
        geo = _geometry(S, mesh)
        f_old = np.zeros((geo.n, 2))
        out = {}
        for k in range(2):
            S.solve(dt, nu, max_iter=1)
            f_old, _ = _compare_update(S, m, F, geo, dt, f_old, k == 0, f"{kw} step {k}", out)
        assert bool(torch.isfinite(S._U.rdev()).all()) and float(S._nut.max()) > 0.0
    # the default path and the other averages
    lib = _lib.load()
    calls = []

    class Spy:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            if name == "ox_dynamic_lagrangian":
                calls.append(name)
            return getattr(self._lib, name)

    for model in (None, ox.Smagorinsky(), ox.DynamicSmagorinsky(), ox.DynamicSmagorinsky(average="local")):
        S, _ = _problem(2, 5, 2, model, nu=nu)
        S._lib = Spy(lib)
        S.solve(dt, nu, max_iter=1)
        assert calls == []
    S, _ = _problem(2, 5, 2, ox.DynamicSmagorinsky(average="lagrangian"), nu=nu)
    S._lib = Spy(lib)
    S.solve(dt, nu, max_iter=1)
    assert calls == ["ox_dynamic_lagrangian"]


# ---- 7. guards ---------------------------------------------------------------------------------------------------------
def test_guards_on_a_live_solver(hip, tmp_path):
    import ctypes as C

    import torch

    import oasisx_amd as ox
    from oasisx_amd import _lib
    from oasisx_amd.parallel import Comm
    from tests.helpers import tg_mesh

    lag = lambda **kw: ox.DynamicSmagorinsky(average="lagrangian", **kw)  # noqa: E731
    with pytest.raises(NotImplementedError, match="rotational"):
        _problem(2, 4, 2, lag(), rotational=True)
    pmesh = tg_mesh(2, 4)
    pmesh.comm = Comm(0, 2, None, transport="host")
    with pytest.raises(NotImplementedError, match="partition"):
        _problem(2, 4, 2, lag(), mesh=pmesh)
    m = lag()
    S, mesh = _problem(2, 4, 2, m)
    for what in ("lagrangian_fields", "vertex_coefficients", "backtrace_status", "products"):
        with pytest.raises(RuntimeError):
            getattr(m, what)()
    with pytest.raises(RuntimeError):
        S.smagorinsky_coefficient()
    with pytest.raises(ValueError, match="dt"):
        S.viscosity_assemble(0.01)
    with pytest.raises(ValueError, match="dt"):
        S.viscosity_assemble(0.01, float("nan"))
    assert m.n_evaluations == 0
    S.assemble_first(0.005, 0.01)
    for what in ("bin_coefficients", "bin_sums"):
        with pytest.raises(RuntimeError, match="lagrangian"):
            getattr(m, what)()
    assert S.smagorinsky_coefficient().shape == (int(mesh.num_cells),)
    m2 = lag(update_every=2)
    S2, _ = _problem(2, 4, 2, m2, mesh=mesh)
    path = str(tmp_path / "fields.npz")
    m.save(path)
    with pytest.raises(ValueError, match="update_every"):
        m2.load(path)
    with pytest.raises(RuntimeError, match="global"):
        ox.DynamicSmagorinsky().save(path)
    # the C entry point refuses what it can see on the host, before any launch
    lib, n = hip, m._patches.n_vertices
    f = [torch.zeros((n, 2), dtype=torch.float64, device=m._cs2.device) for _ in range(2)]
    good = lambda: m.lagrangian_args(0.01, False, m._mom, m._nm, m._src, f[0], f[1], m._cs2v, m._status)  # noqa: E731
    assert lib.ox_dynamic_lagrangian(C.byref(good()), None) == 0
    assert lib.ox_dynamic_lagrangian(None, None) != 0
    for name, value, text in (("f_new", f[0].data_ptr(), b"f_old"), ("loc", None, b"null"), ("gdim", 4, b"gdim"),
                              ("h", -1.0, b"h="), ("h", float("nan"), b"h="), ("time_scale", 0.0, b"time_scale"),
                              ("cs2_floor", 1.0, b"cs2_floor"), ("tol", 1.0, b"tol"), ("u_stride", 1, b"u_stride"),
                              ("n_mesh_cells", 3, b"n_mesh_cells"), ("src", None, b"null"), ("n_vertices", -1, b"n_vertices"),
                              ("n_cells", 0, b"n_cells")):
        a = good()
        setattr(a, name, value)
        assert lib.ox_dynamic_lagrangian(C.byref(a), None) != 0, name
        assert text in lib.ox_last_error(), (name, lib.ox_last_error())
    a = good()
    a.n_vertices = 0
    a.x = None
    assert lib.ox_dynamic_lagrangian(C.byref(a), None) == 0  # n == 0 launches nothing
    torch.cuda.synchronize()


# ---- 8. the demo -------------------------------------------------------------------------------------------------------
def test_demo_prints_both_averages(hip, capsys):
    """demo/lagrangian_les_channel_hip.py at its smallest size: a row per slab for "local" and "lagrangian", the share of
    cells clipped to 0 and the step-to-step change of Cs2 for each.  The local average clips cells to 0; the Lagrangian
    one, which starts from cs2_initial and has a memory, changes less from step to step.

    Observed on one MI355X (N = 8, 4 steps): clipped to 0: local 0.49, lagrangian 0.00; mean |dCs2| per step: local
    7.8e-3, lagrangian 6.2e-4."""
    from demo.lagrangian_les_channel_hip import main

    res = main(["-N", "8", "--steps", "4"])
    out = capsys.readouterr().out
    assert "lagrangian" in out and "local" in out and "clipped to 0" in out
    assert len(res["local"]["rows"]) == len(res["lagrangian"]["rows"]) == 8
    print(f"clipped to 0: local {res['local']['clipped']:.2f}, lagrangian {res['lagrangian']['clipped']:.2f}; "
          f"mean |dCs2| per step: local {res['local']['change']:.2e}, lagrangian {res['lagrangian']['change']:.2e}")
    assert 0.0 <= res["lagrangian"]["clipped"] <= res["local"]["clipped"]
    assert res["lagrangian"]["change"] < res["local"]["change"]
