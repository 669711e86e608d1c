"""Host (no GPU): the numpy model of the Lagrangian average (tests/lagrangian_model.py) against the properties the
back-trace and the relaxation must have, the conditions the GPU tests (tests/test_gpu_lagrangian.py) put on their inputs,
and the construction-time guards and the dt requirement of oasisx_amd.DynamicSmagorinsky(average="lagrangian")."""
import numpy as np
import pytest

from tests import dynamic_model as DM
from tests import lagrangian_model as LM
from tests import viscosity_model as VM

CASES = [(2, 6, 1), (2, 5, 2), (3, 3, 1), (3, 3, 2), (2, 4, 3), (3, 2, 3)]
PERIODIC = [(2, 6, (0, 1)), (3, 4, (0, 1, 2)), (2, 6, (0,))]  # (dim, N, periodic axes); the last: a channel periodic in x
TOL = 1e-10


def _setup(dim, N, deg):
    F = VM.tg_forms(dim, N, deg, 2 if deg == 3 else 1)
    P = DM.Patches(F)
    return F, LM.input_field(F.x_v, dim), LM.Geometry(F.coords, F.cells, P)


def _ox_mesh(dim, N, kind):
    from oasisx_amd import mesh as M
    from tests.helpers import tg_mesh

    if kind == "delaunay":
        return M.create_delaunay_box(None, [[-1.0] * dim, [1.0] * dim], N, seed=2, device="cpu")
    return tg_mesh(dim, N, device="cpu")


def _periodic_mesh(dim, N, axes):
    from oasisx_amd import mesh as M
    from tests.helpers import tg_mesh

    return M.make_periodic(tg_mesh(dim, N, device="cpu"), axes)


def _boundary_vertices(geo):
    """Vertices of the facets that belong to one cell only."""
    import itertools

    d = geo.d
    seen = {}
    for c in geo.cells:
        for f in itertools.combinations(sorted(c.tolist()), d):
            seen[f] = seen.get(f, 0) + 1
    on = np.zeros(geo.coords.shape[0], dtype=bool)
    for f, k in seen.items():
        if k == 1:
            on[list(f)] = True
    return on


# ---- the constructor and dt --------------------------------------------------------------------------------------------
def test_guards_at_construction():
    import oasisx_amd as ox

    m = ox.DynamicSmagorinsky(average="lagrangian")
    assert (m.cs2_initial, m.time_scale, m.cs2_floor, m.filter_ratio, m.cs2_max, m.update_every) == (
        0.0256, 1.5, 1e-24, 2.0, 0.09, 1)
    assert m.needs_dt and m.diffuses_scalars and "lagrangian" in repr(m)
    assert not ox.DynamicSmagorinsky().needs_dt and not ox.DynamicSmagorinsky(average="local").needs_dt
    assert not getattr(ox.Smagorinsky(), "needs_dt", False)
    for kw in ({"axis": 1}, {"cell_bins": np.zeros(4, dtype=np.int64)}, {"axis": 1, "edges": [-1.0, 0.0, 1.0]}, {"edges": [0.0, 1.0]}):
        with pytest.raises(ValueError):
            ox.DynamicSmagorinsky(average="lagrangian", **kw)
    with pytest.raises(ValueError, match="lagrangian"):
        ox.DynamicSmagorinsky(average="lagrangian", axis=1)
    for c in (-0.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cs2_initial"):
            ox.DynamicSmagorinsky(average="lagrangian", cs2_initial=c)
    for t in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="time_scale"):
            ox.DynamicSmagorinsky(average="lagrangian", time_scale=t)
    for f in (-1e-30, 0.1, float("nan")):
        with pytest.raises(ValueError, match="cs2_floor"):
            ox.DynamicSmagorinsky(average="lagrangian", cs2_floor=f)
    ox.DynamicSmagorinsky(average="lagrangian", cs2_floor=0.0, cs2_initial=0.0)
    with pytest.raises(ValueError, match="average"):
        ox.DynamicSmagorinsky(average="plane")
    for what in ("products", "lagrangian_fields", "vertex_coefficients", "backtrace_status"):
        with pytest.raises(RuntimeError):
            getattr(m, what)()
    with pytest.raises(RuntimeError, match="local"):
        ox.DynamicSmagorinsky(average="local").lagrangian_fields()
    with pytest.raises(RuntimeError):
        m.save("unused.npz")


def test_check_model_and_the_dt_requirement_before_the_library():
    """check_model needs no new refusals; rotational and partitions stay refused; evaluate without dt raises before any
    device call (the model is not even bound: the dt guard of a bound model is the GPU guard test's)."""
    import oasisx_amd as ox
    from oasisx_amd.parallel import Comm
    from oasisx_amd.viscosity import check_model
    from tests.helpers import tg_mesh

    mesh = tg_mesh(2, 4, device="cpu")
    m = ox.DynamicSmagorinsky(average="lagrangian")
    check_model(m, mesh, False, None)
    with pytest.raises(NotImplementedError, match="rotational"):
        check_model(m, mesh, True, None)
    pmesh = tg_mesh(2, 4, device="cpu")
    pmesh.comm = Comm(0, 2, None, transport="host")
    with pytest.raises(NotImplementedError, match="partition"):
        check_model(m, pmesh, False, None)
    m._patches = object()  # as if bound: the dt guard comes before the first launch
    for dt in (None, float("nan"), -0.1):
        with pytest.raises(ValueError, match="dt"):
            m.evaluate(None, None, 0.5, dt=dt)
    with pytest.raises(ValueError, match="dt"):
        m.evaluate(None, None, 0.5)


# ---- the back-trace ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_backtrace_preserves_constants_and_linear_fields(dim, N, deg):
    """A constant old field comes back as the constant at every vertex (status 0: the barycentric coordinates sum to one;
    status 1: the vertex keeps its own value); a linear old field a.x + b is reproduced at x' = x_v - h u_v wherever a
    cell was found, to 1e-13 max|F|; h = 0 returns the old values."""
    F, u, geo = _setup(dim, N, deg)
    u_v = LM.sources(F, u, geo.P)[2]
    h = LM.walled_dt(geo, u_v)
    const = np.full((geo.n, 2), [3.25, 7.5])
    B, Bm, status, minlam, xp = geo.backtrace(u_v, h, const)
    assert (status == 0).any() and np.abs(B - const).max() <= 1e-14 * 7.5
    a = np.array([[0.7, -1.3, 0.4], [1.1, 0.6, -0.9]])[:, :dim]
    lin = geo.x_v @ a.T + np.array([2.0, 3.0])
    widths = 2.5 if N >= 3 else 1.2  # cell widths travelled: off the hint and through the grid (N = 2: the box is 2 wide)
    for hh, U in ((h, u_v), (widths * 2.0 / N, np.tile(np.array([0.8, -0.5, 0.33])[:dim] / np.linalg.norm([0.8, -0.5, 0.33][:dim]),
                                                   (geo.n, 1)))):
        B, _, status, _, xp = geo.backtrace(U, hh, lin)
        ok = status == 0
        assert ok.any()
        assert np.abs(B[ok] - (xp[ok] @ a.T + np.array([2.0, 3.0]))).max() <= 1e-13 * np.abs(lin).max()
        assert np.array_equal(B[~ok], lin[~ok])
    B, _, status, _, _ = geo.backtrace(u_v, 0.0, lin)
    assert (status == 0).all() and np.abs(B - lin).max() <= 1e-14 * np.abs(lin).max()
    res = LM.update(geo, lin[:, 0], lin[:, 1], u_v, 0.0, np.abs(lin), False)
    assert (res["eps"] == 0.0).all() and np.abs(res["F"][:, 1] - np.abs(lin)[:, 1]).max() <= 1e-14 * np.abs(lin).max()


@pytest.mark.parametrize("dim,N,deg", CASES)
def test_scaling_of_velocity_and_time(dim, N, deg):
    """u -> a u with dt -> dt / a: the same departure points and Cs2, F_LM and F_MM scale by a^4 (to 1e-12 relative),
    through three updates -- T scales as 1 / a, so eps is unchanged."""
    F, u, geo = _setup(dim, N, deg)
    a = 1.7
    dt = LM.walled_dt(geo, LM.sources(F, u, geo.P)[2])
    m1, m2 = LM.Lagrangian(geo), LM.Lagrangian(geo)
    for k in range(3):
        m1.evaluate(F, u, dt)
        m2.evaluate(F, a * u, dt / a)
        r1, r2 = m1.res, m2.res
        assert np.abs(r2["xp"] - r1["xp"]).max() <= 1e-14 and np.array_equal(r1["status"], r2["status"])
        assert np.abs(r2["F"] - a ** 4 * r1["F"]).max() <= 1e-12 * a ** 4 * np.abs(r1["F"]).max()
        assert np.abs(r2["cs2v"] - r1["cs2v"]).max() <= 1e-12 * np.abs(r1["cs2v"]).max()
        if k:
            assert np.abs(r2["eps"] - r1["eps"]).max() <= 1e-12


@pytest.mark.parametrize("dim,N,deg", [(2, 6, 1), (3, 3, 2)])
def test_zero_field_and_nan(dim, N, deg):
    """A zero field gives Cs2 = 0 and nut = 0 without NaN through three updates (eps = 0: the product is not positive); a
    NaN velocity at one vertex gives status 2 and NaN fields there; max lets a NaN through from either side."""
    F, u, geo = _setup(dim, N, deg)
    m = LM.Lagrangian(geo)
    for k in range(3):
        nut, cs2 = m.evaluate(F, 0.0 * u, 0.1)
        assert np.array_equal(nut, np.zeros_like(nut)) and np.array_equal(cs2, np.zeros_like(cs2))
        assert np.array_equal(m.res["F"], np.zeros_like(m.res["F"])) and (m.res["status"] == 0).all()
    s_lm, s_mm, u_v = LM.sources(F, u, geo.P)
    first = LM.update(geo, s_lm, s_mm, u_v, 0.1, np.zeros((geo.n, 2)), True)
    u_bad = u_v.copy()
    u_bad[3, 0] = np.nan
    res = LM.update(geo, s_lm, s_mm, u_bad, 0.05, first["F"], False)
    assert res["status"][3] == 2 and np.isnan(res["F"][3]).all() and np.isnan(res["cs2v"][3])
    assert np.isfinite(np.delete(res["F"], 3, axis=0)).all() and (np.delete(res["status"], 3) != 2).all()
    assert np.isnan(LM.nanmax(np.array([np.nan]), np.array([1.0])))[0] and np.isnan(LM.nanmax(np.array([1.0]), np.array([np.nan])))[0]
    assert LM.clip(np.array([1.0, -1.0, 1.0, 1.0]), np.array([2.0, 2.0, 0.0, 4.0]), 0.3).tolist() == [0.3, 0.0, 0.0, 0.25]


def test_first_update_relaxation_and_floor():
    """The first update is F_MM = s_MM, F_LM = cs2_initial s_MM; later F stays between the source and the interpolant
    (0 <= eps < 1), and F_LM >= cs2_floor F_MM where the sources push it below."""
    F, u, geo = _setup(2, 6, 1)
    s_lm, s_mm, u_v = LM.sources(F, u, geo.P)
    first = LM.update(geo, s_lm, s_mm, u_v, 0.1, np.zeros((geo.n, 2)), True)
    assert np.array_equal(first["F"][:, 1], s_mm) and np.array_equal(first["F"][:, 0], 0.0256 * s_mm)
    assert (first["status"] == 0).all() and np.abs(first["cs2v"] - 0.0256).max() <= 1e-15
    res = LM.update(geo, -np.abs(s_lm) - 1.0, s_mm, u_v, 50.0, first["F"], False, cs2_floor=1e-3)
    assert (res["eps"] > 0.5).all() and (res["eps"] < 1.0).all()
    assert np.array_equal(res["F"][:, 0], 1e-3 * res["F"][:, 1]) and np.abs(res["cs2v"] - 1e-3).max() <= 1e-15


# ---- the conditions on the inputs of the GPU tests ---------------------------------------------------------------------
def _run_conditions(mesh, deg, field_fn, dt_of, label, walled):
    from oracle import ipcs_oracle as O

    geo, vt = LM.mesh_geometry(mesh, tol=TOL)
    F = O.Forms(mesh.coords.cpu().numpy(), mesh.cells.cpu().numpy().astype(np.int64), deg, 2 if deg == 3 else 1)
    u = field_fn(F.x_v)
    dt = dt_of(geo, LM.sources(F, u, geo.P)[2])
    m = LM.Lagrangian(geo)
    boundary = _boundary_vertices(geo)
    if vt is not None:  # a class is on the boundary when one of its images is, identified faces apart
        on = np.zeros(geo.n, dtype=bool)
        x = geo.coords
        walls = np.zeros(geo.coords.shape[0], dtype=bool)
        for k in range(geo.d):
            if k not in geo.periodic[0]:
                walls |= np.isclose(x[:, k], x[:, k].min()) | np.isclose(x[:, k], x[:, k].max())
        np.logical_or.at(on, vt, walls)
        boundary = on
    for k in range(3):
        m.evaluate(F, u, dt)
        r = m.res
        if k == 0:
            continue
        exits = r["status"] == 1
        print(f"{label} update {k}: status {np.bincount(r['status'], minlength=3).tolist()}, min |min lambda| "
              f"{np.nanmin(np.abs(r['minlam'])):.2e}, near the floor {LM.near_floor(r, 1e-24).mean():.3f}, Cs2_v > 0 "
              f"{(r['cs2v'] > 0).mean():.2f}")
        assert (r["status"] != 2).all()
        if walled:
            assert (np.sqrt((LM.sources(F, u, geo.P)[2] ** 2).sum(axis=1)) * dt).max() < 0.5 * geo.altitude.min()
            assert not (exits & ~boundary).any(), label
        else:
            assert not exits.any(), label
        ml = r["minlam"]
        assert np.isfinite(ml).all()
        assert (np.abs(ml) > 1e-10).all() and (np.abs(ml + TOL) > 1e-10).all(), (label, ml[np.abs(ml) <= 1e-10])
        assert LM.near_floor(r, 1e-24).mean() <= 0.05, label
        assert np.isfinite(r["F"]).all() and (r["F"][:, 1] > 0.0).all()


@pytest.mark.parametrize("kind", ["lattice", "delaunay"])
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_walled_inputs_of_the_gpu_tests(dim, N, deg, kind):
    """With max |u_v| h below half the smallest cell altitude every status-1 vertex is a boundary vertex; no departure
    point has a deciding barycentric coordinate within 1e-10 of 0 or of -tol; at most 5 % of the vertices sit on the
    floor's edge."""
    mesh = _ox_mesh(dim, N, kind)
    _run_conditions(mesh, deg, lambda x: LM.input_field(x, dim), LM.walled_dt, f"{kind} ({dim},{N},{deg})", True)


@pytest.mark.parametrize("dim,N,axes", PERIODIC)
@pytest.mark.parametrize("deg", [1, 2])
def test_periodic_inputs_of_the_gpu_tests(dim, N, axes, deg):
    """Fully periodic: no vertex has status 1 (at a step that carries points across the seam); the channel periodic in x:
    only wall vertices leave."""
    mesh = _periodic_mesh(dim, N, axes)
    full = len(axes) == dim
    fld = LM.periodic_field if full else LM.channel_field
    dt_of = (lambda geo, u_v: 0.3) if full else LM.walled_dt
    _run_conditions(mesh, deg, lambda x: fld(x, dim), dt_of, f"periodic {axes} ({dim},{N},{deg})", not full)
    if full:  # the seam is crossed: some departure point was folded
        geo, _ = LM.mesh_geometry(mesh)
        from oracle import ipcs_oracle as O

        F = O.Forms(mesh.coords.cpu().numpy(), mesh.cells.cpu().numpy().astype(np.int64), deg, 1)
        u_v = LM.sources(F, fld(F.x_v, dim), geo.P)[2]
        raw = geo.x_v - 0.3 * u_v
        assert (raw < -1.0).any() and (geo.fold(raw) >= -1.0).all() and (geo.fold(raw) < 1.0).all()
