"""GPU: scalars that drive the flow (ScalarTransport(buoyancy=...), csrc/ox_scalar.hip: ox_buoyancy_rows) and the scalar
flux through walls (ScalarFlux, ox_scalar_flux) against the numpy model of tests/buoyancy_model.py, which is built on
the oracle's fractional step and forms and pinned by tests/test_buoyancy_host.py.  The model is fed the device's own
numbering: fields compare index by index."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_scalar import _c, _dofs, _forms, _options, left

pytestmark = pytest.mark.gpu

TIGHT = {"ksp_type": "bcgs", "pc_type": "jacobi", "ksp_rtol": 1e-12, "ksp_atol": 1e-30}


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def _solver(dim, N, deg, scalars, nu=0.01, dt=0.005, solver_options=None, options=None, body_force=None, mesh=None):
    """The Taylor-Green set-up of tests.helpers.make_hip_problem with ``scalars=`` and ``body_force=``."""
    import oasisx_amd as ox
    from oracle import ipcs_oracle as O
    from tests.helpers import on_boundary, on_boundary3, tg_mesh

    mesh = tg_mesh(dim, N) if mesh is None else mesh
    clock = {"t": 0.0}
    marker = on_boundary if dim == 2 else on_boundary3
    fns = [O.tg_u, O.tg_v, O.tg_w][:dim]
    bcs_u = [[ox.DirichletBC(lambda x, f=f: f(x, clock["t"], nu), ox.LocatorMethod.GEOMETRICAL, marker)] for f in fns]
    opts = {"sell_window": 256, "low_memory_version": True}
    opts.update(options or {})
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", deg), ("Lagrange", 2 if deg == 3 else 1), bcs_u=bcs_u, bcs_p=[],
                                solver_options=solver_options or _options(), options=opts, scalars=scalars,
                                body_force=body_force)
    for i, f in enumerate(fns):
        S._u2[i].interpolate(lambda x, f=f: f(x, -dt, nu))
        S._u1[i].interpolate(lambda x, f=f: f(x, 0.0, nu))
    S._p.interpolate(lambda x: O.tg_p(x, -dt / 2.0, nu))
    return S, clock, mesh


def _advance(S, clock, dt, nu):
    clock["t"] += dt
    S.solve(dt, nu, max_iter=1)


def _update_bcs(S):
    for bcl in S._bcs_u:
        for bc in bcl:
            bc.update_bc()
    for g in S._scalar_groups:
        for m in g.members:
            for bc in m.bcs:
                bc.update_bc()


# ---- 1. the kernel against the model, row by row -------------------------------------------------------------------------
def _mass_matrix(kind, dim, N, deg, freeze):
    """(M on the device, the oracle's forms in the device's numbering, n rows) of one space -- no solver."""
    from oasisx_amd import _lib, fem
    from oasisx_amd import mesh as M
    from oasisx_amd.la import SellMatrix, assemble_matrix
    from oracle import ipcs_oracle as O
    from tests import hard_meshes as H
    from tests.helpers import tg_mesh

    if kind == "lattice":
        mesh = tg_mesh(dim, N)
    elif kind == "delaunay":
        mesh = M.create_delaunay_box(None, [[-1.0] * dim, [1.0] * dim], N, seed=2)
    else:  # the centre row of a fan of 37 triangles: a row far wider than its slice's others
        mesh = M.from_arrays(*H.fan(37, 3.0, 1.0))
    Vi = fem.FunctionSpace(mesh, deg, window=256)
    geom = Vi.native.nmesh.geom if getattr(Vi, "native", None) is not None else fem.cell_geometry(mesh, Vi.local_cells)
    cells = _lib.ox_cells(mesh.gdim, 0, int(geom.shape[0]), geom.data_ptr())
    Mat = SellMatrix(Vi.pattern, symmetric=True, name="M")
    assemble_matrix(0, Vi, cells, Mat)
    if freeze:
        Mat.freeze()
    F = O.Forms(mesh.coords.cpu().numpy(), Vi.cells_in_kernel_order(), deg, 1, vd=Vi.cell_dofs.cpu().numpy(),
                nv_dofs=Vi.num_dofs)
    return Mat, F, Vi.n_local, geom


CASES = [("lattice", 2, 4, 1), ("lattice", 2, 4, 2), ("lattice", 2, 4, 3), ("lattice", 3, 3, 1), ("lattice", 3, 3, 2),
         ("lattice", 3, 3, 3), ("delaunay", 2, 6, 2), ("delaunay", 3, 4, 1), ("fan", 2, 0, 2)]


@pytest.mark.parametrize("freeze", [True, False])
@pytest.mark.parametrize("kind,dim,N,deg", CASES)
def test_kernel_matches_the_model_row_by_row(hip, kind, dim, N, deg, freeze):
    """b after ox_buoyancy_rows onto a nonzero b equals b + sum coef (M d) of the model to 1e-12 max|.|: 1, 2 and 3 terms,
    two terms from different groups (different nc, col), a term without a second level; components whose coefficients
    are all zero come back bit for bit; the dictionary instantiation runs exactly where M carries value codes."""
    import torch

    from oasisx_amd import _lib
    from tests.buoyancy_model import buoyancy_rows

    Mat, F, n, keep = _mass_matrix(kind, dim, N, deg, freeze)
    if not freeze:
        assert Mat.vcode is None
    elif kind == "lattice" and dim == 2:
        assert Mat.vcode is not None  # (elsewhere M may exceed 256 distinct values: then f64 is read)
    Mref = F.mass_v()
    gen = torch.Generator(device="cpu").manual_seed(7)
    blocks = {nc: (torch.randn(n, nc, generator=gen, dtype=torch.float64).cuda(),
                   torch.randn(n, nc, generator=gen, dtype=torch.float64).cuda()) for nc in (1, 2, 3)}
    b0 = torch.randn(n, dim, generator=gen, dtype=torch.float64).cuda()
    z = [0.0] * dim
    up = z[:-1] + [2.5]
    full = [0.7, -1.1, 0.4][:dim]
    first = [1.5] + z[1:]
    # (nc, col, second level?, reference, coefficients)
    term_sets = {"one": [(1, 0, True, 0.25, up)],
                 "two": [(2, 0, True, 0.0, up), (2, 1, True, -0.5, full)],
                 "three": [(3, 2, True, 0.1, full), (3, 0, True, 0.2, up), (3, 1, True, 0.3, first)],
                 "two groups": [(3, 1, True, 0.5, up), (2, 1, True, 0.0, up)],
                 "no second level": [(2, 1, False, 0.75, up), (1, 0, True, 0.0, up)]}
    for name, spec in term_sets.items():
        arr = (_lib.ox_buoy_term * len(spec))()
        model_terms = []
        for t, (nc, col, second, ref, coef) in zip(arr, spec):
            c1, c2 = blocks[nc]
            t.c1, t.c2 = c1.data_ptr(), (c2.data_ptr() if second else None)
            t.nc, t.col, t.ref = nc, col, ref
            for i in range(3):
                t.coef[i] = coef[i] if i < dim else 0.0
            model_terms.append((c1[:, col].cpu().numpy(), c2[:, col].cpu().numpy() if second else None, ref, coef))
        b = b0.clone()
        _lib.check(hip.ox_profile_begin(16, 1), "ox_profile_begin")
        _lib.check(hip.ox_buoyancy_rows(Mat.ref(), dim, len(spec), arr, _lib.ptr(b), _lib.current_stream()),
                   "ox_buoyancy_rows")
        _lib.check(hip.ox_profile_end(), "ox_profile_end")
        ran = {}
        for dict_ in (0, 1):
            cnt = C.c_longlong(0)
            _lib.check(hip.ox_profile_get(_lib.PROF_TAG_BUOYANCY_ROWS, 2 * len(spec) + dict_, C.byref(cnt), None),
                       "ox_profile_get")
            ran[dict_] = cnt.value
        assert ran == ({0: 0, 1: 1} if Mat.vcode is not None else {0: 1, 1: 0}), (name, ran)
        ref_b = buoyancy_rows(Mref, b0.cpu().numpy(), model_terms)
        err = np.abs(b.cpu().numpy() - ref_b).max()
        print(f"{kind} {dim}-D P{deg} freeze={freeze} {name}: err = {err:.3e}, max|b| = {np.abs(ref_b).max():.3e}")
        assert err <= 1e-12 * np.abs(ref_b).max(), (name, err)
        dead = [i for i in range(dim) if all(s[4][i] == 0.0 for s in spec)]
        assert dead or name in ("two", "three")
        for i in dead:
            assert torch.equal(b[:, i], b0[:, i]), (name, i)
        b2 = b0.clone()
        _lib.check(hip.ox_buoyancy_rows(Mat.ref(), dim, len(spec), arr, _lib.ptr(b2), _lib.current_stream()),
                   "ox_buoyancy_rows")
        assert torch.equal(b, b2)  # fixed order, no atomics


def test_kernel_refuses_bad_arguments(hip):
    from oasisx_amd import _lib

    Mat, F, n, keep = _mass_matrix("lattice", 2, 2, 1, False)
    import torch

    c = torch.zeros(n, 1, dtype=torch.float64, device="cuda")
    b = torch.zeros(n, 2, dtype=torch.float64, device="cuda")
    arr = (_lib.ox_buoy_term * 1)()
    arr[0].c1, arr[0].nc, arr[0].col = c.data_ptr(), 1, 0
    st = _lib.current_stream()
    assert hip.ox_buoyancy_rows(Mat.ref(), 2, 0, arr, _lib.ptr(b), st) != 0
    assert hip.ox_buoyancy_rows(Mat.ref(), 2, 4, arr, _lib.ptr(b), st) != 0
    assert hip.ox_buoyancy_rows(Mat.ref(), 4, 1, arr, _lib.ptr(b), st) != 0
    arr[0].col = 1
    assert hip.ox_buoyancy_rows(Mat.ref(), 2, 1, arr, _lib.ptr(b), st) != 0
    arr[0].col, arr[0].c1 = 0, None
    assert hip.ox_buoyancy_rows(Mat.ref(), 2, 1, arr, _lib.ptr(b), st) != 0


# ---- 2. exact zero -------------------------------------------------------------------------------------------------------
def test_scalar_at_its_reference_forces_nothing(hip):
    """initial == reference: d = 0 in every entry, so after the first solve u and p equal the uncoupled solver's bit for
    bit."""
    import torch

    import oasisx_amd as ox

    nu, dt = 0.01, 0.005
    out = []
    for b in (None, (3.0, -40.0)):
        sc = ox.ScalarTransport("T", diffusivity=0.05, initial=0.3, reference=0.3, buoyancy=b)
        S, clock, _ = _solver(2, 8, 2, [sc], nu=nu, dt=dt, solver_options=_options(guess=True))
        _advance(S, clock, dt, nu)
        out.append((S._U.rdev().clone(), S._P.rdev().clone()))
        assert ("buoyancy_assemble" in S.timings) is False
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_component_with_zero_coefficient_is_untouched(hip):
    """buoyancy=(0, b) with a non-trivial scalar: b_first[:, 0] after assemble_first equals the uncoupled solver's bit for
    bit, b_first[:, 1] does not."""
    import torch

    import oasisx_amd as ox

    nu, dt = 0.01, 0.005
    out = []
    for b in (None, (0.0, 7.0)):
        sc = ox.ScalarTransport("T", diffusivity=0.05, initial=lambda x: np.cos(2.0 * x[0]) + 0.5 * x[1], buoyancy=b)
        S, clock, _ = _solver(2, 8, 2, [sc], nu=nu, dt=dt)
        clock["t"] = dt
        _update_bcs(S)
        S.assemble_first(dt, nu)
        out.append(S._BFIRST.rdev().clone())
    assert torch.equal(out[0][:, 0], out[1][:, 0])
    assert not torch.equal(out[0][:, 1], out[1][:, 1])


# ---- 3. a constant scalar is a constant body force ---------------------------------------------------------------------------
def test_constant_scalar_equals_a_constant_body_force(hip):
    """c = c0 everywhere, no Dirichlet rows: the force b (c0 - reference) M 1 and the body force b (c0 - reference) int phi
    differ only in rounding; u and p agree to 1e-8 relative over three steps."""
    import oasisx_amd as ox

    nu, dt, c0, ref, b = 0.01, 0.005, 1.75, 0.5, 3.0
    so = _options(guess=True)
    sc = ox.ScalarTransport("T", diffusivity=0.05, initial=c0, reference=ref, buoyancy=(0.0, b))
    S, clock, _ = _solver(2, 8, 2, [sc], nu=nu, dt=dt, solver_options=so)
    R, rclock, _ = _solver(2, 8, 2, None, nu=nu, dt=dt, solver_options=so, body_force=(0.0, b * (c0 - ref)))
    for k in range(3):
        _advance(S, clock, dt, nu)
        _advance(R, rclock, dt, nu)
        du, dp = _rel(S._U.rhost(), R._U.rhost()), _rel(S._P.rhost(), R._P.rhost())
        print(f"step {k}: rel diff u {du:.3e}, p {dp:.3e}, max |c - c0| = {np.abs(_c(S, 'T') - c0).max():.3e}")
        assert du < 1e-8 and dp < 1e-8, (k, du, dp)


# ---- 4. steps against the model --------------------------------------------------------------------------------------------
def _coupled_twin(S, mesh, dim, deg, nu, dt, so, scalar_specs):
    """The oracle on the device's numbering with the coupled scalars of ``scalar_specs``:
    (kappa, Dirichlet marker or None, value, initial, source, buoyancy, reference, extrapolate)."""
    from tests.buoyancy_model import CoupledScalar, CoupledStep
    from tests.helpers import make_oracle_twin
    from tests.scalar_model import ScalarModel

    R, rclock = make_oracle_twin(S, mesh, dim, deg, nu, dt, solver_options=so)
    F, x_v = R.F, R.x_v
    scalars = []
    for kappa, marker, value, initial, source, b, ref, ex in scalar_specs:
        m = ScalarModel(F, x_v, kappa, dofs=None if marker is None else _dofs(x_v, marker), value=value, source=source,
                        options=so["scalar_transport"], M=R.M, K=R.K)
        cs = CoupledScalar(m, buoyancy=b, reference=ref, extrapolate=ex)
        cs.interpolate(initial)
        scalars.append(cs)
    return CoupledStep(R, scalars), rclock


@pytest.mark.parametrize("extrapolate", [True, False])
@pytest.mark.parametrize("dim,N,deg", [(2, 8, 2), (3, 3, 1)])
def test_steps_match_the_model(hip, dim, N, deg, extrapolate):
    """3 steps with Taylor-Green velocity data and a non-constant scalar with Dirichlet rows on part of the boundary: u, p
    and c within 1e-8 relative of the model, the scalar's iteration counts within +-1 of the model's."""
    import oasisx_amd as ox

    nu, dt, kappa = 0.01, 0.005, 0.03
    clock_c = {"t": 0.0}
    src = lambda x: 0.5 + x[0]  # noqa: E731
    val = lambda x: 1.0 + x[1] * (1.0 + clock_c["t"])  # noqa: E731
    ini = lambda x: np.cos(np.pi * x[0]) * np.cos(np.pi * x[1])  # noqa: E731
    b = [0.5, -2.0, 0.7][:dim]
    sc = ox.ScalarTransport("T", diffusivity=kappa, source=src, initial=ini, buoyancy=b, reference=0.2,
                            extrapolate=extrapolate, bcs=[ox.DirichletBC(val, ox.LocatorMethod.GEOMETRICAL, left)])
    so = _options()
    S, clock, mesh = _solver(dim, N, deg, [sc], nu=nu, dt=dt, solver_options=so)
    assert (S._scalar_groups[0].C2 is not None) == extrapolate
    twin, rclock = _coupled_twin(S, mesh, dim, deg, nu, dt, so, [(kappa, left, val, ini, src, b, 0.2, extrapolate)])
    T = twin.scalars[0]
    for k in range(3):
        clock_c["t"] = rclock["t"] = (k + 1) * dt
        _advance(S, clock, dt, nu)
        twin.solve(dt, nu)
        c = _c(S, "T")
        du, dp, dc = _rel(S._U.rhost(), twin.S.u1), _rel(S._P.rhost()[:, 0], twin.S.p), _rel(c, T.m.c)
        its = S.iteration_counts()["scalar_transport"]["T"]
        print(f"step {k}: rel diff u {du:.3e}, p {dp:.3e}, c {dc:.3e}; scalar iterations {its} (model {T.m.its})")
        assert T.m.reason > 0
        assert du < 1e-8 and dp < 1e-8 and dc < 1e-8, (k, du, dp, dc)
        assert abs(its - T.m.its) <= 1, (k, its, T.m.its)
        assert np.array_equal(c, _c(S, "T", 1))  # c_1 <- c
        if extrapolate:
            assert _rel(_c(S, "T", 2), T.c2) < 1e-8  # c_2 <- c_1


# ---- 5. the heated cavity on the device ------------------------------------------------------------------------------------
def test_heated_cavity_on_the_device(hip):
    """N = 8, dt = 0.01, 60 steps, Krylov rtol 1e-12: the wall Nusselt numbers from ScalarFlux.totals() lie within 1 % of
    the benchmark's 1.118, hot equals minus cold to 1e-3, and both equal the model's (same Krylov options, the device's
    numbering) to 1e-6 relative."""
    from demo.heated_cavity_hip import build_cavity, nusselt
    from tests.buoyancy_model import BENCHMARK, HeatedCavity

    so = {k: dict(v, ksp_rtol=1e-12) for k, v in _options(TIGHT).items()}
    mesh, tags, S, flux = build_cavity(8, solver_options=so)
    F, x_v = _forms(S, mesh)
    H = HeatedCavity(solver_options=so, scalar_options=so["scalar_transport"], forms=F, x_v=x_v, x_q=S._Q.x.cpu().numpy())
    dt = 0.01
    for n in range(60):
        S.solve(dt, 0.71, max_iter=1)
        H.solve(dt)
    flux.sample(60 * dt, 0.71)
    hot, cold = nusselt(flux)
    m_hot, m_cold, _ = H.wall_totals()
    m_hot = -m_hot
    ref = BENCHMARK["Nu"]
    d_hot, d_cold = abs(hot - m_hot) / m_hot, abs(cold - m_cold) / m_cold
    print(f"device: hot {hot:.8f}, cold {cold:.8f}; model: hot {m_hot:.8f}, cold {m_cold:.8f}; "
          f"rel diff {d_hot:.3e}, {d_cold:.3e}; rel diff u {_rel(S._U.rhost(), H.step.S.u1):.3e}")
    assert abs(hot - ref) <= 0.01 * ref and abs(cold - ref) <= 0.01 * ref
    assert abs(hot - cold) <= 1e-3 * cold
    assert d_hot <= 1e-6 and d_cold <= 1e-6


# ---- 6. the facet flux against the numpy facet model -------------------------------------------------------------------------
def _flux_problem(dim, N, deg, nu=0.4):
    """A solver with two scalars in one group (the flux reads column 1 of an nc = 2 block), a Schmidt number, and the
    exterior facets in two tags: the wall x = -1 and the rest."""
    import oasisx_amd as ox
    from oasisx_amd import mesh as M
    from tests.helpers import tg_mesh

    mesh = tg_mesh(dim, N)
    scalars = [ox.ScalarTransport("a", schmidt=2.0, initial=1.0), ox.ScalarTransport("T", schmidt=2.0)]
    S, clock, mesh = _solver(dim, N, deg, scalars, mesh=mesh)
    wall = M.locate_entities_boundary(mesh, dim - 1, lambda x: np.isclose(x[0], -1.0))
    ext = np.asarray(mesh.exterior_facets())
    rest = np.setdiff1d(ext, wall)
    facets = np.hstack([wall, rest])
    values = np.hstack([np.full_like(wall, 5), np.full_like(rest, 9)]).astype(np.int32)
    srt = np.argsort(facets)
    tags = M.meshtags(mesh, dim - 1, facets[srt], values[srt])
    flux = ox.ScalarFlux(S, "T", facets=(tags, (9, 5)), capacity=1)
    return S, clock, mesh, flux


@pytest.mark.parametrize("dim,N,deg", [(2, 4, 1), (2, 4, 2), (2, 4, 3), (3, 3, 1), (3, 3, 2), (3, 3, 3)])
def test_flux_matches_the_facet_model(hip, dim, N, deg):
    """q, |f| q and the facet mean of c per facet against the numpy facet model to 1e-12 max|.|; a linear field gives
    q = -kappa a . n to 1e-13 relative; the per-tag totals are the sums of the facet values; two weighted samples give
    the weighted mean."""
    from tests.buoyancy_model import facet_flux

    nu = 0.4
    S, clock, mesh, flux = _flux_problem(dim, N, deg, nu)
    kappa = nu / 2.0
    assert flux.n_tags == 2 and list(flux.tags) == [9, 5] and flux.n_facets == len(mesh.exterior_facets())
    F, x_v = _forms(S, mesh)
    fc = S._Vi[0][0].kernel_cell_index(flux.cells)
    fa = flux.local_facets
    f1 = lambda x: np.cos(2.0 * x[0]) + 0.5 * x[1] + x[0] * x[1] + (x[2] ** 2 if dim == 3 else 0.0)  # noqa: E731
    S.scalar("T").interpolate(f1)
    flux.sample(0.0, nu, dt=0.5)
    q, area, cbar, n = facet_flux(F, fc, fa, _c(S, "T"), kappa)
    dq, dfq, dcb = (np.abs(flux.flux().cpu().numpy() - q).max(), np.abs(flux._fq.cpu().numpy() - area * q).max(),
                    np.abs(flux.facet_mean().cpu().numpy() - cbar).max())
    print(f"{dim}-D P{deg}: dq = {dq:.3e} (max {np.abs(q).max():.3e}), dfq = {dfq:.3e}, dcbar = {dcb:.3e}")
    assert dq <= 1e-12 * np.abs(q).max() and dfq <= 1e-12 * np.abs(area * q).max() and dcb <= 1e-12 * np.abs(cbar).max()
    assert np.abs(flux.normals - n).max() < 1e-13 and np.abs(flux.areas - area).max() < 1e-13
    tot = flux.totals()
    for k, tag in enumerate(flux.tags):
        ref = (area * q)[flux.facet_tags == tag].sum()
        assert abs(tot[k] - ref) <= 1e-12 * np.abs(area * q).sum(), (tag, tot[k], ref)
    # a linear field, and the second weighted sample (the ring of capacity 1 doubles)
    a = np.array([0.7, -1.3, 0.4])[:dim]
    S.scalar("T").interpolate(lambda x: sum(a[i] * x[i] for i in range(dim)))
    flux.sample(0.1, nu, dt=0.25)
    q2 = flux.flux().cpu().numpy()
    exact = -kappa * (flux.normals @ a)
    print(f"linear field: max |q + kappa a.n| = {np.abs(q2 - exact).max():.3e}")
    assert np.abs(q2 - exact).max() <= 1e-13 * np.abs(exact).max()
    assert abs(flux.totals().sum()) <= 1e-12 * np.abs(flux.areas * exact).sum()  # a closed surface
    mean = (0.5 * q + 0.25 * exact) / 0.75
    assert flux.total_weight == 0.75 and flux.n_samples == 2 and flux.history().shape == (2, 2)
    assert np.abs(flux.mean_flux().cpu().numpy() - mean).max() <= 1e-12 * np.abs(mean).max()
    assert np.allclose(flux.history()[0], tot, rtol=0, atol=0)
    flux.reset_statistics()
    with pytest.raises(RuntimeError):
        flux.mean_flux()


def test_sampling_changes_nothing_and_save(hip, tmp_path):
    """u, p and c after sample + solve equal solve alone bit for bit; save() writes the .npz and the facets' .vtu."""
    import torch

    import oasisx_amd as ox
    from oasisx_amd import io

    nu, dt = 0.01, 0.005
    out = []
    for sample in (False, True):
        sc = ox.ScalarTransport("T", diffusivity=0.05, initial=lambda x: np.cos(2.0 * x[0]) + 0.5 * x[1], buoyancy=(0.0, 2.0),
                                bcs=[ox.DirichletBC(1.0, ox.LocatorMethod.GEOMETRICAL, left)])
        S, clock, mesh = _solver(2, 8, 2, [sc], nu=nu, dt=dt, solver_options=_options(guess=True))
        flux = ox.ScalarFlux(S, "T")
        for _ in range(2):
            if sample:
                flux.sample(clock["t"], nu, dt=dt)
            _advance(S, clock, dt, nu)
        out.append((S._U.rdev().clone(), S._P.rdev().clone(), S._scalar_groups[0].C.rdev().clone()))
    for x, y in zip(*out):
        assert torch.equal(x, y)
    flux.save(tmp_path / "flux.npz", vtu=tmp_path / "flux.vtu", time=clock["t"])
    z = np.load(tmp_path / "flux.npz")
    assert z["history"].shape == (2, 1) and z["flux"].shape == (flux.n_facets,) and "mean_flux" in z
    back = io.read_vtu(tmp_path / "flux.vtu")
    assert np.allclose(back["cell_data"]["flux"], z["flux"])
    with pytest.raises(KeyError):
        ox.ScalarFlux(S, "nope")
    with pytest.raises(ValueError):
        ox.ScalarFlux(S, "T", capacity=0)
    interior = np.setdiff1d(np.arange(mesh._entities(1)[0].shape[0]), mesh.exterior_facets())[:1]
    with pytest.raises(ValueError, match="interior"):
        ox.ScalarFlux(S, "T", facets=interior)


# ---- 7. repeat and surface ---------------------------------------------------------------------------------------------------
def _coupled_run(steps=3):
    import oasisx_amd as ox

    nu, dt = 0.01, 0.005
    G = ox.LocatorMethod.GEOMETRICAL
    ini = lambda x: np.cos(np.pi * x[0]) * np.cos(np.pi * x[1])  # noqa: E731
    scalars = [ox.ScalarTransport("a", diffusivity=0.03, initial=ini, source=0.2, buoyancy=(0.0, 0.0, 4.0),
                                  bcs=[ox.DirichletBC(1.0, G, left)]),
               ox.ScalarTransport("b", diffusivity=0.03, initial=0.5, bcs=[ox.DirichletBC(2.0, G, left)]),
               ox.ScalarTransport("s", schmidt=3.0, initial=ini, buoyancy=(1.0, 0.0, -2.0), reference=0.1, extrapolate=False)]
    S, clock, _ = _solver(3, 3, 2, scalars, nu=nu, dt=dt, solver_options=_options(TIGHT, guess=True))
    for _ in range(steps):
        _advance(S, clock, dt, nu)
    return S


def test_two_runs_are_bit_identical(hip):
    import torch

    S0, S1 = _coupled_run(), _coupled_run()
    assert len(S0._buoyancy) == 1 and len(S0._buoyancy[0][0]) == 2  # two coupled scalars of two groups, one launch
    assert torch.equal(S0._U.rdev(), S1._U.rdev()) and torch.equal(S0._P.rdev(), S1._P.rdev())
    for name in "abs":
        assert np.array_equal(_c(S0, name), _c(S1, name))
    assert np.array_equal(_c(S0, "a", 2), _c(S1, "a", 2))


def test_second_level_and_surface(hip):
    """scalar(name, level=2): data written there is used by the first step; it raises for a scalar that keeps no second
    level.  The construction errors; buoyancy_assemble outside assemble_first; no timings key without coupling."""
    import oasisx_amd as ox
    from tests.buoyancy_model import buoyancy_rows

    nu, dt, b, ref = 0.01, 0.005, (0.0, 6.0), 0.25
    ini = lambda x: np.cos(2.0 * x[0]) + 0.5 * x[1]  # noqa: E731
    old = lambda x: np.sin(x[0]) - x[1] ** 2  # noqa: E731
    first = {}
    for name, coupled in (("plain", False), ("coupled", True)):
        scalars = [ox.ScalarTransport("T", diffusivity=0.05, initial=ini, buoyancy=b if coupled else None, reference=ref),
                   ox.ScalarTransport("p", diffusivity=0.2, initial=1.0)]
        S, clock, mesh = _solver(2, 4, 2, scalars, nu=nu, dt=dt)
        if coupled:
            assert np.array_equal(_c(S, "T", 2), _c(S, "T", 1))  # set_initial fills c_2 from c_1
            S.scalar("T", level=2).interpolate(old)
        clock["t"] = dt
        _update_bcs(S)
        S.assemble_first(dt, nu)
        first[name] = S._BFIRST.rhost()
    F, x_v = _forms(S, mesh)
    ref_b = buoyancy_rows(F.mass_v(), first["plain"], [(_c(S, "T", 1), _c(S, "T", 2), ref, b)])
    assert np.abs(_c(S, "T", 2) - _c(S, "T", 1)).max() > 0.1
    assert np.abs(first["coupled"] - ref_b).max() <= 1e-12 * np.abs(ref_b).max()
    with pytest.raises(ValueError, match="second time level"):
        S.scalar("p", level=2)
    with pytest.raises(ValueError):
        S.scalar("T", level=3)
    with pytest.raises(RuntimeError, match="inside assemble_first"):
        S.buoyancy_assemble()
    assert "buoyancy_assemble" not in S.timings
    P, _, _ = _solver(2, 4, 2, [ox.ScalarTransport("T", diffusivity=0.05)], nu=nu, dt=dt)
    assert P._buoyancy == [] and P._scalar_groups[0].C2 is None and "buoyancy_assemble" not in P.timings
    with pytest.raises(RuntimeError, match="inside assemble_first"):
        P.buoyancy_assemble()
    with pytest.raises(ValueError, match="buoyancy has 3 entries"):
        _solver(2, 4, 2, [ox.ScalarTransport("T", diffusivity=0.05, buoyancy=(0.0, 0.0, 1.0))])
    with pytest.raises(ValueError, match="buoyancy has 2 entries"):
        _solver(3, 3, 1, [ox.ScalarTransport("T", diffusivity=0.05, buoyancy=(0.0, 1.0))])
    with pytest.raises(ValueError, match="buoyancy"):
        ox.ScalarTransport("T", diffusivity=0.05, buoyancy=(0.0, float("inf")))
    with pytest.raises(ValueError, match="reference"):
        ox.ScalarTransport("T", diffusivity=0.05, buoyancy=(0.0, 1.0), reference=float("nan"))


def test_an_uncoupled_solver_makes_no_new_call(hip, monkeypatch):
    """Passive scalars: assemble_first and solve call neither ox_buoyancy_rows nor ox_scalar_flux; one coupled scalar: one
    ox_buoyancy_rows per assemble_first."""
    import oasisx_amd as ox
    from oasisx_amd import _lib

    class Counting:
        def __init__(self, lib):
            self._lib, self.calls = lib, []

        def __getattr__(self, name):
            if name in ("ox_buoyancy_rows", "ox_scalar_flux"):
                self.calls.append(name)
            return getattr(self._lib, name)

    nu, dt = 0.01, 0.005
    for b, want in ((None, []), ((0.0, 1.0), ["ox_buoyancy_rows"] * 2)):
        S, clock, _ = _solver(2, 4, 2, [ox.ScalarTransport("T", diffusivity=0.05, initial=1.0, buoyancy=b)], nu=nu, dt=dt)
        proxy = Counting(_lib.load())
        monkeypatch.setattr(_lib, "_lib", proxy)
        monkeypatch.setattr(S, "_lib", proxy)
        _advance(S, clock, dt, nu)
        _advance(S, clock, dt, nu)
        monkeypatch.undo()
        assert proxy.calls == want, (b, proxy.calls)
