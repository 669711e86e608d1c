"""GPU: the dynamic Smagorinsky model (oasisx_amd.DynamicSmagorinsky, oasisx_amd.PatchFilter, csrc/ox_dynamic.hip) against
the numpy model of tests/dynamic_model.py, which is built on the oracle's forms and pinned by
tests/test_dynamic_host.py.  The model is fed the device's numbering (cell order, dof tables, vertex classes) and the
device's own u_ab block, so every stage compares index by index."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [(2, 6, 1), (2, 5, 2), (3, 3, 1), (3, 3, 2), (2, 4, 3), (3, 2, 3)]
EDGES = [-1.0, -0.3, 0.4, 1.0]  # slabs along axis 1 of a Delaunay mesh, by centroid
TINY = np.finfo(np.float64).tiny


def _problem(dim, N, deg, model, field=None, nu=0.01, dt=0.005, solver_options=None, options=None, mesh=None,
             low_memory=True, **kw):
    """The Taylor-Green set-up of tests/test_gpu_viscosity.py with ``viscosity_model=``; ``field``: a name of
    tests.dynamic_model.field interpolated into both velocity levels, and held on the boundary, instead of Taylor-Green."""
    import oasisx_amd as ox
    from oracle import ipcs_oracle as O
    from tests import dynamic_model as DM
    from tests.helpers import KRYLOV, on_boundary, on_boundary3, tg_mesh

    mesh = tg_mesh(dim, N) if mesh is None else mesh
    clock = {"t": 0.0}
    marker = on_boundary if dim == 2 else on_boundary3
    fns = [O.tg_u, O.tg_v, O.tg_w][:dim]
    if field is None:
        bcs_u = [[ox.DirichletBC(lambda x, f=f: f(x, clock["t"], nu), ox.LocatorMethod.GEOMETRICAL, marker)] for f in fns]
    else:  # the field's own (steady) boundary values
        bcs_u = [[ox.DirichletBC(lambda x, i=i: DM.field(field, np.asarray(x)[:dim].T, dim)[:, i],
                                 ox.LocatorMethod.GEOMETRICAL, marker)] for i in range(dim)]
    opts = {"sell_window": 256, "low_memory_version": low_memory}
    opts.update(options or {})
    if model is not None:
        kw["viscosity_model"] = model
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", deg), ("Lagrange", 2 if deg == 3 else 1), bcs_u=bcs_u, bcs_p=[],
                                solver_options=solver_options or KRYLOV, options=opts, **kw)
    for i, f in enumerate(fns):
        if field is None:
            S._u2[i].interpolate(lambda x, f=f: f(x, -dt, nu))
            S._u1[i].interpolate(lambda x, f=f: f(x, 0.0, nu))
        else:
            for u in (S._u1[i], S._u2[i]):
                u.interpolate(lambda x, i=i: DM.field(field, np.asarray(x)[:dim].T, dim)[:, i])
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


def _assemble_first(S, clock, dt, nu):
    clock["t"] = dt
    for bcl in S._bcs_u:
        for bc in bcl:
            bc.update_bc()
    S.assemble_first(dt, nu)


def _field_of(dim):
    return "wave" if dim == 2 else "shear"


def _variants(kind, mesh_cells=None):
    """(label, constructor keywords, model keywords given the Forms object)."""
    from tests import dynamic_model as DM

    out = [("global", {}, lambda F: {}), ("local", {"average": "local"}, lambda F: {"average": "local"})]
    if kind == "delaunay":
        out.append(("edges", {"axis": 1, "edges": EDGES}, lambda F: {"bins": DM.slab_bins_of(F, 1, EDGES)}))
    else:
        out.append(("slabs", {"axis": 1}, lambda F: {"bins": DM.slab_bins_of(F, 1)}))
    return out


def _compare_stages(S, m, F, P, uab, mkw, label):
    """The stage-by-stage comparison of one evaluated model; returns the measured relative maxima."""
    from tests import dynamic_model as DM

    out = {}
    rec, mom = DM.record_array(F, uab), DM.vertex_moments(F, uab, P)
    LM, MM = DM.products(F, uab, P, m.filter_ratio)
    for key, dev, ref in (("rec", m._rec, rec), ("mom", m._mom, mom), ("LM", m._lm[:, 0], LM), ("MM", m._lm[:, 1], MM)):
        dev = dev.cpu().numpy()
        assert dev.shape == ref.shape, (key, dev.shape, ref.shape)
        d, mx = np.abs(dev - ref).max(), np.abs(ref).max()
        out[key] = d / mx
        print(f"  {label} {key}: max diff {d:.3e}, max|.| {mx:.3e}, ratio {d / mx:.3e}")
        assert mx > 0.0 and d <= 1e-12 * mx, (label, key, d, mx)
    nut_ref, cs2_ref, info = DM.nut_cells(F, uab, P, filter_ratio=m.filter_ratio, cs2_max=m.cs2_max, **mkw)
    ds = rec[:, -2]
    if m.average == "local":
        dev = m._cs2.cpu().numpy()
        bound = 1e-12 * info["bound"]
        assert np.isfinite(bound).all() and (cs2_ref > 0.0).mean() >= 0.30
        dc = np.abs(dev - cs2_ref)
        out["cs2"] = float((dc / np.maximum(info["bound"], TINY)).max())
        print(f"  {label} local Cs2: max diff {dc.max():.3e}, max diff / ((|LM|)^ / (2 MM^)) {out['cs2']:.3e}, "
              f"share > 0 {(cs2_ref > 0).mean():.2f}")
        assert (dc <= bound).all(), (label, dc.max())
        cbound = bound
    else:
        bins = m._bins.cpu().numpy()
        kap = info["kappa"]
        assert kap.max() <= 100.0, (label, kap)
        bound_b = 1e-12 * kap * np.maximum(np.abs(info["raw"]), TINY)
        for key, col, ref in (("raw", 2, info["raw"]), ("clipped", 3, info["clipped"])):
            db = np.abs(bins[:, col] - ref)
            out[key] = float((db / (kap * np.maximum(np.abs(info["raw"]), TINY))).max())
            print(f"  {label} Cs2 per bin ({key}): {np.round(ref, 5)}, max diff / (kappa |Cs2|) {out[key]:.3e}, kappa <= {kap.max():.3g}")
            assert (db <= bound_b).all(), (label, key, db, bound_b)
        assert np.array_equal(m.bin_coefficients().cpu().numpy(), bins[:, 3])
        assert np.array_equal(m.bin_coefficients(clipped=False).cpu().numpy(), bins[:, 2])
        b = info["bins"]
        cbound = np.where(b >= 0, bound_b[np.maximum(b, 0)], 0.0)
    nut = S._nut.cpu().numpy()
    dn = np.abs(nut - nut_ref)
    out["nut"] = float(dn.max() / nut_ref.max())
    print(f"  {label} nut: max diff {dn.max():.3e}, max nut {nut_ref.max():.3e}, ratio {out['nut']:.3e}")
    assert nut_ref.max() > 0.0 and nut.min() >= 0.0
    assert (dn <= 1e-12 * nut_ref.max() + cbound * ds).all(), (label, dn.max())
    # the accessors: the same arrays in the mesh's cell order
    lc = S._Vi[0][0].local_cells.cpu().numpy()
    lm_mesh, mm_mesh = (t.cpu().numpy() for t in m.products())
    assert lm_mesh.shape == (int(S._mesh.num_cells),)
    assert np.array_equal(lm_mesh[lc], m._lm[:, 0].cpu().numpy()) and np.array_equal(mm_mesh[lc], m._lm[:, 1].cpu().numpy())
    cs2_mesh = S.smagorinsky_coefficient().cpu().numpy()
    cs2_k = m._cs2.cpu().numpy() if m.average == "local" else np.where(
        info["bins"] >= 0, m._bins[:, 3].cpu().numpy()[np.maximum(info["bins"], 0)], 0.0)
    assert cs2_mesh.shape == (int(S._mesh.num_cells),) and np.array_equal(cs2_mesh[lc], cs2_k)
    assert np.array_equal(S.eddy_viscosity().cpu().numpy()[lc], nut)
    return out


# ---- 1. stage by stage -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lattice", "delaunay"])
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_stages_match_the_model(hip, dim, N, deg, kind):
    """The wave (2-D) and shear (3-D) fields: cell records, vertex moments, LM and MM within 1e-12 max|.| of each array;
    Cs2 per bin, unclipped and clipped, within 1e-12 kappa_b max(|Cs2_b|, tiny); the local Cs2 per cell within
    1e-12 (|LM|)^ / (2 MM^); nut within 1e-12 max nut plus the coefficient's bound times D s; products() and
    smagorinsky_coefficient() are the same arrays in the mesh's cell order.  Global, slab (lattice: vertex planes,
    Delaunay: edges=) and local averages.

    Observed on one MI355X, maxima over the cases (and those of the clip and periodic tests): records 8.3e-15, moments
    6.0e-15, LM 9.9e-15, MM 7.9e-15 of max|.|; Cs2 per bin 5.0e-15 of kappa_b |Cs2_b| with kappa <= 17.1; local Cs2 5.7e-14
    of (|LM|)^ / (2 MM^) with at least 59 % of the cells positive; nut 8.2e-15 of max nut."""
    import oasisx_amd as ox
    from tests import dynamic_model as DM

    dt, nu = 0.1, 0.5
    mesh = _delaunay(dim, N) if kind == "delaunay" else None
    for label, ckw, mkw in _variants(kind):
        m = ox.DynamicSmagorinsky(**ckw)
        S, clock, mesh = _problem(dim, N, deg, m, field=_field_of(dim), nu=nu, dt=dt, mesh=mesh)
        F, _, _ = _forms(S, mesh)
        _assemble_first(S, clock, dt, nu)
        P = DM.Patches(F)
        assert P.n_vertices == m._patches.n_vertices
        _compare_stages(S, m, F, P, S._UAB.rhost(), mkw(F), f"{kind} ({dim},{N},{deg}) {label}")


@pytest.mark.parametrize("dim,N,deg", [(2, 6, 1), (2, 5, 2), (2, 4, 3)])
def test_clip_on_both_sides(hip, dim, N, deg):
    """The shifted Taylor-Green field has slabs on both sides of 0: the clipped coefficient is 0 exactly where the model's
    ratio is not positive, and a cell_bins= array with cells left out (-1) gives Cs2 = 0 and nut = 0 there."""
    import oasisx_amd as ox
    from tests import dynamic_model as DM

    dt, nu = 0.1, 0.5
    m = ox.DynamicSmagorinsky(axis=1)
    S, clock, mesh = _problem(dim, N, deg, m, field="shifted_tg", nu=nu, dt=dt)
    F, _, _ = _forms(S, mesh)
    _assemble_first(S, clock, dt, nu)
    P = DM.Patches(F)
    bins = DM.slab_bins_of(F, 1)
    _compare_stages(S, m, F, P, S._UAB.rhost(), {"bins": bins}, f"shifted TG ({dim},{N},{deg}) slabs")
    _, info = DM.coefficient(F, S._UAB.rhost(), P, bins=bins)
    dev = m.bin_coefficients().cpu().numpy()
    assert (info["raw"] > 0).any() and (info["raw"] < 0).any()
    assert np.array_equal(dev == 0.0, info["raw"] <= 0.0)
    # cells left out
    cen = mesh.coords[mesh.cells.long()].mean(dim=1).cpu().numpy()
    cb = np.where(cen[:, 0] < -0.5, -1, (cen[:, 1] > 0.0).astype(np.int64))
    m2 = ox.DynamicSmagorinsky(cell_bins=cb)
    S2, clock2, _ = _problem(dim, N, deg, m2, field="wave", nu=nu, dt=dt, mesh=mesh)
    _assemble_first(S2, clock2, dt, nu)
    lc = S2._Vi[0][0].local_cells.cpu().numpy()
    _compare_stages(S2, m2, F, P, S2._UAB.rhost(), {"bins": cb[lc]}, f"wave ({dim},{N},{deg}) cell_bins")
    out = cb < 0
    assert out.any() and (S2.eddy_viscosity().cpu().numpy()[out] == 0.0).all()
    assert (S2.smagorinsky_coefficient().cpu().numpy()[out] == 0.0).all()
    assert (S2.eddy_viscosity().cpu().numpy()[~out] > 0.0).any()


# ---- 2. periodic -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg", [1, 2])
def test_periodic_patches_wrap_around_the_seam(hip, deg):
    """A make_periodic box, axes (0, 2), N = 4: the stages against the model on the vertex CLASSES.  On the lattice every
    vertex class on a plane parallel to the walls has the same patch size -- which fails if the seam is not wrapped."""
    import torch

    import oasisx_amd as ox
    from oasisx_amd import mesh as M
    from tests import dynamic_model as DM
    from tests.helpers import KRYLOV

    N, dt, nu = 4, 0.1, 0.5
    mesh = M.make_periodic(M.create_box(None, [[-1.0] * 3, [1.0] * 3], [N, N, N]), (0, 2))
    walls = lambda x: np.isclose(np.abs(x[1]), 1.0)  # noqa: E731
    bcs = [[ox.DirichletBC(0.0, ox.LocatorMethod.GEOMETRICAL, walls)] for _ in range(3)]
    for label, ckw, mkw in (("global", {}, lambda F: {}), ("slabs", {"axis": 1}, lambda F: {"bins": DM.slab_bins_of(F, 1)}),
                            ("local", {"average": "local"}, lambda F: {"average": "local"})):
        m = ox.DynamicSmagorinsky(**ckw)
        S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", deg), ("Lagrange", 1), bcs_u=bcs, bcs_p=[], solver_options=KRYLOV,
                                    options={"sell_window": 128, "low_memory_version": True}, viscosity_model=m)
        # periodic along x and z with the box's period 2, sheared across the channel; in the model (checked on the CPU
        # when this test was written): kappa = 1.0 in every slab, Cs2 0.067 globally, 0.04 .. 0.094 per slab -- the two
        # core slabs exceed cs2_max = 0.09 and meet the upper clip.  Plain sines of pi x cancel exactly on four cells
        # per period (kappa ~ 1e15) and are no input for a ratio.
        fns = [lambda x, i=i: np.sin(1.3 * x[1] + 1.1 * i + 2.0) * (1.0 + 0.4 * np.sin(np.pi * x[0] + 0.5 + i)
                                                                   + 0.3 * np.cos(np.pi * x[2] + 0.2 * i)) for i in range(3)]
        for i, f in enumerate(fns):
            S._u1[i].interpolate(f)
            S._u2[i].interpolate(f)
        S.assemble_first(dt, nu)
        F, _, _ = _forms(S, mesh)
        vt = mesh.periodic.vertex_topo
        P = DM.Patches(F, vertex_class=vt)
        p = m._patches
        assert p.n_vertices == int(mesh.periodic.n_free_vertices) == P.n_vertices < int(mesh.coords.shape[0])
        assert np.array_equal(p.cell_verts.cpu().numpy(), P.verts)
        # patch sizes: one per wall-parallel plane
        count = torch.diff(p.ptr.to(torch.int64)).cpu().numpy()
        y = np.zeros(P.n_vertices)
        y[vt] = mesh.coords.cpu().numpy()[:, 1]
        for plane in np.unique(np.round(y, 9)):
            sizes = np.unique(count[np.isclose(y, plane)])
            assert sizes.shape[0] == 1, (plane, sizes)
        _compare_stages(S, m, F, P, S._UAB.rhost(), mkw(F), f"periodic P{deg} {label}")


# ---- 3. the filter alone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lattice", "delaunay"])
@pytest.mark.parametrize("dim,N", [(2, 6), (3, 3)])
def test_patch_filter_matches_the_model(hip, dim, N, kind):
    """PatchFilter.apply for k = 1 and k = 2 (mesh cell order in, mesh cell order out) within 1e-12 max|q| of the model's
    filter; a constant comes back to rounding; k = 3 and a wrong length are refused."""
    import torch

    import oasisx_amd as ox
    from tests import dynamic_model as DM

    mesh = _delaunay(dim, N) if kind == "delaunay" else None
    S, _, mesh = _problem(dim, N, 2, None, mesh=mesh)
    assert S._nut is None
    F, _, _ = _forms(S, mesh)
    P = DM.Patches(F)
    lc = S._Vi[0][0].local_cells.cpu().numpy()
    nc = int(mesh.num_cells)
    flt = ox.PatchFilter(S)
    rng = np.random.default_rng(11)
    for shape in ((nc,), (nc, 1), (nc, 2)):
        q = rng.standard_normal(shape)
        dev = flt.apply(torch.from_numpy(q).to(mesh.device)).cpu().numpy()
        assert dev.shape == q.shape
        ref = P.filter(q[lc])  # kernel order
        d = np.abs(dev[lc] - ref).max()
        print(f"{kind} {dim}-D k = {shape}: max diff {d:.3e} of {np.abs(q).max():.3e}")
        assert d <= 1e-12 * np.abs(q).max()
    c = flt.apply(torch.full((nc, 2), 3.25, dtype=torch.float64, device=mesh.device)).cpu().numpy()
    assert np.abs(c - 3.25).max() <= 8 * np.finfo(float).eps * 3.25
    q = torch.from_numpy(rng.standard_normal((nc, 2))).to(mesh.device)
    assert torch.equal(flt.apply(q), flt.apply(q))
    with pytest.raises(NotImplementedError):
        flt.apply(torch.zeros((nc, 3), dtype=torch.float64, device=mesh.device))
    with pytest.raises(ValueError):
        flt.apply(torch.zeros(nc + 1, dtype=torch.float64, device=mesh.device))


# ---- 4. A and b_first --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_operator_and_rhs_entry_by_entry(hip, dim, N, deg):
    """After assemble_first with the dynamic nut (slab bins, row blocks, value dictionaries): A and b_first equal the
    model's -- weighted_stiffness of the model's nut -- to 1e-12 max|.|, as test_gpu_viscosity.py asks of the constant
    model.  K_nut is at least 0.5 % of max|A|, so the term is visible in the bound.

    Observed on one MI355X: dA <= 3.4e-15 max|A|, db <= 5.7e-15 max|b|, max|K_nut| / max|A| between 0.024 and 0.16."""
    import oasisx_amd as ox
    from tests import dynamic_model as DM
    from tests import viscosity_model as VM

    dt, nu = 0.1, 0.02
    m = ox.DynamicSmagorinsky(axis=1)
    S, clock, mesh = _problem(dim, N, deg, m, field=_field_of(dim), nu=nu, dt=dt,
                              options={"value_dictionary": True, "assemble_row_blocks": True})
    F, x_v, x_q = _forms(S, mesh)
    R, rc = DM.tg_step_model(F, x_v, x_q, {"bins": DM.slab_bins_of(F, 1)}, nu=nu, dt=dt, field=_field_of(dim))
    R.u1[:], R.u2[:] = S._U1.rhost(), S._U2.rhost()
    rc["t"] = dt
    _assemble_first(S, clock, dt, nu)
    R.assemble_first(dt, nu)
    dA = abs(S._A.to_scipy() - R.A).max()
    db = np.abs(S._BFIRST.rhost() - R.b_first).max()
    share = abs(VM.weighted_stiffness(F, R.nut)).max() / abs(R.A).max()
    print(f"({dim},{N},{deg}): dA = {dA:.3e} (max|A| = {abs(R.A).max():.3e}, max|K_nut| / max|A| = {share:.2e}), "
          f"db = {db:.3e} (max|b| = {np.abs(R.b_first).max():.3e})")
    assert share >= 5e-3
    assert dA <= 1e-12 * abs(R.A).max(), dA
    assert db <= 1e-12 * np.abs(R.b_first).max(), db


# ---- 5. whole steps ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("update_every", [1, 2])
@pytest.mark.parametrize("dim,N", [(2, 8), (3, 3)])
def test_steps_match_the_model(hip, dim, N, update_every):
    """Three P2-P1 steps from the wave / shear field (held on the boundary) with the global dynamic model
    against DynamicOracleStep: du < 1e-8, dp < 1e-7, the bounds of test_gpu_viscosity.test_steps_match_the_model; Cs2 is
    recomputed in steps 0 and 2 with update_every = 2.

    Observed on one MI355X: du <= 1.5e-11, dp <= 1.0e-9, the global Cs2 within 6.3e-13 of the model's."""
    import oasisx_amd as ox
    from tests import dynamic_model as DM
    from tests.helpers import KRYLOV

    nu, dt = 0.01, 0.005
    m = ox.DynamicSmagorinsky(update_every=update_every)
    S, clock, mesh = _problem(dim, N, 2, m, field=_field_of(dim), nu=nu, dt=dt)
    F, x_v, x_q = _forms(S, mesh)
    R, rc = DM.tg_step_model(F, x_v, x_q, {}, update_every=update_every, nu=nu, dt=dt, solver_options=KRYLOV,
                             field=_field_of(dim))
    R.u1[:], R.u2[:] = S._U1.rhost(), S._U2.rhost()
    for k in range(3):
        clock["t"] = rc["t"] = (k + 1) * dt
        S.solve(dt, nu, max_iter=1)
        R.solve(dt, nu, max_iter=1)
        du = float(np.abs(S._U.rhost() - R.u1).max())
        dp = float(np.abs(S._P.rhost()[:, 0] - R.p).max())
        dn = float(np.abs(S._nut.cpu().numpy() - R.nut).max())
        dc = abs(float(m.bin_coefficients()[0]) - R.info["clipped"][0])
        print(f"step {k}: du = {du:.3e}, dp = {dp:.3e}, d nut = {dn:.3e} (max nut {R.nut.max():.3e}), d Cs2 = {dc:.3e} "
              f"(Cs2 {R.info['clipped'][0]:.5f})")
        assert du < 1e-8 and dp < 1e-7, (k, du, dp)
        assert (m.n_evaluations, m.n_updates) == (R.n_evaluations, R.n_updates) == (k + 1, k // update_every + 1)
    assert R.nut.max() > 0.0


# ---- 6. behaviour ------------------------------------------------------------------------------------------------------
def _evaluated(dim, N, deg, ckw, field, scale=1.0, shift=None, mesh=None):
    import oasisx_amd as ox

    m = ox.DynamicSmagorinsky(**ckw)
    S, clock, mesh = _problem(dim, N, deg, m, field=field, nu=0.5, dt=0.1, mesh=mesh)
    if scale != 1.0 or shift is not None:
        for U in (S._U1, S._U2):
            t = U.dev()
            t[: S._n_u] = t[: S._n_u] * scale + (0.0 if shift is None else shift.to(t.device))
    _assemble_first(S, clock, 0.1, 0.5)
    return S, m, mesh


@pytest.mark.parametrize("average", ["global", "slabs", "local"])
@pytest.mark.parametrize("dim,N,deg", [(2, 5, 2), (3, 3, 2)])
def test_reproducible_scaling_and_galilean_invariance(hip, dim, N, deg, average):
    """Two evaluations on the same state are torch.equal; u -> a u gives LM, MM -> a^4 ., Cs2 unchanged, nut -> a nut to
    1e-12 relative; u -> u + U, |U| ~ 3, leaves LM within 1e-12 gdim max|u + U|^2 max|M| (the host test's bounds)."""
    import torch

    from tests import dynamic_model as DM

    ckw = {"global": {}, "slabs": {"axis": 1}, "local": {"average": "local"}}[average]
    name = _field_of(dim)
    S, m, mesh = _evaluated(dim, N, deg, ckw, name)
    nut, lm, cs2 = S._nut.clone(), m._lm.clone(), S.smagorinsky_coefficient()
    S.viscosity_assemble(0.5)
    assert torch.equal(S._nut, nut) and torch.equal(m._lm, lm) and torch.equal(S.smagorinsky_coefficient(), cs2)
    a = 1.7
    S2, m2, _ = _evaluated(dim, N, deg, ckw, name, scale=a, mesh=mesh)
    for k, key in ((0, "LM"), (1, "MM")):
        d, mx = float((m2._lm[:, k] - a ** 4 * lm[:, k]).abs().max()), a ** 4 * float(lm[:, k].abs().max())
        print(f"scaling {key}: {d:.3e} of {mx:.3e}")
        assert d <= 1e-12 * mx
    dc, dn = float((S2.smagorinsky_coefficient() - cs2).abs().max()), float((S2._nut - a * nut).abs().max())
    print(f"scaling Cs2: {dc:.3e} of {float(cs2.max()):.3e}; nut: {dn:.3e} of {a * float(nut.max()):.3e}")
    assert dc <= 1e-12 * float(cs2.abs().max()) and dn <= 1e-12 * a * float(nut.abs().max())
    U = torch.tensor([2.0, -1.8, 1.3][:dim], dtype=torch.float64)
    S3, m3, _ = _evaluated(dim, N, deg, ckw, name, shift=U, mesh=mesh)
    F, _, _ = _forms(S, mesh)
    _, _, M = DM.tensors(F, S._UAB.rhost(), DM.Patches(F))
    bound = 1e-12 * dim * float(np.abs(S3._UAB.rhost()).max()) ** 2 * np.abs(M).max()
    d = float((m3._lm[:, 0] - lm[:, 0]).abs().max())
    print(f"Galilean LM: {d:.3e}, bound {bound:.3e}")
    assert d <= bound


@pytest.mark.parametrize("dim,N,deg", [(2, 4, 3), (3, 3, 1)])
def test_zero_field_nan_and_one_bin(hip, dim, N, deg):
    """A zero field gives zeros (no NaN); a NaN in u_ab reaches nut; the global average equals cell_bins = zeros bit for
    bit."""
    import torch

    name = _field_of(dim)
    for ckw in ({}, {"axis": 1}, {"average": "local"}):
        S, m, mesh = _evaluated(dim, N, deg, ckw, name, scale=0.0)
        assert torch.equal(S._nut, torch.zeros_like(S._nut)) and torch.equal(m._lm, torch.zeros_like(m._lm))
        assert torch.equal(S.smagorinsky_coefficient(), torch.zeros_like(S.smagorinsky_coefficient()))
        S, m, mesh = _evaluated(dim, N, deg, ckw, name)
        S._UAB.dev()[int(S._Vi[0][0].cell_dofs[0, 0]), 0] = float("nan")
        m.n_evaluations = 0
        S.viscosity_assemble(0.5)
        assert bool(torch.isnan(S._nut[0])) and (ckw != {} or bool(torch.isnan(S._nut).all()))
    S1, m1, mesh = _evaluated(dim, N, deg, {}, name)
    S2, m2, _ = _evaluated(dim, N, deg, {"cell_bins": np.zeros(int(mesh.num_cells), dtype=np.int64)}, name, mesh=mesh)
    assert m1.n_bins == m2.n_bins == 1 and m1.bin_coefficients().shape == (1,)
    assert torch.equal(m1._bins, m2._bins) and torch.equal(S1._nut, S2._nut) and float(S1._nut.max()) > 0.0


def test_scalars_full_stress_and_storage_modes(hip):
    """turbulent_schmidt= runs with scalar_diffusivity == kappa + nut / Sc_t; stress_form="full" and low_memory_version
    False take steps; the default path stays untouched: a solver without a model has S._nut None and calls none of the
    new entry points."""
    import torch

    import oasisx_amd as ox
    from oasisx_amd import _lib

    nu, dt, kappa, sct = 0.01, 0.005, 0.2, 0.7
    sc = ox.ScalarTransport("T", diffusivity=kappa, turbulent_schmidt=sct)
    S, clock, mesh = _problem(2, 5, 2, ox.DynamicSmagorinsky(axis=1), field="wave", nu=nu, dt=dt, scalars=[sc])
    S.scalar("T").interpolate(lambda x: np.sin(x[0]) * np.cos(x[1]))
    clock["t"] = dt
    S.solve(dt, nu, max_iter=1)
    assert torch.equal(S.scalar_diffusivity("T", nu), kappa + S.eddy_viscosity() / sct)
    assert float(S.scalar_diffusivity("T", nu).max()) > kappa and bool(torch.isfinite(S._U.rdev()).all())
    for kw in ({"stress_form": "full"}, {"low_memory": False}):
        for ckw in ({}, {"average": "local"}):
            S, clock, _ = _problem(3, 3, 2, ox.DynamicSmagorinsky(**ckw), field="shear", nu=nu, dt=dt, **kw)
            for k in range(2):
                clock["t"] = (k + 1) * dt
                S.solve(dt, nu, max_iter=1)
            assert bool(torch.isfinite(S._U.rdev()).all()) and float(S._nut.max()) > 0.0
    # the default path
    lib = _lib.load()
    new = ["ox_dynamic_cells", "ox_dynamic_vertices", "ox_dynamic_products", "ox_dynamic_bin_sums",
           "ox_dynamic_bin_coefficients", "ox_patch_filter_vertices", "ox_patch_filter_cells", "ox_dynamic_clip"]
    calls, tables = [], []  # tables: per ox_cell_viscosity call, whether the block carries a table of Cs2

    class Spy:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            if name in new:
                calls.append(name)
            fn = getattr(self._lib, name)
            if name != "ox_cell_viscosity":
                return fn

            def cell_viscosity(cells, args, stream):
                tables.append(args._obj.cs2 is not None)
                return fn(cells, args, stream)

            return cell_viscosity

    S, clock, _ = _problem(2, 5, 2, None)
    assert S._nut is None
    S._lib = Spy(lib)
    clock["t"] = dt
    S.solve(dt, nu, max_iter=1)
    assert calls == [] and tables == []
    S, clock, _ = _problem(2, 5, 2, ox.Smagorinsky())
    S._lib = Spy(lib)
    clock["t"] = dt
    S.solve(dt, nu, max_iter=1)
    assert calls == [] and tables != [] and not any(tables)  # (the constant form: never a table)
    S, clock, _ = _problem(2, 5, 2, ox.DynamicSmagorinsky())
    S._lib = Spy(lib)
    clock["t"] = dt
    S.solve(dt, nu, max_iter=1)
    assert "ox_dynamic_cells" in calls and any(tables)  # (the spy sees the new calls)


def test_guards(hip):
    import ctypes as C

    import torch

    import oasisx_amd as ox
    from oasisx_amd import _lib
    from oasisx_amd.parallel import Comm
    from tests.helpers import tg_mesh

    with pytest.raises(NotImplementedError, match="rotational"):
        _problem(2, 4, 2, ox.DynamicSmagorinsky(), rotational=True)
    pmesh = tg_mesh(2, 4)
    pmesh.comm = Comm(0, 2, None, transport="host")
    with pytest.raises(NotImplementedError, match="partition"):
        _problem(2, 4, 2, ox.DynamicSmagorinsky(), mesh=pmesh)
    with pytest.raises(ValueError, match="cell_bins"):
        _problem(2, 4, 2, ox.DynamicSmagorinsky(cell_bins=np.zeros(5, dtype=np.int64)))
    with pytest.raises(ValueError):
        ox.DynamicSmagorinsky(average="local", axis=0)
    with pytest.raises(TypeError):
        ox.DynamicSmagorinsky(damping=None)
    S, _, _ = _problem(2, 4, 2, ox.Smagorinsky())
    with pytest.raises(RuntimeError, match="DynamicSmagorinsky"):
        S.smagorinsky_coefficient()
    S, _, _ = _problem(2, 4, 2, ox.DynamicSmagorinsky())
    with pytest.raises(RuntimeError):
        S._viscosity_model.products()
    # the C entry points refuse what they can see on the host
    lib, m, Vi = hip, S._viscosity_model, S._Vi[0][0]
    p = m._patches
    assert lib.ox_dynamic_cells(Vi.degree, C.byref(S._cells), None, S._UAB.rptr(), _lib.ptr(m._rec), None) != 0
    assert b"null" in lib.ox_last_error()
    assert lib.ox_dynamic_cells(4, C.byref(S._cells), _lib.ptr(Vi.cell_dofs), S._UAB.rptr(), _lib.ptr(m._rec), None) != 0
    assert lib.ox_dynamic_vertices(4, p.n_vertices, _lib.ptr(p.ptr), _lib.ptr(p.idx), p.n_cells, _lib.ptr(m._rec),
                                   _lib.ptr(m._mom), None) != 0
    assert lib.ox_dynamic_vertices(2, p.n_vertices, _lib.ptr(p.ptr), _lib.ptr(p.idx), 1 << 31, _lib.ptr(m._rec),
                                   _lib.ptr(m._mom), None) != 0
    assert lib.ox_dynamic_products(2, p.n_cells, _lib.ptr(p.cell_verts), p.n_vertices, _lib.ptr(m._rec), _lib.ptr(m._mom),
                                   1.0, _lib.ptr(m._lm), None) != 0
    assert b"filter_ratio" in lib.ox_last_error()
    assert lib.ox_dynamic_bin_coefficients(1, _lib.ptr(m._plan["bin_chunk_ptr"]), _lib.ptr(m._partials), -1.0,
                                           _lib.ptr(m._bins), None) != 0
    q = torch.zeros((p.n_cells, 3), dtype=torch.float64, device=m._rec.device)
    assert lib.ox_patch_filter_cells(3, 2, p.n_cells, _lib.ptr(p.cell_verts), p.n_vertices, _lib.ptr(q), _lib.ptr(q),
                                     None) != 0
    for stride in (0, 4):  # cs2_stride < 1; per cell (no cell_bin): n_coef = 1 is not n_cells
        args = _lib.ox_viscosity_args(0, Vi.degree, _lib.ptr(Vi.cell_dofs), S._UAB.rptr(), _lib.ptr(S._nut), 0.0, None, 0,
                                      None, _lib.ptr(m._bins), stride, 1, None)
        assert lib.ox_cell_viscosity(C.byref(S._cells), C.byref(args), None) != 0
        assert (b"cs2_stride" if stride == 0 else b"n_coef") in lib.ox_last_error()
    torch.cuda.synchronize()


# ---- 7. the demo -------------------------------------------------------------------------------------------------------
def test_demo_prints_a_profile_that_vanishes_towards_the_walls(hip, capsys):
    """demo/dynamic_les_channel_hip.py at its smallest size (N = 8 slabs, 2-D): the dynamic Cs2 of the two wall slabs is
    smaller than the mean of the core slabs, where constant-Cs Smagorinsky has the same Cs2 everywhere.

    Observed on one MI355X: wall slabs Cs2 <= 0.00444, core mean 0.01085 (the constant model: 0.17^2 = 0.0289)."""
    from demo.dynamic_les_channel_hip import main

    res = main(["-N", "8"])
    out = capsys.readouterr().out
    assert "Cs2" in out and "van Driest" in out
    rows = res["rows"]
    assert len(rows) == 8
    wall = max(rows[0]["cs2"], rows[-1]["cs2"])
    core = float(np.mean([r["cs2"] for r in rows[2:-2]]))
    print(f"wall slabs Cs2 <= {wall:.5f}, core mean {core:.5f}")
    assert 0.0 <= wall < core
    assert all(r["nut"] >= 0.0 and np.isfinite(r["nut"]) for r in rows)
