"""GPU: flow rates, lumped outlet models and the backflow stabilisation (oasisx_amd/outlet.py, csrc/ox_outlet.hip) against
the numpy model of tests/outlet_model.py, which uses coordinates, the facet rule and ``fem.lagrange_basis`` only and is
pinned by tests/test_outlet_host.py.  The model is fed the device's dof numbering.  The bound is the project's bound on
assembled quantities, 1e-12 times the scale named with each item."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [(2, 6, 1), (2, 5, 2), (3, 3, 1), (3, 3, 2), (2, 4, 3), (3, 2, 3)]
KINDS = ["lattice", "delaunay", "rolled"]
WK = dict(Rp=0.7, C=0.4, Rd=3.0, p_distal=1.5, p0=0.25, rho=1.25)
RES = dict(R=2.0, p_distal=0.5, rho=0.8)
ids_all = (10, 11, 12, 13, 14, 15)


def _mesh(dim, N, kind):
    from oasisx_amd import mesh as M
    from tests.helpers import tg_mesh
    from tests.test_gpu_viscosity import _delaunay

    if kind == "lattice":
        return tg_mesh(dim, N)
    mesh = _delaunay(dim, N)
    if kind == "rolled":  # the vertices of cell c rotated c times: every local facet index occurs
        cells = mesh.cells.cpu().numpy()
        idx = (np.arange(dim + 1)[None, :] + np.arange(cells.shape[0])[:, None]) % (dim + 1)
        mesh = M.from_arrays(mesh.coords.cpu().numpy(), np.take_along_axis(cells, idx, axis=1))
    return mesh


def _fields(dim, nu, amp, t, sign=None):
    """Per component: Taylor-Green plus the non-solenoidal perturbation of the viscosity tests; ``sign = +-1``: instead a
    field whose components are ``sign`` times a positive function -- of one sign on every side; ``sign = "mixed"``: u_i =
    0.8 sin(2.1 x_{i+1} + ...) + 0.3 cos(1.7 x_i), whose normal component changes sign along every side (2.1 x runs over
    (-2.1, 2.1), the sine over (-0.86, 0.86), the offset is 0.3 cos(1.7) = -0.04)."""
    from oracle import ipcs_oracle as O
    from tests.test_gpu_viscosity import _perturbed

    if sign == "mixed":
        return [(lambda x, i=i: 0.8 * np.sin(2.1 * x[(i + 1) % dim] + 0.5 * i + t) + 0.3 * np.cos(1.7 * x[i])) for i in range(dim)]
    if sign is not None:
        return [(lambda x, i=i: (sign if i == 0 else 0.3) * (1.0 + 0.2 * np.sin(1.3 * x[1] + 0.4 * i + t))) for i in range(dim)]
    return [_perturbed(f, i, t, nu, amp) for i, f in enumerate([O.tg_u, O.tg_v, O.tg_w][:dim])]


def _outlet_solver(dim, N, deg, kind, make_bcs_p, dirichlet=(10,), mesh=None, nu=0.5, dt=0.1, solver_options=None):
    """[-1, 1]^dim with the side tags of the wall-stress tests (10 + 2 axis + upper): Dirichlet velocity on the sides
    ``dirichlet``, the pressure boundaries of ``make_bcs_p(tags)``, the other sides natural; u1, u2: perturbed Taylor-Green."""
    import oasisx_amd as ox
    from tests.helpers import KRYLOV
    from tests.test_gpu_wall_stress import _side_tags

    mesh = _mesh(dim, N, kind) if mesh is None else mesh
    tags, ids = _side_tags(mesh)
    bcs_u = [[ox.DirichletBC(f, ox.LocatorMethod.TOPOLOGICAL, (tags, g)) for g in dirichlet] for f in _fields(dim, nu, 0.3, dt)]
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", deg), ("Lagrange", 2 if deg == 3 else 1), bcs_u=bcs_u,
                                bcs_p=make_bcs_p(tags), solver_options=solver_options or KRYLOV,
                                options={"sell_window": 256})
    _set_levels(S, dim, nu, dt)
    return S, mesh, tags, ids


def _set_levels(S, dim, nu, dt, shift=0.0, sign=None):
    for i, (f2, f1) in enumerate(zip(_fields(dim, nu, 0.3, shift - dt, sign), _fields(dim, nu, 0.3, shift, sign))):
        S._u2[i].interpolate(f2)
        S._u1[i].interpolate(f1)


def _generations(S):
    """(generation of U, of U1) once the host check-outs of interpolate() have been copied back (that copy counts)."""
    S._U.rdev(), S._U1.rdev()
    return S._U.generation, S._U1.generation


def _facets_of(S, mesh, ids):
    """(mesh cell, opposite local vertex) of mesh facet ids, in that order."""
    from oasisx_amd.wall import facet_table

    return facet_table(mesh, np.asarray(ids, dtype=np.int64))


def _model_args(S, mesh):
    from tests.test_gpu_wall_stress import _tables

    vd, _ = _tables(S, mesh)
    return mesh.coords.cpu().numpy(), mesh.cells.cpu().numpy().astype(np.int64), vd


# ---- 1. flux = model -------------------------------------------------------------------------------------------------------
def _tag_scales(S, mesh, FR, u):
    """sum_{f in tag} |f| |ubar_f| per tag, from the model."""
    from tests import outlet_model as OM

    coords, cells, vd = _model_args(S, mesh)
    ubar = OM.facet_mean_u(coords, cells, FR.cells, FR.local_facets, vd, u, S._Vi[0][0].degree)
    _, meas, _ = OM.WM.facet_geometry(coords, cells, FR.cells, FR.local_facets)
    return OM.tag_sums(meas * np.linalg.norm(ubar, axis=1), FR.facet_tags, FR.tags)


def _check_flux(S, mesh, FR, u, what):
    """Per facet and per tag: |device - model| <= 1e-12 times the tag's sum_f |f| |ubar_f|."""
    from tests import outlet_model as OM

    coords, cells, vd = _model_args(S, mesh)
    ref = OM.facet_flux(coords, cells, FR.cells, FR.local_facets, vd, u, S._Vi[0][0].degree)
    scale = _tag_scales(S, mesh, FR, u)
    dev = FR.facet_flux().cpu().numpy()
    Q_ref = OM.tag_sums(ref, FR.facet_tags, FR.tags)
    Q = FR.rates()[-1]
    k_of = np.searchsorted(FR.tags, FR.facet_tags)
    rf, rq = (np.abs(dev - ref) / scale[k_of]).max(), (np.abs(Q - Q_ref) / scale).max()
    print(f"{what}: max |d flux| / scale = {rf:.3e}, max |dQ| / scale = {rq:.3e} (scales {scale.min():.3e} .. {scale.max():.3e})")
    assert scale.min() > 0.0 and np.abs(Q_ref).max() > 1e-3 * scale.max()
    assert rf <= 1e-12 and rq <= 1e-12
    return Q


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_flux_equals_the_model(hip, dim, N, deg, kind):
    """Perturbed Taylor-Green in u and another level in u1, one tag per side: per facet and per tag the device equals the
    model to 1e-12 sum_f |f| |ubar_f|; areas and normals equal WallStress's; the facets are ordered by tag, then by id.

    Observed on one MI355X, maximum over the cases (scale: the tag's sum): 3.8e-16 per facet, 7.0e-16 per tag."""
    import oasisx_amd as ox
    from tests.test_gpu_wall_stress import _set_tg, _side_tags, _solver

    nu = 0.5
    S, clock, mesh = _solver(dim, N, deg, kind, nu=nu, perturb=0.3)
    _set_tg(S, dim, nu)
    tags, ids = _side_tags(mesh)
    FR = ox.FlowRate(S, facets=(tags, ids))
    W = ox.WallStress(S, facets=(tags, ids))
    assert FR.n_tags == 2 * dim and FR.n_facets == mesh.exterior_facets().shape[0]
    assert np.array_equal(FR.facets, W.facets) and np.array_equal(FR.facet_tags, W.facet_tags)
    assert np.array_equal(FR.tags, np.asarray(ids))
    assert np.array_equal(FR.areas, W.areas) and np.array_equal(FR.normals, W.normals)
    if kind == "rolled":
        assert set(FR.local_facets.tolist()) == set(range(dim + 1))
    gen = _generations(S)
    FR.sample(0.0)
    _check_flux(S, mesh, FR, S._U.rhost(), f"{kind} ({dim},{N},{deg}) u")
    FR.sample(1.0, level=1)
    _check_flux(S, mesh, FR, S._U1.rhost(), f"{kind} ({dim},{N},{deg}) u1")
    assert (S._U.generation, S._U1.generation) == gen
    assert FR.rates().shape == (2, 2 * dim) and np.array_equal(FR.times, [0.0, 1.0])
    with pytest.raises(ValueError):
        FR.sample(2.0, level=2)


def test_flux_of_300_facets_in_one_tag(hip, tmp_path):
    """3-D lattice N = 5, all sides in one tag: 300 facets cross a block edge of the flux kernel and wrap the lanes of the
    update kernel; capacity 1 doubles twice without loss; save() round-trips.

    Observed on one MI355X: 1.9e-18 per facet, 1.3e-17 for the tag."""
    import oasisx_amd as ox
    from tests.test_gpu_wall_stress import _set_tg, _solver

    nu = 0.5
    S, clock, mesh = _solver(3, 5, 1, "lattice", nu=nu, perturb=0.3)
    FR = ox.FlowRate(S, capacity=1)
    assert FR.n_facets == 300 and FR.n_tags == 1
    Qs = []
    for k in range(3):
        _set_tg(S, 3, nu, t=0.1 * k)
        FR.sample(0.1 * k)
        Qs.append(_check_flux(S, mesh, FR, S._U.rhost(), f"300 facets, sample {k}")[0])
    assert FR.capacity == 4 and np.array_equal(FR.rates()[:, 0], Qs) and len(set(Qs)) == 3
    FR.save(tmp_path / "flow.npz")
    z = np.load(tmp_path / "flow.npz")
    assert np.array_equal(z["rates"], FR.rates()) and np.array_equal(z["facets"], FR.facets)


# ---- 2. exactness --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_polynomial_fields_give_the_closed_forms(hip, dim, N, deg, kind):
    """The closed forms of the host test on the device: a random polynomial field of degree <= DU gives, per side,
    s int u_k(x | x_k = s) dS; the fluxes of a polynomial solenoidal field sum to zero: 1e-12 sum_f |f| |ubar_f|.

    Per tag, the scale is the tag's sum_f |f| |ubar_f|; for the zero sum, the sum of those.

    Observed on one MI355X, maximum over the cases: 2.2e-16 for the closed forms, 4.1e-17 for the zero sum."""
    import oasisx_amd as ox
    from tests import test_outlet_host as H
    from tests.test_gpu_wall_stress import _side_tags, _solver

    S, clock, mesh = _solver(dim, N, deg, kind)
    tags, ids = _side_tags(mesh)
    FR = ox.FlowRate(S, facets=(tags, ids))
    if kind == "rolled":  # every local facet index: every row of the facet-mean tables, every instantiation of the kernel
        assert set(FR.local_facets.tolist()) == set(range(dim + 1))
    rng = np.random.default_rng(3 + 10 * dim + deg)
    for name, field in (("random", [H.poly_random(dim, deg, rng) for _ in range(dim)]),
                        ("solenoidal", H.solenoidal_field(dim, deg, rng))):
        for i in range(dim):
            S._u[i].interpolate(lambda x, i=i: H.poly_eval(field[i], x[:dim].T))
        FR.sample(0.0)
        Q = FR.rates()[-1]
        scale = _tag_scales(S, mesh, FR, S._U.rhost())
        exact = np.array([(1.0 if g % 2 else -1.0) * H.poly_side_integral(field[(g - 10) // 2], (g - 10) // 2,
                                                                           1.0 if g % 2 else -1.0) for g in ids])
        err = (np.abs(Q - exact) / scale).max()
        print(f"{kind} ({dim},{N},{deg}) {name}: max |Q - exact| / scale = {err:.3e}, |sum Q| / sum scale = "
              f"{abs(Q.sum()) / scale.sum():.3e}")
        assert err <= 1e-12
        if name == "solenoidal":
            assert np.abs(Q).max() > 1e-3 and abs(Q.sum()) <= 1e-12 * scale.sum()


# ---- 3. models -------------------------------------------------------------------------------------------------------------
def _model_outlet(S, mesh, bcp, value):
    from tests import outlet_model as OM

    fc, fa = _facets_of(S, mesh, np.sort(bcp._facets))
    return OM.Outlet(fc, fa, value, bcp.backflow)


def _wk_tuple(p):
    return ("windkessel", p["Rp"], p["C"], p["Rd"], p["p_distal"], p["p0"], p["rho"])


def _check_models(S, mesh, pairs, dt, h_before):
    """After an assemble_first: h of every outlet equals the model's P / rho on its dofs (1e-12 max |P / rho|) and is
    bit-unchanged elsewhere; returns the flow-rate scale."""
    from tests import outlet_model as OM

    coords, cells, vd = _model_args(S, mesh)
    u1 = S._U1.rhost()
    deg = S._Vi[0][0].degree
    scales = []
    for (bcp, o), h0 in zip(pairs, h_before):
        Q = float(OM.facet_flux(coords, cells, o.fc, o.fa, vd, u1, deg).sum())
        scales.append(OM.flux_scale(coords, cells, o.fc, o.fa, vd, u1, deg))
        want = o.advance(Q, dt)
        h = bcp._h.cpu().numpy()
        on = np.zeros(h.shape[0], dtype=bool)
        on[bcp._dofs] = True
        err = np.abs(h[on] - want).max() / abs(want)
        print(f"  outlet {bcp._subdomain_id}: Q = {Q:+.6e}, P / rho = {want:+.6e}, max |dh| / |P / rho| = {err:.3e}")
        assert err <= 1e-12
        assert np.array_equal(h[~on].view(np.int64), h0.cpu().numpy()[~on].view(np.int64))  # bit-unchanged elsewhere
    return scales


def _check_history(model, o, scale_q):
    """times, Q (1e-12 scale_q), P and Pc (1e-12 (max |P|, |Pc| + (Rp + Rd) scale_q): the model's P is Pc + Rp Q and one
    step moves Pc by at most Rd times a change of Q) equal the model's, entry by entry."""
    H = model.history()
    n = len(o.history["times"])
    assert all(H[k].shape == (n,) for k in ("times", "Q", "P", "Pc"))
    assert np.allclose(H["times"], o.history["times"], rtol=0, atol=1e-15 * n)
    assert np.abs(H["Q"] - o.history["Q"]).max() <= 1e-12 * scale_q
    size = max(np.abs(o.history["P"]).max(), np.abs(o.history["Pc"]).max()) + (model.Rp + model.Rd) * scale_q
    assert np.abs(H["P"] - o.history["P"]).max() <= 1e-12 * size
    assert np.abs(H["Pc"] - o.history["Pc"]).max() <= 1e-12 * size
    assert abs(model.state() - o.Pc) <= 1e-12 * size


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_three_outlets_in_one_solver(hip, dim, N, deg, kind):
    """A float, a Resistance and a Windkessel (capacity 2) on three sides of one solver; after each of three
    assemble_first calls (u1 changed in between): h on each outlet's dofs equals the model's P / rho, scale max |P / rho|,
    and is bit-unchanged elsewhere; the histories equal the model's; a stray update_bc(), surface_vector_host() or
    add_surface_terms() between the steps changes nothing; the ring of capacity 2 doubles without loss; the generations
    of U and U1 are those the interpolation left.

    Observed on one MI355X, maximum over the cases: max |dh| / |P / rho| = 2.6e-14 (where Pc and Rp Q cancel to P / rho =
    0.024; the scale is |P / rho| itself)."""
    import torch

    import oasisx_amd as ox

    nu, dt = 0.5, 0.1
    res, wk = ox.Resistance(**RES), ox.Windkessel(capacity=2, **WK)
    S, mesh, tags, ids = _outlet_solver(dim, N, deg, kind, lambda tags: [ox.PressureBC(4.0, (tags, 11)),
                                                                           ox.PressureBC(res, (tags, 12)),
                                                                           ox.PressureBC(wk, (tags, 13))], nu=nu, dt=dt)
    bcs = S._bcs_p
    pairs = [(bcs[0], _model_outlet(S, mesh, bcs[0], 4.0)),
             (bcs[1], _model_outlet(S, mesh, bcs[1], ("resistance", RES["R"], RES["p_distal"], RES["rho"]))),
             (bcs[2], _model_outlet(S, mesh, bcs[2], _wk_tuple(WK)))]
    # before the first step: the models' initial values on their dofs
    assert float(bcs[2]._h[torch.from_numpy(bcs[2]._dofs).long().to(bcs[2]._h.device)].min()) == WK["p0"] / WK["rho"]
    scale_q = 0.0
    for k in range(3):
        _set_levels(S, dim, nu, dt, shift=0.37 * k)
        gen = _generations(S)
        h_before = [b._h.clone() for b in bcs]
        S.assemble_first(dt, nu)
        assert (S._U.generation, S._U1.generation) == gen
        print(f"{kind} ({dim},{N},{deg}) step {k}:")
        scale_q = max([scale_q] + _check_models(S, mesh, pairs, dt, h_before))
        # stray calls between the steps do not advance the models
        snap = (S._outlet_models._state.clone(), [b._h.clone() for b in bcs], len(S._outlet_models._times))
        for b in bcs:
            b.update_bc()
            b.surface_vector_host(0)
            b.add_surface_terms(S._WRK)
        assert torch.equal(S._outlet_models._state, snap[0]) and len(S._outlet_models._times) == snap[2]
        assert all(torch.equal(b._h, h) for b, h in zip(bcs, snap[1]))
    assert S._outlet_models.capacity == 4
    _check_history(res, pairs[1][1], scale_q)
    _check_history(wk, pairs[2][1], scale_q)
    assert np.array_equal(res.history()["Pc"], np.full(3, RES["p_distal"]))
    # the histories are not constant, and reset() puts Pc back
    assert len(set(wk.history()["Q"].tolist())) == 3
    wk.reset()
    assert wk.state() == WK["p0"]
    wk.reset(p0=2.0)
    assert wk.state() == 2.0 and len(wk.history()["times"]) == 3


def test_602_pressure_dofs_on_one_outlet(hip):
    """3-D lattice N = 5, P3-P2, all six sides one outlet: 602 pressure dofs, more than the 256 lanes that write h; 300
    facets in the one tag.

    Observed on one MI355X: max |dh| / |P / rho| = 1.7e-15."""
    import oasisx_amd as ox

    nu, dt = 0.5, 0.1
    wk = ox.Windkessel(**WK)
    S, mesh, tags, ids = _outlet_solver(3, 5, 3, "lattice", lambda tags: [ox.PressureBC(wk, (tags, ids_all))],
                                        dirichlet=(), nu=nu, dt=dt)
    bcp = S._bcs_p[0]
    assert bcp._dofs.shape[0] == 602 and bcp._facets.shape[0] == 300
    pairs = [(bcp, _model_outlet(S, mesh, bcp, _wk_tuple(WK)))]
    for k in range(2):
        _set_levels(S, 3, nu, dt, shift=0.37 * k)
        h_before = [bcp._h.clone()]
        S.assemble_first(dt, nu)
        scale_q = _check_models(S, mesh, pairs, dt, h_before)[0]
    _check_history(wk, pairs[0][1], scale_q)



# ---- 4. backflow ---------------------------------------------------------------------------------------------------------
def _assembled(S, dt, nu):
    S.assemble_first(dt, nu)
    return S._A.to_scipy(), S._BFIRST.rhost().copy()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_backflow_operator(hip, dim, N, deg, kind):
    """Outlets on x = +1 (beta 0.5) and y = +1 (beta 1.0), which share the rim x = y = 1; Dirichlet velocity on x = -1,
    whose rim with y = +1 carries backflow rows that the identity rows replace.  u_ab . n changes sign across both outlets.
    A(beta) - A(0) = (beta/2) B_model off the Dirichlet rows, scale max |A|; b_first(beta) - b_first(0) = -(beta/2) B u1,
    scale max |b_first|; the Dirichlet rows are identity rows; two runs are bit-identical; with u_ab . n > 0 on both
    outlets A and b_first are array_equal to the beta = 0 ones: of the same solver with its backflow table taken away
    (the call is not made), and of the solver built with beta = 0 once both use the same outlet operators S_i -- those
    are summed with index_add_ at set-up (PressureBC.create_bcs), atomically on the device, so two builds may differ in
    the last bit of an entry (the test prints how many did), which shows in b_first by an ulp in a row or two.

    Observed on one MI355X, maximum over the cases: 1.1e-16 max |A| for A, 7.5e-17 max |b_first| for b_first."""
    import torch

    import oasisx_amd as ox
    from tests import outlet_model as OM

    nu, dt = 0.5, 0.1
    mesh = _mesh(dim, N, kind)
    S, _, tags, ids = _outlet_solver(dim, N, deg, kind, lambda tags: [ox.PressureBC(4.0, (tags, 11), backflow=0.5),
                                                                       ox.PressureBC(1.0, (tags, 13), backflow=1.0)],
                                     mesh=mesh, nu=nu, dt=dt)
    S0, _, _, _ = _outlet_solver(dim, N, deg, kind, lambda tags: [ox.PressureBC(4.0, (tags, 11)),
                                                                   ox.PressureBC(1.0, (tags, 13))], mesh=mesh, nu=nu, dt=dt)
    assert S._outlet_backflow is not None and S0._outlet_backflow is None and S0._outlet_models is None
    for T in (S, S0):
        _set_levels(T, dim, nu, dt, sign="mixed")
    A, b = _assembled(S, dt, nu)
    A0, b0 = _assembled(S0, dt, nu)
    coords, cells, vd = _model_args(S, mesh)
    uab, u1 = S._UAB.rhost(), S._U1.rhost()
    nv = S._Vi[0][0].num_dofs
    B = None
    for bcp in S._bcs_p:
        fc, fa = _facets_of(S, mesh, np.sort(bcp._facets))
        un = np.einsum("fk,fk->f", OM.facet_mean_u(coords, cells, fc, fa, vd, uab, deg),
                       OM.WM.facet_geometry(coords, cells, fc, fa)[0])
        assert un.min() < 0.0 < un.max()  # the flow enters through part of the outlet and leaves through the rest
        Bk = OM.backflow_matrix(coords, cells, fc, fa, vd, uab, deg, bcp.backflow, nv)
        B = Bk if B is None else B + Bk
    bf = S._outlet_backflow
    ptr, pair_beta = bf.row_ptr.cpu().numpy(), bf.beta.cpu().numpy()[bf.pair_facet.cpu().numpy()]
    shared = [i for i in range(bf.n_rows) if len(set(pair_beta[ptr[i]:ptr[i + 1]].tolist())) == 2]
    assert shared  # rim rows that the two outlets, with their different beta, share
    db_ref = -0.5 * (B @ u1)
    dirichlet = np.unique(np.concatenate([bc._dofs for bc in S._bcs_u[0]]))
    keep = np.ones(nv)
    keep[dirichlet] = 0.0
    import scipy.sparse as sp

    dA_ref = sp.diags(keep) @ (0.5 * B)
    assert np.intersect1d(dirichlet, bf.rows.cpu().numpy()[: bf.n_rows]).size > 0  # identity rows replace backflow rows
    ea = abs((A - A0) - dA_ref).max() / abs(A0).max()
    eb = np.abs((b - b0) - db_ref).max() / np.abs(b0).max()
    print(f"{kind} ({dim},{N},{deg}): max |dA - (beta/2) B| / max |A| = {ea:.3e} (max |dA| / max |A| = "
          f"{abs(dA_ref).max() / abs(A0).max():.3e}), max |db + (beta/2) B u1| / max |b| = {eb:.3e}")
    assert abs(dA_ref).max() > 1e-6 * abs(A0).max() and np.abs(db_ref).max() > 1e-6 * np.abs(b0).max()
    assert ea <= 1e-12 and eb <= 1e-12
    Ad = A[dirichlet].tocoo()
    assert np.array_equal(Ad.data[Ad.data != 0.0], np.ones(dirichlet.shape[0]))
    assert np.array_equal(dirichlet[Ad.row[Ad.data != 0.0]], Ad.col[Ad.data != 0.0])
    # bit-identical when run again
    vals, bf = S._A.vals.clone(), S._BFIRST.rdev().clone()
    S.assemble_first(dt, nu)
    assert torch.equal(S._A.vals, vals) and torch.equal(S._BFIRST.rdev(), bf)
    # pure outflow: u = (+, +, ...) leaves through x = +1 and y = +1
    for T in (S, S0):
        _set_levels(T, dim, nu, dt, sign=1.0)
    A, b = _assembled(S, dt, nu)
    table, S._outlet_backflow = S._outlet_backflow, None  # the same solver at beta = 0: the backflow call is not made
    A_off, b_off = _assembled(S, dt, nu)
    S._outlet_backflow = table
    assert np.array_equal(A.toarray(), A_off.toarray()) and np.array_equal(b, b_off)
    # ... and the solver BUILT with beta = 0.  Its outlet operators S_i (PressureBC.create_bcs) sum the facets'
    # contributions with index_add_, which on the device adds atomically, in no fixed order: two builds of the same
    # PressureBC may differ in the last bit of an entry.  That is set-up of the parent's code, not the backflow pass: the
    # operators of the one solver are handed to the other, after which b_first must agree bit for bit
    n_ulp = 0
    for bcp, bcp0 in zip(S._bcs_p, S0._bcs_p):
        for Sm, Sm0 in zip(bcp._S, bcp0._S):
            n_ulp += int((Sm.vals != Sm0.vals).sum())
            Sm0.vals.copy_(Sm.vals)
    A0, b0 = _assembled(S0, dt, nu)
    print(f"  pure outflow: {n_ulp} entries of the outlet operators differed between the two builds; "
          f"max |b - b(beta = 0 solver)| = {np.abs(b - b0).max():.3e}")
    assert np.array_equal(A.toarray(), A0.toarray()) and np.array_equal(b, b0)
    # ... and the same field reversed enters everywhere: B is not zero
    for T in (S, S0):
        _set_levels(T, dim, nu, dt, sign=-1.0)
    A, b = _assembled(S, dt, nu)
    A0, b0 = _assembled(S0, dt, nu)
    assert abs(A - A0).max() > 1e-6 * abs(A0).max()


def test_backflow_with_a_warm_started_tentative_solve(hip):
    """ksp_initial_guess_nonzero: a plain solver keeps the A u1 by-product of the fused kernel for the tentative solve; with
    backflow > 0 it is not asked for (A changes after the fused kernel: the product would be one of the matrix without
    (beta/2) B), and two warm-started steps of the channel with a Windkessel and backflow = 0.5 follow the model loop run
    with the same options.  Bounds: those of tests/test_gpu_pressure_bc.py::test_tentative_with_outlet for a step of this
    set-up, du < 1e-8 and dp < 1e-7; a stale product would be wrong by (beta/2) B u1, of the order 1e-2 max |A u1|.

    Observed on one MI355X: du = 4.5e-10, dp = 6.4e-10, with and without backflow."""
    from tests.helpers import KRYLOV

    warm = {k: dict(v, ksp_initial_guess_nonzero=True) for k, v in KRYLOV.items()}
    for beta, want in ((0.0, True), (0.5, False)):
        S, R, clock, dt, nu, wk, out = _channel(2, WK, beta, solver_options=warm)
        clock["t"] = dt
        for bcl in S._bcs_u:
            for bc in bcl:
                bc.update_bc()
        S.assemble_first(dt, nu)
        assert S._AU1_valid is want
        # fresh objects for the steps (the assemble_first above has advanced the model once)
        S, R, clock, dt, nu, wk, out = _channel(2, WK, beta, solver_options=warm)
        for k in range(2):
            clock["t"] = (k + 1) * dt
            S.solve(dt, nu, max_iter=1)
            R.solve(dt, nu, max_iter=1)
        du = float(np.abs(S._U.rhost() - R.u).max())
        dp = float(np.abs(S._P.rhost()[:, 0] - R.p).max())
        print(f"beta = {beta}: warm-started steps du = {du:.3e}, dp = {dp:.3e}")
        assert du < 1e-8 and dp < 1e-7


# ---- 5. whole steps --------------------------------------------------------------------------------------------------------
# (max |du|, max |dp|) of the plain PressureBC(4.0) run against the oracle, measured on one MI355X: see
# test_three_steps_with_windkessel_and_backflow
PLAIN = {1: (1.776357e-14, 2.131628e-14), 2: (3.103210e-09, 3.558682e-09)}


def _channel(u_deg, value, beta, solver_options=None):
    """The set-up of tests/test_gpu_pressure_bc.py::test_tentative_with_outlet: the device solver and the model loop."""
    import oasisx_amd as ox
    from oasisx_amd import mesh as M
    from oracle import ipcs_oracle as O
    from tests import outlet_model as OM
    from tests.helpers import KRYLOV
    from tests.test_gpu_pressure_bc import _facet_pairs

    KRYLOV = solver_options or KRYLOV
    dt, nu = 0.1, 0.5
    mesh = M.create_unit_square(None, 10, 10)
    left = M.locate_entities_boundary(mesh, 1, lambda x: np.isclose(x[0], 0))
    tb = M.locate_entities_boundary(mesh, 1, lambda x: np.isclose(x[1], 0) | np.isclose(x[1], 1))
    right = M.locate_entities_boundary(mesh, 1, lambda x: np.isclose(x[0], 1))
    facets = np.hstack([left, tb, right])
    values = np.hstack([np.full_like(left, 1), np.full_like(tb, 2), np.full_like(right, 3)]).astype(np.int32)
    srt = np.argsort(facets)
    tags = M.meshtags(mesh, 1, facets[srt], values[srt])
    clock = {"t": 0.0}
    inlet = lambda x: (1 + clock["t"]) * np.sin(np.pi * x[1])  # noqa: E731
    bc_tb = ox.DirichletBC(0.0, ox.LocatorMethod.TOPOLOGICAL, (tags, 2))
    bc_in_x = ox.DirichletBC(inlet, ox.LocatorMethod.TOPOLOGICAL, (tags, 1))
    bc_in_y = ox.DirichletBC(0.0, ox.LocatorMethod.TOPOLOGICAL, (tags, 1))
    dev_value = ox.Windkessel(**value) if isinstance(value, dict) else value
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", u_deg), ("Lagrange", 1), bcs_u=[[bc_in_x, bc_tb], [bc_in_y, bc_tb]],
                                bcs_p=[ox.PressureBC(dev_value, (tags, 3), backflow=beta)], solver_options=KRYLOV,
                                options={"sell_window": 128})
    Vi, Q = S._Vi[0][0], S._Q
    F = O.Forms(mesh.coords.cpu().numpy(), Vi.cells_in_kernel_order(), u_deg, 1, vd=Vi.cell_dofs.cpu().numpy(),
                qd=Q.cell_dofs.cpu().numpy(), nv_dofs=Vi.num_dofs, nq_dofs=Q.num_dofs)
    xv = Vi.x.cpu().numpy()
    ld = np.nonzero(np.isclose(xv[:, 0], 0))[0]
    td = np.nonzero(np.isclose(xv[:, 1], 0) | np.isclose(xv[:, 1], 1))[0]
    obcs = [[O.DirichletData(ld, lambda x: (1 + clock["t"]) * np.sin(np.pi * x[1])), O.DirichletData(td, 0.0)],
            [O.DirichletData(ld, 0.0), O.DirichletData(td, 0.0)]]
    fc, fa = _facet_pairs(F, mesh, right)
    fc = Vi.kernel_cell_index(fc)
    out = OM.Outlet(fc, fa, _wk_tuple(value) if isinstance(value, dict) else value, beta)
    R = OM.OutletOracle(F, xv, Q.x.cpu().numpy(), obcs, [out], solver_options=KRYLOV)
    X = np.zeros((3, xv.shape[0]))
    X[:2] = xv.T
    for i in range(2):
        for t, (a, b) in ((-2 * dt, (S._u2, R.u2)), (-dt, (S._u1, R.u1))):
            clock["t"] = t
            a[i].interpolate(inlet)
            b[:, i] = (1 + t) * np.sin(np.pi * X[1])
    S._p.interpolate(lambda x: x[1])
    R.p[:] = Q.x.cpu().numpy()[:, 1]
    return S, R, clock, dt, nu, dev_value, out


def _three_steps(u_deg, value, beta):
    """(max |u - u_model|, max |p - p_model|) after three solve() calls, and the objects."""
    S, R, clock, dt, nu, dev_value, out = _channel(u_deg, value, beta)
    for k in range(3):
        clock["t"] = (k + 1) * dt
        S.solve(dt, nu, max_iter=1)
        R.solve(dt, nu, max_iter=1)
    du = float(np.abs(S._U.rhost() - R.u).max())
    dp = float(np.abs(S._P.rhost()[:, 0] - R.p).max())
    return du, dp, S, R, dev_value, out


@pytest.mark.parametrize("u_deg", [1, 2])
def test_three_steps_with_windkessel_and_backflow(hip, u_deg):
    """The set-up of test_tentative_with_outlet (10 x 10 unit square, sin inlet, walls, outlet tag 3), three solve() calls
    with a Windkessel outlet and backflow = 0.5 against the model loop (OutletOracle).

    The bound: the same three steps with the plain PressureBC(4.0) -- a run that touches no code of the outlet models --
    differ from the oracle by PLAIN[u_deg] = (max |du|, max |dp|) at the same Krylov tolerances; ten times that is
    allowed here, for the feedback of a flux error through Rp and Rd into h.

    Measured on one MI355X (PLAIN holds the first pair of each line):
        u_deg = 1: plain  du = 1.776e-14, dp = 2.132e-14;  with the Windkessel and backflow  du = 8.438e-15, dp = 2.043e-14
        u_deg = 2: plain  du = 3.103e-09, dp = 3.559e-09;  with the Windkessel and backflow  du = 1.971e-09, dp = 2.212e-09
    (bounds: 1.8e-13 / 2.1e-13 and 3.1e-08 / 3.6e-08).  The P1 runs agree to rounding: device and oracle take the same
    Krylov iterates; the P2 runs stop within rtol 1e-11 of different iterates.
    """
    du, dp, S, R, wk, out = _three_steps(u_deg, WK, 0.5)
    bu, bp = PLAIN[u_deg]
    print(f"u_deg = {u_deg}: du = {du:.3e} (plain {bu:.3e}), dp = {dp:.3e} (plain {bp:.3e})")
    H = wk.history()
    print("  Q  ", H["Q"], "\n  P  ", H["P"], "\n  ref", np.asarray(out.history["P"]))
    assert np.abs(R.u).max() > 0.5 and np.isfinite(du) and np.isfinite(dp)
    assert du <= 10.0 * bu and dp <= 10.0 * bp
    assert H["Q"].shape == (3,) and np.allclose(H["times"], [0.1, 0.2, 0.3])
    assert np.abs(H["P"] - out.history["P"]).max() <= 10.0 * bp + 1e-12 * np.abs(H["P"]).max()


# ---- 6. guards -------------------------------------------------------------------------------------------------------------
def test_guards(hip):
    import oasisx_amd as ox
    from oasisx_amd.parallel import Comm
    from tests.test_gpu_wall_stress import _side_tags, _solver

    S, clock, mesh = _solver(2, 4, 2, "lattice")
    _, cf = mesh._entities(1)
    interior = int(np.nonzero(np.bincount(cf.ravel()) == 2)[0][0])
    with pytest.raises(ValueError, match="interior"):
        ox.FlowRate(S, facets=np.array([int(mesh.exterior_facets()[0]), interior]))
    with pytest.raises(ValueError):
        ox.FlowRate(S, capacity=0)
    tags, ids = _side_tags(mesh)
    with pytest.raises(ValueError):
        ox.PressureBC(4.0, (tags, 11), backflow=1.5)
    with pytest.raises(ValueError):
        ox.PressureBC(4.0, (tags, 11), backflow=-0.5)
    old = mesh.comm
    try:
        mesh.comm = Comm(0, 2, None, transport="host")
        with pytest.raises(NotImplementedError, match="partition"):
            ox.FlowRate(S)
        for bcp in (ox.PressureBC(ox.Resistance(1.0), (tags, 11)), ox.PressureBC(4.0, (tags, 11), backflow=0.5)):
            with pytest.raises(NotImplementedError, match="comm.size > 1"):
                ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_u=[[], []], bcs_p=[bcp])
    finally:
        mesh.comm = old
    with pytest.raises(RuntimeError):
        S.outlet_assemble(0.1)
    with pytest.raises(RuntimeError):
        S.backflow_assemble()
    FR = ox.FlowRate(S, facets=mesh.exterior_facets()[:3])
    assert FR.n_facets == 3 and FR.n_tags == 1


class _Counting:
    """The library handle with the ox_outlet_* entry points counted."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        if name.startswith("ox_outlet_"):
            self.calls.append(name)
        return getattr(self._lib, name)


def test_a_solver_without_outlet_objects_makes_none_of_the_calls(hip, monkeypatch):
    """A float PressureBC with backflow = 0: assemble_first calls none of ox_outlet_flux / _update / _backflow; with a model
    it calls flux and update once each; with backflow, the backflow pass once."""
    import oasisx_amd as ox
    from oasisx_amd import _lib

    nu, dt = 0.5, 0.1
    want = {"plain": [], "model": ["ox_outlet_flux", "ox_outlet_update"], "backflow": ["ox_outlet_backflow"],
            "both": ["ox_outlet_flux", "ox_outlet_update", "ox_outlet_backflow"]}
    make = {"plain": lambda tags: [ox.PressureBC(4.0, (tags, 11))],
            "model": lambda tags: [ox.PressureBC(ox.Resistance(1.0), (tags, 11))],
            "backflow": lambda tags: [ox.PressureBC(4.0, (tags, 11), backflow=0.5)],
            "both": lambda tags: [ox.PressureBC(ox.Windkessel(1.0, 1.0, 1.0), (tags, 11), backflow=0.5)]}
    for name in want:
        S, mesh, tags, ids = _outlet_solver(2, 4, 2, "lattice", make[name], nu=nu, dt=dt)
        proxy = _Counting(_lib.load())
        monkeypatch.setattr(_lib, "_lib", proxy)
        monkeypatch.setattr(S, "_lib", proxy)
        S.assemble_first(dt, nu)
        S.assemble_first(dt, nu)
        monkeypatch.undo()
        assert proxy.calls == want[name] * 2, (name, proxy.calls)


# ---- 7. demo ---------------------------------------------------------------------------------------------------------------
def test_demo(hip, capsys):
    """demo/windkessel_channel_hip.py at -N 8 --steps 3 runs and prints Q and P per step."""
    from demo.windkessel_channel_hip import main

    rows = main(["-N", "8", "--steps", "3"])
    out = capsys.readouterr().out
    assert len(rows) == 3 and "Q" in out and "P" in out
    assert all(np.isfinite(r["Q"]) and np.isfinite(r["P"]) and r["Q"] > 0.0 for r in rows)
