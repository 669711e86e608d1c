"""GPU: the cell locator, ``Function.eval`` and ``Probes`` (csrc/ox_probe.hip) against the numpy model of
tests/probe_model.py -- location, polynomial exactness for P1 / P2 / P3, probes in a time loop (read-only, bit-identical
to a run without probes), mesh partitions (8 rank threads and one 2-process job) and interpolation between spaces.

Bounds.  Values: 1e-12 * max|u| -- model and kernel evaluate the same <= 20-term sum in f64 and differ by summation order
and contraction (about nd * eps * sum|phi_a u_a| ~ 1e-14 max|u| with the P3 Lebesgue constant) plus the rounding of lambda
(~ eps |x| / h ~ 4e-15 on these meshes: |x| <= 1, h >= 1/16) times |dphi/dlambda| <= 7; two orders are left.  Partitioned
against serial samples: 4e-8 / 4e-7 = the 1e-8 / 1e-7 the rehearsals allow on the dofs times a bound of 4 on sum|phi_a|."""
import logging
import os
import socket

import numpy as np
import pytest
import torch

from tests import probe_model as PM

pytestmark = pytest.mark.gpu


def _mesh(kind, comm=None):
    from oasisx_amd import mesh as M

    if kind == "box2":
        return M.create_rectangle(comm, [[-1.0, -1.0], [1.0, 1.0]], [16, 16])
    if kind == "box3":
        return M.create_box(comm, [[-1.0] * 3, [1.0] * 3], [8, 8, 8])
    if kind == "box3c":
        return M.create_box(comm, [[-1.0] * 3, [1.0] * 3], [4, 4, 4])
    return M.create_delaunay_box(comm, [[-1.0] * 3, [1.0] * 3], 6, seed=4)


def _boundary_points(mesh, n, seed=3):
    ev = mesh._entities(mesh.gdim - 1)[0][mesh.exterior_facets()]
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, ev.shape[0], n)
    return mesh.coords.cpu().numpy()[ev[pick]].mean(axis=1)


def _points(mesh, seed=0):
    return np.concatenate([PM.sample_points(mesh, 300, 60, 60, seed=seed, n_centroids=40, n_faces=60),
                           _boundary_points(mesh, 40)], axis=0)


def _poly(degree, d, shift=0.0):
    """x (3, n) -> (n,): a polynomial of exactly that degree."""
    def f(x):
        y = x[1] if d == 2 else x[1] - 0.5 * x[2]
        v = 0.3 + shift + 0.7 * x[0] - 0.4 * y
        if degree >= 2:
            v = v + 0.9 * x[0] * y - 0.5 * y ** 2 + 0.25 * x[0] ** 2
        if degree >= 3:
            v = v + 0.6 * x[0] ** 2 * y - 0.35 * y ** 3 + 0.45 * x[0] * y ** 2 + (0.2 * x[0] * x[1] * x[2] if d == 3 else 0.0)
        return v
    return f


def _at(f, x, d):
    X = np.zeros((3, x.shape[0]))
    X[:d] = x[:, :d].T
    return f(X)


# ---- 1. location -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["box2", "box3", "delaunay"])
def test_location_equals_the_model(hip, kind):
    from oasisx_amd import geometry as G

    mesh = _mesh(kind)
    d = mesh.gdim
    coords, cells = mesh.coords.cpu().numpy(), mesh.cells.cpu().numpy()
    x = _points(mesh)
    outside = np.concatenate([np.full((1, d), 7.0), np.full((1, d), 1.0 + 1e-6), np.full((1, d), np.nan),
                              np.array([[0.1] * (d - 1) + [-1.0 - 1e-7]])])
    xa = np.concatenate([x, outside])
    want, wbary = PM.locate(coords, cells, xa)
    assert (want[: x.shape[0]] >= 0).all() and (want[x.shape[0]:] == -1).all()  # the model leaves no point out
    tree = G.bb_tree(mesh, d)
    info = tree.info()
    assert info["cells"] == mesh.num_cells and 0.25 * mesh.num_cells <= info["bins"] <= 4 * mesh.num_cells, info
    x3 = np.zeros((xa.shape[0], 3))
    x3[:, :d] = xa
    adj = G.compute_colliding_cells(mesh, G.compute_collisions_points(tree, x3), x3)
    got = np.array([adj.links(i)[0] if len(adj.links(i)) else -1 for i in range(xa.shape[0])])
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    assert adj.offsets[-1] == x.shape[0] and adj.array.shape[0] == x.shape[0]
    c1, b1 = tree.find(torch.from_numpy(xa).cuda())  # (n, gdim) device tensor
    c2, b2 = tree.find(x3)
    assert np.array_equal(c1.cpu().numpy(), want) and torch.equal(c1, c2)
    assert torch.equal(b1[: x.shape[0]], b2[: x.shape[0]]) and bool(torch.isnan(b1[x.shape[0]:]).all())  # identical calls
    assert np.abs(b1[: x.shape[0]].cpu().numpy() - wbary[: x.shape[0]]).max() < 1e-12
    # given cells: the same coordinates as the search found
    b3 = tree.bary(xa, c1)
    assert torch.equal(b3[: x.shape[0]], b1[: x.shape[0]]) and bool(torch.isnan(b3[x.shape[0]:]).all())
    # a tree over some cells only: the model restricted to them
    sub = np.arange(1, mesh.num_cells, 3)
    wsub, _ = PM.locate(coords, cells, xa, cell_ids=sub)
    csub, _ = G.bb_tree(mesh, d, entities=sub[::-1].copy()).find(xa)
    assert np.array_equal(csub.cpu().numpy(), wsub) and (wsub >= 0).sum() > 100


# ---- 2. polynomial exactness -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,degree", [("box2", 1), ("box2", 2), ("box2", 3), ("box3", 1), ("box3", 2), ("box3c", 3),
                                         ("delaunay", 2)])
def test_eval_is_exact_for_polynomials(hip, kind, degree):
    from oasisx_amd import fem

    mesh = _mesh(kind)
    d = mesh.gdim
    coords, cells = mesh.coords.cpu().numpy(), mesh.cells.cpu().numpy()
    x = _points(mesh, seed=degree)
    cell, _ = PM.locate(coords, cells, x)
    V = fem.FunctionSpace(mesh, degree, window=128)
    fs = [_poly(degree, d, 0.1 * i) for i in range(d)]
    # a scalar function
    u = fem.Function(V)
    u.interpolate(fs[0])
    # a block of d interleaved columns: its components, and the blocked function over it
    W = fem.VectorFunctionSpace(V, d)
    w = fem.Function(W)
    comps = [fem.Function(V, f"w{i}", w._storage, i) for i in range(d)]
    for c, f in zip(comps, fs):
        c.interpolate(f)
    exact = np.stack([_at(f, x, d) for f in fs], axis=1)
    umax = float(np.abs(exact).max())
    block = w._storage.rhost()
    cases = [("scalar", u, u._storage.rhost()[:, 0], exact[:, :1]), ("component", comps[d - 1], block[:, d - 1], exact[:, d - 1:]),
             ("blocked", w, block, exact)]
    gen = (u._storage.generation, w._storage.generation)  # (after the host check-outs of interpolate went back)
    for name, fn, dofs, ex in cases:
        model = PM.evaluate(V, dofs, x, cell)
        for how, got in (("given cells", fn.eval(x, cell)), ("located", fn.eval(x))):
            assert got.shape == model.shape == ex.shape
            dm, de = float(np.abs(got - model).max()), float(np.abs(got - ex).max())
            print(f"{kind} P{degree} {name} ({how}): |eval - model| = {dm:.3e}, |eval - polynomial| = {de:.3e}, max|u| = {umax:.3f}")
            assert dm <= 1e-12 * umax, (name, how, dm)
            assert de <= 1e-12 * umax, (name, how, de)
    assert gen == (u._storage.generation, w._storage.generation)  # evaluation is read-only
    # a cell id of -1 and a point outside: NaN rows, the others untouched
    cm = cell.copy()
    cm[::7] = -1
    got = w.eval(x, cm)
    assert np.isnan(got[::7]).all() and not np.isnan(np.delete(got, np.s_[::7], axis=0)).any()
    far = np.concatenate([x[:3], np.full((1, d), 5.0)])
    got = u.eval(far)
    assert np.isnan(got[3]).all() and not np.isnan(got[:3]).any()


# ---- 3. probes in a time loop --------------------------------------------------------------------------------------------
def _tg(kind, N, comm, steps, points=None, capacity=2, touch=False, extra=None):
    """Taylor-Green P2-P1 set up as the partition rehearsals do (tests.helpers.KRYLOV, warm start, max_iter=1); with
    ``points`` a Probes object on (u, p) is sampled after every step."""
    import oasisx_amd as ox
    from oasisx_amd import mesh as M
    from oracle import ipcs_oracle as O
    from tests.helpers import KRYLOV, on_boundary3

    nu, dt = 0.01, 0.005
    if kind == "delaunay":
        mesh = M.create_delaunay_box(comm, [[-1.0] * 3, [1.0] * 3], N, seed=4)
    else:
        mesh = M.create_box(comm, [[-1.0] * 3, [1.0] * 3], [N, N, N])
    clock = {"t": 0.0}
    fns = [O.tg_u, O.tg_v, O.tg_w]
    bcs = [[ox.DirichletBC(lambda x, f=f: f(x, clock["t"], nu), ox.LocatorMethod.GEOMETRICAL, on_boundary3)] for f in fns]
    opts = {k: dict(v, ksp_initial_guess_nonzero=True) for k, v in KRYLOV.items()}
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_u=bcs, bcs_p=[], solver_options=opts,
                                options={"sell_window": 128})
    for i, f in enumerate(fns):
        S._u2[i].interpolate(lambda x, f=f: f(x, -dt, nu))
        S._u1[i].interpolate(lambda x, f=f: f(x, 0.0, nu))
    S._p.interpolate(lambda x: O.tg_p(x, -dt / 2, nu))
    probes = ox.Probes(points, [S.u, S._p], capacity=capacity) if points is not None else None
    evals = []
    for _ in range(steps):
        clock["t"] += dt
        S.solve(dt, nu, max_iter=1)
        if probes is not None:
            probes.sample(clock["t"])
            if extra is not None:
                evals.append(extra(S, probes))
        if touch:
            S._U.dev()  # a writable hand-out between two steps
    return S, probes, evals


def test_probes_in_a_time_loop_are_read_only_and_lose_nothing(hip, caplog, tmp_path):
    caplog.set_level(logging.INFO, logger="oasisx")
    note = "u was handed out writable"
    mesh = _mesh("box3")
    x = _points(mesh, seed=9)[::4]
    steps = 5

    tokens = []

    def after(S, probes):  # Function.eval after that step
        if not tokens:
            # the first step always says it (u1 was written by interpolate, not copied from u): start listening after it
            assert S._shortcut_note
            S._shortcut_note = False
            caplog.clear()
        vals = np.concatenate([S.u.eval(x), S._p.eval(x)], axis=1)
        tokens.append(S._u_is_u1 == (S._U.generation, S._U1.generation))  # "u still is u1": the next step's free mat-vec
        return vals

    S, probes, evals = _tg("box", 8, None, steps, x, capacity=2, extra=after)
    assert tokens == [True] * steps
    assert not any(note in r.getMessage() for r in caplog.records)  # sampling (and eval) is read-only
    A = probes.array()
    assert A.shape == (steps, x.shape[0], 4) and probes.capacity >= steps and probes.n_samples == steps  # the ring grew: 2 -> 8
    assert np.allclose(probes.times, 0.005 * np.arange(1, steps + 1)) and np.array_equal(probes.local_indices, np.arange(x.shape[0]))
    for k in range(steps):  # (a) bit for bit what Function.eval gave after that step
        assert np.array_equal(A[k], evals[k]), k
    assert not np.isnan(A).any() and float(np.abs(A[-1] - A[0]).max()) > 0.0
    # (b) the same run without probes
    S0, _, _ = _tg("box", 8, None, steps)
    assert torch.equal(S._U.rdev(), S0._U.rdev()) and torch.equal(S._P.rdev(), S0._P.rdev())
    assert {k: list(v) for k, v in S.iteration_counts().items()} == {k: list(v) for k, v in S0.iteration_counts().items()}
    # (control: after the same reset the note IS logged when u is handed out writable between two steps)
    tokens.clear()
    caplog.clear()
    _tg("box", 8, None, 2, x, touch=True, extra=after)
    assert any(note in r.getMessage() for r in caplog.records)
    # save()
    probes.save(tmp_path / "probes.npz")
    z = np.load(tmp_path / "probes.npz")
    assert np.array_equal(z["values"], A) and np.array_equal(z["points"], x) and list(z["names"]) == ["u", "p"]


def test_probes_refuse_or_mark_points_outside(hip):
    import oasisx_amd as ox
    from oasisx_amd import fem

    mesh = _mesh("box2")
    u = fem.Function(fem.FunctionSpace(mesh, 2, window=128))
    u.interpolate(_poly(2, 2))
    x = np.array([[0.25, 0.5, 0.0], [3.0, 0.0, 0.0], [-1.0, 1.0, 0.0]])
    with pytest.raises(ValueError, match="no cell"):
        ox.Probes(x, u)
    pr = ox.Probes(x, u, allow_missing=True, capacity=1)
    pr.sample(0.0)
    pr.sample(1.0)
    a = pr.array()
    assert a.shape == (2, 3, 1) and np.isnan(a[:, 1]).all() and np.array_equal(a[0], a[1], equal_nan=True)
    assert np.abs(a[0, [0, 2], 0] - _at(_poly(2, 2), x[[0, 2]], 2)).max() < 1e-12


# ---- 4. mesh partitions --------------------------------------------------------------------------------------------------
def _rank_job(kind, N, comm, x, serial):
    """One rank of a partitioned job: a quadratic on its velocity space and two Taylor-Green steps, probed at ``x``."""
    import oasisx_amd as ox
    from oasisx_amd import fem

    S, probes, _ = _tg(kind, N, comm, 2, x, capacity=1)
    torch.cuda.synchronize()
    Vi = S._Vi[0][0]
    assert Vi.part is not None
    li = probes.local_indices
    A = probes.array()
    du = float(np.abs(A[:, :, :3] - serial[:, li, :3]).max()) if li.size else 0.0
    dp = float(np.abs(A[:, :, 3] - serial[:, li, 3]).max()) if li.size else 0.0
    f = _poly(2, 3)
    q = fem.Function(Vi)
    q.interpolate(f)
    pq = ox.Probes(x, q)
    pq.sample()
    assert np.array_equal(pq.local_indices, li)  # the same owner on every run
    exact = _at(f, x[li], 3)
    got = pq.array()[0, :, 0]
    model = PM.evaluate(Vi, q._storage.rhost()[:, 0], x[li], pq.cells)[:, 0]
    dq = max(float(np.abs(got - exact).max()), float(np.abs(got - model).max())) if li.size else 0.0
    # explicit cells: any local cell evaluates, a cell the rank does not hold raises
    lc = Vi.local_cells.cpu().numpy()
    cen = S._Q.mesh.coords[S._Q.mesh.cells[Vi.local_cells[:5]]].mean(dim=1).cpu().numpy()
    assert np.abs(q.eval(cen, lc[:5])[:, 0] - _at(f, cen, 3)).max() <= 1e-12 * float(np.abs(exact).max() if li.size else 1.0) + 1e-12
    others = np.setdiff1d(np.arange(S._Q.mesh.num_cells), lc)
    raised = False
    try:
        q.eval(cen[:1], others[:1])
    except ValueError:
        raised = True
    assert raised or others.size == 0
    # cells=None on a partition: NaN rows for the points of other ranks
    e = q.eval(x)[:, 0]
    mine = np.zeros(x.shape[0], dtype=bool)
    mine[li] = True
    assert np.isnan(e[~mine]).all() and np.array_equal(e[mine], got)
    return {"li": li.tolist(), "du": du, "dp": dp, "dq": dq, "umax": float(np.abs(exact).max()) if li.size else 1.0}


def _check_ranks(res, n_points):
    count = np.zeros(n_points, dtype=np.int64)
    for r in res:
        count[np.asarray(r["li"], dtype=np.int64)] += 1
    assert (count == 1).all(), np.unique(count, return_counts=True)  # every point on exactly one rank
    for r in res:
        print("rank: points %d, |u - serial| = %.3e, |p - serial| = %.3e, |q - polynomial| = %.3e" % (
            len(r["li"]), r["du"], r["dp"], r["dq"]))
        assert r["dq"] <= 1e-12 * max(x_["umax"] for x_ in res)
        assert r["du"] <= 4e-8 and r["dp"] <= 4e-7, r


@pytest.mark.parametrize("kind,N", [("box", 8), ("delaunay", 6)])
def test_eight_rank_threads_own_every_probe_once(hip, kind, N):
    from tests.helpers import run_rank_threads

    x = _points(_mesh("box3" if kind == "box" else "delaunay"), seed=2)[::2]
    G, gp, _ = _tg(kind, N, None, 2, x)
    torch.cuda.synchronize()
    serial = gp.array()
    res, _ = run_rank_threads(8, lambda comm: _rank_job(kind, N, comm, x, serial))
    _check_ranks(res, x.shape[0])
    assert sum(1 for r in res if r["li"]) >= 4  # the points are spread over the ranks


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    import torch.distributed as dist

    os.environ["OX_TRANSPORT"] = "host"
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oasisx_amd.parallel import init_comm

        comm = init_comm()
        assert comm.size == world
        x = _points(_mesh("box3"), seed=2)[::2]
        G, gp, _ = _tg("box", 8, None, 2, x)
        out[rank] = _rank_job("box", 8, comm, x, gp.array())
    finally:
        dist.destroy_process_group()


def test_two_processes_own_every_probe_once(hip):
    import torch.multiprocessing as mp

    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    assert len(out) == 2, dict(out)
    n = _points(_mesh("box3"), seed=2)[::2].shape[0]
    _check_ranks([out[0], out[1]], n)


# ---- 5. interpolation between spaces ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["box2", "box3"])
def test_interpolation_between_spaces(hip, kind):
    from oasisx_amd import fem
    from oasisx_amd import mesh as M

    mesh = _mesh(kind)
    d = mesh.gdim
    f = _poly(2, d)
    V2, V1 = fem.FunctionSpace(mesh, 2, window=128), fem.FunctionSpace(mesh, 1, window=128)
    u2 = fem.Function(V2)
    u2.interpolate(f)
    umax = float(np.abs(u2._storage.rhost()).max())
    # P2 -> P1 on the same mesh: the quadratic at the vertices
    u1 = fem.Function(V1)
    u1.interpolate(u2)
    e1 = float(np.abs(u1._storage.rhost()[:, 0] - _at(f, V1.x.cpu().numpy(), d)).max())
    # coarse P2 -> fine P2: exact for a quadratic
    fine = (M.create_rectangle(None, [[-1.0, -1.0], [1.0, 1.0]], [24, 24]) if d == 2
            else M.create_box(None, [[-1.0] * 3, [1.0] * 3], [12, 12, 12]))
    Vf = fem.FunctionSpace(fine, 2, window=128)
    uf = fem.Function(Vf)
    uf.interpolate(u2)
    ef = float(np.abs(uf._storage.rhost()[:, 0] - _at(f, Vf.x.cpu().numpy(), d)).max())
    # a blocked function onto the fine mesh
    W2, Wf = fem.VectorFunctionSpace(V2, d), fem.VectorFunctionSpace(Vf, d)
    w2, wf = fem.Function(W2), fem.Function(Wf)
    w2.interpolate(lambda x: np.stack([_poly(2, d, 0.1 * i)(x) for i in range(d)]))
    wf.interpolate(w2)
    ex = np.stack([_at(_poly(2, d, 0.1 * i), Vf.x.cpu().numpy(), d) for i in range(d)], axis=1)
    ew = float(np.abs(wf._storage.rhost() - ex).max())
    print(f"{kind}: P2 -> P1 {e1:.3e}, coarse -> fine {ef:.3e}, blocked {ew:.3e}, max|u| = {umax:.3f}")
    assert max(e1, ef, ew) <= 1e-12 * umax
    # the same space (and a twin of it): still a copy of the array
    v = fem.Function(V2)
    v.interpolate(u2)
    t = fem.Function(fem.FunctionSpace(mesh, 2, window=128))
    t.interpolate(u2)
    assert np.array_equal(v._storage.rhost(), u2._storage.rhost()) and np.array_equal(t._storage.rhost(), u2._storage.rhost())
    with pytest.raises(ValueError):
        fem.Function(Wf).interpolate(u2)  # one value into d


# ---- the demo ------------------------------------------------------------------------------------------------------------
def test_probe_demo_runs(hip, tmp_path):
    import importlib.util

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("probes_hip_demo", os.path.join(root, "demo", "probes_hip.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    out = tmp_path / "line.npz"
    probes, rows = demo.run_probes(N=16, steps=3, n_points=41, out=str(out))
    assert len(rows) == 3 and probes.array().shape == (3, 41, 3) and out.exists()
    # P2 velocity on h = 1/8: the interpolation error of cos(pi x) sin(pi y) is about (pi h)^3 / 10 ~ 6e-3; a wrong cell,
    # a wrong basis or a wrong column would be O(1)
    assert all(np.isfinite(r[1]) and np.isfinite(r[2]) and r[1] < 5e-2 for r in rows), rows
