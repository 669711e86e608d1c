"""GPU: Lagrangian tracers (``oasisx_amd.Tracers`` / ``ox_tracer_advance`` of csrc/ox_probe.hip) against closed-form
trajectories on fields the finite-element space holds exactly and against the numpy model of tests/tracer_model.py.

Bounds.  Positions, ages and path lengths against the model: 1e-12 on values of order one -- point evaluation agrees
with its model to a few 1e-15 (tests/test_gpu_probes.py) and at most 40 substeps of four stages accumulate; a wrong cell,
basis, level or weight is an error of the order of h = 0.05 or larger.  Two levels on one step: 1e-14 (one to four
substeps of exactly represented constants).  Frozen positions: 1e-13 (at most eight substeps of a constant field).
Status vectors and exit times: equal, on seeds none of whose located points comes within 1e-6 of the boundary."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import probe_model as PM
from tests import tracer_model as TM

pytestmark = pytest.mark.gpu

SCHEMES = ("euler", "rk2", "rk4")


def _mesh(kind):
    from oasisx_amd import mesh as M

    if kind == "box2":
        return M.create_rectangle(None, [[-1.0, -1.0], [1.0, 1.0]], [8, 8])
    if kind == "box3":
        return M.create_box(None, [[-1.0] * 3, [1.0] * 3], [4, 4, 4])
    return M.create_delaunay_box(None, [[-1.0] * 3, [1.0] * 3], 6, seed=4)


def _space(kind, degree):
    from oasisx_amd import fem

    mesh = _mesh(kind)
    V = fem.FunctionSpace(mesh, degree, window=128)
    return mesh, V, fem.VectorFunctionSpace(V, mesh.gdim)


def _function(W, comps):
    """A blocked Function whose component i interpolates comps[i] (x of shape (3, n) -> (n,))."""
    from oasisx_amd import fem

    w = fem.Function(W)
    w.interpolate(lambda x: np.stack([c(x) + 0.0 * x[0] for c in comps]))
    return w


def _seeds(d, n, lo, hi, seed):
    return np.random.default_rng(seed).uniform(lo, hi, (n, d))


# field name -> (v(x (n, d), theta) -> (n, d), components for interpolation, lowest degree, seeds, dt per advance, substeps
# per advance, advances, closed form x(T) of (x0, T) or None)
def _fields(d):
    zero = lambda x: 0.0 * x[0]  # noqa: E731
    uni = np.array([0.2, -0.15, 0.1])[:d]
    disc = _seeds(d, 600, -0.8, 0.8, 1)
    disc = disc[np.hypot(disc[:, 0], disc[:, 1]) <= 0.8][:500]
    strip = _seeds(d, 500, -0.9, 0.9, 2)
    strip[:, 0] = -0.9 + 0.2 * (strip[:, 0] + 0.9)  # x0 in [-0.9, -0.54]: x0 + 1.2 (1 - y0^2) stays below 0.7

    def rot(x, th):
        v = np.zeros_like(x)
        v[:, 0], v[:, 1] = -x[:, 1], x[:, 0]
        return v

    def shift(f):  # x(T) = x0 + T f(y0) e_x
        def exact(x0, T):
            x = x0.copy()
            x[:, 0] += T * f(x0[:, 1])
            return x
        return exact

    def along_x(f):
        def v(x, th):
            out = np.zeros_like(x)
            out[:, 0] = f(x[:, 1])
            return out
        return v

    pois = lambda y: 1.0 - y * y  # noqa: E731
    cubic = lambda y: 0.5 + 0.4 * y ** 3 - 0.3 * y * y  # noqa: E731
    return {
        "uniform": (lambda x, th: np.broadcast_to(uni, x.shape).copy(), [lambda x, c=c: c + 0.0 * x[0] for c in uni], 1,
                    _seeds(d, 500, -0.5, 0.5, 3), 0.5, 10, 4, lambda x0, T: x0 + T * uni),
        "rotation": (rot, [lambda x: -x[1], lambda x: x[0], zero][:d], 1, disc, 0.5, 10, 4, None),
        "poiseuille": (along_x(pois), [lambda x: pois(x[1]), zero, zero][:d], 2, strip, 0.4, 8, 3, shift(pois)),
        "cubic shear": (along_x(cubic), [lambda x: cubic(x[1]), zero, zero][:d], 3, strip, 0.4, 8, 3, shift(cubic)),
    }


# ---- 1. exact fields -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,degree", [("box2", 1), ("box2", 2), ("box2", 3), ("box3", 1), ("box3", 2), ("box3", 3),
                                         ("delaunay", 2)])
def test_exact_fields_follow_the_closed_forms_and_the_model(hip, kind, degree):
    import oasisx_amd as ox

    mesh, V, W = _space(kind, degree)
    d = mesh.gdim
    coords, cells = mesh.coords.cpu().numpy(), mesh.cells.cpu().numpy()
    box = TM.BoxLocator([-1.0] * d, [1.0] * d)  # (the mesh fills the box and no particle leaves: the model needs no cells)
    worst = 0.0
    for name, (v, comps, min_degree, x0, dt, substeps, advances, exact) in _fields(d).items():
        if degree < min_degree:
            continue
        w = _function(W, comps)
        w._storage.rdev()  # (the host check-out of interpolate goes back)
        gen = w._storage.generation
        for scheme in SCHEMES:
            T = ox.Tracers(w, x0, scheme=scheme, substeps=substeps)
            Mo = TM.Tracers(TM.AnalyticField(v), box, x0, scheme=scheme, substeps=substeps)
            for _ in range(advances):
                T.advance(dt)
                Mo.advance(dt)
            X, total = T.positions(), dt * advances
            dx = float(np.abs(X - Mo.x).max())
            da = float(np.abs(T.age() - total).max())
            dp = float(np.abs(T.path_length() - Mo.path).max())
            de = float(np.abs(X - exact(x0, total)).max()) if exact is not None else float("nan")
            worst = max(worst, dx, dp)
            print(f"{kind} P{degree} {name} {scheme}: |x - model| = {dx:.3e}, |age - T| = {da:.3e}, |path - model| = {dp:.3e}, "
                  f"|x - closed form| = {de:.3e}")
            assert (Mo.status == 0).all() and (T.status() == 0).all(), (name, scheme)
            assert dx <= 1e-12 and da <= 1e-12 and dp <= 1e-12, (name, scheme, dx, da, dp)
            assert np.isnan(T.exit_time()).all() and abs(T.t - total) <= 1e-15
            if exact is not None:
                assert de <= 1e-12, (name, scheme, de)
            elif scheme == "rk4":  # the rotation by `total` radians, to RK4's truncation error: T r h^4 / 120 < 1e-7
                c, s = np.cos(total), np.sin(total)
                R = x0.copy()
                R[:, 0], R[:, 1] = c * x0[:, 0] - s * x0[:, 1], s * x0[:, 0] + c * x0[:, 1]
                assert float(np.abs(X - R).max()) <= 1e-7
            cell = T.cells()
            assert (cell >= 0).all() and (cell < mesh.num_cells).all()
            assert TM.cell_barycentric(coords, cells, cell, X).min() >= -T.tol, (name, scheme)
        assert w._storage.generation == gen  # advancing reads
    print(f"{kind} P{degree}: largest deviation from the model {worst:.3e}")


# ---- 2. two time levels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["box2", "box3"])
def test_two_time_levels_blend_by_theta(hip, kind):
    import oasisx_amd as ox

    mesh, V, W = _space(kind, 1)
    d = mesh.gdim
    zero = lambda x: 0.0 * x[0]  # noqa: E731
    a = _function(W, [lambda x: 1.0 + 0.0 * x[0], zero, zero][:d])
    b = _function(W, [lambda x: 3.0 + 0.0 * x[0], zero, zero][:d])
    x0 = _seeds(d, 500, -0.9, 0.9, 5)
    x0[:, 0] = -0.9 + 0.2 * (x0[:, 0] + 0.9)
    dt = 0.2
    ua, ub = a._storage.rhost(), b._storage.rhost()
    for scheme in SCHEMES:
        for m in (1, 4):
            T = ox.Tracers(a, x0, scheme=scheme, substeps=m)
            T.advance(dt, a, b)
            Mo = TM.Tracers(TM.FEField(V, ua, ub), TM.MeshLocator(mesh), x0, scheme=scheme, substeps=m)
            Mo.advance(dt)
            move = 2.0 * dt if scheme != "euler" else dt * (1.0 + (m - 1.0) / m)
            X = T.positions()
            dc = float(np.abs(X[:, 0] - (x0[:, 0] + move)).max())
            dm = float(np.abs(X - Mo.x).max())
            print(f"{kind} {scheme} substeps {m}: |x - closed form| = {dc:.3e}, |x - model| = {dm:.3e}")
            assert dc <= 1e-14 and dm <= 1e-14 and np.array_equal(X[:, 1:], x0[:, 1:]), (scheme, m, dc, dm)
            assert (T.status() == 0).all() and np.abs(T.path_length() - move).max() <= 1e-14
    T = ox.Tracers(a, x0)
    with pytest.raises(ValueError):
        T.advance(dt, a)  # one level only
    with pytest.raises(ValueError):
        T.advance(float("nan"))
    other = _function(_space(kind, 1)[2], [zero] * d)
    with pytest.raises(ValueError):
        T.advance(dt, a, other)  # another space


# ---- 3. leaving the mesh -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,degree", [("box2", 2), ("box3", 1)])
def test_particles_that_leave_freeze_inside_with_their_exit_time(hip, kind, degree):
    import oasisx_amd as ox

    mesh, V, W = _space(kind, degree)
    d = mesh.gdim
    coords, cells = mesh.coords.cpu().numpy(), mesh.cells.cpu().numpy()
    vel = np.array([1.0, 0.3, 0.2])[:d]
    w = _function(W, [lambda x, c=c: c + 0.0 * x[0] for c in vel])
    x0 = _seeds(d, 1000, -0.9, 0.9, 12)  # (this seed keeps every located point 2e-5 or more from the boundary planes)
    gap = [np.inf]

    def watch(p):  # the distance of every coordinate of every located point from the planes of the boundary
        gap[0] = min(gap[0], float(np.abs(np.abs(p) - 1.0).min()))

    Mo = TM.Tracers(TM.FEField(V, w._storage.rhost()), TM.MeshLocator(mesh), x0, scheme="rk4", substeps=2, watch=watch)
    T = ox.Tracers(w, x0, scheme="rk4", substeps=2)
    dt, advances = 0.25, 4
    for _ in range(advances):
        T.advance(dt)
        Mo.advance(dt)
    assert gap[0] > 1e-6, gap  # a condition on the seeds: no decision of the model is closer than this to the boundary
    gone = Mo.status == 1
    print(f"{kind}: {int(gone.sum())} of {x0.shape[0]} particles left, closest located point {gap[0]:.3e} from the boundary")
    assert x0.shape[0] / 3 <= gone.sum() <= 2 * x0.shape[0] / 3 and (Mo.status[~gone] == 0).all()
    S, X, E = T.status(), T.positions(), T.exit_time()
    assert np.array_equal(S, Mo.status)
    assert np.array_equal(E, Mo.t_exit, equal_nan=True) and not np.isnan(E[gone]).any() and np.isnan(E[~gone]).all()
    assert float(np.abs(X - Mo.x).max()) <= 1e-13
    assert not np.isnan(X).any() and not np.isnan(T.age()).any() and not np.isnan(T.path_length()).any()
    assert (PM.locate(coords, cells, X)[0] >= 0).all()  # frozen or not: inside the mesh
    assert np.array_equal(T.cells() >= 0, ~gone) and (T.cells()[gone] == -1).all()
    assert np.abs(T.age() - Mo.age).max() <= 1e-13 and np.abs(T.path_length() - Mo.path).max() <= 1e-13
    assert (T.age()[gone] < dt * advances).all() and np.allclose(T.age()[gone], E[gone])  # age stops at the exit time
    before = (X.copy(), T.age(), T.path_length(), E.copy(), S.copy())
    T.advance(dt)
    after = (T.positions(), T.age(), T.path_length(), T.exit_time(), T.status())
    for b, a in zip(before, after):
        assert np.array_equal(b[gone], a[gone], equal_nan=True)
    # seeds outside the mesh
    out = np.concatenate([x0[:3], np.full((1, d), 1.5), np.full((1, d), np.nan)])
    with pytest.raises(ValueError, match="no cell"):
        ox.Tracers(w, out)
    T2 = ox.Tracers(w, out, allow_missing=True)
    assert T2.status().tolist() == [0, 0, 0, 1, 1] and T2.cells()[3:].tolist() == [-1, -1]
    T2.advance(0.01)
    assert T2.status().tolist() == [0, 0, 0, 1, 1] and np.array_equal(T2.positions()[3:], out[3:], equal_nan=True)
    assert T2.exit_time()[3:].tolist() == [0.0, 0.0] and (T2.age()[3:] == 0.0).all()


# ---- 4. hint and sorting ---------------------------------------------------------------------------------------------
def _rotation_run(w, x0, records=False, **kw):
    import oasisx_amd as ox

    T = ox.Tracers(w, x0, scheme="rk4", substeps=10, **kw)
    for _ in range(4):
        T.advance(0.5)
        if records:
            T.record(capacity=2)
    return T


def _state(T):
    return (T.positions(), T.status(), T.cells(), T.age(), T.path_length(), T.exit_time())


@pytest.mark.parametrize("kind,degree", [("box2", 2), ("box3", 2)])
def test_hint_and_sorting_change_nothing_but_rounding(hip, kind, degree):
    mesh, V, W = _space(kind, degree)
    d = mesh.gdim
    _, comps, _, x0, *_ = _fields(d)["rotation"]
    w = _function(W, comps)
    plain = _rotation_run(w, x0, records=True, hint=True, sort_every=0)
    again = _rotation_run(w, x0, records=True, hint=True, sort_every=0)
    nohint = _rotation_run(w, x0, hint=False)
    srt = _rotation_run(w, x0, records=True, hint=True, sort_every=1)
    srt3 = _rotation_run(w, x0, hint=True, sort_every=3)
    dh = float(np.abs(plain.positions() - nohint.positions()).max())
    print(f"{kind} P{degree}: |hint - no hint| = {dh:.3e}")
    assert dh <= 1e-12 and (nohint.status() == 0).all()
    assert srt._ids is not None and not torch.equal(srt._ids, torch.arange(srt.n, device=srt._ids.device))  # it did sort
    for other in (again, srt, srt3):
        for a, b in zip(_state(plain), _state(other)):
            assert np.array_equal(a, b, equal_nan=True)
    for other in (again, srt):
        for a, b in zip(plain.trajectories(), other.trajectories()):
            assert np.array_equal(a, b)
    nh2 = _rotation_run(w, x0, hint=False, sort_every=2)
    assert np.array_equal(nohint.positions(), nh2.positions())


# ---- 5. inject and record --------------------------------------------------------------------------------------------
def test_inject_and_record(hip, tmp_path):
    import oasisx_amd as ox

    mesh, V, W = _space("box2", 2)
    _, comps, _, x0, *_ = _fields(2)["rotation"]
    w = _function(W, comps)
    extra = _seeds(2, 100, -0.5, 0.5, 11)
    ref = ox.Tracers(w, x0, substeps=5)
    T = ox.Tracers(w, x0, substeps=5, sort_every=2)
    snaps, times = [], []
    for k in range(6):
        if k == 3:
            ids = T.inject(extra)
            assert np.array_equal(ids, np.arange(x0.shape[0], x0.shape[0] + 100))
            assert (T.age()[ids] == 0.0).all() and np.array_equal(T.positions()[ids], extra) and (T.status()[ids] == 0).all()
        ref.advance(0.25)
        T.advance(0.25)
        T.record(capacity=2)
        snaps.append(T.positions())
        times.append(T.t)
    n0 = x0.shape[0]
    for a, b in zip(_state(ref), _state(T)):  # the old particles: bit for bit what they are without the injection
        assert np.array_equal(a, b[:n0], equal_nan=True)
    assert np.allclose(T.age()[n0:], 0.75) and np.allclose(T.age()[:n0], 1.5)
    X, S, tt = T.trajectories()
    assert X.shape == (6, n0 + 100, 2) and S.shape == (6, n0 + 100) and T.n_records == 6  # the ring grew: 2 -> 4 -> 8
    assert np.array_equal(tt, np.asarray(times)) and np.allclose(tt, 0.25 * np.arange(1, 7))
    for k in range(6):
        if k < 3:  # before the injection: the later particles are not there yet
            assert np.isnan(X[k, n0:]).all() and (S[k, n0:] == -1).all()
            assert np.array_equal(X[k, :n0], snaps[k]) and (S[k, :n0] == 0).all()
        else:
            assert np.array_equal(X[k], snaps[k]) and (S[k] == 0).all()
    T.save(tmp_path / "tracers.npz")
    z = np.load(tmp_path / "tracers.npz")
    assert np.array_equal(z["positions"], X, equal_nan=True) and np.array_equal(z["final_positions"], T.positions())
    assert np.array_equal(z["times"], tt) and np.array_equal(z["age"], T.age()) and float(z["t"]) == T.t


# ---- 6. in a time loop -----------------------------------------------------------------------------------------------
def _tg_loop(dim, N, u_deg, steps, x0=None):
    """Taylor-Green with ``steps`` steps; with seeds a Tracers object on the solver advanced after every solve and the
    model fed that step's host copies of u^n and u^{n+1}."""
    import oasisx_amd as ox
    from tests.helpers import make_hip_problem

    nu, dt = 0.01, 0.005
    S, clock, mesh = make_hip_problem(dim, N, u_deg, nu, dt)
    Vs = S._Vi[0][0]
    T = Mo = None
    if x0 is not None:
        T = ox.Tracers(S, x0, scheme="rk4", substeps=2)
        Mo = TM.Tracers(None, TM.MeshLocator(mesh), x0, scheme="rk4", substeps=2)
    dev, tokens = [], []
    for k in range(steps):
        clock["t"] += dt
        S.solve(dt, nu, max_iter=1)
        if T is not None:
            gen = (S._U.generation, S._U1.generation, S._U2.generation)
            T.advance(dt)
            assert gen == (S._U.generation, S._U1.generation, S._U2.generation)
            tokens.append(S._u_is_u1 == (S._U.generation, S._U1.generation))
            Mo.advance(dt, TM.FEField(Vs, S._U2.rhost(), S._U1.rhost()))
            dev.append(float(np.abs(T.positions() - Mo.x).max()))
    return S, T, Mo, dev, tokens


@pytest.mark.parametrize("dim,N,u_deg,steps", [(2, 8, 2, 5), (3, 4, 1, 3)])
def test_tracers_in_a_time_loop_are_read_only(hip, dim, N, u_deg, steps):
    x0 = _seeds(dim, 500, -0.9, 0.9, 13)
    S, T, Mo, dev, tokens = _tg_loop(dim, N, u_deg, steps, x0)
    print(f"{dim}-D TG: |x - model| after each step = {['%.2e' % v for v in dev]}")
    assert tokens == [True] * steps  # "u still is u1" survives every advance
    assert max(dev) <= 1e-12 and (T.status() == 0).all() and (Mo.status == 0).all()
    assert float(np.abs(T.positions() - x0).max()) > 1e-4 and abs(T.t - 0.005 * steps) < 1e-15  # they did move
    S0, *_ = _tg_loop(dim, N, u_deg, steps)
    assert torch.equal(S._U.rdev(), S0._U.rdev()) and torch.equal(S._P.rdev(), S0._P.rdev())
    assert {k: list(v) for k, v in S.iteration_counts().items()} == {k: list(v) for k, v in S0.iteration_counts().items()}


# ---- 7. the demo -----------------------------------------------------------------------------------------------------
def test_tracer_demo_runs(hip, tmp_path, capsys):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("tracers_hip_demo", os.path.join(root, "demo", "tracers_hip.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    out = tmp_path / "tracers.npz"
    s = demo.main(["-N", "8", "--steps", "40", "--dt", "0.05", "--every", "10", "--seeds", "32", "--out", str(out)])
    line = capsys.readouterr().out
    assert "exited" in line and "residence time" in line and out.exists()
    # 4 x 32 particles; the centre line moves at 1.5 and leaves the 1.9 left of the channel within the 2.0 of the run
    assert s["n"] == 128 and s["invalid"] == 0 and 0 < s["exited"] < 128 and 1.0 < s["mean"] <= s["max"] <= 2.0, s
    z = np.load(out)
    assert z["positions"].shape[1:] == (128, 2) and z["status"].shape[1] == 128
