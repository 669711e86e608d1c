"""GPU: inertial particles (``oasisx_amd.InertialParticles`` / ``ox_particle_advance`` of csrc/ox_probe.hip) against closed
forms and against the numpy model of tests/particle_model.py.

Bounds.  Closed forms of a uniform field: 1e-13 relative to max(1, |value|) (the substep is the exact flow map; at most 20
substeps of a few roundings each).  Positions, velocities, ages and path lengths against the model: 1e-12 on values of
order one, the bound of the tracer tests (header of tests/test_gpu_tracers.py): point evaluation agrees with its model to
a few 1e-15 and at most 40 substeps accumulate; exp / expm1 / pow add a few ulp per substep.  Status, facet, wraps and exit
times: EQUAL on every particle; the model reports the smallest margin of every decisive test (a barycentric coordinate at
a locate decision, the gap between the two nearest facets, a folded coordinate against its box) and the seeds are such
that it is >= 1e-9 -- seven orders above the rounding differences between the device and the model.  Massless limit
against ``Tracers``: 1e-13 (the same operations in the same order; at most 12 substeps)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import particle_model as PMo
from tests import tracer_model as TM

pytestmark = pytest.mark.gpu

SCHEMES = ("exp1", "exp2")
NU, RHO = 0.01, 1000.0


def _mesh(kind):
    from oasisx_amd import mesh as M

    if kind in ("sq", "psq"):
        mesh = M.create_unit_square(None, 4, 4)
    else:
        mesh = M.create_unit_cube(None, 3, 3, 3)
    return M.make_periodic(mesh, (0,)) if kind.startswith("p") else mesh


def _space(kind, degree):
    from oasisx_amd import fem

    mesh = _mesh(kind)
    V = fem.FunctionSpace(mesh, degree, window=128)
    return mesh, V, fem.VectorFunctionSpace(V, mesh.gdim)


def _function(W, comps):
    from oasisx_amd import fem

    w = fem.Function(W)
    w.interpolate(lambda x: np.stack([c(x) + 0.0 * x[0] for c in comps]))
    w._storage.rdev()
    return w


def _uniform(W, u):
    return _function(W, [lambda x, c=c: c + 0.0 * x[0] for c in u])


def _bottom_tags(mesh, marker=lambda x: np.isclose(x[1], 0.0), value=1):
    from oasisx_amd import mesh as M

    facets = M.locate_entities_boundary(mesh, mesh.gdim - 1, marker)
    return M.meshtags(mesh, mesh.gdim - 1, facets, np.full(facets.shape[0], value, dtype=np.int32))


def _state(P):
    return (P.positions(), P.velocities(), P.status(), P.cells(), P.age(), P.path_length(), P.exit_time(), P.wraps(), P.facet())


# ---- 1. closed forms on the device -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,degree", [("sq", 1), ("cube", 2)])
def test_uniform_field_follows_the_closed_form(hip, kind, degree):
    import oasisx_amd as ox

    mesh, V, W = _space(kind, degree)
    d, h, substeps, advances = mesh.gdim, 0.02, 5, 4
    rng = np.random.default_rng(3)
    x0, v0 = rng.uniform(0.3, 0.6, (64, d)), rng.uniform(-0.2, 0.2, (64, d))
    for ratio in PMo.RATIOS:
        tau, u, g, beta = PMo.exact_case(ratio, d, h)
        w = _uniform(W, u)
        for scheme in SCHEMES:
            # beta = 1 - rho_f / rho_p = 0.75: rho_p = 4 rho_f
            P = ox.InertialParticles(w, x0, 1e-3, 4.0, fluid_density=1.0, nu=NU, gravity=g, velocities=v0, scheme=scheme,
                                     substeps=substeps, response_time=tau)
            for _ in range(advances):
                P.advance(h * substeps)
            xe, ve = PMo.closed_form(x0, v0, u, g, beta, tau, h * substeps * advances)
            ex, ev = PMo.rel_err(P.positions(), xe), PMo.rel_err(P.velocities(), ve)
            print(f"{kind} P{degree} h/tau = {ratio} {scheme}: |x - closed form| = {ex:.3e}, |v - closed form| = {ev:.3e}")
            assert (P.status() == 0).all(), (ratio, scheme)
            assert ex <= 1e-13 and ev <= 1e-13, (ratio, scheme, ex, ev)
            assert np.abs(P.age() - h * substeps * advances).max() <= 1e-14 and (P.facet() == -1).all()


# ---- 2. the device against the model -----------------------------------------------------------------------------------
def _smooth(d, amp):
    """A smooth non-polynomial field of period 1 in x (so that it lives on the periodic meshes too)."""
    two_pi = 2.0 * np.pi
    comps = [lambda x: amp * (0.3 + 0.2 * np.sin(two_pi * x[0]) * np.cos(x[1])),
             lambda x: amp * 0.15 * np.cos(two_pi * x[0]) * np.sin(1.3 * x[1] + 0.2),
             lambda x: amp * 0.1 * np.sin(two_pi * x[0] + x[2])]
    return comps[:d]


# (kind, degree) -> seed of the particles: seeds for which the model's smallest decision margin is >= 1e-9 (asserted)
MODEL_CASES = [("sq", 1, 21), ("sq", 2, 22), ("sq", 3, 23), ("cube", 1, 24), ("cube", 2, 25), ("cube", 3, 26), ("psq", 2, 27),
               ("pcube", 1, 28)]


@pytest.mark.parametrize("kind,degree,seed", MODEL_CASES)
def test_device_against_the_model(hip, kind, degree, seed):
    import oasisx_amd as ox

    mesh, V, W = _space(kind, degree)
    d = mesh.gdim
    a, b = _function(W, _smooth(d, 1.0)), _function(W, _smooth(d, 1.35))
    ua, ub = a._storage.rhost().copy(), b._storage.rhost().copy()
    rng = np.random.default_rng(seed)
    n, dt, substeps, advances = 200, 0.1, 4, 3
    x0 = rng.uniform(0.04, 0.96, (n, d))
    x0[:30, 1] = rng.uniform(0.02, 0.1, 30)  # close above the tagged wall: some of these settle on it
    x0[30:50, 0] = rng.uniform(0.9, 0.98, 20)  # close to the side x = 1: some of these leave (or wrap)
    h = dt / substeps
    tau = h * 10.0 ** rng.uniform(-3.0, 3.0, n)  # tau_p / h from 1e-3 to 1e3
    diam = np.sqrt(18.0 * NU * tau / RHO)
    g = np.array([0.0, -1.5, 0.0])[:d]
    tags = _bottom_tags(mesh)
    ids, xyz = PMo.exterior_xyz(mesh)
    action = np.isin(ids, tags.find(1)).astype(np.int32)
    v0 = PMo.Particles(TM.FEField(V, ua), TM.MeshLocator(mesh), x0, None, 0.0).v  # the constructor's field (a) at the seeds
    worst = 0.0
    for scheme in SCHEMES:
        for drag in ("stokes", "schiller_naumann"):
            P = ox.InertialParticles(a, x0, diam, RHO, fluid_density=1.0, nu=NU, gravity=g, drag=drag, scheme=scheme,
                                     substeps=substeps, walls=(tags, 1))
            Mo = PMo.Particles(TM.FEField(V, ua, ub), TM.MeshLocator(mesh), x0, v0, PMo.response_time(diam, RHO, 1.0, NU),
                               diameter=diam, beta=1.0 - 1.0 / RHO, gravity=g, nu=NU, drag=drag, scheme=scheme,
                               substeps=substeps, periodic=PMo.periodic_of(mesh), facet_xyz=xyz, action=action)
            assert float(np.abs(P.velocities() - Mo.v).max()) <= 1e-14  # the fluid velocity of level b at the seeds
            for _ in range(advances):
                P.advance(dt, a, b)
                Mo.advance(dt)
            dx = float(np.abs(P.positions() - Mo.x).max())
            dv = float(np.abs(P.velocities() - Mo.v).max())
            da = float(np.abs(P.age() - Mo.age).max())
            dp = float(np.abs(P.path_length() - Mo.path).max())
            worst = max(worst, dx, dv, da, dp)
            counts = [int((Mo.status == s).sum()) for s in range(4)]
            print(f"{kind} P{degree} {scheme} {drag}: |x - model| = {dx:.3e}, |v - model| = {dv:.3e}, |age| = {da:.3e}, "
                  f"|path| = {dp:.3e}; model margin {Mo.margin:.3e}; status counts {counts}")
            assert Mo.margin >= 1e-9, Mo.margin  # a condition on the seeds, checked on the model alone
            assert np.array_equal(P.status(), Mo.status)
            assert np.array_equal(P.facet(), np.where(Mo.facet >= 0, ids[np.clip(Mo.facet, 0, None)], -1))
            assert np.array_equal(P.wraps(), Mo.wraps) and np.array_equal(P.exit_time(), Mo.t_exit, equal_nan=True)
            assert np.array_equal(P.cells() >= 0, Mo.status == 0)
            assert dx <= 1e-12 and dv <= 1e-12 and da <= 1e-12 and dp <= 1e-12, (scheme, drag, dx, dv, da, dp)
            assert counts[3] > 0 and counts[0] > n // 2 and counts[2] == 0, counts  # some settle on the tagged wall
            if not kind.startswith("p"):
                assert counts[1] > 0, counts  # and some leave through the other sides
            assert int(P.deposition().sum()) == counts[3]
    print(f"{kind} P{degree}: largest deviation from the model {worst:.3e}")


def test_a_non_finite_velocity_gives_status_2(hip):
    import oasisx_amd as ox

    mesh, V, W = _space("sq", 1)
    w = _uniform(W, [0.1, 0.0])
    x0 = np.array([[0.3, 0.3], [0.7, 0.6]])
    P = ox.InertialParticles(w, x0, 1e-3, RHO, nu=NU, velocities=np.array([[0.0, 0.0], [np.nan, 0.0]]), substeps=2)
    P.advance(0.1)
    assert P.status().tolist() == [0, 2] and P.exit_time()[1] == 0.0 and P.cells()[1] == -1 and P.facet().tolist() == [-1, -1]
    assert np.array_equal(P.positions()[1], x0[1]) and P.age().tolist()[1] == 0.0


# ---- 3. the massless limit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,degree", [("sq", 2), ("cube", 1)])
def test_massless_particles_are_tracers(hip, kind, degree):
    import oasisx_amd as ox

    mesh, V, W = _space(kind, degree)
    d = mesh.gdim
    a, b = _function(W, _smooth(d, 1.0)), _function(W, _smooth(d, 1.35))
    x0 = np.random.default_rng(31).uniform(0.04, 0.96, (200, d))
    for scheme, rk in (("exp1", "euler"), ("exp2", "rk2")):
        P = ox.InertialParticles(a, x0, 1e-3, nu=NU, response_time=0.0, scheme=scheme, substeps=4)
        T = ox.Tracers(a, x0, scheme=rk, substeps=4)
        for _ in range(3):
            P.advance(0.1, a, b)
            T.advance(0.1, a, b)
        dx = float(np.abs(P.positions() - T.positions()).max())
        print(f"{kind} P{degree} {scheme} against {rk}: |x - tracer| = {dx:.3e}, {int((T.status() == 1).sum())} left")
        assert dx <= 1e-13 and np.array_equal(P.status(), T.status()) and (T.status() == 1).any()
        assert np.array_equal(P.exit_time(), T.exit_time(), equal_nan=True) and np.abs(P.path_length() - T.path_length()).max() <= 1e-13


# ---- 4. the periodic wrap ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["psq", "pcube"])
def test_particles_wrap_where_tracers_freeze(hip, kind):
    import oasisx_amd as ox

    mesh, V, W = _space(kind, 1)
    d = mesh.gdim
    u = np.array([1.3, 0.0, 0.0])[:d]
    w = _uniform(W, u)
    x0 = np.random.default_rng(41).uniform(0.1, 0.9, (100, d))
    dt, advances = 0.25, 10
    P = ox.InertialParticles(w, x0, 1e-3, RHO, nu=NU, scheme="exp2", substeps=2)  # (starts at the fluid velocity: stays there)
    T = ox.Tracers(w, x0, scheme="rk2", substeps=2)
    for _ in range(advances):
        P.advance(dt)
        T.advance(dt)
    end = x0 + dt * advances * u
    X, Wr = P.positions(), P.wraps()
    du = float(np.abs(P.unfolded_positions() - end).max())
    print(f"{kind}: |unfolded - closed form| = {du:.3e}, wraps {Wr[:, 0].min()}..{Wr[:, 0].max()}")
    assert (P.status() == 0).all() and du <= 1e-13  # nobody freezes
    assert np.array_equal(Wr[:, 0], np.floor(end[:, 0]).astype(np.int32)) and (Wr[:, 1:] == 0).all() and Wr[:, 0].min() >= 3
    assert (X[:, 0] >= 0.0).all() and (X[:, 0] < 1.0).all() and np.abs(P.path_length() - 1.3 * dt * advances).max() <= 1e-13
    assert (T.status() == 1).all() and (T.positions()[:, 0] < 1.0).all()  # the documented behaviour of Tracers: no wrap


# ---- 5. deposition -----------------------------------------------------------------------------------------------------
def _demo():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("particle_deposition_hip_demo", os.path.join(root, "demo", "particle_deposition_hip.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    return demo


def test_deposition_times_in_the_channel(hip):
    import oasisx_amd as ox

    demo = _demo()
    mesh, u, tags = demo.build_channel(4)
    rng = np.random.default_rng(51)
    n, g, dt, substeps, steps = 200, 2.0, 0.1, 2, 15
    x0 = np.stack([rng.uniform(0.0, 3.0, n), rng.uniform(-0.95, 0.95, n)], axis=1)
    P = ox.InertialParticles(u, x0, 0.03, RHO, nu=0.1, gravity=(0.0, -g), velocities=np.zeros_like(x0), substeps=substeps,
                             walls=(tags, 1))
    tau = float(P.response_time()[0])
    t_d = demo.deposition_time(x0[:, 1] + 1.0, tau, tau * (1.0 - 1.0 / RHO) * g)
    for _ in range(steps):
        P.advance(dt)
    T, h = dt * steps, dt / substeps
    within = t_d < T - 1e-9
    S, E = P.status(), P.exit_time()
    print(f"channel: {int(within.sum())} of {n} deposit by the closed form, {int((S == 3).sum())} on the device; "
          f"largest |exit time - t_d| = {np.abs(E[within] - t_d[within]).max():.3e} (h = {h})")
    assert 20 < within.sum() < n - 20
    assert (S[within] == ox.DEPOSITED).all() and np.isin(P.facet()[within], tags.find(1)).all()
    assert (np.abs(E[within] - t_d[within]) <= h + 1e-12).all() and (E[within] <= t_d[within] + 1e-12).all()
    assert (S[t_d > T + 1e-9] == 0).all() and (P.velocities()[S == 3] == 0.0).all()
    assert int(P.deposition().sum()) == int((S == 3).sum()) and P.deposition().shape == mesh.exterior_facets().shape
    assert P.wraps()[:, 0].max() >= 1  # the stream carried some through the seam on the way down


def test_an_outlet_lets_particles_out(hip):
    import oasisx_amd as ox
    from oasisx_amd import mesh as M

    mesh, V, W = _space("sq", 1)
    w = _uniform(W, [0.0, 0.0])
    wall = M.locate_entities_boundary(mesh, 1, lambda x: np.isclose(x[1], 0.0) & (x[0] <= 0.5 + 1e-12))
    outlet = M.locate_entities_boundary(mesh, 1, lambda x: np.isclose(x[1], 0.0) & (x[0] >= 0.5 - 1e-12))
    tags = M.meshtags(mesh, 1, np.concatenate([wall, outlet]),
                      np.concatenate([np.full(wall.shape[0], 1), np.full(outlet.shape[0], 2)]).astype(np.int32))
    rng = np.random.default_rng(52)
    x0 = np.stack([np.concatenate([rng.uniform(0.05, 0.45, 40), rng.uniform(0.55, 0.95, 40)]), rng.uniform(0.1, 0.4, 80)], axis=1)
    P = ox.InertialParticles(w, x0, 0.05, RHO, nu=0.1, gravity=(0.0, -3.0), substeps=4, walls=(tags, 1))
    for _ in range(10):
        P.advance(0.2)
    S, F = P.status(), P.facet()
    assert (S[:40] == ox.DEPOSITED).all() and np.isin(F[:40], tags.find(1)).all()
    assert (S[40:] == 1).all() and np.isin(F[40:], tags.find(2)).all()
    dep = P.deposition()
    assert int(dep.sum()) == 40 and dep[~np.isin(mesh.exterior_facets(), tags.find(1))].sum() == 0
    none = ox.InertialParticles(w, x0, 0.05, RHO, nu=0.1, gravity=(0.0, -3.0), substeps=4)  # walls=None: nothing deposits
    for _ in range(10):
        none.advance(0.2)
    assert (none.status() == 1).all() and np.array_equal(none.facet(), F) and none.deposition().sum() == 0


# ---- 6. bookkeeping ----------------------------------------------------------------------------------------------------
def _settling_run(a, b, x0, diam, tags, records=False, **kw):
    import oasisx_amd as ox

    P = ox.InertialParticles(a, x0, diam, RHO, nu=NU, gravity=(0.0, -1.5), drag="schiller_naumann", substeps=2,
                             walls=(tags, 1), **kw)
    for _ in range(4):
        P.advance(0.1, a, b)
        if records:
            P.record(capacity=2)
    return P


def test_hint_and_sorting_change_nothing_but_rounding(hip):
    mesh, V, W = _space("sq", 2)
    a, b = _function(W, _smooth(2, 1.0)), _function(W, _smooth(2, 1.35))
    rng = np.random.default_rng(61)
    x0, diam = rng.uniform(0.04, 0.96, (200, 2)), 10.0 ** rng.uniform(-4.0, -1.5, 200)
    tags = _bottom_tags(mesh)
    plain = _settling_run(a, b, x0, diam, tags, records=True, hint=True, sort_every=0)
    nohint = _settling_run(a, b, x0, diam, tags, hint=False, sort_every=0)
    srt = _settling_run(a, b, x0, diam, tags, records=True, hint=True, sort_every=1)
    dh = max(float(np.abs(plain.positions() - nohint.positions()).max()), float(np.abs(plain.velocities() - nohint.velocities()).max()))
    print(f"|hint - no hint| = {dh:.3e}; status counts {np.bincount(plain.status(), minlength=4).tolist()}")
    assert dh <= 1e-12 and np.array_equal(plain.status(), nohint.status()) and np.array_equal(plain.facet(), nohint.facet())
    assert (plain.status() == 3).any() and (plain.status() == 0).any()
    assert srt._ids is not None and not torch.equal(srt._ids, torch.arange(srt.n, device=srt._ids.device))  # it did sort
    for x, y in zip(_state(plain), _state(srt)):
        assert np.array_equal(x, y, equal_nan=True)
    for x, y in zip(plain.trajectories(), srt.trajectories()):
        assert np.array_equal(x, y, equal_nan=True)
    assert np.array_equal(plain.deposition(), srt.deposition())


def test_inject_record_save_and_load(hip, tmp_path):
    import oasisx_amd as ox

    mesh, V, W = _space("psq", 2)
    a, b = _function(W, _smooth(2, 1.0)), _function(W, _smooth(2, 1.35))
    rng = np.random.default_rng(62)
    x0, extra = rng.uniform(0.04, 0.96, (120, 2)), rng.uniform(0.2, 0.8, (30, 2))
    diam, diam2 = 10.0 ** rng.uniform(-4.0, -1.5, 120), 10.0 ** rng.uniform(-4.0, -1.5, 30)
    tags = _bottom_tags(mesh)
    kw = dict(nu=NU, gravity=(0.0, -1.5), substeps=2, walls=(tags, 1), sort_every=2)
    ref = ox.InertialParticles(a, x0, diam, RHO, **kw)
    P = ox.InertialParticles(a, x0, diam, RHO, **kw)
    for k in range(6):
        if k == 3:
            ids = P.inject(extra, diameter=diam2, density=RHO)
            assert np.array_equal(ids, np.arange(120, 150)) and (P.age()[ids] == 0.0).all()
            assert np.array_equal(P.positions()[ids], extra) and (P.status()[ids] == 0).all()
            P.save(tmp_path / "restart.npz")
        ref.advance(0.1, a, b)
        P.advance(0.1, a, b)
        P.record(capacity=2)
    for x, y in zip(_state(ref), _state(P)):  # the old particles: bit for bit what they are without the injection
        assert np.array_equal(x, y[:120], equal_nan=True)
    assert np.allclose(P.age()[120:][P.status()[120:] == 0], 0.3)
    X, Vl, S, tt = P.trajectories()
    assert X.shape == (6, 150, 2) and Vl.shape == (6, 150, 2) and S.shape == (6, 150) and P.n_records == 6
    assert np.allclose(tt, 0.1 * np.arange(1, 7))
    assert np.isnan(X[:3, 120:]).all() and np.isnan(Vl[:3, 120:]).all() and (S[:3, 120:] == -1).all()
    assert not np.isnan(X[3:]).any() and np.array_equal(X[5], P.positions()) and np.array_equal(Vl[5], P.velocities())
    assert np.array_equal(S[5], P.status())
    # restart: the state saved at the injection, loaded into a fresh object, then the same three advances
    Q = ox.InertialParticles(a, x0[:1], diam[:1], RHO, **kw)
    Q.load(tmp_path / "restart.npz")
    assert Q.n == 150 and Q.t == pytest.approx(0.3, abs=1e-15)
    for _ in range(3):
        Q.advance(0.1, a, b)
    for x, y in zip(_state(P), _state(Q)):
        assert np.array_equal(x, y, equal_nan=True)
    assert Q.t == P.t and np.array_equal(Q.deposition(), P.deposition())


def _tg_loop(steps, x0=None):
    import oasisx_amd as ox
    from tests.helpers import make_hip_problem

    nu, dt = 0.01, 0.005
    S, clock, mesh = make_hip_problem(2, 8, 2, nu, dt)
    P = None
    if x0 is not None:
        P = ox.InertialParticles(S, x0, 0.01, RHO, nu=nu, gravity=(0.0, -1.0), drag="schiller_naumann", substeps=2)
    for _ in range(steps):
        clock["t"] += dt
        S.solve(dt, nu, max_iter=1)
        if P is not None:
            gen = (S._U.generation, S._U1.generation, S._U2.generation)
            P.advance(dt)
            assert gen == (S._U.generation, S._U1.generation, S._U2.generation)
    return S, P


def test_particles_in_a_time_loop_are_read_only(hip):
    x0 = np.random.default_rng(63).uniform(-0.9, 0.9, (200, 2))
    S, P = _tg_loop(3, x0)
    S0, _ = _tg_loop(3)
    assert torch.equal(S._U.rdev(), S0._U.rdev()) and torch.equal(S._P.rdev(), S0._P.rdev())
    assert (P.status() == 0).all() and float(np.abs(P.positions() - x0).max()) > 1e-4 and abs(P.t - 0.015) < 1e-15


# ---- 7. refusals -------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    import oasisx_amd as ox
    from oasisx_amd import fem
    from oasisx_amd.parallel import MeshPartition

    mesh, V, W = _space("sq", 1)
    w = _uniform(W, [0.1, 0.0])
    x = np.array([[0.3, 0.3], [0.6, 0.6]])
    for diameter, density, kw in ((-1e-3, RHO, {}), (np.nan, RHO, {}), (1e-3, -RHO, {}), (1e-3, np.inf, {}), (1e-3, 0.0, {}),
                                  (1e-3, None, {}), (1e-3, RHO, dict(nu=-0.1)), (1e-3, RHO, dict(nu=np.nan)),
                                  (1e-3, RHO, dict(scheme="rk4")), (1e-3, RHO, dict(drag="newton")), (1e-3, RHO, dict(substeps=0)),
                                  ([1e-3] * 3, RHO, {}), (1e-3, None, dict(response_time=-1.0))):
        with pytest.raises(ValueError):
            ox.InertialParticles(w, x, diameter, density, **{"nu": NU, **kw})
    with pytest.raises(ValueError, match="density <= 0"):
        ox.InertialParticles(w, x, 1e-3, 0.0, nu=NU)
    with pytest.raises(ValueError, match="no cell"):
        ox.InertialParticles(w, np.array([[1.5, 0.5]]), 1e-3, RHO, nu=NU)
    with pytest.raises(ValueError, match="not exterior"):
        ox.InertialParticles(w, x, 1e-3, RHO, nu=NU, walls=np.setdiff1d(np.arange(40), mesh.exterior_facets())[:2])
    assert ox.InertialParticles(w, x, 1e-3, nu=NU, response_time=0.0).response_time().tolist() == [0.0, 0.0]
    with pytest.raises(TypeError):
        ox.InertialParticles(fem.Function(V), x, 1e-3, RHO, nu=NU)
    hi = fem.Function(fem.functionspace(mesh, ("Lagrange", 4)))
    with pytest.raises(NotImplementedError):
        ox.InertialParticles(hi, x, 1e-3, RHO, nu=NU)
    Vp = fem.FunctionSpace(mesh, 1, window=64, part=MeshPartition(mesh, 0, 2))
    with pytest.raises(NotImplementedError, match="mesh partition"):
        ox.InertialParticles(fem.Function(fem.VectorFunctionSpace(Vp, 2)), x, 1e-3, RHO, nu=NU)
    P = ox.InertialParticles(w, x, 1e-3, RHO, nu=NU)
    with pytest.raises(ValueError):
        P.advance(float("nan"))
    with pytest.raises(ValueError):
        P.advance(0.1, w)
    empty = ox.InertialParticles(w, np.zeros((0, 2)), 1e-3, RHO, nu=NU)
    empty.advance(0.1)  # n == 0: nothing is launched
    assert empty.n == 0 and empty.deposition().sum() == 0


# ---- 8. the demo -------------------------------------------------------------------------------------------------------
def test_particle_deposition_demo_runs(hip, tmp_path, capsys):
    out = tmp_path / "deposition.vtu"
    s = _demo().main(["-N", "4", "--steps", "20", "--dt", "0.1", "--seeds", "64", "--out", str(out)])
    text = capsys.readouterr().out
    assert "PASS" in text and "mean streamwise distance" in text and out.exists()
    assert s["ok"] and 0 < s["deposited"] < 64 and s["late"] <= s["h"] + 1e-9 and int(s["deposition"].sum()) == s["deposited"]
