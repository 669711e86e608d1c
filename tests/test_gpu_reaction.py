"""GPU: reacting scalars -- ``FractionalStep_AB_CN(reactions=ReactionNetwork(...))`` (oasisx_amd/reaction.py,
``ox_scalar_react`` and ``ox_reaction_rates`` of csrc/ox_reaction.hip) against the numpy model of
tests/reaction_model.py, which tests/test_reaction_host.py pins.

The yardstick of the kernel tests is not a constant: the device's distance from the longdouble model, per species and
relative to max|c_s|, is held to 8 x the float64 model's own distance from the longdouble model on the same inputs plus
64 eps.  The device differs from the float64 model only by fused multiply-adds, its ``exp`` and, at near ties, the pivot
row."""
import numpy as np
import pytest

from tests.test_gpu_scalar import TIGHT, _c, _dofs, _forms, _options, left

pytestmark = pytest.mark.gpu

MESHES = [(2, 3, 1, 16), (2, 5, 2, 121), (3, 3, 2, 343)]  # (dim, N, degree, dofs): < one wave; odd; no multiple of 64 / 256
KAPPAS = [0.1, 0.1, 0.2, 0.3, 0.3, 0.4]  # equal diffusivities share a group: columns of nc = 1, 2 and 3 blocks
EPS = np.finfo(np.float64).eps


def _problem(dim, N, deg, scalars, reactions="absent", nu=0.01, dt=0.005, solver_options=None, mesh=None, **kw):
    """The Taylor-Green set-up of tests/test_gpu_scalar.py with ``reactions=`` (left out altogether for "absent")."""
    import oasisx_amd as ox
    from oracle import ipcs_oracle as O
    from tests.helpers import on_boundary, on_boundary3, tg_mesh

    mesh = tg_mesh(dim, N) if mesh is None else mesh
    clock = {"t": 0.0}
    marker = on_boundary if dim == 2 else on_boundary3
    fns = [O.tg_u, O.tg_v, O.tg_w][:dim]
    bcs_u = [[ox.DirichletBC(lambda x, f=f: f(x, clock["t"], nu), ox.LocatorMethod.GEOMETRICAL, marker)] for f in fns]
    if reactions != "absent":
        kw["reactions"] = reactions
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", deg), ("Lagrange", 1), bcs_u=bcs_u, bcs_p=[], scalars=scalars,
                                solver_options=solver_options or _options(),
                                options={"sell_window": 256, "low_memory_version": True}, **kw)
    for i, f in enumerate(fns):
        S._u2[i].interpolate(lambda x, f=f: f(x, -dt, nu))
        S._u1[i].interpolate(lambda x, f=f: f(x, 0.0, nu))
    S._p.interpolate(lambda x: O.tg_p(x, -dt / 2.0, nu))
    return S, clock, mesh


def _X(S):
    x_v = S._Vi[0][0].x.cpu().numpy()
    X = np.zeros((3, x_v.shape[0]))
    X[: x_v.shape[1]] = x_v.T
    return X


def _set(S, name, vals, levels=(0, 1)):
    for lvl in levels:
        S.scalar(name, lvl).x.array[:] = vals


def _state(S, names, level=0):
    return np.stack([_c(S, n, level) for n in names])


def _held(S, net):
    """(species, dofs) bool: the species' own Dirichlet rows."""
    n = S._n_u
    out = np.zeros((len(net.species), n), dtype=bool)
    for s, name in enumerate(net.species):
        out[s, S._scalar_index[name][0].rows_dev.cpu().numpy()] = True
    return out


def _models(net, X):
    from tests.reaction_model import ReactionModel

    return ReactionModel.from_network(net, X), ReactionModel.from_network(net, X, dtype=np.longdouble)


def _judge(what, dev, m64, mld):
    """The yardstick of the module docstring; returns the largest ratio distance / bound."""
    from tests.reaction_model import yardstick

    d, bound = yardstick(dev, m64, mld)
    print(f"{what}: device-longdouble {np.array2string(d, precision=2)}, bound {np.array2string(bound, precision=2)}, "
          f"ratio {np.max(d / bound):.3f}")
    assert (d <= bound).all(), (what, d, bound)
    return float(np.max(d / bound))


def _kx(x):
    return 1.5 + np.sin(x[0]) * np.cos(x[1])


def _chain(S_, rng):
    """A decay chain s0 -> s1 -> ... -> (nothing) plus one bimolecular step with a per-dof rate coefficient."""
    import oasisx_amd as ox

    names = [f"s{i}" for i in range(S_)]
    rx = [ox.Reaction(rng.uniform(0.5, 3.0), {names[i]: 1}, {names[i + 1]: 1}) for i in range(S_ - 1)]
    rx.append(ox.Reaction(rng.uniform(0.5, 3.0), {names[-1]: 1}, {}))
    if S_ == 1:
        rx.append(ox.Reaction(_kx, {"s0": 2}, {}))
    elif S_ == 2:
        rx.append(ox.Reaction(_kx, {"s0": 2}, {"s1": 1}))
    else:
        rx.append(ox.Reaction(_kx, {"s0": 1, "s1": 1}, {"s2": 1}))
    return names, rx


# ---- 1. the kernel against the model -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_species", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("dim,N,deg,ndofs", MESHES)
def test_kernel_matches_the_model(hip, dim, N, deg, ndofs, n_species):
    """``scalar_react(h)`` with 1..6 species (one per template instance) spread over blocks of nc = 1, 2 and 3, substeps 1 and
    3, random positive data: every species under the yardstick, c and c_1 the same bits, and a scalar in no reaction that
    shares a block with a species bit-unchanged."""
    import oasisx_amd as ox

    rng = np.random.default_rng(100 * n_species + dim)
    names, rx = _chain(n_species, rng)
    scalars = [ox.ScalarTransport(n, diffusivity=k) for n, k in zip(names, KAPPAS)]
    scalars.append(ox.ScalarTransport("inert", diffusivity=KAPPAS[n_species - 1]))
    h = 0.3
    for substeps in (1, 3):
        net = ox.ReactionNetwork(rx, substeps=substeps)
        assert net.species == names
        S, _, _ = _problem(dim, N, deg, scalars, net)
        assert S._n_u == ndofs
        g_last, col = S._scalar_index[names[-1]]
        assert S._scalar_index["inert"][0] is g_last and g_last.nc >= 2
        if n_species >= 4:
            assert {S._scalar_index[n][0].nc for n in names} >= {1, 2}
        y0 = rng.uniform(0.1, 2.0, (n_species, ndofs))
        for n, v in zip(names, y0):
            _set(S, n, v, levels=(1,))
        inert = rng.uniform(0.1, 2.0, (2, ndofs))
        _set(S, "inert", inert[0], levels=(0,))
        _set(S, "inert", inert[1], levels=(1,))
        S.scalar_react(h)
        dev = _state(S, names)
        assert np.array_equal(dev, _state(S, names, 1))
        assert np.array_equal(_c(S, "inert"), inert[0]) and np.array_equal(_c(S, "inert", 1), inert[1])
        m64, mld = _models(net, _X(S))
        assert np.abs(dev - y0).max() > 1e-3
        _judge(f"S = {n_species}, substeps = {substeps}, {ndofs} dofs", dev, m64.step(y0, h, substeps), mld.step(y0, h, substeps))
        assert "scalar_react" in S.timings


# ---- 2. the stiff case -------------------------------------------------------------------------------------------------------
def test_stiff_case(hip):
    """A <-> B with k h = 1e6 both ways and y' = -k y with k h = 1e6: finite, within [0, max y0] up to the model's own
    undershoot, under the yardstick (W is ill-conditioned: the float64 model's own error is the measure)."""
    import oasisx_amd as ox

    k = 1e6
    net = ox.ReactionNetwork([ox.Reaction(k, {"A": 1}, {"B": 1}), ox.Reaction(k, {"B": 1}, {"A": 1}), ox.Reaction(k, {"D": 1}, {})])
    S, _, _ = _problem(2, 5, 2, [ox.ScalarTransport(n, diffusivity=0.1 * (i + 1)) for i, n in enumerate("ABD")], net)
    rng = np.random.default_rng(7)
    y0 = rng.uniform(0.0, 2.0, (3, S._n_u))
    for n, v in zip("ABD", y0):
        _set(S, n, v)
    S.scalar_react(1.0)
    dev = _state(S, "ABD")
    m64, mld = _models(net, _X(S))
    r64, rld = m64.step(y0, 1.0, 1), mld.step(y0, 1.0, 1)
    _judge("stiff", dev, r64, rld)
    under = min(0.0, float(r64.min()))
    print(f"stiff: device range [{dev.min():.3e}, {dev.max():.3e}], model undershoot {under:.3e}")
    assert np.isfinite(dev).all()
    slack = 64 * EPS * y0.max()
    assert dev.min() >= under - slack and dev.max() <= y0.max() + slack
    assert np.abs(dev[0] - dev[1]).max() <= 1e-5 * y0.max()  # A and B are at equilibrium
    assert np.abs(dev[2]).max() <= 1e-5 * y0.max()  # L-stability: the decayed species is gone


# ---- 3. bit-exact properties -------------------------------------------------------------------------------------------------
def _abc(rate=4.0, **kw):
    import oasisx_amd as ox

    return ox.ReactionNetwork([ox.Reaction(rate, {"A": 1, "B": 1}, {"C": 1})], **kw)


def _abc_scalars(bcs_a=(), **kw):
    """A (its own group: Dirichlet rows where ``bcs_a``), B and C (one group of two)."""
    import oasisx_amd as ox

    return [ox.ScalarTransport("A", diffusivity=0.03, bcs=list(bcs_a), **kw),
            ox.ScalarTransport("B", diffusivity=0.05, **kw), ox.ScalarTransport("C", diffusivity=0.05, **kw)]


def _abc_run(rate=4.0, y0=None, bcs_a=(), h=0.2, substeps=2):
    S, _, _ = _problem(3, 3, 2, _abc_scalars(bcs_a), _abc(rate, substeps=substeps))
    for n, v in zip("ABC", y0):
        _set(S, n, v)
    S.scalar_react(h)
    return S, _state(S, "ABC")


def test_bit_exact_properties(hip):
    """Two runs are bit-equal; a rate that is zero on half the dofs leaves them bit-unchanged in every species; A's Dirichlet
    rows keep their bits while B and C react there; a NaN planted in one dof of one species reaches only that dof."""
    import oasisx_amd as ox

    y0 = np.random.default_rng(11).uniform(0.1, 2.0, (3, 343))
    _, a = _abc_run(y0=y0)
    _, b = _abc_run(y0=y0)
    assert np.array_equal(a, b) and np.abs(a - y0).min() > 0.0
    half = lambda x: np.where(x[0] > 0.0, 4.0, 0.0)  # noqa: E731
    S, c = _abc_run(rate=half, y0=y0)
    off = ~(_X(S)[0] > 0.0)
    assert off.sum() > 100 and np.array_equal(c[:, off], y0[:, off]) and np.array_equal(c[:, ~off], a[:, ~off])
    S, d = _abc_run(y0=y0, bcs_a=[ox.DirichletBC(1.0, ox.LocatorMethod.GEOMETRICAL, left)])
    rows = _dofs(S._Vi[0][0].x.cpu().numpy(), left)
    assert rows.size == 49 and S._scalar_index["A"][0].nc == 1
    assert np.array_equal(d[0, rows], y0[0, rows])  # held, whatever the value
    assert np.array_equal(d[1:, rows], a[1:, rows]) and (d[1:, rows] != y0[1:, rows]).all()  # the others react with it
    free = np.setdiff1d(np.arange(343), rows)
    assert np.array_equal(d[:, free], a[:, free])
    y1 = y0.copy()
    y1[1, 200] = np.nan
    _, e = _abc_run(y0=y1)
    assert np.isnan(e[:, 200]).all()
    keep = np.arange(343) != 200
    assert np.array_equal(e[:, keep], a[:, keep])


@pytest.mark.parametrize("splitting", ["strang", "lie"])
def test_levels_are_bit_equal_after_solve(hip, splitting):
    ini = lambda x: 1.0 + 0.5 * np.cos(np.pi * x[0]) * np.cos(np.pi * x[1])  # noqa: E731
    S, clock, _ = _problem(2, 5, 2, _abc_scalars(initial=ini), _abc(splitting=splitting))
    for _ in range(2):
        clock["t"] += 0.005
        S.solve(0.005, 0.01, max_iter=1)
        assert np.array_equal(_state(S, "ABC"), _state(S, "ABC", 1))
    assert np.abs(_c(S, "C") - 1.0).max() > 1e-3


# ---- 4. invariants, Arrhenius, rates ---------------------------------------------------------------------------------------------
def test_invariants(hip):
    """A + B -> C: A + C and B + C per dof drift no more than 8 x the float64 model's drift plus 64 eps max|c|."""
    y0 = np.random.default_rng(13).uniform(0.1, 2.0, (3, 343))
    S, dev = _abc_run(y0=y0, h=0.5, substeps=3)
    net = S._reactions
    W = net.invariants()
    assert W.shape == (2, 3) and np.abs(W @ net.stoichiometry()).max() <= 1e-15
    m64, _ = _models(net, _X(S))
    r64 = m64.step(y0, 0.5, 3)
    for w in (np.array([1.0, 0.0, 1.0]), np.array([0.0, 1.0, 1.0])):
        drift = np.abs(w @ dev - w @ y0).max()
        drift64 = np.abs(w @ r64 - w @ y0).max()
        bound = 8.0 * drift64 + 64 * EPS * np.abs(y0).max()
        print(f"invariant {w}: device drift {drift:.3e}, float64 model {drift64:.3e}, bound {bound:.3e}")
        assert drift <= bound


def test_arrhenius_and_rates(hip):
    """F -> P with arrhenius=("T", Ta) and the heat release q on T against the model, and ``reaction_rates()`` before and
    after, under the yardstick; T = 0 is not guarded: what comes of it stays in its dof."""
    import oasisx_amd as ox

    Ta, q = 2.0, 0.7
    net = ox.ReactionNetwork([ox.Reaction(3.0, {"F": 1}, {"P": 1, "T": q}, arrhenius=("T", Ta)),
                              ox.Reaction(_kx, {"P": 2}, {"F": 1}, orders={"P": 2, "F": 1})], substeps=2)
    sc = [ox.ScalarTransport("F", diffusivity=0.1), ox.ScalarTransport("P", diffusivity=0.1), ox.ScalarTransport("T", diffusivity=0.2)]
    S, _, _ = _problem(2, 5, 2, sc, net)
    assert net.species == ["F", "P", "T"]
    y0 = np.random.default_rng(17).uniform(0.5, 2.0, (3, S._n_u))
    for n, v in zip(net.species, y0):
        _set(S, n, v)
    m64, mld = _models(net, _X(S))
    r = S.reaction_rates().cpu().numpy()
    assert r.shape == (2, S._n_u)
    _judge("rates before", r, m64.rates(y0), mld.rates(y0))
    S.scalar_react(0.25)
    dev = _state(S, net.species)
    _judge("arrhenius", dev, m64.step(y0, 0.25, 2), mld.step(y0, 0.25, 2))
    assert (dev[2] > y0[2]).all()  # the heat release
    _judge("rates after", S.reaction_rates().cpu().numpy(), m64.rates(dev), mld.rates(dev))
    y1 = y0.copy()
    y1[2, 5] = 0.0  # no guard: exp(-Ta / 0) = 0 and 0 / 0 in the Jacobian -- whatever comes of it stays in that dof
    for n, v in zip(net.species, y1):
        _set(S, n, v)
    S.scalar_react(0.25)
    e = _state(S, net.species)
    keep = np.arange(S._n_u) != 5
    assert np.array_equal(e[:, keep], dev[:, keep])


def test_periodic_box(hip):
    """The kernel runs per dof of the reduced space of a make_periodic mesh."""
    import oasisx_amd as ox
    from tests.test_gpu_periodic import _solver, _tg_mesh

    net = _abc(substeps=2)
    S = _solver(_tg_mesh(2, 4), 2, solver_options=_options(), scalars=_abc_scalars(), reactions=net)
    n = S._n_u
    assert n == 64  # (2 N)^2: the identified dofs are counted once
    y0 = np.random.default_rng(19).uniform(0.1, 2.0, (3, n))
    for nm, v in zip("ABC", y0):
        _set(S, nm, v)
    S.scalar_react(0.2)
    m64, mld = _models(net, _X(S))
    _judge("periodic", _state(S, "ABC"), m64.step(y0, 0.2, 2), mld.step(y0, 0.2, 2))


# ---- 5. whole steps ------------------------------------------------------------------------------------------------------------
INI = {"A": lambda x: 1.0 + 0.5 * np.cos(np.pi * x[0]) * np.cos(np.pi * x[1]),
       "B": lambda x: 0.8 + 0.3 * np.sin(np.pi * x[0]), "C": lambda x: 0.2 + 0.1 * x[1]}
KAPPA = {"A": 0.03, "B": 0.05, "C": 0.05}


@pytest.mark.parametrize("variant", ["strang", "lie", "supg", "buoyancy"])
def test_whole_steps_match_the_composed_model(hip, variant):
    """Three solves on the 2-D N = 5 P2 problem of tests/test_gpu_scalar.py with A + B -> C (A with Dirichlet rows on x = -1)
    against tests/reaction_model.whole_step composed with the scalar model, fed the device's u_ab: relative max difference
    below 1e-8 and equal iteration counts (the bounds of the scalar tests' three steps); both splittings, once with
    stabilization=SUPG(), once with buoyancy= on a species."""
    import oasisx_amd as ox
    from tests.reaction_model import ReactionModel, whole_step
    from tests.scalar_model import ScalarModel
    from tests.scalar_supg_model import ScalarSupgModel

    nu, dt = 0.01, 0.005
    splitting = "lie" if variant == "lie" else "strang"
    kw = {"stabilization": ox.SUPG()} if variant == "supg" else {}
    val = lambda x: 1.0 + 0.5 * x[1]  # noqa: E731
    scalars = [ox.ScalarTransport("A", diffusivity=KAPPA["A"], initial=INI["A"], source=0.3,
                                  bcs=[ox.DirichletBC(val, ox.LocatorMethod.GEOMETRICAL, left)], **kw),
               ox.ScalarTransport("B", diffusivity=KAPPA["B"], initial=INI["B"], **kw),
               ox.ScalarTransport("C", diffusivity=KAPPA["C"], initial=INI["C"],
                                  **(dict(kw, buoyancy=(0.0, 2.0), reference=0.2) if variant == "buoyancy" else kw))]
    net = ox.ReactionNetwork([ox.Reaction(5.0, {"A": 1, "B": 1}, {"C": 1})], substeps=2, splitting=splitting)
    so = _options(guess=True)
    S, clock, mesh = _problem(2, 5, 2, scalars, net, nu=nu, dt=dt, solver_options=so)
    assert [g.nc for g in S._scalar_groups] == [1, 2]
    assert (S._scalar_groups[1].C2 is not None) == (variant == "buoyancy")
    F, x_v = _forms(S, mesh)
    models = []
    for n in "ABC":
        a = dict(dofs=_dofs(x_v, left), value=val, source=0.3) if n == "A" else {}
        cls = ScalarSupgModel if variant == "supg" else ScalarModel
        m = cls(F, x_v, KAPPA[n], options=so["scalar_transport"], **a)
        m.interpolate(INI[n])
        models.append(m)
    rm = ReactionModel.from_network(net, _X(S))
    held = _held(S, net)
    assert held[0].sum() == 11 and not held[1:].any()
    for k in range(3):
        clock["t"] += dt
        S.solve(dt, nu, max_iter=1)
        whole_step(rm, models, S._UAB.rhost(), dt, splitting, 2, held)
        its = S.iteration_counts()["scalar_transport"]
        for n, m in zip("ABC", models):
            c = _c(S, n)
            rel = np.abs(c - m.c).max() / np.abs(m.c).max()
            print(f"{variant}, step {k}, {n}: rel diff {rel:.3e}, iterations {its[n]} (model {m.its})")
            assert m.reason > 0
            assert rel < 1e-8, (variant, k, n, rel)
            assert its[n] == m.its, (variant, k, n, its[n], m.its)
            assert np.array_equal(c, _c(S, n, 1))
    assert np.abs(_c(S, "C") - INI["C"](_X(S))).max() > 1e-3  # (it did react)


def test_uniform_fields_are_the_reaction_alone(hip):
    """Uniform fields, no Dirichlet rows: the transport step is the identity up to the solver tolerance (rtol 1e-12), so one
    solve equals the model's two half steps to 1e-9 (the bound of test_constant_is_preserved)."""
    import oasisx_amd as ox

    dt = 0.05
    y0 = {"A": 1.0, "B": 0.7, "C": 0.1}
    sc = [ox.ScalarTransport(n, diffusivity=0.1 * (i + 1), initial=y0[n]) for i, n in enumerate("ABC")]
    net = _abc(6.0, substeps=1)
    S, clock, _ = _problem(2, 5, 2, sc, net, dt=dt, solver_options=_options(TIGHT))
    clock["t"] += dt
    S.solve(dt, 0.01, max_iter=1)
    m64, _ = _models(net, _X(S))
    y = np.array([[y0[n]] for n in "ABC"])
    ref = m64.step(m64.step(y, 0.5 * dt, 1), 0.5 * dt, 1)
    d = np.abs(_state(S, "ABC") - ref).max()
    print("uniform fields: max |c - two half steps| =", d, "reacted by", np.abs(ref - y).max())
    assert d < 1e-9 and np.abs(ref - y).max() > 1e-2


# ---- 6. the calls made -----------------------------------------------------------------------------------------------------------
NEW = ("ox_scalar_react", "ox_reaction_rates")


class Counting:
    """The library with a list of the calls of the two reaction entries."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        if name in NEW:
            self.calls.append(name)
        return getattr(self._lib, name)


def test_calls_made(hip, monkeypatch):
    """Without reactions= neither new entry is called and three steps give the bits of a solver built without the argument;
    with a network ox_scalar_react is called twice per step under "strang" and once under "lie"."""
    from oasisx_amd import _lib

    nu, dt = 0.01, 0.005
    ini = INI["A"]
    out = {}
    for what, want in (("absent", []), (None, []), ("strang", ["ox_scalar_react"] * 6), ("lie", ["ox_scalar_react"] * 3)):
        rx = _abc(splitting=what) if isinstance(what, str) and what != "absent" else what
        S, clock, _ = _problem(2, 5, 2, _abc_scalars(initial=ini), rx, nu=nu, dt=dt)
        proxy = Counting(_lib.load())
        monkeypatch.setattr(_lib, "_lib", proxy)
        monkeypatch.setattr(S, "_lib", proxy)
        for _ in range(3):
            clock["t"] += dt
            S.solve(dt, nu, max_iter=1)
        monkeypatch.undo()
        assert proxy.calls == want, (what, proxy.calls)
        assert ("scalar_react" in S.timings) == bool(want)
        out[what] = (_state(S, "ABC"), S._U.rhost(), S._P.rhost())
        if not want:
            for f in (lambda: S.scalar_react(dt), S.reaction_rates):
                with pytest.raises(RuntimeError, match="without reactions"):
                    f()
    for a, b in zip(out["absent"], out[None]):
        assert np.array_equal(a, b)
    assert not np.array_equal(out["strang"][0], out[None][0]) and not np.array_equal(out["strang"][0], out["lie"][0])
    assert np.array_equal(out["strang"][1], out[None][1])  # passive species: the flow is the same flow


def test_kernels_refuse_bad_arguments(hip):
    import ctypes as C

    from oasisx_amd import _lib

    S, _, _ = _problem(2, 3, 1, _abc_scalars(), _abc())
    rx = S._reactions
    st = _lib.current_stream()
    n = int(S._n_u)

    def react(net=None, sp=None, n=n, substeps=1):
        net_, sp_ = rx._records(True)
        return hip.ox_scalar_react(C.byref(net or net_), sp or sp_, n, 0.1, substeps, st)

    def copy(**kw):
        net_, _ = rx._records(True)
        c = _lib.ox_react_net.from_buffer_copy(net_)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    assert react() == 0 and react(n=0) == 0
    assert react(substeps=0) != 0 and react(n=-1) != 0
    assert react(net=copy(S=0)) != 0 and react(net=copy(S=7)) != 0
    assert react(net=copy(R=0)) != 0 and react(net=copy(R=13)) != 0
    bad = copy()
    bad.order[0][0] = 4
    assert react(net=bad) != 0
    bad = copy()
    bad.arr[0] = 3
    assert react(net=bad) != 0
    _, sp_ = rx._records(True)
    sp = (_lib.ox_react_species * 3)()
    C.memmove(sp, sp_, C.sizeof(sp))
    sp[1].col = sp[1].nc
    assert react(sp=sp) != 0
    sp[1].col, sp[2].out = 0, None
    assert react(sp=sp) != 0
    assert hip.ox_reaction_rates(C.byref(copy()), sp_, n, None, st) != 0
