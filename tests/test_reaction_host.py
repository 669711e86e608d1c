"""Host: the numpy model of the reacting-scalar kernels (tests/reaction_model.py) and the public classes of
oasisx_amd/reaction.py -- the order and the stability function of ROS2, the linear invariants, the validation errors and
the solver's scope guards (no library call is reached, no GPU)."""
import numpy as np
import pytest


def _abcd(k1=2.0, k2=1.0, **kw):
    """A + B -> C, C -> D."""
    import oasisx_amd as ox

    return ox.ReactionNetwork([ox.Reaction(k1, {"A": 1, "B": 1}, {"C": 1}), ox.Reaction(k2, {"C": 1}, {"D": 1})], **kw)


# ---- the scheme ----------------------------------------------------------------------------------------------------------
def test_model_reaches_order_two():
    """A + B -> C, C -> D over H = 1 from (1, 0.8, 0.1, 0): the error against the longdouble model at 4096 substeps falls,
    substeps 2, 4, ..., 32, with a last measured order above 1.7."""
    from tests.reaction_model import ReactionModel

    net = _abcd()
    assert net.species == ["A", "B", "C", "D"]
    y0 = np.array([[1.0], [0.8], [0.1], [0.0]])
    ref = ReactionModel.from_network(net, dtype=np.longdouble).step(y0, 1.0, 4096)
    m = ReactionModel.from_network(net)
    errs = [float(np.abs(m.step(y0, 1.0, n) - ref).max()) for n in (2, 4, 8, 16, 32)]
    orders = [float(np.log2(errs[i] / errs[i + 1])) for i in range(len(errs) - 1)]
    print("errors", errs, "orders", orders)
    assert all(errs[i + 1] < errs[i] for i in range(len(errs) - 1))
    assert orders[-1] > 1.7, orders


def test_model_equals_the_stability_function():
    """y' = z y, |z| <= 1: n steps give R(z/n)^n to 1e-14, R(z) = (1 + (1 - 2 g) z + (g^2 - 2 g + 1/2) z^2) / (1 - g z)^2;
    R is bounded for z -> -inf (L-stability: R -> 0)."""
    from tests.reaction_model import ReactionModel

    z = np.linspace(-1.0, 1.0, 41)
    m = ReactionModel([[1.0]], [[1]], [z])
    g = float(m.gamma)
    assert g == 1.7071067811865475  # the constant of the kernel's launcher

    def R(z):
        return (1.0 + (1.0 - 2.0 * g) * z + (g * g - 2.0 * g + 0.5) * z * z) / (1.0 - g * z) ** 2

    for n in (1, 2, 5):
        y = m.step(np.ones((1, z.size)), 1.0, n)[0]
        ref = R(z / n) ** n
        assert np.abs(y - ref).max() <= 1e-14 * np.abs(ref).max(), (n, np.abs(y - ref).max())
    big = -np.logspace(2, 12, 11)
    yb = ReactionModel([[1.0]], [[1]], [big]).step(np.ones((1, big.size)), 1.0, 1)[0]
    assert np.isfinite(yb).all() and (np.abs(yb) < 0.05).all() and abs(yb[-1]) < 1e-9, yb


def test_invariants_span_the_left_null_space_and_are_kept():
    from tests.reaction_model import ReactionModel

    net = _abcd()
    nu = net.stoichiometry()
    assert np.array_equal(nu, np.array([[-1.0, 0.0], [-1.0, 0.0], [1.0, -1.0], [0.0, 1.0]]))
    W = net.invariants()
    assert W.shape == (nu.shape[0] - np.linalg.matrix_rank(nu), nu.shape[0]) == (2, 4)
    assert np.abs(W @ nu).max() <= 1e-14
    assert np.linalg.matrix_rank(W) == 2 and np.abs(W @ W.T - np.eye(2)).max() <= 1e-14
    for w in ([1.0, -1.0, 0.0, 0.0], [1.0, 0.0, 1.0, 1.0]):  # A - B and A + C + D lie in the span
        w = np.asarray(w)
        assert np.abs(W.T @ (W @ w) - w).max() <= 1e-14
    rng = np.random.default_rng(3)
    y0 = rng.uniform(0.1, 2.0, (4, 50))
    y = ReactionModel.from_network(net).step(y0, 0.7, 3)
    drift = np.abs(W @ y - W @ y0).max()
    print("invariant drift", drift)
    assert drift <= 32 * np.finfo(np.float64).eps * np.abs(y0).max()
    # a full-rank nu has no invariant
    import oasisx_amd as ox

    assert ox.ReactionNetwork([ox.Reaction(1.0, {"A": 1}, {})]).invariants().shape == (0, 1)


def test_model_leaves_zero_rates_and_held_values_alone():
    from tests.reaction_model import ReactionModel

    rng = np.random.default_rng(5)
    y0 = rng.uniform(0.1, 2.0, (3, 10))
    k = np.where(np.arange(10) % 2 == 0, 0.0, 3.0)
    m = ReactionModel([[-1.0], [-1.0], [1.0]], [[1, 1, 0]], [k])
    held = np.zeros((3, 10), dtype=bool)
    held[0, 1] = True
    y = m.step(y0, 0.5, 2, held)
    assert np.array_equal(y[:, ::2], y0[:, ::2])
    assert y[0, 1] == y0[0, 1] and y[1, 1] != y0[1, 1]
    r = m.rates(y0)
    assert r.shape == (1, 10) and np.allclose(r[0], k * y0[0] * y0[1], rtol=1e-15, atol=0)


# ---- the public classes ----------------------------------------------------------------------------------------------------
def test_classes_are_exported_and_tables_are_right():
    import oasisx_amd as ox
    from oasisx_amd import reaction

    assert ox.Reaction is reaction.Reaction and ox.ReactionNetwork is reaction.ReactionNetwork
    assert (reaction.MAX_SPECIES, reaction.MAX_REACTIONS) == (6, 12)
    r = ox.Reaction(2.0, {"F": 1}, {"P": 1, "T": 0.25}, arrhenius=("T", 3.0))
    assert r.names() == ["F", "P", "T"] and r.orders == {"F": 1}
    net = ox.ReactionNetwork([r, ox.Reaction(1.0, {"P": 2.5}, {"F": 1}, orders={"P": 2, "T": 1})], substeps=3, splitting="lie")
    assert net.species == ["F", "P", "T"] and net.substeps == 3 and net.splitting == "lie"
    assert np.array_equal(net.stoichiometry(), np.array([[-1.0, 1.0], [1.0, -2.5], [0.25, 0.0]]))
    assert np.array_equal(net.orders(), np.array([[1, 0, 0], [0, 2, 1]]))
    assert net.arrhenius() == [(2, 3.0), (-1, 0.0)]
    assert ox.ReactionNetwork([ox.Reaction(1.0, {"A": 1})]).splitting == "strang"
    with pytest.raises(RuntimeError, match="solver"):
        net.update()


def test_validation_errors():
    import oasisx_amd as ox

    R, N = ox.Reaction, ox.ReactionNetwork
    for bad in (-1.0, float("nan"), float("inf"), "fast"):
        with pytest.raises(ValueError, match="rate"):
            R(bad, {"A": 1})
    for bad in ({"A": -1}, {"A": float("nan")}, {"A": "x"}, {"": 1}):
        with pytest.raises(ValueError):
            R(1.0, bad)
        with pytest.raises(ValueError):
            R(1.0, {"A": 1}, bad)
    with pytest.raises(TypeError):
        R(1.0, ["A"])
    with pytest.raises(ValueError, match="neither"):
        R(1.0, {}, {})
    for bad in ({"A": 4}, {"A": 1.5}):  # default orders: the reactant coefficients, integers 0..3
        with pytest.raises(ValueError, match="order"):
            R(1.0, bad)
    assert R(1.0, {"A": 1.5}, orders={"A": 2}).orders == {"A": 2}
    for bad in ({"A": 4}, {"A": -1}, {"A": 1.0}, {"A": True}):
        with pytest.raises(ValueError, match="0..3"):
            R(1.0, {"A": 1}, orders=bad)
    with pytest.raises(TypeError):
        R(1.0, {"A": 1}, orders=[1])
    for bad in ("T", ("T",), ("T", float("inf")), (3, 1.0), ("T", "hot")):
        with pytest.raises(ValueError, match="arrhenius"):
            R(1.0, {"A": 1}, arrhenius=bad)
    with pytest.raises(ValueError, match="no reactions"):
        N([])
    with pytest.raises(TypeError):
        N(["A -> B"])
    r = R(1.0, {"A": 1}, {"B": 1})
    with pytest.raises(ValueError, match="duplicate"):
        N([r, r])
    with pytest.raises(ValueError, match="duplicate"):
        N([r, R(1.0, {"A": 1}, {"B": 1.0})])
    N([r, R(2.0, {"A": 1}, {"B": 1})])  # another rate: another reaction
    for bad in ("godunov", "Strang", None):
        with pytest.raises(ValueError, match="splitting"):
            N([r], splitting=bad)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="substeps"):
            N([r], substeps=bad)
    chain = [R(1.0, {f"s{i}": 1}, {f"s{i + 1}": 1}) for i in range(6)]  # 7 species
    with pytest.raises(NotImplementedError, match="species"):
        N(chain)
    assert len(N(chain[:5]).species) == 6
    many = [R(float(i + 1), {"A": 1}, {"B": 1}) for i in range(13)]
    with pytest.raises(NotImplementedError, match="reactions"):
        N(many)
    assert len(N(many[:12]).reactions) == 12


# ---- the solver's scope guards (no library call is reached) ---------------------------------------------------------------
def _build(**kw):
    import oasisx_amd as ox
    from tests.helpers import KRYLOV, tg_mesh

    mesh = tg_mesh(2, 3, device="cpu")
    return ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_u=[[], []], bcs_p=[], solver_options=KRYLOV,
                                   **kw)


def test_construction_errors_of_the_solver():
    import oasisx_amd as ox

    net = _abcd()
    with pytest.raises(ValueError, match="without scalars"):
        _build(reactions=net)
    with pytest.raises(ValueError, match="without scalars"):
        _build(reactions=net, scalars=[])
    with pytest.raises(TypeError, match="ReactionNetwork"):
        _build(reactions=[ox.Reaction(1.0, {"A": 1})], scalars=[ox.ScalarTransport("A", diffusivity=0.1)])
    with pytest.raises(ValueError, match=r"unknown species \['C', 'D'\]"):
        _build(reactions=net, scalars=[ox.ScalarTransport(n, diffusivity=0.1) for n in "AB"])
    with pytest.raises(ValueError, match="unknown species"):
        _build(reactions=ox.ReactionNetwork([ox.Reaction(1.0, {"A": 1}, arrhenius=("T", 1.0))]),
               scalars=[ox.ScalarTransport("A", diffusivity=0.1)])
