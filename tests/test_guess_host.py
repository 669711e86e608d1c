"""CPU: ksp_guess_type fischer -- how KSPSolver resolves the options (fake operators), and the numpy model of the
projected initial guesses (tests/guess_model.py): the guess against the Gram-system projection, A-orthonormality, the
restart and skip rules, and a replay of the oracle's Taylor-Green velocity updates."""
import logging

import numpy as np
import pytest
import scipy.sparse as sp

from oasisx_amd.ksp import KSPSolver, fischer_model
from oracle import ipcs_oracle as O
from tests.guess_model import FischerModel, projected_guess

CG = {"ksp_type": "cg", "pc_type": "jacobi", "ksp_rtol": 1e-8, "ksp_guess_type": "fischer"}


class _Comm:
    size = 1


def _op(symmetric=True, partitioned=False):
    class _Pattern:
        dist = object() if partitioned else None
        n_rows = 10

    class _Op:
        pattern = _Pattern()

    o = _Op()
    o.symmetric = symmetric
    return o


def _audit(caplog, opts, nc=1, **op):
    ksp = KSPSolver(_Comm(), dict(opts))
    ksp.setOperators(_op(**op))
    with caplog.at_level(logging.WARNING, logger="oasisx"):
        caplog.clear()
        ksp._audit_options(nc)
    return ksp, [r.getMessage() for r in caplog.records if r.levelno >= logging.WARNING]


@pytest.mark.parametrize("extra,partitioned,nc", [
    ({}, False, 1),
    ({}, False, 3),
    ({"pc_type": "none"}, False, 2),
    ({"pc_type": "gamg"}, False, 1),
    ({"pc_type": "bjacobi", "sub_pc_type": "gamg"}, True, 1),
    ({"ksp_cg_single_reduction": 1, "ksp_guess_fischer_model": "2,4"}, True, 3),
])
def test_fischer_with_cg_is_honoured_silently(caplog, extra, partitioned, nc):
    ksp, warned = _audit(caplog, dict(CG, **{"ksp_guess_fischer_model": "1,10", **extra}), nc=nc, partitioned=partitioned)
    assert ksp._guess_on()
    assert warned == []


@pytest.mark.parametrize("opts,op,needle", [
    ({"ksp_guess_type": "pod"}, {}, "ksp_guess_type=pod is not available on the device (fischer is): ignored"),
    ({"ksp_guess_fischer_model": "3,4"}, {}, "model 3 is not available: runs model 1"),
    ({"ksp_guess_fischer_model": "1,0"}, {}, "size 0 is clamped to 1 (1..32)"),
    ({"ksp_guess_fischer_model": (1, 64)}, {}, "size 64 is clamped to 32 (1..32)"),
    ({"ksp_guess_fischer_model": "ten"}, {}, "is not 'model,size': runs 1,10"),
    ({"ksp_type": "bcgs"}, {}, "applies to CG on an operator flagged symmetric only (here: BiCGStab"),
    ({}, {"symmetric": False}, "(here: CG, a non-symmetric operator): ignored"),
    ({"ksp_type": "gmres"}, {"symmetric": False}, "(here: BiCGStab, a non-symmetric operator): ignored"),
    ({"ksp_type": "preonly", "pc_type": "lu"}, {}, "a direct solve takes no initial guess: ignored"),
])
def test_fischer_reports(caplog, opts, op, needle):
    ksp, warned = _audit(caplog, dict(CG, **opts), **op)
    hits = [w for w in warned if "ksp_guess" in w]
    assert len(hits) == 1 and needle in hits[0], warned
    with caplog.at_level(logging.WARNING, logger="oasisx"):  # once per solver
        caplog.clear()
        ksp._audit_options(1)
    assert "ksp_guess" not in caplog.text


def test_fischer_model_parsing():
    assert fischer_model("2,5") == fischer_model((2, 5)) == fischer_model([2, 5]) == fischer_model(" (2, 5) ") == (2, 5, None)
    assert fischer_model(None) == (1, 10, None)
    assert fischer_model("3,4")[:2] == (1, 4)
    assert fischer_model("1,40")[:2] == (1, 32)
    assert fischer_model("2,-1")[:2] == (2, 1)


def test_no_guess_without_the_option():
    ksp = KSPSolver(_Comm(), {"ksp_type": "cg"})
    ksp.setOperators(_op())
    assert not ksp._guess_on() and ksp.guess_dim == 0


# ---- the numpy model ------------------------------------------------------------------------------------------------
def _spd(n=60, seed=0):
    rng = np.random.default_rng(seed)
    Q = sp.random(n, n, density=0.1, random_state=seed) + sp.eye(n) * 3.0
    return (Q @ Q.T + sp.eye(n)).tocsr(), rng


@pytest.mark.parametrize("model", [1, 2])
@pytest.mark.parametrize("warm", [False, True])
def test_guess_is_the_projection_and_basis_is_orthonormal(model, warm):
    A, rng = _spd()
    n, nc = A.shape[0], 2
    G = FischerModel(A, nc=nc, model=model, size=5)
    for step in range(7):
        b = rng.standard_normal((n, nc))
        xw = rng.standard_normal((n, nc)) if warm else None
        x0 = G.form(b, xw)
        if G.k == 0:
            assert x0 is None
        else:
            for c in range(nc):
                X = G.basis(c)
                ref = projected_guess(A, X, b[:, c], np.zeros(n) if xw is None else xw[:, c])
                assert np.abs(x0[:, c] - ref).max() <= 1e-12 * np.abs(ref).max()
        x = np.stack([sp.linalg.spsolve(A.tocsc(), b[:, c]) for c in range(nc)], axis=1)
        k_before = G.k
        G.update(x)
        assert G.k == (1 if k_before == 5 else k_before + 1)
        for c in range(nc):
            X = G.basis(c)
            assert np.abs(X.T @ (A @ X) - np.eye(G.k)).max() < 1e-10


def test_restart_and_skip_rules():
    A, rng = _spd(40, seed=1)
    n = A.shape[0]
    G = FischerModel(A, nc=1, model=1, size=3)
    s = rng.standard_normal((n, 2))
    xs = [s[:, 0], s[:, 1], s[:, 0] + 2.0 * s[:, 1]]  # the third lies in the span of the first two
    for x in xs:  # (no guess formed: d = x itself is orthogonalised)
        G.update(x.copy())
    assert G.k == 3
    assert G.sigma[0][0] > 0 and G.sigma[1][0] > 0 and G.sigma[2][0] == 0.0  # skip rule: a zero slot
    X = G.basis(0)
    assert np.all(X[:, 2] == 0.0)
    # the guess for anything in the span is exact, the zero slot contributes nothing
    x = 3.0 * s[:, 0] - s[:, 1]
    x0 = G.form(A @ x)
    assert np.abs(x0[:, 0] - x).max() < 1e-10 * np.abs(x).max()
    # restart: a full basis is replaced by the latest solution alone
    xn = rng.standard_normal(n)
    G.update(xn)
    assert G.k == 1
    assert np.allclose(G.basis(0)[:, 0] * np.sqrt(xn @ (A @ xn)), xn)
    # a direction the operator annihilates (a constant on a singular operator) is skipped
    L = sp.diags([-np.ones(n - 1), 2 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]).tolil()
    L[0, 0] = L[n - 1, n - 1] = 1.0
    L = L.tocsr()
    H = FischerModel(L, nc=1, model=2, size=4)
    H.update(np.ones(n))
    assert H.k == 1 and H.sigma[0][0] == 0.0


def _record_tg_updates(steps=6):
    """The velocity-update systems (b, warm start u*) of the oracle's 3-D Taylor-Green P2-P1 at N = 6."""
    opts = {"ksp_type": "cg", "pc_type": "jacobi", "ksp_rtol": 1e-8, "ksp_initial_guess_nonzero": True}
    R, clock = O.taylor_green_problem(6, 3, u_deg=2, p_deg=1, nu=0.01, dt=0.005,
                                      solver_options={"tentative": dict(opts, ksp_type="bcgs"), "pressure": opts,
                                                      "scalar": opts})
    rec = []
    inner = R.solver_c.solve

    def solve(b, x):
        rec.append((b.copy(), x.copy()))
        return inner(b, x)

    R.solver_c.solve = solve
    t = 0.0
    for _ in range(steps):
        t += 0.005
        clock["t"] = t
        R.solve(0.005, 0.01, max_iter=1)
    return R.M, rec


def test_replay_of_the_velocity_update_needs_fewer_iterations():
    M, rec = _record_tg_updates()
    dinv = 1.0 / M.diagonal()
    base = fisch = 0
    models = [FischerModel(M, nc=1, model=1, size=4) for _ in range(3)]
    for i, (b, xw) in enumerate(rec):
        G = models[i % 3]  # one basis per velocity component, as the three columns of the device solve
        _, r0, it0, _ = O.jacobi_cg(M, b, xw, 1e-8, dinv=dinv)
        x0 = G.form(b, xw)
        x0 = xw if x0 is None else x0[:, 0]
        x, r1, it1, _ = O.jacobi_cg(M, b, x0, 1e-8, dinv=dinv)
        assert r0 > 0 and r1 > 0
        G.update(x)
        if i >= 6:  # from the third step on
            base += it0
            fisch += it1
    assert fisch < base, (fisch, base)
