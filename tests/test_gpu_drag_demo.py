"""GPU: demo/porous_channel_hip.py at its small size (P2, N = 8), held against the numpy model of tests/drag_model.py
time-stepped on the device's numbering -- not against a constant chosen in advance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def model_errors(F, x_v, x_q, steps, dt, nu, sigma, f, solver_options):
    """max |u_h - u| / u(0) of the first component after every step of DragOracleStep on the Brinkman channel: Dirichlet
    data on the whole boundary, every level on the parabola, p = 0, sigma on every cell, theta = 1."""
    from demo.porous_channel_hip import brinkman_profile, parabola
    from oracle import ipcs_oracle as O
    from tests import drag_model as DM

    bd = O.boundary_dofs(x_v, F.coords.min(axis=0), F.coords.max(axis=0))
    bcs = [[O.DirichletData(bd, lambda x: brinkman_profile(x[1], nu, sigma, f))], [O.DirichletData(bd, 0.0)]]
    zones = [DM.Zone(np.arange(F.cells.shape[0]), alpha=sigma)]
    R = DM.DragOracleStep(F, x_v, x_q, bcs, solver_options=solver_options, body_force=(f, 0.0), zones=zones, theta=1.0)
    R.u[:, 0] = R.u1[:, 0] = R.u2[:, 0] = parabola(x_v[:, 1], nu, sigma, f)
    exact = brinkman_profile(x_v[:, 1], nu, sigma, f)
    out = []
    for _ in range(steps):
        R.solve(dt, nu, max_iter=1)
        out.append(float(np.abs(R.u1[:, 0] - exact).max() / brinkman_profile(0.0, nu, sigma, f)))
    return out, R


def test_demo_reaches_the_models_steady_state(hip, capsys):
    """60 steps of dt = 0.1: the printed error against the closed form equals the model's time-stepped value to 1e-8 after
    every step; it ends within a factor 1.5 of the 7.5e-5 of the direct solve (the splitting's pressure accounts for the
    rest); the force on the medium equals f |Omega| minus the friction on the boundary to the accuracy of that friction.

    Observed on one MI355X: error after 60 steps 8.693924e-05 on both sides, largest difference over the steps 2.2e-15;
    force on the medium 2.0719, f |Omega| - friction 2.1041 (1.5 % apart), last change per step 2.1e-4."""
    from demo.porous_channel_hip import KRYLOV, main
    from tests.test_gpu_viscosity import _forms

    steps, dt, nu, sigma, f = 60, 0.1, 0.5, 2.0, 1.0
    rows = main(["-N", "8", "--steps", str(steps), "--dt", str(dt)])
    out = capsys.readouterr().out
    assert "max error / u(0)" in out and "force on the medium" in out
    r = rows[0]
    S = r["solver"]
    F, x_v, x_q = _forms(S, S._mesh)
    ref, R = model_errors(F, x_v, x_q, steps, dt, nu, sigma, f, KRYLOV)
    d = np.abs(np.array(r["errors"]) - np.array(ref))
    print(f"error after {steps} steps: demo {r['error']:.6e}, model {ref[-1]:.6e}, largest difference over the steps "
          f"{d.max():.2e}; "
          f"force {r['force'][0]:.8f}, f |Omega| - friction {r['balance']:.8f}, last change {r['change']:.2e}")
    assert d.max() <= 1e-8, d.max()
    assert f"{r['error']:.6e}" in out
    assert 7.5e-5 < ref[-1] < 1.5 * 7.5e-5
    assert abs(r["volume"] - 4.0) <= 1e-12
    # the friction is nu times facet means of the P2 gradient: off by about h^2 |u'''| / 12 = 0.02 per unit length of wall
    # (h = 1/4, |u'''| = (f / sigma) m^3 tanh m = 3.9), 0.04 in all or 2 % of the force of 2.07; the bound is 2.5 x that
    assert abs(r["force"][0] - r["balance"]) <= 5e-2 * abs(r["force"][0])
    assert abs(r["force"][1]) <= 1e-2 * abs(r["force"][0])
