"""GPU: demo/reacting_scalars_hip.py at its smallest sizes -- the batch reactor against the closed form of second-order
kinetics, the plug-flow reactor against the numpy model (tests/reaction_model.whole_step) on the same mesh."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_batch_reactor_order(hip):
    """A + B -> C at rest, uniform fields, T = 1 in 8 and 16 Strang steps on the 4 x 4 P2 lattice: the error against the
    closed form falls with a measured order above 1.7 (the numpy model alone gives 1.82 for this pair)."""
    from demo.reacting_scalars_hip import run_batch

    e8, e16 = run_batch(4, 2, 8), run_batch(4, 2, 16)
    order = float(np.log2(e8 / e16))
    print(f"batch reactor: errors {e8:.6e}, {e16:.6e}, order {order:.3f}")
    assert e16 < e8 and order > 1.7, (e8, e16, order)


def test_plug_flow_profile(hip):
    """A -> B in the uniform flow, 40 steps of dt = 0.075 on the 6 x 6 P2 lattice: max |A - exp(-k (x + 1) / U)| stays within
    1.5 x the error of the composed numpy model on the same mesh, numbering and steps."""
    from demo.reacting_scalars_hip import TIGHT, inflow, pfr_exact, run_pfr
    from tests.reaction_model import ReactionModel, whole_step
    from tests.scalar_model import ScalarModel
    from tests.test_gpu_scalar import _dofs, _forms

    steps, dt, k, U, kappa = 40, 0.075, 2.0, 1.0, 0.01
    S, mesh, err = run_pfr(6, 2, steps, dt, k=k, U=U, kappa=kappa)
    F, x_v = _forms(S, mesh)
    rows = _dofs(x_v, inflow)
    models = [ScalarModel(F, x_v, kappa, dofs=rows, value=v, options=TIGHT) for v in (1.0, 0.0)]
    rm = ReactionModel.from_network(S._reactions)
    held = np.zeros((2, x_v.shape[0]), dtype=bool)
    held[:, rows] = True
    uab = S._UAB.rhost()
    assert np.array_equal(uab, np.tile([U, 0.0], (x_v.shape[0], 1)))
    for _ in range(steps):
        whole_step(rm, models, uab, dt, "strang", 1, held)
    X = np.zeros((3, x_v.shape[0]))
    X[:2] = x_v.T
    err_model = float(np.abs(models[0].c - pfr_exact(X, k, U)).max())
    print(f"plug flow: device error {err:.6e}, model error {err_model:.6e}")
    assert err_model < 0.2  # (the profile is there: exp(-k (x + 1) / U) falls from 1 to 0.018)
    assert err <= 1.5 * err_model, (err, err_model)
