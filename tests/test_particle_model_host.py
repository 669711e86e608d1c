"""Host: the numpy model of the inertial particles (tests/particle_model.py) against closed forms -- no GPU.

(a) A uniform steady field with gravity: the substep is the exact flow map, so the model equals
    v(t) = w + (v0 - w) e^{-t/tau},  x(t) = x0 + w t + tau (v0 - w)(1 - e^{-t/tau}),  w = u + tau beta g
    to 1e-13 relative to max(1, |value|), for h / tau_p in {1e-6, 1, 1e6} and tau_p = 0.  Gravity is scaled so that the
    settling velocity tau beta g stays of order one: at tau = 1e6 h a gravity of order one makes w of order 1e5 and the
    closed form itself then loses eleven digits in w t - tau w (1 - e^{-t/tau}) -- nothing an integrator could be held to.
(b) Solid-body rotation u = (-y, x) with Stokes drag is a linear ODE; its exact solution is a matrix exponential.  exp2
    converges with order >= 1.8, exp1 with order >= 0.9, over three halvings of h.
(c) The fold and its image counts, the tie rule of the classification, deposit against exit on a mesh with one tagged wall.
"""
import numpy as np
import pytest

from tests import particle_model as PMo
from tests import tracer_model as TM

RATIOS = PMo.RATIOS


@pytest.mark.parametrize("scheme", ["exp1", "exp2"])
@pytest.mark.parametrize("ratio", RATIOS)
def test_uniform_field_is_integrated_exactly(ratio, scheme):
    d, h, substeps, advances = 2, 0.02, 5, 4
    tau, u, g, beta = PMo.exact_case(ratio, d, h)
    rng = np.random.default_rng(3)
    x0, v0 = rng.uniform(0.3, 0.6, (64, d)), rng.uniform(-0.2, 0.2, (64, d))
    P = PMo.Particles(TM.AnalyticField(lambda x, th: np.broadcast_to(u, x.shape).copy()), TM.BoxLocator([-9.0] * d, [9.0] * d),
                      x0, v0, tau, beta=beta, gravity=g, scheme=scheme, substeps=substeps)
    for _ in range(advances):
        P.advance(h * substeps)
    xe, ve = PMo.closed_form(x0, v0, u, g, beta, tau, h * substeps * advances)
    ex, ev = PMo.rel_err(P.x, xe), PMo.rel_err(P.v, ve)
    print(f"h/tau = {ratio}, {scheme}: |x - closed form| = {ex:.3e}, |v - closed form| = {ev:.3e}")
    assert (P.status == 0).all() and ex <= 1e-13 and ev <= 1e-13, (ex, ev)
    assert np.abs(P.age - h * substeps * advances).max() <= 1e-14


def rotation_exact(x0, v0, tau, t):
    """(x, v)(t) of dx/dt = v, dv/dt = (R x - v) / tau, R = [[0, -1], [1, 0]]: exp(A t) through A's eigenvectors."""
    R = np.array([[0.0, -1.0], [1.0, 0.0]])
    A = np.block([[np.zeros((2, 2)), np.eye(2)], [R / tau, -np.eye(2) / tau]])
    lam, V = np.linalg.eig(A)
    M = (V @ np.diag(np.exp(lam * t)) @ np.linalg.inv(V)).real
    y = np.concatenate([x0, v0], axis=1) @ M.T
    return y[:, :2], y[:, 2:]


@pytest.mark.parametrize("scheme,order", [("exp2", 1.8), ("exp1", 0.9)])
def test_convergence_in_solid_body_rotation(scheme, order):
    tau, T = 0.5, 1.0
    rng = np.random.default_rng(5)
    x0 = rng.uniform(-0.5, 0.5, (32, 2))
    v0 = np.stack([-x0[:, 1], x0[:, 0]], axis=1) + rng.uniform(-0.1, 0.1, (32, 2))
    xe, ve = rotation_exact(x0, v0, tau, T)
    field = TM.AnalyticField(lambda x, th: np.stack([-x[:, 1], x[:, 0]], axis=1))
    errs = []
    for m in (4, 8, 16, 32):
        P = PMo.Particles(field, TM.BoxLocator([-9.0, -9.0], [9.0, 9.0]), x0, v0, tau, scheme=scheme, substeps=m)
        P.advance(T)
        errs.append(max(float(np.abs(P.x - xe).max()), float(np.abs(P.v - ve).max())))
    rates = [float(np.log2(errs[k] / errs[k + 1])) for k in range(3)]
    overall = float(np.log2(errs[0] / errs[3]) / 3.0)
    print(f"{scheme}: errors {['%.3e' % e for e in errs]}, orders {['%.2f' % r for r in rates]}, overall {overall:.2f}")
    assert overall >= order and min(rates) >= order - 0.1, (errs, rates)


def test_fold_counts_images():
    per = ((0,), np.array([0.0, 0.0]), np.array([2.0, 1.0]), np.array([2.0, 0.0]))
    x = np.array([[0.5, 0.3], [2.0, 0.3], [4.5, 0.9], [-0.25, 0.1], [-4.0, 0.5], [1.999, 1.7]])
    f, w, gap = PMo.fold(x, per)
    assert np.array_equal(w, [[0, 0], [1, 0], [2, 0], [-1, 0], [-2, 0], [0, 0]])
    assert np.allclose(f[:, 0], [0.5, 0.0, 0.5, 1.75, 0.0, 1.999]) and np.array_equal(f[:, 1], x[:, 1])  # axis 1 is not folded
    assert (f[:, 0] >= 0.0).all() and (f[:, 0] < 2.0).all() and gap == 0.0
    assert np.allclose(f + w * per[3][None, :], x, atol=1e-15)
    # a uniform field across the seam: nobody freezes, the unfolded position is the closed form
    u = np.array([1.3, 0.0])
    x0 = np.random.default_rng(1).uniform([0.1, 0.2], [1.9, 0.8], (50, 2))
    P = PMo.Particles(TM.AnalyticField(lambda x, th: np.broadcast_to(u, x.shape).copy()), TM.BoxLocator([0.0, 0.0], [2.0, 1.0]),
                      x0, None, 0.0, scheme="exp2", substeps=4, periodic=per)
    for _ in range(5):
        P.advance(1.0)
    assert (P.status == 0).all() and np.abs(P.unfolded() - (x0 + 5.0 * u)).max() <= 1e-13
    assert np.array_equal(P.wraps[:, 0], np.floor((x0[:, 0] + 6.5) / 2.0).astype(np.int64)) and (P.wraps[:, 1] == 0).all()
    assert (P.x[:, 0] >= 0.0).all() and (P.x[:, 0] < 2.0).all() and np.abs(P.path - 6.5).max() <= 1e-13


def test_ties_go_to_the_lower_facet():
    # two segments that meet at (0.5, 0): a point straight below the shared vertex is equally far from both
    xyz = np.array([[[1.0, 0.0], [0.5, 0.0]], [[0.0, 0.0], [0.5, 0.0]], [[0.0, 1.0], [0.0, 0.0]]])
    field = TM.AnalyticField(lambda x, th: np.broadcast_to(np.array([0.0, -1.0]), x.shape).copy())
    for action, status in (([1, 0, 0], 3), ([0, 1, 0], 1)):
        P = PMo.Particles(field, TM.BoxLocator([0.0, 0.0], [1.0, 1.0]), [[0.5, 0.125]], None, 0.0, scheme="exp1",
                          facet_xyz=xyz, action=action)
        P.advance(0.25)
        assert P.facet.tolist() == [0] and P.status.tolist() == [status] and P.margin == 0.0
        assert P.x.tolist() == [[0.5, 0.125]] and P.t_exit.tolist() == [0.0] and P.cell.tolist() == [-1]
        assert P.v.tolist() == ([[0.0, 0.0]] if status == 3 else [[0.0, -1.0]])


def test_deposit_against_exit_on_a_tagged_wall():
    import torch

    from oasisx_amd import mesh as M

    mesh = M.create_unit_square(None, 4, 4, device=torch.device("cpu"))
    ids, xyz = PMo.exterior_xyz(mesh)
    assert ids.shape[0] == 16
    mid = xyz.mean(axis=1)
    bottom = np.abs(mid[:, 1]) < 1e-12
    action = bottom.astype(np.int32)  # the wall y = 0 deposits; the rest lets particles out
    rng = np.random.default_rng(7)
    x0 = rng.uniform(0.2, 0.8, (60, 2))
    v0 = np.zeros((60, 2))
    v0[:20, 1], v0[20:40, 0], v0[40:, 1] = -1.0, 1.0, 0.05  # down to the wall, out to the right, slowly up: stays inside
    field = TM.AnalyticField(lambda x, th: np.zeros_like(x))
    P = PMo.Particles(field, TM.MeshLocator(mesh), x0, v0, 1e3, scheme="exp2", substeps=4, facet_xyz=xyz, action=action)
    for _ in range(4):
        P.advance(0.25)
    assert (P.status[:20] == 3).all() and (P.status[20:40] == 1).all() and (P.status[40:] == 0).all()
    assert bottom[P.facet[:20]].all() and (np.abs(mid[P.facet[20:40], 0] - 1.0) < 1e-12).all() and (P.facet[40:] == -1).all()
    assert (P.v[:20] == 0.0).all() and (P.v[20:40, 0] > 0.9).all()
    h = 0.25 / 4
    t_hit = x0[:20, 1] / 1.0  # (tau = 1e3: ballistic to 1e-3)
    assert (P.t_exit[:20] <= t_hit + 1e-3).all() and (P.t_exit[:20] >= t_hit - h - 1e-3).all()
    assert np.isnan(P.t_exit[40:]).all() and (P.cell[:40] == -1).all() and P.margin >= 1e-9
    # the facet under the deposition point: the one whose x-range holds the particle
    lo, hi = xyz[P.facet[:20], :, 0].min(axis=1), xyz[P.facet[:20], :, 0].max(axis=1)
    assert ((P.x[:20, 0] >= lo) & (P.x[:20, 0] <= hi)).all()
