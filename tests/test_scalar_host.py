"""Passive scalar transport without a GPU: the numpy model the device is compared with (tests/scalar_model.py) and the
argument checking of ScalarTransport."""
import numpy as np
import pytest

from oracle import ipcs_oracle as O
from tests.scalar_model import ScalarModel, exact_solution_error

TIGHT = {"ksp_type": "bcgs", "pc_type": "jacobi", "ksp_rtol": 1e-12, "ksp_atol": 1e-30}


@pytest.mark.parametrize("dim,N,deg", [(2, 6, 2), (3, 3, 2), (2, 6, 1)])
def test_model_preserves_constants(dim, N, deg):
    """c_1 = 1, no Dirichlet rows, no source, any u_ab: C 1 = K 1 = 0, so b_c = (M/dt) 1 = A_c 1 and the step returns 1."""
    if dim == 2:
        coords, cells = O.create_rectangle_mesh([-1, -1], [1, 1], [N, N])
    else:
        coords, cells = O.create_box_mesh([-1, -1, -1], [1, 1, 1], [N, N, N])
    F = O.Forms(coords, cells, deg, 1)
    m = ScalarModel(F, F.x_v, kappa=0.3, options=TIGHT)
    m.interpolate(lambda x: np.ones_like(x[0]))
    uab = np.random.default_rng(0).standard_normal((F.nv, dim))
    for _ in range(2):
        c = m.step(uab, 0.05)
    assert m.reason > 0
    print("max |c - 1| =", np.abs(c - 1.0).max())
    assert np.abs(c - 1.0).max() < 1e-9  # solver tolerance 1e-12 relative on the preconditioned residual


def test_model_converges_to_the_exact_solution():
    """c = cos(pi x) cos(pi y) exp(-2 kappa pi^2 t) in the Taylor-Green velocity, exact Dirichlet data, P2: the L2 error
    at t = 0.05 falls with the mesh at an order above 2 (dt = 0.005: the Crank-Nicolson error, ~1e-7, is far below)."""
    errs = [exact_solution_error(N) for N in (4, 8, 16)]
    orders = [float(np.log2(errs[i] / errs[i + 1])) for i in range(2)]
    print("L2 errors N = 4, 8, 16:", errs, "observed orders:", orders)
    assert all(o > 2.0 for o in orders), (errs, orders)


def test_model_exact_solution_does_not_depend_on_kappa_in_form():
    """The same solution family for another kappa (u . grad c = 0 for any): still converging above order 2."""
    errs = [exact_solution_error(N, kappa=0.5) for N in (4, 8)]
    assert np.log2(errs[0] / errs[1]) > 2.0, errs


def test_scalar_transport_arguments():
    from oasisx_amd import DirichletBC, LocatorMethod, ScalarTransport

    s = ScalarTransport("T", diffusivity=0.1)
    assert s.kappa(0.01) == 0.1 and s.source == 0.0 and s.initial is None and s.bcs == []
    s = ScalarTransport("dye", schmidt=4.0, source=1, initial=2)
    assert s.kappa(0.02) == 0.005 and s.source == 1.0 and s.initial == 2.0
    with pytest.raises(ValueError, match="exactly one"):
        ScalarTransport("T")
    with pytest.raises(ValueError, match="exactly one"):
        ScalarTransport("T", diffusivity=0.1, schmidt=1.0)
    with pytest.raises(ValueError):
        ScalarTransport("", diffusivity=0.1)
    with pytest.raises(ValueError):
        ScalarTransport("T", diffusivity=-1.0)
    with pytest.raises(ValueError):
        ScalarTransport("T", schmidt=0.0)
    with pytest.raises(TypeError):
        ScalarTransport("T", diffusivity=0.1, bcs=[1.0])
    bc = DirichletBC(1.0, LocatorMethod.GEOMETRICAL, lambda x: np.isclose(x[0], -1.0))
    assert ScalarTransport("T", diffusivity=0.0, bcs=[bc], source=lambda x: x[0]).bcs == [bc]
