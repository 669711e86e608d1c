"""Lagrangian tracers without a GPU: the numpy model (tests/tracer_model.py) on closed-form fields -- orders of accuracy,
the theta convention of the two time levels, the freeze rule -- the argument validation of ``oasisx_amd.Tracers`` that
needs no device, and the host checks of ``ox_tracer_advance``."""
import ctypes as C

import numpy as np
import pytest

from oasisx_amd import fem
from oasisx_amd import mesh as M
from tests import tracer_model as TM

BIG = TM.BoxLocator([-10.0, -10.0], [10.0, 10.0])


# ---- the model on closed-form fields ---------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,order", [("euler", 1), ("rk2", 2), ("rk4", 4)])
def test_model_orders_of_accuracy_on_a_rigid_rotation(scheme, order):
    """v = omega (-y, x), one turn: the particle comes back to its seed; h halved three times."""
    omega = 1.0
    field = TM.AnalyticField(lambda x, th: omega * np.stack([-x[:, 1], x[:, 0]], axis=1))
    x0 = np.array([[0.7, 0.0], [0.3, -0.4]])
    errs = []
    for n in (80, 160, 320, 640):
        T = TM.Tracers(field, BIG, x0, scheme=scheme, substeps=n)
        T.advance(2.0 * np.pi / omega)
        assert (T.status == 0).all() and np.allclose(T.age, 2.0 * np.pi)
        errs.append(float(np.abs(T.x - x0).max()))
    orders = np.log2(np.asarray(errs[:-1]) / np.asarray(errs[1:]))
    print(scheme, "errors", errs, "observed orders", orders)
    assert np.abs(orders - order).max() <= 0.2, (errs, orders)


def test_model_theta_convention_of_the_two_levels():
    """v = (1 + 2 theta, 0) = the blend of (1, 0) at theta = 0 and (3, 0) at theta = 1: the midpoint rule and RK4 integrate
    it exactly (2 dt per step); Euler with m substeps samples theta = s / m: dt (1 + (m - 1) / m)."""
    field = TM.AnalyticField(lambda x, th: np.stack([1.0 + 2.0 * th + 0.0 * x[:, 0], 0.0 * x[:, 0]], axis=1))
    x0 = np.zeros((3, 2))
    dt = 0.5
    for scheme in ("rk2", "rk4"):
        T = TM.Tracers(field, BIG, x0, scheme=scheme, substeps=1)
        T.advance(dt)
        assert np.abs(T.x[:, 0] - 2.0 * dt).max() <= 4e-16 and (T.x[:, 1] == 0.0).all(), (scheme, T.x)
        assert np.abs(T.path - 2.0 * dt).max() <= 4e-16 and (T.age == dt).all() and T.t == dt
    for m in (1, 2, 4, 5):
        T = TM.Tracers(field, BIG, x0, scheme="euler", substeps=m)
        T.advance(dt)
        assert np.abs(T.x[:, 0] - dt * (1.0 + (m - 1.0) / m)).max() <= 4e-16, (m, T.x)
    # the blend itself, as the finite-element field forms it
    assert TM.blend(np.array([1.0]), np.array([3.0]), 0.25)[0] == 1.5


def test_model_freeze_rule_in_one_dimension():
    """v = 1 on the box [0, 1], RK4, two substeps of h = 0.25: from x = 0.6 the first substep ends at 0.85; in the second
    the stage points at c = 1/2 (0.975) are inside and the one at c = 1 (1.1) is not: frozen at 0.85, the start of that
    substep, with exit_time = t + dt / 2."""
    field = TM.AnalyticField(lambda x, th: np.ones_like(x))
    box = TM.BoxLocator([0.0], [1.0])
    seen = []
    T = TM.Tracers(field, box, np.array([[0.35], [0.1]]), scheme="rk4", substeps=2, watch=lambda p: seen.append(p.copy()))
    T.advance(0.25)
    assert np.allclose(T.x[:, 0], [0.6, 0.35]) and (T.status == 0).all() and T.t == 0.25
    seen.clear()
    T.advance(0.5)
    pts = np.concatenate(seen)[:, 0]
    assert np.isclose(pts, 0.975).any() and np.isclose(pts, 1.1).any()  # c = 1/2 inside, c = 1 outside
    assert T.status.tolist() == [1, 0] and T.cell.tolist() == [-1, 0]
    assert np.allclose(T.x[:, 0], [0.85, 0.85]) and T.t_exit[0] == 0.25 + 0.5 * 0.5 and np.isnan(T.t_exit[1])
    assert np.allclose(T.age, [0.5, 0.75]) and np.allclose(T.path, [0.5, 0.75])
    before = (T.x.copy(), T.age.copy(), T.path.copy(), T.t_exit.copy())
    T.advance(0.1)  # frozen particles are skipped
    assert T.x[0, 0] == before[0][0, 0] and T.age[0] == before[1][0] and T.path[0] == before[2][0] and T.t_exit[0] == before[3][0]
    assert np.isclose(T.x[1, 0], 0.95) and T.status[1] == 0
    # the end point counts: Euler steps to 1.05 from 0.95 and stays at 0.95
    T.scheme, T.n_stages = "euler", 1
    T.advance(0.2)
    assert T.status[1] == 1 and np.isclose(T.x[1, 0], 0.95) and np.isclose(T.t_exit[1], 0.85)
    # a non-finite velocity: invalid, frozen the same way
    bad = TM.Tracers(TM.AnalyticField(lambda x, th: np.full_like(x, np.nan)), box, np.array([[0.5]]), scheme="rk2", substeps=1)
    bad.advance(0.1)
    assert bad.status.tolist() == [2] and bad.x[0, 0] == 0.5 and bad.t_exit[0] == 0.0 and bad.age[0] == 0.0


# ---- validation that needs no device -----------------------------------------------------------------------------------
def test_tracers_refuse_bad_arguments_before_any_device_call():
    import oasisx_amd as ox
    from oasisx_amd import _lib, tracers
    from oasisx_amd.parallel import MeshPartition

    assert ox.Tracers is tracers.Tracers and "Tracers" in ox.__all__
    mesh = M.create_rectangle(None, [[-1.0, -1.0], [1.0, 1.0]], [4, 4], device="cpu")
    V = fem.FunctionSpace(mesh, 2, window=64)
    u = fem.Function(fem.VectorFunctionSpace(V, 2))
    x = np.array([[0.1, 0.2, 0.0], [0.3, -0.2, 0.0]])
    for kw in (dict(scheme="rk3"), dict(scheme=None), dict(substeps=0), dict(substeps=1025), dict(substeps=1.5),
               dict(tol=0.5), dict(tol=-1e-12), dict(tol=float("nan")), dict(sort_every=-1)):
        with pytest.raises(ValueError):
            ox.Tracers(u, x, **kw)
    for bad in (np.zeros((4, 4)), np.zeros((2, 2, 3))):
        with pytest.raises(ValueError):
            ox.Tracers(u, bad)
    with pytest.raises(TypeError):
        ox.Tracers(fem.Function(V), x)  # a scalar field
    with pytest.raises(TypeError):
        ox.Tracers(fem.Function(V, "c", u._storage, 0), x)  # one component of a block
    with pytest.raises(TypeError):
        ox.Tracers(object(), x)
    dg = fem.Function(fem.functionspace(mesh, ("DG", 1)))
    with pytest.raises(NotImplementedError, match="DGSpace"):
        ox.Tracers(dg, x)
    hi = fem.Function(fem.functionspace(mesh, ("Lagrange", 4)))
    with pytest.raises(NotImplementedError, match="HighOrderLagrangeSpace"):
        ox.Tracers(hi, x)
    Vp = fem.FunctionSpace(mesh, 1, window=64, part=MeshPartition(mesh, 0, 2))
    with pytest.raises(NotImplementedError, match="one GPU: particles that cross ranks need migration"):
        ox.Tracers(fem.Function(fem.VectorFunctionSpace(Vp, 2)), x)
    with pytest.raises(_lib.OasisxHipError):  # no CPU fallback: the locator is a device object, as for bb_tree
        ox.Tracers(u, x)


# ---- the host checks of the C ABI ------------------------------------------------------------------------------------
class _LocGrid(C.Structure):  # struct LocGrid of csrc/ox_probe.hip
    _fields_ = [("lo", C.c_double * 3), ("hi", C.c_double * 3), ("inv_h", C.c_double * 3), ("nb", C.c_int * 3)]


class _Locator(C.Structure):  # struct ox_locator of csrc/ox_probe.hip (the host checks read gdim, n_cells, tol and ids)
    _fields_ = [("gdim", C.c_int), ("n_cells", C.c_int64), ("n_bins", C.c_int64), ("n_list", C.c_int64), ("tol", C.c_double),
                ("grid", _LocGrid), ("mem", C.c_void_p), ("mem_grid", C.c_void_p), ("mem_list", C.c_void_p),
                ("x0", C.c_void_p), ("grad", C.c_void_p), ("box", C.c_void_p), ("ids", C.c_void_p),
                ("bin_ptr", C.c_void_p), ("list", C.c_void_p)]


def test_tracer_advance_checks_its_arguments_before_any_device_call():
    """``ox_tracer_advance`` refuses every bad argument with a message that names it -- on the host, before the first HIP
    call (this test runs without a device; the locator is a host image of the library's struct that no kernel sees)."""
    from oasisx_amd import _lib

    lib = _lib.load()
    assert [f for f, _ in _lib.ox_tracer_args._fields_] == [
        "loc", "degree", "gdim", "nc", "cell_dofs", "n_cells", "n_rows", "cell_inv", "n_mesh_cells", "u_a", "u_b", "t", "dt",
        "substeps", "scheme", "use_hint", "tol", "n", "x", "cell", "status", "age", "path", "t_exit"]
    loc = _Locator()
    loc.gdim, loc.n_cells, loc.tol = 2, 32, 1e-10
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value

    def args(**kw):
        a = _lib.ox_tracer_args(C.addressof(loc), 2, 2, 2, p, 32, 81, p, 32, p, p, 0.0, 0.1, 1, 2, 1, 1e-10, 4, p, p, p, p,
                                p, p)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(a, *words):
        rc = lib.ox_tracer_advance(C.byref(a) if a is not None else None, None)
        msg = lib.ox_last_error().decode()
        assert rc != 0 and "ox_tracer_advance" in msg and all(w in msg for w in words), (rc, msg)

    refused(None, "null argument")
    refused(args(loc=None), "null argument", "loc")
    refused(args(gdim=4), "gdim=4")
    refused(args(gdim=1), "gdim=1")
    refused(args(degree=0), "degree 0")
    refused(args(degree=4), "degree 4")
    refused(args(nc=1), "nc=1")
    refused(args(nc=4), "nc=4")
    refused(args(substeps=0), "substeps=0")
    refused(args(substeps=1025), "substeps=1025")
    refused(args(scheme=3), "scheme=3")
    refused(args(scheme=-1), "scheme=-1")
    refused(args(dt=float("nan")), "dt=nan")
    refused(args(dt=float("inf")), "dt=inf")
    refused(args(gdim=3, nc=3), "loc->gdim=2", "gdim=3")
    refused(args(n_mesh_cells=31), "n_mesh_cells=31", "32")
    refused(args(tol=1e-6), "tol=1e-06")
    refused(args(n=-1), "n=-1")
    for name in ("cell_dofs", "cell_inv", "u_a", "u_b", "x", "cell", "status", "age", "path", "t_exit"):
        refused(args(**{name: None}), "null argument", name)
    loc.ids = p
    refused(args(), "selection")
    loc.ids = None
    assert lib.ox_tracer_advance(C.byref(args(n=0)), None) == 0  # nothing to do: no launch
