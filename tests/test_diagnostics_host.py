"""CPU: the reference of the flow diagnostics and statistics (tests/diagnostics_model.py) against closed forms, the
generated tables of the kernel (csrc/fe_tables_d.h) against that reference, the float64 West recurrence against the
extended two-pass moments, and the argument checks of oasisx_amd/diagnostics.py."""
import importlib.util
import os
import re
import types

import numpy as np
import pytest

from oracle import ipcs_oracle as O
from tests import assembly_model as AM
from tests import diagnostics_model as DM
from tests import viscosity_model as VM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(2, 4, 1), (2, 3, 2), (3, 2, 1), (3, 2, 2), (2, 3, 3), (3, 2, 3)]


def _close(a, b, scale, tol=1e-13):
    return float(np.max(np.abs(AM.to_f64(a - b)))) <= tol * scale


@pytest.mark.parametrize("dim,N,deg", CASES)
def test_linear_field_closed_forms(dim, N, deg):
    """u = A x on [-1, 1]^d: per cell every gradient integral is |cell| times its formula in A; the kinetic energy of
    the box is 1/2 |box| sum A_dk^2 / 3; the centroid fields are the constants of A and cfl = dt max_a |u_c . G_a|."""
    F = VM.tg_forms(dim, N, deg, 2 if deg == 3 else 1)
    A = np.array([[0.3, -1.1, 0.4], [0.7, 0.2, -0.5], [-0.6, 0.9, 0.8]])[:dim, :dim]
    u = F.x_v @ A.T
    nu = 0.37
    val, B, n = DM.cell_integrals(DM.geometry_of_forms(F), F.vd, deg, u, nu)
    vol = AM.to_f64(val[:, 0])
    assert abs(vol.sum() - 2.0 ** dim) < 1e-13
    S, W = 0.5 * (A + A.T), 0.5 * (A - A.T)
    om2 = 2.0 * np.sum(W * W)  # |curl u|^2 = 2 W:W
    want = {2: 2.0 * np.sum(S * S), 3: nu * 2.0 * np.sum(S * S), 4: 0.5 * om2, 5: np.trace(A) ** 2, 6: np.trace(A)}
    for k, f in want.items():
        assert _close(val[:, k], vol * f, np.abs(vol * f).max() + 1e-300), DM.COLUMNS[k]
    assert abs(float(val[:, 1].sum()) - 0.5 * 2.0 ** dim * np.sum(A * A) / 3.0) < 1e-12
    assert (B >= np.abs(AM.to_f64(val)) * (1 - 1e-12)).all() and int(n.max()) <= AM.N_MAX
    c = DM.centroid_fields(F, u, 0.1)
    assert np.allclose(c["shear"], np.sqrt(2.0 * np.sum(S * S)), rtol=1e-12)
    assert np.allclose(c["divc"], np.trace(A), rtol=1e-12) and np.allclose(c["q"], 0.5 * np.sum(W * W - S * S), rtol=1e-11)
    cen = F.coords[F.cells].mean(axis=1)
    assert np.allclose(c["cfl"], 0.1 * np.abs(np.einsum("cd,cad->ca", cen @ A.T, F.G)).max(axis=1), rtol=1e-11, atol=1e-14)


@pytest.mark.parametrize("dim,N,deg", CASES)
def test_rigid_rotation(dim, N, deg):
    """u = Omega x (-y, x, 0): strain2 = div = 0, vorticity 2 Omega, q > 0."""
    F = VM.tg_forms(dim, N, deg, 2 if deg == 3 else 1)
    om = 1.7
    u = np.zeros((F.x_v.shape[0], dim))
    u[:, 0], u[:, 1] = -om * F.x_v[:, 1], om * F.x_v[:, 0]
    val, _, _ = DM.cell_integrals(DM.geometry_of_forms(F), F.vd, deg, u, 0.01)
    v = AM.to_f64(val)
    scale = v[:, 0].max() * om * om
    assert np.abs(v[:, [2, 3, 5, 6]]).max() <= 1e-12 * scale
    assert np.allclose(v[:, 4], 0.5 * v[:, 0] * (2 * om) ** 2, rtol=1e-12)
    c = DM.centroid_fields(F, u, 0.1)
    assert np.allclose(c["omega"][:, -1], 2.0 * om, rtol=1e-12) and (c["q"] > 0).all()
    assert np.abs(c["shear"]).max() < 1e-6 * om and np.abs(c["divc"]).max() < 1e-12 * om  # (sqrt of a rounding residue)


@pytest.mark.parametrize("dim,N,deg", CASES)
def test_kinetic_energy_of_a_polynomial(dim, N, deg):
    """u = (x^p, y^p[, x y]) with p = deg is in the space: 1/2 int |u|^2 over the box is analytic."""
    F = VM.tg_forms(dim, N, deg, 2 if deg == 3 else 1)
    x = F.x_v
    cols = [x[:, 0] ** deg, x[:, 1] ** deg] + ([x[:, 0] * x[:, 1] if deg > 1 else x[:, 2]] if dim == 3 else [])
    u = np.stack(cols, axis=1)
    val, _, _ = DM.cell_integrals(DM.geometry_of_forms(F), F.vd, deg, u, 0.01)
    side = 2.0 / (2 * deg + 1)  # int_-1^1 x^(2 p)
    want = 2.0 * side * 2.0 ** (dim - 1)
    if dim == 3:
        want += (2.0 / 3.0) ** 2 * 2.0 if deg > 1 else (2.0 / 3.0) * 4.0
    assert abs(float(val[:, 1].sum()) - 0.5 * want) < 1e-12 * want


def _header_arrays():
    """{name: ndarray} of the double tables in csrc/fe_tables_d.h."""
    txt = open(os.path.join(ROOT, "oasisx_amd", "csrc", "fe_tables_d.h")).read()
    out = {}
    for m in re.finditer(r"double (OX_[A-Z]+\d_\d)((?:\[\d+\])+) = (\{.*?\});", txt, flags=re.S):
        shape = [int(s) for s in re.findall(r"\[(\d+)\]", m.group(2))]
        out[m.group(1)] = np.array([float(t) for t in re.findall(r"[-+0-9.eE]+", m.group(3))]).reshape(shape)
    return out


@pytest.mark.parametrize("dim,deg", [(d, p) for d in (2, 3) for p in (1, 2, 3)])
def test_generated_tables_match_the_reference(dim, deg):
    """The kernel's tables against the exact reference tensors and the oracle's tabulation; and the kernel's way to the
    gradient integrals (its rule, in float64 numpy) against the exact ones on the perturbed Taylor-Green field: the rule
    has the degree the products of two first derivatives need."""
    T = _header_arrays()
    tag = f"{dim}_{deg}"
    fact = float(np.prod(np.arange(1, dim + 1)))
    assert np.abs(T["OX_MASSD" + tag] - AM.to_f64(AM.ref("mass", dim, deg)) * fact).max() < 1e-15
    bary, w = DM.kernel_rule(dim, deg)
    phi, dphi = O.tabulate(dim, deg, bary)
    assert (T["OX_QWD" + tag] > 0).all() and np.abs(T["OX_QWD" + tag] - w).max() < 1e-15
    assert np.abs(T["OX_DPHID" + tag] - dphi).max() < 2e-13
    cphi, _ = O.tabulate(dim, deg, np.full((1, dim + 1), 1.0 / (dim + 1)))
    assert np.abs(T["OX_PHIC" + tag] - cphi[0]).max() < 1e-14
    F = VM.tg_forms(dim, 3 if dim == 2 else 2, deg, 2 if deg == 3 else 1)
    X = np.zeros((3, F.x_v.shape[0]))
    X[:dim] = F.x_v.T
    u = DM.stat_levels(X, dim, K=1)[0]
    val, B, n = DM.cell_integrals(DM.geometry_of_forms(F), F.vd, deg, u, 0.01)
    g = np.einsum("cid,qib,cbk->cqdk", u[F.vd], T["OX_DPHID" + tag], F.G)
    vol = F.adet / fact
    S = 0.5 * (g + np.swapaxes(g, 2, 3))
    s2 = vol * np.einsum("q,cq->c", T["OX_QWD" + tag], 2.0 * np.einsum("cqdk,cqdk->cq", S, S))
    d2 = vol * np.einsum("q,cq->c", T["OX_QWD" + tag], np.einsum("cqdd->cq", g) ** 2)
    ke = 0.5 * vol * np.einsum("cid,ij,cjd->c", u[F.vd], T["OX_MASSD" + tag], u[F.vd])
    for k, dev in ((1, ke), (2, s2), (5, d2)):
        ok, r, allow = AM.check(dev, val[:, k], B[:, k], np.full(dev.shape, n[k]), extra=1e-13 * B[:, k])
        assert ok, (DM.COLUMNS[k], r, allow)


def test_west_recurrence_in_float64():
    """On the inputs of the GPU statistics test: West's update in float64 meets its running bound against the extended
    recurrence; on a mean of 1e6 its covariance stays within 1e-8 of the extended two-pass value while raw sums lose it
    (the gap the GPU test's tolerance sits in)."""
    rng_x = np.linspace(-1.0, 1.0, 37)
    X = np.stack([rng_x, rng_x[::-1] * 0.7, 0.3 * rng_x ** 2])
    ws = DM.STAT_WEIGHTS
    K = len(ws)
    for nc in (1, 2, 3):
        xs = DM.stat_levels(X, nc)
        m64, c64, _, _ = DM.west(xs, ws, dtype=np.float64)
        mx, cx, Bm, Bc = DM.west(xs, ws)
        assert (np.abs(m64 - mx) <= (DM.C_MEAN * K + 2) * DM.U * Bm).all()
        assert (np.abs(c64 - cx) <= (DM.C_COV * K + 2) * DM.U * Bc).all()
        m2, c2 = DM.two_pass(xs, ws)
        assert np.abs(AM.to_f64(cx - c2)).max() <= 1e-15 * np.abs(AM.to_f64(c2)).max()
        # the cancellation case
        xo = DM.stat_levels(X, nc, offset=1.0e6)
        _, co, _, _ = DM.west(xo, ws, dtype=np.float64)
        _, c2o = DM.two_pass(xo, ws)
        ref = AM.to_f64(c2o)
        scale = np.abs(ref).max(axis=0)
        west_err = (np.abs(co - ref).max(axis=0) / scale).max()
        raw_err = (np.abs(DM.raw_sums(xo, ws)[1] - ref).max(axis=0) / scale).max()
        print(f"ncomp {nc}: West {west_err:.2e}, raw sums {raw_err:.2e}")
        assert west_err <= 1e-8 < raw_err


def test_regenerating_the_tables_reproduces_the_committed_file(tmp_path):
    spec = importlib.util.spec_from_file_location("gen_tables_diag", os.path.join(ROOT, "tools", "gen_tables_diag.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    out = tmp_path / "fe_tables_d.h"
    gen.emit(str(out))
    assert out.read_bytes() == open(os.path.join(ROOT, "oasisx_amd", "csrc", "fe_tables_d.h"), "rb").read()


def _stub_solver(comm=None):
    """What FlowDiagnostics / FlowStatistics read of a solver before their first launch, on the host."""
    from oasisx_amd import fem
    from oasisx_amd import mesh as M

    m = M.create_unit_square(None, 3, 3, device="cpu")
    if comm is not None:
        m.comm = comm
    Vi, Q = fem.FunctionSpace(m, 2, window=64), fem.FunctionSpace(m, 1, window=64)

    def scalar(name):
        raise KeyError(f"no scalar named {name!r} (have: [])")

    return types.SimpleNamespace(_mesh=m, _geom=fem.cell_geometry(m, Vi.local_cells), _Vi=[(Vi, None)] * 2, _Q=Q,
                                 _V=fem.VectorFunctionSpace(Vi, 2), _U=fem.FieldStorage(Vi.n_local, 2, "cpu"),
                                 _P=fem.FieldStorage(Q.n_local, 1, "cpu"), _gdim=2, _n_u=Vi.n_local, _n_q=Q.n_local, _nut=None,
                                 scalar=scalar)


def test_argument_validation():
    import oasisx_amd as ox
    from oasisx_amd.parallel import Comm

    S = _stub_solver()
    D = ox.FlowDiagnostics(S, fields=("cfl", "vorticity"), capacity=2)
    for dt in (0.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="dt"):
            D.sample(0.0, dt, 0.01)
    with pytest.raises(ValueError, match="nu"):
        D.sample(0.0, 0.1, -1.0)
    with pytest.raises(ValueError, match="unknown field"):
        ox.FlowDiagnostics(S, fields=("vort",))
    with pytest.raises(ValueError, match="unknown field"):
        D.cell_field("helicity")
    with pytest.raises(ValueError, match="not among"):
        D.cell_field("shear_rate")
    with pytest.raises(RuntimeError):
        D.latest()
    with pytest.raises(ValueError, match="capacity"):
        ox.FlowDiagnostics(S, capacity=0)
    T = ox.FlowStatistics(S)
    assert T.names == ("u", "p") and T.total_weight == 0.0
    for dt in (0.0, -1.0, float("inf")):
        with pytest.raises(ValueError, match="dt"):
            T.sample(dt)
    with pytest.raises(ValueError, match="unknown field"):
        ox.FlowStatistics(S, fields=("w",))
    with pytest.raises(ValueError, match="no scalar named"):
        ox.FlowStatistics(S, scalars=("T",))
    with pytest.raises(RuntimeError):
        T.mean("u")
    with pytest.raises(ValueError, match="no statistics"):
        T._get("T")
    P = _stub_solver(Comm(0, 2, None, transport="host"))
    with pytest.raises(NotImplementedError, match="comm.size > 1"):
        ox.FlowDiagnostics(P)
    with pytest.raises(NotImplementedError, match="comm.size > 1"):
        ox.FlowStatistics(P)
