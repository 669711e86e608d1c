"""No GPU: the numpy model of the wall-stress evaluation (tests/wall_stress_model.py) pinned by analytic fields, and the
generated facet-mean tables (oasisx_amd/csrc/fe_tables_f.h, tools/gen_tables_facet.py) against the model's quadrature."""
import os
import re

import numpy as np
import pytest

from tests import wall_stress_model as WM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(2, 6, 1), (2, 5, 2), (3, 3, 1), (3, 3, 2), (2, 4, 3), (3, 2, 3)]
EPS = np.finfo(np.float64).eps


def _tables():
    """name -> ndarray of every table of fe_tables_f.h."""
    text = open(os.path.join(ROOT, "oasisx_amd", "csrc", "fe_tables_f.h")).read()
    out = {}
    for m in re.finditer(r"static constexpr double (\w+)((?:\[\d+\])+) = \{(.*?)\};", text, re.S):
        shape = tuple(int(s) for s in re.findall(r"\[(\d+)\]", m.group(2)))
        vals = np.array([float(v) for v in re.findall(r"-?\d+\.\d+(?:e-?\d+)?", m.group(3))])
        out[m.group(1)] = vals.reshape(shape)
    return out


def test_every_table_is_there():
    T = _tables()
    want = {f"OX_DPHIF{d}_{k}" for d in (2, 3) for k in (1, 2, 3)} | {f"OX_PHIF{d}_{k}" for d in (2, 3) for k in (1, 2)}
    assert set(T) == want
    for d, nds in ((2, (3, 6, 10)), (3, (4, 10, 20))):
        for k, nd in zip((1, 2, 3), nds):
            assert T[f"OX_DPHIF{d}_{k}"].shape == (d + 1, nd, d + 1)
            if k <= 2:
                assert T[f"OX_PHIF{d}_{k}"].shape == (d + 1, nd)


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("degree", [1, 2, 3])
def test_tables_equal_the_models_facet_means(d, degree):
    """For a random coefficient vector c the contraction sum_i c_i T[a][i][b] with the generated table equals the one with
    the model's quadrature means M.

    Tolerance.  A table entry is the exact mean rounded once (relative error eps/2).  A model mean is a sum of nq
    products w_q dphi_i(x_q) of rounded factors: |dM_i| <= (nq + 2) eps A_i with A_i = sum_q w_q |dphi_i(x_q)| >= |M_i|.
    For degree 3 dphi itself comes from the numerically inverted 10 x 10 / 20 x 20 monomial Vandermonde matrix V of the
    P3 nodes: relative error cond(V) eps in the coefficients, so (nq + 2 + cond(V)) eps A_i.  Each contraction is a sum
    of nd terms: another nd eps sum_i |c_i| A_i for both sides together.  Hence

        |sum_i c_i (T_i - M_i)| <= (2 nd + nq + 3 + cond(V) [degree 3]) eps sum_i |c_i| A_i
    """
    from oasisx_amd import fem

    T = _tables()
    rng = np.random.default_rng(17 + 10 * d + degree)
    nq = WM.facet_rule(d)[1].shape[0]
    cond = float(np.linalg.cond(fem._p3_mono(d, fem.p3_nodes(d))[0])) if degree == 3 else 0.0
    for a in range(d + 1):
        phi, dphi, absd = WM.facet_means(d, degree, a)
        nd = phi.shape[0]
        c = rng.standard_normal(nd)
        tab = T[f"OX_DPHIF{d}_{degree}"][a]
        err = np.abs(c @ tab - c @ dphi)
        tol = (2 * nd + nq + 3 + cond) * EPS * (np.abs(c) @ absd)
        print(f"d={d} degree={degree} facet {a}: max err {err.max():.3e}, min tol {tol[tol > 0].min():.3e}")
        assert (err <= tol).all(), (a, err, tol)
        if degree <= 2:
            p, w = WM.facet_points(d, a)
            absp = w @ np.abs(fem.lagrange_basis(d, degree, p))
            e2 = abs(c @ T[f"OX_PHIF{d}_{degree}"][a] - c @ phi)
            assert e2 <= (2 * nd + nq + 3) * EPS * (np.abs(c) @ absp), (a, e2)


def _forms(dim, N, deg, kind):
    from oracle import ipcs_oracle as O
    from tests import viscosity_model as VM
    from tests.helpers import delaunay_box_mesh

    p_deg = 2 if deg == 3 else 1
    if kind == "lattice":
        return VM.tg_forms(dim, N, deg, p_deg), p_deg
    coords, cells = delaunay_box_mesh(N, dim=dim, seed=2)
    return O.Forms(coords, cells, deg, p_deg), p_deg


# the analytic fields: u_i = b_i + A_i . x + x^T Q_i x (Q = 0 for degree 1), p = c + a . x + x^T P x (P = 0 for P1)
def _fields(dim, deg, p_deg, seed=5):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((dim, dim))
    b = rng.standard_normal(dim)
    Q = rng.standard_normal((dim, dim, dim)) if deg >= 2 else np.zeros((dim, dim, dim))
    Q = 0.5 * (Q + np.swapaxes(Q, 1, 2))
    a = rng.standard_normal(dim)
    P = rng.standard_normal((dim, dim)) if p_deg == 2 else np.zeros((dim, dim))
    P = 0.5 * (P + P.T)
    u = lambda x: b + x @ A.T + np.einsum("nk,ikl,nl->ni", x, Q, x)  # noqa: E731
    gu = lambda x: A[None] + 2.0 * np.einsum("ikl,nl->nik", Q, x)  # noqa: E731  (n, i, k) = d u_i / d x_k
    p = lambda x: 0.3 + x @ a + np.einsum("nk,kl,nl->n", x, P, x)  # noqa: E731
    return u, gu, p


def _facet_vertices(coords, cells, fcell, fopp):
    d = coords.shape[1]
    idx = np.array([[k for k in range(d + 1) if k != a] for a in fopp])
    return coords[cells[fcell][np.arange(fcell.shape[0])[:, None], idx]]  # (nf, d, d)


def _mean_of_quadratic(p, xf):
    """Exact facet mean of a polynomial of degree <= 2 from the facet's vertices: Simpson on an edge, the mean of the
    three edge midpoints on a triangle."""
    if xf.shape[1] == 2:
        return (p(xf[:, 0]) + 4.0 * p(0.5 * (xf[:, 0] + xf[:, 1])) + p(xf[:, 1])) / 6.0
    return (p(0.5 * (xf[:, 0] + xf[:, 1])) + p(0.5 * (xf[:, 1] + xf[:, 2])) + p(0.5 * (xf[:, 0] + xf[:, 2]))) / 3.0


@pytest.mark.parametrize("kind", ["lattice", "delaunay"])
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_model_is_exact_for_polynomial_fields(dim, N, deg, kind):
    """u linear (degree 1) or quadratic (degree >= 2), p linear (P1) or quadratic (P2): grad u is linear, so its facet
    mean is its value at the facet midpoint; the mean of p comes from the facet's vertices.  Traction, shear and the
    force per side of the box equal the closed forms to 1e-12 max|t|."""
    F, p_deg = _forms(dim, N, deg, kind)
    coords, cells = F.coords, F.cells
    fcell, fopp = WM.exterior_facets(cells)
    assert len(set(fopp.tolist())) >= 2  # (which local vertices lie opposite the boundary depends on the mesh)
    u, gu, p = _fields(dim, deg, p_deg)
    nu = 0.37
    t, wss = WM.wall_stress(coords, cells, fcell, fopp, F.vd, F.qd, u(F.x_v), p(F.x_q), deg, p_deg, nu)
    n, meas, mid = WM.facet_geometry(coords, cells, fcell, fopp)
    # the box [-1, 1]^dim: every exterior facet lies in a side, its normal is that side's, the measures add up
    side = np.argmax(np.abs(mid), axis=1)
    assert np.allclose(np.abs(mid[np.arange(mid.shape[0]), side]), 1.0, atol=1e-14)
    want_n = np.zeros_like(n)
    want_n[np.arange(n.shape[0]), side] = np.sign(mid[np.arange(mid.shape[0]), side])
    assert np.abs(n - want_n).max() < 1e-13
    assert abs(meas.sum() - 2 * dim * 2.0 ** (dim - 1)) < 1e-12
    g = gu(mid)
    pbar = _mean_of_quadratic(p, _facet_vertices(coords, cells, fcell, fopp))
    t_ref = -pbar[:, None] * want_n + nu * np.einsum("nik,nk->ni", g + np.swapaxes(g, 1, 2), want_n)
    wss_ref = t_ref - np.einsum("ni,ni->n", t_ref, want_n)[:, None] * want_n
    scale = np.abs(t_ref).max()
    dt_, dw = np.abs(t - t_ref).max(), np.abs(wss - wss_ref).max()
    print(f"{kind} ({dim},{N},{deg}): |dt| / max|t| = {dt_ / scale:.3e}, |dwss| / max|t| = {dw / scale:.3e}")
    assert dt_ <= 1e-12 * scale and dw <= 1e-12 * scale
    assert np.abs(np.einsum("ni,ni->n", wss, n)).max() <= 1e-12 * scale  # the shear is tangential
    tag = 2 * side + (want_n[np.arange(n.shape[0]), side] > 0)
    tags = np.unique(tag)
    assert tags.shape[0] == 2 * dim
    Fm = WM.forces(t, meas, tag, tags, rho=1.7)
    Fr = WM.forces(t_ref, meas, tag, tags, rho=1.7)
    assert np.abs(Fm - Fr).max() <= 1e-12 * np.abs(Fr).max()


@pytest.mark.parametrize("dim,N,deg", CASES)
def test_model_satisfies_the_gauss_identities(dim, N, deg):
    """On the closed boundary: u = 0, p = a . x + c gives sum F = rho a |Omega|; for degree >= 2, u = (y^2, 0[, 0]) gives
    the viscous force -rho nu (2 |Omega|, 0[, 0]).  The sums cancel: the bound is relative to sum |f| |t_f|."""
    F, p_deg = _forms(dim, N, deg, "delaunay")
    coords, cells = F.coords, F.cells
    fcell, fopp = WM.exterior_facets(cells)
    _, meas, _ = WM.facet_geometry(coords, cells, fcell, fopp)
    rho, nu, vol = 1.3, 0.2, 2.0 ** dim
    zero_tag = np.zeros(fcell.shape[0], dtype=int)
    a = np.array([0.7, -1.1, 0.4])[:dim]
    t, _ = WM.wall_stress(coords, cells, fcell, fopp, F.vd, F.qd, np.zeros((F.x_v.shape[0], dim)), F.x_q @ a + 0.25, deg,
                          p_deg, nu)
    tot = WM.forces(t, meas, zero_tag, [0], rho)[0]
    assert np.abs(tot - rho * a * vol).max() <= 1e-12 * rho * (meas * np.linalg.norm(t, axis=1)).sum()
    if deg >= 2:
        u = np.zeros((F.x_v.shape[0], dim))
        u[:, 0] = F.x_v[:, 1] ** 2
        t, _ = WM.wall_stress(coords, cells, fcell, fopp, F.vd, F.qd, u, np.zeros(F.x_q.shape[0]), deg, p_deg, nu)
        tot = WM.forces(t, meas, zero_tag, [0], rho)[0]
        want = np.zeros(dim)
        want[0] = -rho * nu * 2.0 * vol
        assert np.abs(tot - want).max() <= 1e-12 * rho * (meas * np.linalg.norm(t, axis=1)).sum()
