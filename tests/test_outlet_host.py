"""No GPU: the numpy model of the outlet kernels (tests/outlet_model.py) pinned by closed forms, and the generated tables
of csrc/fe_tables_o.h (tools/gen_tables_outlet.py) against the model's rule and basis."""
import itertools
import os
import re

import numpy as np
import pytest

from tests import outlet_model as OM
from tests import wall_stress_model as WM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(2, 6, 1), (2, 5, 2), (3, 3, 1), (3, 3, 2), (2, 4, 3), (3, 2, 3)]
KINDS = ["lattice", "delaunay", "rolled"]
EPS = np.finfo(np.float64).eps


# ---- polynomials: {exponent tuple: coefficient} ------------------------------------------------------------------------
def poly_random(dim, degree, rng):
    return {e: float(rng.standard_normal()) for e in itertools.product(range(degree + 1), repeat=dim) if sum(e) <= degree}


def poly_diff(p, k):
    out = {}
    for e, c in p.items():
        if e[k] > 0:
            f = e[:k] + (e[k] - 1,) + e[k + 1:]
            out[f] = out.get(f, 0.0) + c * e[k]
    return out


def poly_sub(p, q):
    out = dict(p)
    for e, c in q.items():
        out[e] = out.get(e, 0.0) - c
    return out


def poly_eval(p, x):
    """x: (n, dim)."""
    out = np.zeros(x.shape[0])
    for e, c in p.items():
        out = out + c * np.prod(x ** np.asarray(e)[None, :], axis=1)
    return out


def poly_side_integral(p, axis, sign):
    """int of p over the side x_axis = sign of [-1, 1]^dim."""
    tot = 0.0
    for e, c in p.items():
        v = c * float(sign) ** e[axis]
        for j, ej in enumerate(e):
            if j != axis:
                v *= 0.0 if ej % 2 else 2.0 / (ej + 1)
        tot += v
    return tot


def solenoidal_field(dim, degree, rng):
    """A polynomial field of degree <= ``degree`` with zero divergence: the curl of a random potential of degree + 1."""
    if dim == 2:
        psi = poly_random(2, degree + 1, rng)
        return [poly_diff(psi, 1), {e: -c for e, c in poly_diff(psi, 0).items()}]
    A = [poly_random(3, degree + 1, rng) for _ in range(3)]
    return [poly_sub(poly_diff(A[2], 1), poly_diff(A[1], 2)), poly_sub(poly_diff(A[0], 2), poly_diff(A[2], 0)),
            poly_sub(poly_diff(A[1], 0), poly_diff(A[0], 1))]


def sides_of(mid):
    """(axis, sign) of the side of [-1, 1]^dim a facet midpoint lies on."""
    axis = np.argmax(np.abs(mid), axis=1)
    return axis, np.sign(mid[np.arange(mid.shape[0]), axis])


def _forms(dim, N, deg, kind):
    from tests.test_wall_stress_host import _forms as forms

    if kind == "rolled":  # the Delaunay mesh with the vertices of cell c rotated c times: every local facet index occurs
        from oracle import ipcs_oracle as O
        from tests.helpers import delaunay_box_mesh

        coords, cells = delaunay_box_mesh(N, dim=dim, seed=2)
        idx = (np.arange(dim + 1)[None, :] + np.arange(cells.shape[0])[:, None]) % (dim + 1)
        F = O.Forms(coords, np.take_along_axis(cells, idx, axis=1), deg, 2 if deg == 3 else 1)
    else:
        F, _ = forms(dim, N, deg, kind)
    fc, fa = F.exterior_facets()
    order = np.lexsort((fa, fc))
    if kind == "rolled":
        assert set(fa.tolist()) == set(range(dim + 1))
    return F, fc[order], fa[order]


def _closed_form_check(F, fc, fa, u_dofs, field, what):
    """Per side: model flux = the closed form, to 1e-12 sum_f |f| |ubar_f| (the scale the device test uses)."""
    dim = F.d
    flux = OM.facet_flux(F.coords, F.cells, fc, fa, F.vd, u_dofs, F.u_deg)
    _, meas, mid = WM.facet_geometry(F.coords, F.cells, fc, fa)
    axis, sign = sides_of(mid)
    ubar_n = np.abs(flux)  # |f| |n . ubar| <= |f| |ubar|
    worst = 0.0
    for k in range(dim):
        for s in (-1.0, 1.0):
            sel = (axis == k) & (sign == s)
            exact = s * poly_side_integral(field[k], k, s)
            scale = max(ubar_n[sel].sum(), meas[sel].sum() * np.abs(u_dofs).max())
            worst = max(worst, abs(flux[sel].sum() - exact) / scale)
    print(f"{what}: max |Q - exact| / scale = {worst:.3e}")
    return flux, worst


# ---- 1. flux -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_flux_of_polynomial_fields_equals_the_closed_form(dim, N, deg, kind):
    """A random polynomial field of degree <= DU, interpolated at the dofs: the flux through each side of [-1, 1]^d equals
    s int u_k(x | x_k = s) dS, monomial by monomial."""
    F, fc, fa = _forms(dim, N, deg, kind)
    rng = np.random.default_rng(3 + 10 * dim + deg)
    field = [poly_random(dim, deg, rng) for _ in range(dim)]
    u = np.stack([poly_eval(p, F.x_v) for p in field], axis=1)
    _, worst = _closed_form_check(F, fc, fa, u, field, f"{kind} ({dim},{N},{deg})")
    assert worst <= 1e-12


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_fluxes_of_a_solenoidal_field_sum_to_zero(dim, N, deg, kind):
    F, fc, fa = _forms(dim, N, deg, kind)
    field = solenoidal_field(dim, deg, np.random.default_rng(7 + 10 * dim + deg))
    u = np.stack([poly_eval(p, F.x_v) for p in field], axis=1)
    flux, worst = _closed_form_check(F, fc, fa, u, field, f"{kind} ({dim},{N},{deg}) solenoidal")
    assert worst <= 1e-12
    assert np.abs(flux).sum() > 0.1 and abs(flux.sum()) <= 1e-12 * np.abs(flux).sum()


# ---- 2. the recurrences --------------------------------------------------------------------------------------------------
def test_windkessel_recurrence():
    """One step equals the formula; with a constant Q, Pc -> p_distal + Rd Q (the contraction factor per step is
    1 / (1 + dt/(Rd C)): after n steps the distance has shrunk by that to the n)."""
    Rp, C, Rd, pd, dt, Q = 0.7, 0.4, 3.0, 1.5, 0.05, 2.0
    Pc1, P1 = OM.windkessel_step(0.25, Q, dt, Rp, C, Rd, pd)
    want = (0.25 + (dt / C) * (Q + pd / Rd)) / (1.0 + dt / (Rd * C))
    assert Pc1 == want and P1 == want + Rp * Q
    # it solves the backward-Euler equation C (Pc1 - Pc0) / dt = Q - (Pc1 - pd) / Rd
    assert abs(C * (Pc1 - 0.25) / dt - (Q - (Pc1 - pd) / Rd)) <= 16 * EPS * Q
    Pc, n = 0.25, 400
    for _ in range(n):
        Pc, P = OM.windkessel_step(Pc, Q, dt, Rp, C, Rd, pd)
    lim = pd + Rd * Q
    rate = 1.0 / (1.0 + dt / (Rd * C))
    assert abs(Pc - lim) <= abs(0.25 - lim) * rate ** n * (1 + 1e-9) + 64 * EPS * lim
    assert abs(P - (lim + Rp * Q)) <= 1e-6 * lim


def test_resistance_is_the_limit_without_the_capacitor():
    """C -> 0: the capacitor follows at once, Pc = p_distal + Rd Q, so P = p_distal + (Rp + Rd) Q = Resistance(Rp + Rd);
    the step's distance to that limit is |Pc0 - limit| / (1 + dt/(Rd C)) <= |Pc0 - limit| Rd C / dt."""
    Rp, Rd, pd, dt, Q, C = 0.7, 3.0, 1.5, 0.05, -2.0, 1e-13
    _, P = OM.windkessel_step(0.25, Q, dt, Rp, C, Rd, pd)
    want = OM.resistance(Q, Rp + Rd, pd)
    assert abs(P - want) <= abs(0.25 - (pd + Rd * Q)) * Rd * C / dt + 1e-12 * abs(want)
    o = OM.Outlet([], [], ("resistance", 2.0, 0.5, 1.25))
    assert o.advance(3.0, 0.1) == (0.5 + 2.0 * 3.0) / 1.25


# ---- 3. the backflow matrix ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_backflow_matrix_properties(dim, N, deg, kind):
    """B on the side x_0 = +1: symmetric; x^T B x >= 0; zero when u_ab . n >= 0 on every facet; for u_ab = -c n it is c
    times the facet mass matrix, whose entries sum to c |Gamma| (the rule integrates phi_r phi_s, degree 2 DU, exactly)."""
    F, fc, fa = _forms(dim, N, deg, kind)
    _, meas, mid = WM.facet_geometry(F.coords, F.cells, fc, fa)
    axis, sign = sides_of(mid)
    sel = (axis == 0) & (sign > 0)
    fc, fa, area = fc[sel], fa[sel], meas[sel].sum()
    assert abs(area - 2.0 ** (dim - 1)) <= 1e-12
    rng = np.random.default_rng(11)
    # a field whose normal component changes sign across the side
    uab = np.zeros((F.nv, dim))
    uab[:, 0] = F.x_v[:, 1] + 0.3 * rng.standard_normal(F.nv)
    B = OM.backflow_matrix(F.coords, F.cells, fc, fa, F.vd, uab, deg, 1.0, F.nv)
    assert B.nnz > 0 and abs(B - B.T).max() <= 1e-15 * abs(B).max()
    for _ in range(5):
        x = rng.standard_normal(F.nv)
        assert x @ (B @ x) >= -1e-14 * abs(B).max() * (x @ x)
    uab[:, 0] = np.abs(uab[:, 0]) * (F.x_v[:, 0] > -2.0)  # u . n >= 0 at every dof ...
    if deg == 1:  # ... which, for P1, means everywhere on the facet
        assert abs(OM.backflow_matrix(F.coords, F.cells, fc, fa, F.vd, uab, deg, 1.0, F.nv)).max() == 0.0
    uab[:, 0] = 0.8  # pure outflow: exactly zero for every degree (a constant is reproduced up to rounding << 0.8)
    assert abs(OM.backflow_matrix(F.coords, F.cells, fc, fa, F.vd, uab, deg, 1.0, F.nv)).max() == 0.0
    c = 1.7
    uab[:, 0] = -c
    Bm = OM.backflow_matrix(F.coords, F.cells, fc, fa, F.vd, uab, deg, 1.0, F.nv)
    assert abs(Bm.sum() - c * area) <= 1e-12 * c * area
    # the facet mass matrix itself, with a rule of higher order
    Mref = np.zeros((F.nv, F.nv))
    for f, (cell, a) in enumerate(zip(fc, fa)):
        pts, w = WM.facet_points(dim, a)
        from oasisx_amd import fem

        phi = fem.lagrange_basis(dim, deg, pts)
        dofs = F.vd[cell]
        Mref[np.ix_(dofs, dofs)] += meas[sel][f] * np.einsum("q,qr,qs->rs", w, phi, phi)
    if 2 * deg <= 5:  # (the reference rule is exact to degree 5)
        assert np.abs(Bm.toarray() - c * Mref).max() <= 1e-12 * c * np.abs(Mref).max()
    # beta per facet scales the facet's block
    beta = np.linspace(0.1, 1.0, fc.shape[0])
    B2 = OM.backflow_matrix(F.coords, F.cells, fc, fa, F.vd, uab, deg, beta, F.nv)
    assert abs(B2.sum() - c * (beta * meas[sel]).sum()) <= 1e-12 * c * area


# ---- 4. parameters -------------------------------------------------------------------------------------------------------
def test_parameter_validation():
    """Invalid parameters raise ValueError at construction, with no GPU and no library."""
    import oasisx_amd as ox

    for bad in (lambda: ox.Resistance(-1.0), lambda: ox.Resistance(1.0, rho=0.0), lambda: ox.Resistance(float("inf")),
                lambda: ox.Windkessel(-0.1, 1.0, 1.0), lambda: ox.Windkessel(0.1, 1.0, -1.0),
                lambda: ox.Windkessel(0.1, 0.0, 1.0), lambda: ox.Windkessel(0.1, -2.0, 1.0),
                lambda: ox.Windkessel(0.1, 1.0, 1.0, rho=-1.0), lambda: ox.Windkessel(0.1, 1.0, float("nan")),
                lambda: ox.Windkessel(0.1, 1.0, 1.0, p_distal=float("inf")), lambda: ox.Windkessel(0.1, 1.0, 1.0, p0=float("nan")),
                lambda: ox.PressureBC(1.0, (None, 1), backflow=-0.1), lambda: ox.PressureBC(1.0, (None, 1), backflow=1.01),
                lambda: ox.PressureBC(1.0, (None, 1), backflow=float("nan"))):
        with pytest.raises(ValueError):
            bad()
    w = ox.Windkessel(0.1, 2.0, 3.0, p_distal=0.5)
    assert w.p0 == 0.5 and w.initial_h() == 0.5 and ox.Windkessel(0.1, 2.0, 3.0, p0=4.0, rho=2.0).initial_h() == 2.0
    assert ox.Resistance(0.0).R == 0.0 and ox.PressureBC(1.0, (None, 1)).backflow == 0.0
    with pytest.raises(RuntimeError):
        w.history()


# ---- 5. the generated tables ---------------------------------------------------------------------------------------------
def _tables():
    text = open(os.path.join(ROOT, "oasisx_amd", "csrc", "fe_tables_o.h")).read()
    out = {}
    for m in re.finditer(r"static constexpr (?:double|int) (\w+)((?:\[\d+\])+) = \{(.*?)\};", text, re.S):
        shape = tuple(int(s) for s in re.findall(r"\[(\d+)\]", m.group(2)))
        vals = np.array([float(v) for v in re.findall(r"-?\d+(?:\.\d+(?:e-?\d+)?)?", m.group(3))])
        out[m.group(1)] = vals.reshape(shape)
    return out


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("degree", [1, 2, 3])
def test_tables_equal_the_models_rule(d, degree):
    """Weights, facet dofs and the basis at the rule's points equal the model's, point by point in the model's order (the
    generator builds the rule the same way); the P3 facet means equal the model's quadrature means.

    Tolerance: a table entry is the exact value rounded once; the model's weights and points come from scipy's
    Gauss-Jacobi roots (a few eps), its P3 basis from the numerically inverted monomial Vandermonde matrix V of the P3
    nodes, relative error cond(V) eps in the coefficients: (64 + cond(V) [degree 3]) eps on values of size <= ~1."""
    from oasisx_amd import fem
    from oasisx_amd.outlet import facet_dofs

    T = _tables()
    cond = float(np.linalg.cond(fem._p3_mono(d, fem.p3_nodes(d))[0])) if degree == 3 else 0.0
    tol = (64 + cond) * EPS
    _, w = OM.facet_rule(d, degree)
    assert T[f"OX_OW{d}_{degree}"].shape == w.shape and np.abs(T[f"OX_OW{d}_{degree}"] - w).max() <= tol
    for a in range(d + 1):
        pts, _ = OM.facet_points(d, degree, a)
        phi = fem.lagrange_basis(d, degree, pts)
        on = facet_dofs(d, degree, a)
        assert np.array_equal(T[f"OX_OFD{d}_{degree}"][a].astype(np.int64), on)
        off = np.setdiff1d(np.arange(phi.shape[1]), on)
        assert np.abs(phi[:, off]).max(initial=0.0) <= tol  # the other functions vanish on the facet
        err = np.abs(T[f"OX_OPHI{d}_{degree}"] - phi[:, on]).max()  # one table for every local facet
        print(f"d={d} degree={degree} facet {a}: max |table - model| = {err:.3e} (tol {tol:.3e})")
        assert err <= tol
        if degree == 3:
            assert np.abs(T[f"OX_PHIF{d}_3"][a] - w @ phi).max() <= (w.shape[0] + 1) * tol
