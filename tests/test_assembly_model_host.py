"""CPU: the extended-precision assembly model (tests/assembly_model.py) and the mesh zoo (tests/hard_meshes.py).

* the model against ``oracle.ipcs_oracle.Forms`` -- another correct evaluation, in float64 and in a different order -- on an
  ordinary mesh and on every zoo mesh, entry by entry, under the criterion of the device tests;
* identities of the model itself, each to the bound of the extended type;
* the criterion can fail: it flags a dropped (row, cell) contribution and a relative 1e-10 change of one small entry,
  which the suite's older ``1e-12 * max`` criterion accepts -- the gap the device tests close;
* the zoo has the properties it was designed for (row widths, aspect ratios, orientation, entry ranges)."""
import numpy as np
import pytest

from oracle import ipcs_oracle as O
from tests import assembly_model as AM
from tests import hard_meshes as H

X_EPS = float(np.finfo(np.longdouble).eps) if AM.EXTENDED else 10.0 ** (1 - AM.mpmath.mp.dps)

ELEMENTS = {2: [(1, 1), (2, 1), (3, 2)], 3: [(1, 1), (2, 1), (3, 2)]}


def _cases():
    out = []
    for d in (2, 3):
        for u_deg, p_deg in ELEMENTS[d]:
            names = ["ordinary"] + list(H.zoo(d, u_deg))
            if d == 3 and u_deg == 3:
                names = ["stretched", "spindle254"]
            out += [(d, u_deg, p_deg, name) for name in names]
    return out


def _mesh(d, u_deg, name):
    return H.lattice(d, 3 if d == 2 else 2) if name == "ordinary" else H.zoo(d, u_deg)[name]


def _oracle_and_model(d, u_deg, p_deg, name):
    pts, cells = _mesh(d, u_deg, name)
    F = O.Forms(pts, cells, u_deg, p_deg)
    rec = np.concatenate([F.G[:, 1:, :].reshape(F.G.shape[0], -1), F.adet[:, None]], axis=1)
    rec = np.concatenate([rec, np.zeros((rec.shape[0], (6 if d == 2 else 10) - rec.shape[1]))], axis=1)
    # the oracle's own float64 geometry records: its LAPACK inversion is not what this comparison is about
    geo = AM.geometry_from_records(rec)
    Mo = AM.Model(geo, F.vd, F.nv, u_deg, F.qd, F.nq, p_deg)
    # P3: the oracle's coefficient table is a float64 inverse; what that does to an entry is bounded by the same assembly
    # with the table's measured error added to the absolute tables (the device's tables were made in mpmath: no such term)
    Mo.with_oracle_error = AM.Model(geo, F.vd, F.nv, u_deg, F.qd, F.nq, p_deg, tab_err={3: AM.p3_coefficient_error(d)}) \
        if u_deg == 3 else None
    return F, Mo


@pytest.mark.parametrize("d,u_deg,p_deg,name", _cases())
def test_model_matches_the_oracle_entry_by_entry(d, u_deg, p_deg, name):
    F, Mo = _oracle_and_model(d, u_deg, p_deg, name)
    rng = np.random.default_rng(5)
    uab, u, p = rng.standard_normal((F.nv, d)), rng.standard_normal((F.nv, d)), rng.standard_normal(F.nq)
    worst = {}

    Me = Mo.with_oracle_error

    def hold(what, dev, form, *args):
        res = getattr(Mo, form)(*args)
        val, B, n = (res.val, res.B, res.n) if isinstance(res, AM.Entries) else res
        extra = None
        if Me is not None:
            r2 = getattr(Me, form)(*args)
            extra = (r2.B if isinstance(r2, AM.Entries) else r2[1]) - B
        dev = dev(res) if callable(dev) else dev
        ok, r, allow = AM.check(dev, val, B, n, extra)
        worst[what] = r
        assert ok, (what, r, allow)

    for what, form, args, A in (("M", "mass", ("v",), F.mass_v()), ("Mq", "mass", ("q",), F.mass_q()),
                                ("K", "stiffness", ("v",), F.stiffness_v()), ("Kq", "stiffness", ("q",), F.stiffness_q()),
                                ("C", "convection", (uab,), F.convection(uab))):
        hold(what, lambda E, A=A: E.lookup(A), form, *args)
    for fam, mats in ((0, F.p_vdxi_mat), (1, F.grad_p_mat), (2, F.divu_mat)):
        hold("rect%d" % fam, lambda E, mats=mats: np.stack([E.lookup(mats(i)) for i in range(d)], axis=1), "rect", fam)
    hold("grad0", np.stack([F.p_vdxi_vec(p, i) for i in range(d)], axis=1), "grad_vector", 0, p)
    hold("grad1", np.stack([F.grad_p_vec(p, i) for i in range(d)], axis=1), "grad_vector", 1, p)
    hold("div", F.divu_vec(u), "div_vector", u)
    hold("weights", F.body_force_vec(1.0), "weights", "v")
    print(f"model vs oracle {d}-D P{u_deg}-P{p_deg} {name}: max err / (u B) " + " ".join(f"{k}={v:.1f}" for k, v in worst.items()))


@pytest.mark.parametrize("d,u_deg,p_deg,name", [(2, 2, 1, "stretched"), (2, 3, 2, "fan254"), (3, 2, 1, "flipped"), (3, 1, 1, "squashed")])
def test_identities_of_the_model(d, u_deg, p_deg, name):
    F, Mo = _oracle_and_model(d, u_deg, p_deg, name)
    rng = np.random.default_rng(6)
    uab, u, p = rng.standard_normal((F.nv, d)), rng.standard_normal((F.nv, d)), rng.standard_normal(F.nq)
    x = Mo._e
    ones_v = x(np.ones(F.nv))

    def zero(what, val, B, n):  # |val| <= eps of the extended type * (n + 2) B, entry by entry
        r = AM.to_f64(AM.absx(val)) / (X_EPS * (np.asarray(n) + 2) * np.maximum(B, 1e-300))
        assert float(np.max(r)) <= 1.0, (what, float(np.max(r)))

    def rowsum(E, val=None, B=None):
        Bs = np.zeros((E.shape[0],) + E.B.shape[1:])
        np.add.at(Bs, E.rows, E.B * (E.n + 2 if E.B.ndim == 1 else (E.n + 2)[:, None]))
        return Bs

    K, M, C = Mo.stiffness("v"), Mo.mass("v"), Mo.convection(uab)
    zero("rows of K", K.matvec(ones_v), rowsum(K), 1)
    zero("rows of C", C.matvec(ones_v), rowsum(C), 1)
    vol = Mo.geo.adet.sum() / (2 if d == 2 else 6)
    tot = M.val.sum()
    assert abs(float(tot - vol)) <= X_EPS * float(((M.n + 2) * M.B).sum())
    w, Bw, nw = Mo.weights("v")
    zero("weights = row sums of M", M.matvec(ones_v) - w, rowsum(M) + Bw * (nw + 2), 1)
    # matrix forms times a vector = the matrix-free vector forms
    for fam, vec, xin in ((0, Mo.grad_vector(0, p), p), (1, Mo.grad_vector(1, p), p)):
        E = Mo.rect(fam)
        zero("rect%d p" % fam, E.matvec(x(xin)) - vec[0], rowsum(E) * np.abs(p).max() + vec[1] * (vec[2] + 2), 1)
    E = Mo.rect(2)
    dv = Mo.div_vector(u)
    got = (E.val * x(u)[E.cols]).sum(axis=1)
    acc = np.zeros(F.nq, dtype=got.dtype) + got[0] * 0
    np.add.at(acc, E.rows, got)
    zero("rect2 u", acc - dv[0], rowsum(E).sum(axis=1) * np.abs(u).max() + dv[1] * (dv[2] + 2), 1)


def test_load_vector_of_a_polynomial_is_exact():
    """The table sum over a positive rule of enough degree equals the exact integral of (l1 . (1, x)) (l2 . (1, x)) phi_i."""
    pts, cells = H.stretched(2)
    F, Mo = _oracle_and_model(2, 2, 1, "stretched")
    a1, a2 = np.array([0.3, 1e-4, -0.7]), np.array([-1.1, 2e-4, 0.4])
    xe = Mo._e(pts)
    l1 = (xe @ Mo._e(a1[1:]) + Mo._e(a1[0]))[cells]
    l2 = (xe @ Mo._e(a2[1:]) + Mo._e(a2[0]))[cells]
    exact = Mo.load_vector_poly(l1, l2)
    bary, w = O.simplex_quadrature(2, 3)  # degree 5 >= 2 + 2
    phi, _ = O.tabulate(2, 2, bary)
    be = AM._einsum("cqa,ca->cq", Mo._e(np.broadcast_to(bary, (cells.shape[0],) + bary.shape).copy()), l1)
    fq = be * AM._einsum("cqa,ca->cq", Mo._e(np.broadcast_to(bary, (cells.shape[0],) + bary.shape).copy()), l2)
    tab = Mo.geo.adet[:, None] * AM._einsum("qi,cq->ci", Mo._e(w[:, None] * phi), fq)
    val, _, _ = AM._scatter_vec(tab, F.vd, F.nv)
    Bv = np.zeros(F.nv)
    np.add.at(Bv, F.vd.ravel(), (Mo.geo.aadet[:, None] * np.einsum("qi,cq->ci", np.abs(w[:, None] * phi), np.abs(AM.to_f64(fq)))).ravel())
    # the rule's own nodes and weights are float64 roundings: the table sum is exact to float64's, not the extended type's
    assert np.max(AM.to_f64(AM.absx(val - exact)) / Bv) <= 64 * AM.U


# ---- the criterion can fail ------------------------------------------------------------------------------------------
def test_the_criterion_flags_what_the_max_norm_accepts():
    F, Mo = _oracle_and_model(2, 2, 1, "stretched")
    K = Mo.stiffness("v")
    dev = AM.to_f64(K.val)  # a correctly rounded device result
    assert AM.check(dev, K.val, K.B, K.n)[0]
    big = np.abs(dev).max()
    old_accepts = lambda a: np.abs(a - dev).max() <= 1e-12 * big  # noqa: E731 -- the criterion of test_gpu_parity & co.
    # one (row, cell) contribution removed: the cell whose contribution to some small entry is largest relative to it
    Ae, Be = Mo._stiff_e(2)
    small = np.nonzero((np.abs(dev) <= 1e-5 * big) & (np.abs(dev) > 0))[0]
    assert small.size > 0
    k = small[np.argmax(np.abs(dev[small]))]
    r, c = int(K.rows[k]), int(K.cols[k])
    cell, i = next((e, i) for e in range(F.vd.shape[0]) for i in range(F.vd.shape[1])
                   if F.vd[e, i] == r and c in F.vd[e] and float(abs(Ae[e, i, list(F.vd[e]).index(c)])) > 0)
    Ae2 = Ae.copy()
    Ae2[cell, i, :] = 0
    _, _, val2, _, _ = AM._scatter(Ae2, F.vd, F.vd, (F.nv, F.nv))
    dropped = AM.to_f64(val2)
    assert not AM.check(dropped, K.val, K.B, K.n)[0]
    # one entry of magnitude <= 1e-5 max changed by a relative 1e-10
    nudged = dev.copy()
    nudged[k] *= 1.0 + 1e-10
    assert abs(dev[k]) <= 1e-5 * big and nudged[k] != dev[k]
    ok, ratio, allow = AM.check(nudged, K.val, K.B, K.n)
    assert not ok and ratio > allow
    assert old_accepts(nudged)  # the gap: ten orders above rounding, accepted
    # an entry that is NaN (a slot the kernel never wrote: the device tests pre-fill their outputs with NaN) or infinite
    for poison in (np.nan, np.inf, -np.inf):
        broken = dev.copy()
        broken[k] = poison
        ok, ratio, allow = AM.check(broken, K.val, K.B, K.n)
        assert not ok and not ratio <= allow
    two_d = np.stack([dev, dev], axis=1)
    two_d[3, 1] = np.nan
    assert not AM.check(two_d, np.stack([K.val, K.val], axis=1), np.stack([K.B, K.B], axis=1), K.n)[0]
    # (a correct value in another order of summation stays inside: the float64 oracle)
    assert AM.check(K.lookup(F.stiffness_v()), K.val, K.B, K.n)[0]


# ---- the zoo -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [1, 2, 3])
def test_designed_row_widths(degree):
    for k, width in H.FAN_K[degree]:
        row = H.widest_row(H.fan(k), degree)
        assert row == H.fan_row(k, degree) and H.width_of(row) == width, ("fan", degree, k, row)
    for k, width in H.SPINDLE_K[degree]:
        row = H.widest_row(H.spindle(k), degree)
        assert row == H.spindle_row(k, degree) and H.width_of(row) == width, ("spindle", degree, k, row)
    # each neighbouring pair straddles one switch point of the row launch; the last is the widest the position bytes hold
    for table in (H.FAN_K[degree], H.SPINDLE_K[degree]):
        w = [x[1] for x in table]
        for lim in (67, 70, 134, 140):
            assert any(a <= lim for a in w) and any(a > lim for a in w)
        assert max(w) <= 254 and max(w) >= 252
    assert H.width_of(H.fan_row(H.WIDEST[("fan", degree)] + 1, degree)) > 255
    assert H.width_of(H.spindle_row(H.WIDEST[("spindle", degree)] + 1, degree)) > 255


@pytest.mark.parametrize("kind,degree", [("fan", 1), ("fan", 2), ("spindle", 1), ("spindle", 2)])
def test_widths_of_the_built_pattern_and_the_refusal_of_the_torch_set_up(kind, degree):
    """The torch twin of the set-up on the host: the widest fan / spindle has a 254 (252) wide row; one k more is refused."""
    from oasisx_amd import fem
    from oasisx_amd import mesh as M

    k = H.WIDEST[(kind, degree)]
    make = (lambda kk: H.fan(kk, 3.0, 1.0)) if kind == "fan" else H.spindle
    V = fem.FunctionSpace(M.from_arrays(*make(k), device="cpu"), degree, window=256)
    row = H.fan_row(k, degree) if kind == "fan" else H.spindle_row(k, degree)
    assert int(V.pattern.row_len.max()) == row and int(V.pattern.widths.max()) == H.width_of(row) in (252, 254)
    with pytest.raises(ValueError, match="longer than 255 entries"):
        fem.FunctionSpace(M.from_arrays(*make(k + 1), device="cpu"), degree, window=256)


def test_zoo_shapes_orientation_and_entry_ranges():
    # aspect ratios
    assert H.aspect_ratio(H.stretched(2)).min() > 1e3 and H.aspect_ratio(H.stretched(3)).min() > 1e3
    assert H.aspect_ratio(H.squashed()).min() > 1e5
    assert H.aspect_ratio(H.widest("fan", 1)).min() > 10 and H.aspect_ratio(H.widest("spindle", 1)).min() > 10  # slivers
    sq_pts, sq_cells = H.squashed()
    edges = np.linalg.norm(sq_pts[sq_cells[:, 1:]] - sq_pts[sq_cells[:, :1]], axis=2)
    assert edges.max() > 0.5  # O(1) edges on nearly flat cells
    tf = H.tiny_far(3)[0]
    assert tf.min() > 999.0 and np.ptp(tf, axis=0).max() < 3e-3
    # orientation: flipping changes the sign of every second cell; both signs are present
    for d in (2, 3):
        base, fl = H.signed_det(H.stretched(d)), H.signed_det(H.flipped(H.stretched(d)))
        sel = H.flipped_cells(base.shape[0])
        keep = np.setdiff1d(np.arange(base.shape[0]), sel)
        assert sel.shape[0] == base.shape[0] // 2
        assert (np.sign(fl[sel]) == -np.sign(base[sel])).all() and (np.sign(fl[keep]) == np.sign(base[keep])).all()
        assert (fl > 0).sum() >= fl.shape[0] // 4 and (fl < 0).sum() >= fl.shape[0] // 4
    # entry ranges of at least 1e5 (non-zero entries, relative to the largest)
    rng = np.random.default_rng(2)
    # (the stretched lattices are the ones designed for the range; the elliptic fan reaches 4e4 with P2)
    for d, name, forms, span in ((2, "stretched", ("K", "C"), 1e5), (3, "stretched", ("K", "C"), 1e5), (2, "fan254", ("K",), 1e4)):
        F, Mo = _oracle_and_model(d, 2, 1, name)
        for f in forms:
            E = Mo.stiffness("v") if f == "K" else Mo.convection(rng.standard_normal((F.nv, d)))
            a = np.abs(AM.to_f64(E.val))
            a = a[a > 64 * AM.U * E.B]  # entries that are not zero by cancellation
            assert a.max() / a.min() >= span, (d, name, f, a.max() / a.min())


def test_geometry_closed_forms_against_exact_rationals():
    """geometry_from_coords against the same closed forms over Fractions on a few cells of every zoo mesh."""
    from fractions import Fraction

    for mesh in (H.stretched(2), H.tiny_far(2), H.squashed(), H.flipped(H.stretched(3)), H.widest("spindle", 1)):
        pts, cells = mesh[0], mesh[1][:4]
        rec, tol, cancel = AM.geometry_from_coords(pts, cells)
        d = pts.shape[1]
        for c in range(cells.shape[0]):
            x = [[Fraction(float(v)) for v in pts[cells[c, a]]] for a in range(d + 1)]
            J = [[x[a + 1][k] - x[0][k] for a in range(d)] for k in range(d)]  # columns = edge vectors
            inv = AM._solve(J, d)
            det = J[0][0] * J[1][1] - J[0][1] * J[1][0] if d == 2 else sum(
                J[0][i] * (J[1][(i + 1) % 3] * J[2][(i + 2) % 3] - J[1][(i + 2) % 3] * J[2][(i + 1) % 3]) for i in range(3))
            want = [inv[a][k] for a in range(d) for k in range(d)] + [abs(det)]
            for j, wv in enumerate(want):
                assert abs(float(rec[c, j]) - float(wv)) <= 4 * X_EPS * max(cancel[c], 1.0) * abs(float(wv)) + 1e-300


def test_the_model_runs_in_mpmath_where_longdouble_is_no_wider():
    """The fallback of the extended type (arrays of mpmath.mpf): same code, same values."""
    pts, cells = H.lattice(2, 2)
    F = O.Forms(pts, cells, 2, 1)
    rec = np.concatenate([F.G[:, 1:, :].reshape(-1, 4), F.adet[:, None], np.zeros((cells.shape[0], 1))], axis=1)
    uab = np.random.default_rng(1).standard_normal((F.nv, 2))
    got = {}
    for extended in ([True, False] if AM.EXTENDED else [False]):
        Mo = AM.Model(AM.geometry_from_records(rec, extended), F.vd, F.nv, 2, F.qd, F.nq, 1)
        got[extended] = (Mo.stiffness("v"), Mo.convection(uab), Mo.grad_vector(0, np.arange(F.nq) * 0.25, scale=-2.0))
    K, C, g = got[False]
    assert K.val.dtype == object
    assert AM.check(K.lookup(F.stiffness_v()), K.val, K.B, K.n)[0] and AM.check(C.lookup(F.convection(uab)), C.val, C.B, C.n)[0]
    if AM.EXTENDED:
        for a, b in zip(got[True], got[False]):
            va, vb = (a.val, b.val) if hasattr(a, "val") else (a[0], b[0])
            assert np.max(np.abs(AM.to_f64(va) - AM.to_f64(vb))) <= 4 * AM.U * np.max(np.abs(AM.to_f64(va)))


@pytest.mark.parametrize("d,degree", [(2, 1), (2, 2), (2, 3), (3, 1), (3, 2), (3, 3)])
def test_bases_are_nodal_and_sum_to_one(d, degree):
    nd = AM.nodes(d, degree)
    for j, x in enumerate(nd):
        vals = AM.basis_at(d, degree, x)
        assert all(abs(float(v) - (1.0 if i == j else 0.0)) < 1e-40 for i, v in enumerate(vals))
    w = AM.ref("weights", d, degree)
    assert abs(float(w.sum()) - (0.5 if d == 2 else 1.0 / 6.0)) < 1e-18


def test_tabulated_rect_tensor_of_the_p3_tetrahedron_is_the_exact_one():
    """``OX_RECT0_3H`` (csrc/fe_tables_h3.h, written by tools/gen_tables_p3_tet.py): int psi_j d(phi_i)/d(lambda_b), b = 1..3,
    against the model's tensor -- two independent mpmath evaluations (the rule in 40 digits there, monomial integrals
    here): equal to the last bit of float64 where the value is not zero, exact zeros where it is."""
    import os
    import re

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oasisx_amd", "csrc", "fe_tables_h3.h")
    with open(path) as fh:
        m = re.search(r"OX_RECT0_3H\[20\]\[10\]\[3\] = (\{.*?\});", fh.read(), re.S)
    T = np.array([float(v) for v in re.findall(r"[-+]?\d+\.?\d*(?:[eE][-+]?\d+)?", m.group(1))]).reshape(20, 10, 3)
    exact = AM._tensor(3, [(2, None), (3, 1)]), AM._tensor(3, [(2, None), (3, 2)]), AM._tensor(3, [(2, None), (3, 3)])
    assert all(abs(float(v)) < 1e-45 for v in AM._tensor(3, [(2, None), (3, 0)]).ravel())  # the lambda_0 column
    for b in range(3):
        for j in range(10):
            for i in range(20):
                want = float(exact[b][j, i])  # (mpf -> float64: rounded once)
                assert T[i, j, b] == (want if abs(want) > 1e-40 else 0.0), (i, j, b, T[i, j, b], want)
    assert np.abs(T).max() > 0.05
