"""Entry-by-entry reference of the assembly kernels in extended precision (plain numpy + mpmath: importable without a GPU).

Written from the forms (reference fracstep.py lines as quoted in oracle/ipcs_oracle.py), not from the kernels and not from
``oracle.ipcs_oracle.Forms``:

* the Lagrange bases are polynomials in barycentric monomials lambda^alpha: written down over ``fractions.Fraction`` for
  P1 / P2 (exact); for P3 the solution of the Vandermonde system at the nodes in ``mpmath`` at 50 digits -- its edge nodes
  are the Gauss-Lobatto-Legendre points (1 -+ 1/sqrt 5)/2 (``oracle.ipcs_oracle.GLL3`` is their float64 rounding);
* reference tensors come from the exact simplex formula  int_K lambda^alpha = |K| d! alpha! / (|alpha| + d)!;
* everything downstream is ``np.longdouble`` (``EXTENDED``, the convention of tests/krylov_steps_model.py); where that is
  no wider than float64 the arrays hold ``mpmath.mpf`` objects instead (same code, slower).

Geometry has two entry points: ``geometry_from_coords`` (the closed forms of k_geometry / fem.cell_geometry in extended
precision, with the running bound of those expressions) and ``geometry_from_records`` (the device's float64 rows
``[grad lambda_1..d, |det J|]`` promoted exactly) -- the assembly comparisons use the device's own records, so the
ill-conditioned inversion on flat cells is tested once and not mixed into every matrix tolerance.

Every form returns ``(value, B, n)`` per entry.  ``B`` is the running error bound: the same assembly with every factor
replaced by its absolute value (|G| with |G_0| := sum_a |G_a|, the absolute basis values under a positive-weight rule of
the oracle -- two correct digits are enough --, |u|, |M|, |K|, 1/dt, nu).  ``n`` is the length of the longest rounded
chain: the cells that meet in the entry + the per-cell chain of the form (``chain`` below, counted from the kernel lines
it quotes, one rounding for each tabulated constant) + the epilogue.  The criterion is the standard forward bound
``|dev - value| <= (n + 2) 2^-53 B``: it holds for any summation order, with or without fma.  ``n <= 1024`` is asserted
everywhere, so no tolerance exceeds about 1.2e-13 B.

(``B`` is the running bound of a kernel whose own rule has positive weights.  The P3-tetrahedron kernels tabulate on the
70-point Grundmann-Moeller rule, sum |w| / sum w = 25.4: their terms are that much larger than ``B``, and their measured
errors stand out accordingly; family 0 of ox_assemble_rect, which missed the criterion that way, now contracts a tabulated
tensor instead -- tests/test_gpu_assembly_entries.py)

The scalar row kernels (``scalar_rows``, ``scalar_rows_cellvisc``, ``scalar_rows_supg``: DESIGN.md sections 13, 25, 32) take
the device's own A, M, K and the device's own SUPG records (w_c, tau_c), promoted exactly; ``supg_cells`` models those
records, tau_c under a propagated absolute bound (tests/test_gpu_scalar_rows_entries.py)."""
from __future__ import annotations

import itertools
import math
from fractions import Fraction

import mpmath
import numpy as np

from oracle import ipcs_oracle as O
from tests.krylov_steps_model import EXTENDED

U = 2.0 ** -53
N_MAX = 1024
mpmath.mp.dps = 50


# ---- the extended type ---------------------------------------------------------------------------------------------
def ext(a, extended=None):
    """float64 (or Fraction / mpf) data promoted exactly to the extended type."""
    extended = EXTENDED if extended is None else extended
    a = np.asarray(a)
    if extended:
        if a.dtype == object:
            flat = [np.longdouble(mpmath.nstr(_mpf(v), 30)) for v in a.ravel()]
            return np.array(flat, dtype=np.longdouble).reshape(a.shape)
        return a.astype(np.longdouble)
    if a.dtype == object:
        return np.array([_mpf(v) for v in a.ravel()], dtype=object).reshape(a.shape)
    return np.array([mpmath.mpf(float(v)) for v in a.ravel()], dtype=object).reshape(a.shape)


def _mpf(v):
    if isinstance(v, Fraction):
        return mpmath.mpf(v.numerator) / mpmath.mpf(v.denominator)
    return mpmath.mpf(v)


def to_f64(a):
    a = np.asarray(a)
    return a.astype(np.float64) if a.dtype != object else np.array([float(v) for v in a.ravel()]).reshape(a.shape)


def absx(a):
    return np.abs(a) if a.dtype != object else np.array([abs(v) for v in a.ravel()], dtype=object).reshape(a.shape)


# ---- bases as polynomials in barycentric monomials -----------------------------------------------------------------
def monomials(d: int, degree: int):
    """Exponents (over lambda_0..lambda_d) of the monomials the basis of ``degree`` is written in -- the form the kernels'
    tabulation differentiates, so that no gradient of a barycentric coordinate enters an entry it does not enter there:
    P1: lambda_a;  P2: lambda_a^2, lambda_a, lambda_a lambda_b (phi = 2 lambda_a^2 - lambda_a, 4 lambda_a lambda_b);
    P3: every monomial of degree <= 3 in lambda_1..lambda_d alone (lambda_0 = 1 - sum eliminated, as in Basix' and the
    oracle's tabulation: the derivative with respect to lambda_0 is identically zero)."""
    nv = d + 1
    unit = lambda *on: tuple(sum(1 for o in on if o == b) for b in range(nv))  # noqa: E731
    if degree == 1:
        return [unit(a) for a in range(nv)]
    if degree == 2:
        return [unit(a, a) for a in range(nv)] + [unit(a) for a in range(nv)] + [unit(a, b) for a, b in O.local_edges(d)]
    return [(0,) + a for a in itertools.product(range(4), repeat=d) if sum(a) <= 3]


def nodes(d: int, degree: int):
    """Barycentric node coordinates in the product's local dof order (vertices, edges in ``local_edges`` order, then the
    cell's own dof / the faces): Fractions for P1 / P2, mpf for P3."""
    nv = d + 1
    one, zero = (Fraction(1), Fraction(0)) if degree < 3 else (mpmath.mpf(1), mpmath.mpf(0))
    out = [[one if b == a else zero for b in range(nv)] for a in range(nv)]
    if degree == 2:
        for a, b in O.local_edges(d):
            out.append([Fraction(1, 2) if c in (a, b) else zero for c in range(nv)])
    if degree == 3:
        s5 = 1 / mpmath.sqrt(5)
        gll = ((1 - s5) / 2, (1 + s5) / 2)
        assert all(abs(float(g) - h) < 1e-15 for g, h in zip(gll, O.GLL3))
        for a, b in O.local_edges(d):
            for t in gll:
                v = [zero] * nv
                v[a], v[b] = 1 - t, t
                out.append(v)
        third = mpmath.mpf(1) / 3
        faces = [(0, 1, 2)] if d == 2 else O.local_faces(3)
        for f in faces:
            out.append([third if c in f else zero for c in range(nv)])
    return out


def _solve(V, rhs_identity_n):
    """Gauss-Jordan inverse over any exact / multiprecision field (partial pivoting)."""
    n = rhs_identity_n
    one, zero = V[0][0] * 0 + 1, V[0][0] * 0
    A = [list(V[i]) + [one if j == i else zero for j in range(n)] for i in range(n)]
    for c in range(n):
        p = max(range(c, n), key=lambda r: abs(A[r][c]))
        A[c], A[p] = A[p], A[c]
        piv = A[c][c]
        A[c] = [v / piv for v in A[c]]
        for r in range(n):
            if r != c and A[r][c] != 0:
                f = A[r][c]
                A[r] = [vr - f * vc for vr, vc in zip(A[r], A[c])]
    return [row[n:] for row in A]


def _power(x, e):
    out = x[0] * 0 + 1
    for xv, ev in zip(x, e):
        out = out * xv ** ev
    return out


_BASIS = {}


def basis(d: int, degree: int):
    """(exponents [nm], coefficients C[m][i]): phi_i = sum_m C[m][i] lambda^exponents[m].  P1 / P2: written down
    (Fractions); P3: the inverse of the Vandermonde matrix at the nodes (mpmath)."""
    if (d, degree) not in _BASIS:
        ex = monomials(d, degree)
        nd = nodes(d, degree)
        nv = d + 1
        if degree < 3:
            C = [[Fraction(0)] * len(nd) for _ in ex]
            for a in range(nv):
                if degree == 1:
                    C[a][a] = Fraction(1)
                else:
                    C[a][a], C[nv + a][a] = Fraction(2), Fraction(-1)
            if degree == 2:
                for k in range(len(O.local_edges(d))):
                    C[2 * nv + k][nv + k] = Fraction(4)
        else:
            assert len(ex) == len(nd)
            C = _solve([[_power(x, e) for e in ex] for x in nd], len(ex))  # V[node][monomial]^-1: (monomial, function)
        assert len(nd) == O.num_cell_dofs(d, degree)
        _BASIS[(d, degree)] = (ex, np.array(C, dtype=object))
    return _BASIS[(d, degree)]


def p3_coefficient_error(d: int):
    """What the float64 coefficient table of the oracle's P3 basis (a LAPACK inverse) is off by, as absolute errors of its
    tabulation anywhere on the simplex (|monomial| <= 1, |d monomial / d lambda_b| <= its exponent): (nd,), (nd, d + 1)."""
    ex, C = basis(d, 3)
    dC = np.abs(np.array([[float(_mpf(float(co)) - c) for co, c in zip(ro, r)] for ro, r in zip(O._p3_coefficients(d), C)]))
    eb = np.array(ex, dtype=np.float64)  # (nm, d + 1)
    return dC.sum(axis=0), np.einsum("mi,mb->ib", dC, eb)


def basis_at(d: int, degree: int, x):
    """phi_i at one barycentric point (the field of ``x``)."""
    ex, C = basis(d, degree)
    m = [_power(x, e) for e in ex]
    return [sum((C[k][i] * m[k] for k in range(len(ex))), m[0] * 0) for i in range(C.shape[1])]


def _terms(d, degree, deriv=None):
    """The monomials of the basis (deriv None) or of its formal derivative d/d lambda_deriv: [(factor, exponents)]."""
    ex, _ = basis(d, degree)
    if deriv is None:
        return [(1, e) for e in ex]
    return [(e[deriv], tuple(v - (1 if b == deriv and v > 0 else 0) for b, v in enumerate(e))) for e in ex]


def _monomial_integral(d, e) -> Fraction:
    """int over the reference simplex of lambda^e, per unit |det J|: alpha! / (|alpha| + d)!."""
    num = 1
    for v in e:
        num *= math.factorial(v)
    return Fraction(num, math.factorial(sum(e) + d))


def _tensor(d, factors):
    """int prod_f (basis function or derivative) over the reference simplex per unit |det J|; ``factors`` = [(degree,
    deriv or None)]; result indexed [i_0, i_1, ...] in the order of ``factors`` (object array, Fraction or mpf)."""
    terms = [_terms(d, deg, dv) for deg, dv in factors]
    coefs = [basis(d, deg)[1] for deg, _ in factors]
    multi = any(deg == 3 for deg, _ in factors)
    shape = [len(t) for t in terms]
    base = np.empty(shape, dtype=object)
    cache = {}
    for idx in itertools.product(*[range(s) for s in shape]):
        f, e = 1, [0] * (d + 1)
        for t, i in zip(terms, idx):
            f *= t[i][0]
            if f == 0:
                break
            e = [a + b for a, b in zip(e, t[i][1])]
        if f == 0:
            base[idx] = Fraction(0)
            continue
        key = tuple(sorted(e))
        if key not in cache:
            cache[key] = _monomial_integral(d, key)
        base[idx] = f * cache[key]
    if multi:
        base = np.array([_mpf(v) for v in base.ravel()], dtype=object).reshape(shape)
        coefs = [np.array([_mpf(v) for v in c.ravel()], dtype=object).reshape(c.shape) for c in coefs]
    out = base
    for c in coefs:  # contract the leading (monomial) axis with C[m][i]; the new axis goes last: the order is kept
        out = np.tensordot(out, c, axes=([0], [0]))
    return out


_REF = {}


def ref(kind: str, d: int, *degs, extended=None):
    """Reference tensors in the extended type, cached.
    mass (p): [i][j]; stiff (p): [i][a][j][b]; conv (p): [i][k][j][b]; weights (p): [i];
    val_grad (p, q): [i in p][j in q][b] = int phi_i d psi_j / d lambda_b;  tri (p): [i][a][b] = int phi_i lambda_a lambda_b."""
    extended = EXTENDED if extended is None else extended
    key = (kind, d, degs, extended)
    if key not in _REF:
        nv = d + 1
        if kind == "mass":
            t = _tensor(d, [(degs[0], None), (degs[0], None)])
        elif kind == "weights":
            t = _tensor(d, [(degs[0], None)])
        elif kind == "stiff":
            t = np.stack([np.stack([_tensor(d, [(degs[0], a), (degs[0], b)]) for b in range(nv)], axis=-1)
                          for a in range(nv)], axis=1)  # [i][a][j][b]
        elif kind == "conv":
            t = np.stack([_tensor(d, [(degs[0], None), (degs[0], None), (degs[0], b)]) for b in range(nv)], axis=-1)
        elif kind == "val_grad":
            t = np.stack([_tensor(d, [(degs[0], None), (degs[1], b)]) for b in range(nv)], axis=-1)
        elif kind == "tri":
            t = _tensor(d, [(degs[0], None), (1, None), (1, None)])
        else:
            raise ValueError(kind)
        _REF[key] = ext(t, extended)
    return _REF[key]


# ---- geometry --------------------------------------------------------------------------------------------------------
class Geometry:
    """G (nc, d + 1, d) = grad lambda_a and adet (nc,) = |det J| in the extended type; aG / aadet: float64 absolute
    values for the bounds, with |G_0| := sum_a |G_a|."""

    def __init__(self, G1, adet, extended=None):
        self.extended = EXTENDED if extended is None else extended
        self.G = np.concatenate([-G1.sum(axis=1, keepdims=True), G1], axis=1)
        self.adet = adet
        a1 = np.abs(to_f64(G1))
        self.aG = np.concatenate([a1.sum(axis=1, keepdims=True), a1], axis=1)
        self.aadet = np.abs(to_f64(adet))
        self.nc, self.d = G1.shape[0], G1.shape[2]


def geometry_from_records(geom, extended=None) -> Geometry:
    """The device's records ``[grad lambda_1..d (row-major), |det J|, ...]`` promoted exactly."""
    geom = np.asarray(geom, dtype=np.float64)
    d = 2 if geom.shape[1] == 6 else 3
    return Geometry(ext(geom[:, : d * d].reshape(-1, d, d), extended), ext(geom[:, d * d], extended), extended)


def geometry_from_coords(points, cells, extended=None):
    """The closed forms of k_geometry (ox_setup.hip) / fem.cell_geometry in extended precision.

    Returns (records (nc, d d + 1) extended: grad lambda_1..d row-major, then |det J|;  tol (nc, d d + 1) float64: the
    running bound of those float64 expressions, 2^-53 included;  cancel (nc,): sum |products| / |det|).
    Chains (float64 evaluation, coordinates exact): an edge component is one rounded difference; a 2 x 2 determinant or
    a cross-product component is two products of two edge components and a difference: 4 roundings against
    sum |products|; the 3 x 3 determinant adds one edge component, one product and two sums: 8; a quotient adds the
    numerator's chain, the determinant's (weighted by the cancellation sum |products| / |det|) and the division."""
    x = ext(np.asarray(points, dtype=np.float64), extended)[np.asarray(cells)]
    d = x.shape[2]
    e = x[:, 1:, :] - x[:, :1, :]  # rows = edge vectors
    ae = absx(e)
    if d == 2:
        a, b, c, dd = e[:, 0, 0], e[:, 1, 0], e[:, 0, 1], e[:, 1, 1]
        det = a * dd - b * c
        Bdet = ae[:, 0, 0] * ae[:, 1, 1] + ae[:, 1, 0] * ae[:, 0, 1]
        num = np.stack([dd, -b, -c, a], axis=1)
        Bnum, n_num, n_det = absx(num), 1, 4
    else:
        def cross(p, q):
            return np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2],
                             p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], axis=1)

        def across(p, q):
            return np.stack([p[:, 1] * q[:, 2] + p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] + p[:, 0] * q[:, 2],
                             p[:, 0] * q[:, 1] + p[:, 1] * q[:, 0]], axis=1)
        e1, e2, e3 = e[:, 0], e[:, 1], e[:, 2]
        c23 = cross(e2, e3)
        det = (e1 * c23).sum(axis=1)
        Bdet = (ae[:, 0] * across(ae[:, 1], ae[:, 2])).sum(axis=1)
        num = np.concatenate([c23, cross(e3, e1), cross(e1, e2)], axis=1)
        Bnum = np.concatenate([across(ae[:, 1], ae[:, 2]), across(ae[:, 2], ae[:, 0]), across(ae[:, 0], ae[:, 1])], axis=1)
        n_num, n_det = 4, 8
    rec = np.concatenate([num / det[:, None], absx(det)[:, None]], axis=1)
    adet, Bdet, Bnum, anum = np.abs(to_f64(det)), to_f64(Bdet), to_f64(Bnum), np.abs(to_f64(num))
    cancel = Bdet / adet
    assert (n_det + 2) * U * cancel.max() < 1e-3, "a determinant with no correct digit: the first-order bound does not hold"
    tol_g = U * 1.01 * ((n_num + 2) * Bnum / adet[:, None] + anum / adet[:, None] * ((n_det + 2) * cancel[:, None] + 1))
    tol = np.concatenate([tol_g, ((n_det + 2) * U * Bdet)[:, None]], axis=1)
    return rec, tol, cancel


# ---- per-cell chains of the kernels (oasisx_amd/csrc/ox_assemble.hip) ----------------------------------------------
def kernel_nq(d, *degs):
    """Points of the rule the kernels tabulate on (OX_RULE_OF: the degree-9 rule next to a P3 space)."""
    return ((25 if d == 2 else 70) if 3 in degs else (7 if d == 2 else 14))


def chain(form, d, deg, deg2=None, nut=False, n_table=0):
    """Rounded operations one (row, cell) pair adds to an entry, tabulated constants included (one each)."""
    nq = kernel_nq(d, deg, deg2 or deg)
    nd = O.num_cell_dofs(d, deg)
    g0 = d  # load_geom :255-262: G_0 = -sum_a G_a, d subtractions
    last = 2  # :531 adet * c[j] and the accumulation (every form ends like this)
    if form == "mass":  # :405-411: wphi = w * phi (:79: 2 constants, 1 product), NQ fma with the constant phi
        return 3 + 1 + nq + last
    if form == "stiff":  # :412-436: gi (d + 1 fma, constant dphi), h (d fma, * w), c (NQ (d + 1) fma, constant dphi)
        return g0 + (d + 1) + 1 + d + 2 + nq * (d + 1) + 1 + last
    if form == "conv" and d == 3 and deg == 3:
        # :437-484 by quadrature: uq (ND fma, constant phi), G.uq (d fma), * wq (:79: 3), [nut: gi d fma + constant,
        # wn = w * nut (2), h d fma, fma], c (NQ d fma, constant dphi)
        return nd + 1 + d + 4 + ((d + 1 + 2 + d + 1) if nut else 0) + nq * d + 1 + last
    if form == "conv":
        # :485-527 tensor form: T (:150-162: NQ sums of w phi phi dphi: NQ + 2 + 4), gam (d fma), cm (ND fma), c += cm
        # (d + 1); [nut :506-524: S (:190-203: NQ + 2 + 3), G_a.G_b (d fma, * nut; G_0 in both), d + 1 fma]
        n = g0 + (nq + 6) + d + nd + (d + 1)
        if nut:
            n += (nq + 5) + g0 + d + 1 + (d + 1)
        return n + last
    if form == "weights":  # :76-84 iphi = sum_q w phi (NQ + 3); :850 one fma per cell
        return nq + 3 + 1
    if form == "load":  # :888-891: n_q fma over the given table, one fma per cell
        return n_table + 1
    # -- the per-cell chains of scalar_cellvisc_slice (ox_scalar_rows_cellvisc, ox_scalar_rows_supg) -----------------------
    quad = d == 3 and deg == 3  # the P3 tetrahedron: the quadrature branches
    tab = nq + 5  # an entry of StiffTab / SupgTab (:191-204, :228-240): NQ sums of w f g: NQ + 2 products + 3 constants
    if form == "kt":  # K_t alone (SUPG = false)
        if quad:  # :986-1011: gi (d fma, constant dphi), wn = w nut (2), h (d fma), sb = wn h, c (NQ d fma, constant dphi)
            return (d + 1) + 2 + d + 1 + nq * d + 1 + last
        # :1013-1035: gg = nut (G_a . G_b) (d fma, 1 product; G_0 in both factors: 2 g0), cm (d + 1 fma over the table),
        # c[j] += cm (the (j, b) pairs of one j: d + 1)
        return 2 * g0 + d + 1 + tab + (d + 1) + (d + 1) + last
    if form == "kt_s":  # K_t + S/(2t) through the ONE contraction, and the fma of the time term that lands on the same c[j] (:1054)
        # th = (tau / 2) (1 / t): the quotient (formed by the entry) and the product: 2
        if quad:
            # :954-985: wa (d fma), wg (d fma, constant dphi), ws = w th wg (constant, 2 products, th: 2), sb = fma(ws, wa_b,
            # wn h): the longer branch is ws wa_b = (d + d + 1) + 5 + d against (d + 1) + 2 + d + 1 of (w nut) h; + the fma
            return (3 * d + 6) + 1 + nq * d + 1 + 1 + last
        # :945-950 wa (d fma; G_0: g0), :1024 gg = fma(th wa_a, wa_b, nut v): the longer branch th wa_a wa_b carries
        # 2 (g0 + d) + 3 against 2 g0 + d + 1; + the fma; then the contraction as for "kt"
        return 2 * (g0 + d) + 4 + tab + (d + 1) + (d + 1) + 1 + last
    nr = (2 * d + 1 + 2 + nq + 1) if quad else (g0 + d + tab + (d + 1))
    # nr[j] = int (w . grad phi_i) phi_j / |J|: :968-983 wt = w wg (wa, wg: 2 d + 1; constant, product), NQ fma, constant phi;
    # :1037-1041: wa (g0 + d), d + 1 fma over the table
    if form == "n_time":  # :1046 tdt = tau (0.5 two_idt) (1 / t) (2 / dt, 1 / t, two products), :1054 c[j] = fma(tdt, nr[j], c[j])
        return nr + 4 + 1 + last
    if form == "supg":  # the accumulator entry K_t + (N/dt + S/2) / t of one (row, cell): its longest chain
        return max(chain("kt_s", d, deg), chain("n_time", d, deg))
    if form == "supg_rhs":
        # :1053-1063: fma(two_idt, c1, fh) (two_idt: 1), ND fma with nr[j], adet tau, rs = fma(adet tau, r, rs)
        return nr + 2 + nd + 1 + 1
    ndp = O.num_cell_dofs(d, deg2)
    if form == "grad0":  # :1049-1056: pq (ND_p fma, constant phi, * w), S (NQ fma, constant dphi); :1069-1075 (d + 1 fma, fma)
        return g0 + ndp + 3 + nq + 1 + (d + 1) + 1
    if form == "grad1":  # :1058-1066: wp (3), gp (ND_p fma, constant dphi), S (NQ fma)
        return g0 + 3 + ndp + 1 + nq + (d + 1) + 1
    if form == "div":  # :1219-1246: gu (d fma), dv (ND_u (d + 1) fma, constant dphi), s (NQ fma, wphi: 3), fma per cell
        return g0 + d + ndp * (d + 1) + 1 + nq + 3 + 1
    if form == "rect0" and d == 3 and deg == 3:  # :1326-1335, the Rect0Tab33 branch: tabulated tensor (1), d fma; :1373
        return 1 + d + last
    if form == "rect0":  # :1338-1353: gi (d + 1 fma, constant, * w: 2), c (NQ fma, constant phi), :1373 adet * c, +=
        return g0 + (d + 1) + 3 + nq + 1 + last
    if form in ("rect1", "rect2"):  # :1354-1365: f = wp * dphi (3 + 1 + 1), c (NQ (d + 1) fma); :1373
        return g0 + 5 + nq * (d + 1) + last
    raise ValueError(form)


# ---- entries ---------------------------------------------------------------------------------------------------------
class Entries:
    """Sparse result of a matrix form: ``rows``, ``cols`` (sorted by row, then column), ``val`` (extended; (nnz,) or
    (nnz, k)), ``B`` (float64, same shape) and ``n`` (int (nnz,))."""

    def __init__(self, rows, cols, val, B, n, shape):
        self.rows, self.cols, self.val, self.B, self.n, self.shape = rows, cols, val, B, n, shape
        assert int(np.max(n)) <= N_MAX, int(np.max(n))

    def lookup(self, A):
        """Values of a scipy sparse matrix at this pattern (float64)."""
        return np.asarray(A.tocsr()[self.rows, self.cols]).ravel()

    def matvec(self, x, val=None):
        """(value) @ x in the extended type; x (ncols,) or (ncols, k) extended."""
        v = self.val if val is None else val
        xv = x[self.cols]
        prod = v * xv if xv.ndim == v.ndim else (v[:, None] * xv if v.ndim == 1 else v * xv[:, None])
        out = np.zeros((self.shape[0],) + prod.shape[1:], dtype=prod.dtype) + prod.ravel()[0] * 0
        np.add.at(out, self.rows, prod)
        return out


def _scatter(Ae, rd, cd, shape, extra=()):
    """Sum element tensors Ae (nc, nr, ncol[, k]) into sorted unique (row, col) entries; ``extra``: float64 tensors of the
    same leading shape summed the same way.  Returns (rows, cols, values, [extras], cells per entry)."""
    nr, ncol = rd.shape[1], cd.shape[1]
    rows = np.repeat(rd, ncol, axis=1).ravel().astype(np.int64)
    cols = np.tile(cd, (1, nr)).ravel().astype(np.int64)
    keys, inv = np.unique(rows * shape[1] + cols, return_inverse=True)
    inv = inv.ravel()
    tail = Ae.shape[3:]

    def summed(T):
        flat = T.reshape((-1,) + tail)
        out = np.zeros((keys.shape[0],) + tail, dtype=flat.dtype) + flat.ravel()[0] * 0
        np.add.at(out, inv, flat)
        return out
    return keys // shape[1], keys % shape[1], summed(Ae), [summed(np.asarray(E, dtype=np.float64)) for E in extra], \
        np.bincount(inv, minlength=keys.shape[0])


def _scatter_vec(be, rd, n, extra=()):
    def summed(T):
        flat = T.reshape((-1,) + T.shape[2:])
        out = np.zeros((n,) + T.shape[2:], dtype=flat.dtype) + flat.ravel()[0] * 0
        np.add.at(out, rd.ravel(), flat)
        return out
    return summed(be), [summed(np.asarray(E, dtype=np.float64)) for E in extra], np.bincount(rd.ravel(), minlength=n)


def _einsum(spec, *ops):
    return np.einsum(spec, *ops, optimize=False) if any(o.dtype == object for o in ops) else np.einsum(spec, *ops, optimize=True)


class Model:
    """The forms over one mesh in kernel cell order: ``geo`` (Geometry), the cell -> dof tables ``vd`` (velocity
    component space, degree ``u_deg``, ``nv`` dofs) and ``qd`` (pressure space, ``p_deg``, ``nq`` dofs): any numbering."""

    def __init__(self, geo: Geometry, vd, nv, u_deg, qd=None, nq=0, p_deg=None, tab_err=None):
        """``tab_err`` {degree: (dphi_err (nd,), dgrad_err (nd, d + 1))}: absolute errors of SOMEONE ELSE's tabulation, added
        to the absolute tables of the bounds -- B(with) - B(without) then bounds what those errors do to an entry."""
        self.geo, self.d = geo, geo.d
        self.tab_err = tab_err or {}
        self.vd, self.nv, self.u_deg = np.asarray(vd, dtype=np.int64), int(nv), u_deg
        self.qd, self.nq, self.p_deg = (None if qd is None else np.asarray(qd, dtype=np.int64)), int(nq), p_deg
        self.x = geo.extended
        # a positive-weight rule of the oracle and its tabulation, for the bounds only
        self.bary, self.w = O.simplex_quadrature(self.d, 5 if 3 in (u_deg, p_deg) else 4)
        assert (self.w > 0).all()
        self._tab = {}

    def _abs_tab(self, deg):
        if deg not in self._tab:
            phi, dphi = O.tabulate(self.d, deg, self.bary)
            aphi, adphi = np.abs(phi), np.abs(dphi)
            if deg in self.tab_err:
                aphi, adphi = aphi + self.tab_err[deg][0][None], adphi + self.tab_err[deg][1][None]
            agrad = np.einsum("qib,cbk->cqik", adphi, self.geo.aG, optimize=True)  # sum_b |dphi_b| |G_b|: (nc, Q, nd, d)
            self._tab[deg] = (aphi, agrad)
        return self._tab[deg]

    def _space(self, which):
        return (self.vd, self.nv, self.u_deg) if which == "v" else (self.qd, self.nq, self.p_deg)

    def _ref(self, kind, *degs):
        return ref(kind, self.d, *degs, extended=self.x)

    def _e(self, a):
        return ext(a, self.x)

    # -- element tensors -------------------------------------------------------------------------------------------------
    def _mass_e(self, deg):
        g = self.geo
        aphi, _ = self._abs_tab(deg)
        Ae = g.adet[:, None, None] * self._ref("mass", deg)[None]
        Be = g.aadet[:, None, None] * np.einsum("q,qi,qj->ij", self.w, aphi, aphi)[None]
        return Ae, Be

    def _stiff_e(self, deg):
        g = self.geo
        _, agrad = self._abs_tab(deg)
        GG = _einsum("cad,cbd->cab", g.G, g.G)
        Ae = g.adet[:, None, None] * _einsum("cab,iajb->cij", GG, self._ref("stiff", deg))
        Be = g.aadet[:, None, None] * np.einsum("q,cqik,cqjk->cij", self.w, agrad, agrad, optimize=True)
        return Ae, Be

    def _conv_e(self, uab):
        g, deg = self.geo, self.u_deg
        aphi, agrad = self._abs_tab(deg)
        gam = _einsum("cbd,ckd->ckb", g.G, self._e(uab)[self.vd])
        Ae = g.adet[:, None, None] * _einsum("ikjb,ckb->cij", self._ref("conv", deg), gam)
        auq = np.einsum("qk,ckd->cqd", aphi, np.abs(np.asarray(uab, dtype=np.float64))[self.vd], optimize=True)
        t = np.einsum("cqd,cqjd->cqj", auq, agrad, optimize=True)
        Be = g.aadet[:, None, None] * np.einsum("q,qi,cqj->cij", self.w, aphi, t, optimize=True)
        return Ae, Be

    # -- matrices ----------------------------------------------------------------------------------------------------------
    def _matrix(self, Ae, Be, which, form):
        dofs, n, deg = self._space(which)
        rows, cols, val, (B,), cnt = _scatter(Ae, dofs, dofs, (n, n), extra=(Be,))
        return Entries(rows, cols, val, B, cnt + chain(form, self.d, deg), (n, n))

    def mass(self, which="v"):
        """u v dx (fracstep.py:292,373)."""
        return self._matrix(*self._mass_e(self._space(which)[2]), which, "mass")

    def stiffness(self, which="v"):
        """inner(grad u, grad v) dx (fracstep.py:297-299,321-324,375,379)."""
        return self._matrix(*self._stiff_e(self._space(which)[2]), which, "stiff")

    def convection(self, uab, nut=None):
        """inner(dot(uab, nabla_grad(u)), v) dx (fracstep.py:355-358) [+ sum_e nut_e K_e]."""
        Ae, Be = self._conv_e(uab)
        if nut is not None:
            Ke, BKe = self._stiff_e(self.u_deg)
            Ae = Ae + self._e(nut)[:, None, None] * Ke
            Be = Be + np.abs(np.asarray(nut, dtype=np.float64))[:, None, None] * BKe
        rows, cols, val, (B,), cnt = _scatter(Ae, self.vd, self.vd, (self.nv, self.nv), extra=(Be,))
        return Entries(rows, cols, val, B, cnt + chain("conv", self.d, self.u_deg, nut=nut is not None), (self.nv, self.nv))

    def rect(self, family):
        """0: p v.dx(i) dx (rows V, cols Q; :311-315); 1: p.dx(i) v dx (rows V, cols Q; :348-352); 2: u.dx(i) q dx (rows Q,
        cols V; :332-336): values (nnz, d)."""
        g = self.geo
        (rd, nr, rdeg), (cd, ncl, cdeg) = (self._space("v"), self._space("q")) if family < 2 else (self._space("q"), self._space("v"))
        aphi_r, agrad_r = self._abs_tab(rdeg)
        aphi_c, agrad_c = self._abs_tab(cdeg)
        if family == 0:
            T = self._ref("val_grad", cdeg, rdeg)  # [c][r][b] = int psi_c d phi_r / d lambda_b
            Ae = g.adet[:, None, None, None] * _einsum("srb,cbd->crsd", T, g.G)
            Be = np.einsum("q,cqrd,qs->crsd", self.w, agrad_r, aphi_c, optimize=True)
        else:
            T = self._ref("val_grad", rdeg, cdeg)  # [r][c][b] = int phi_r d psi_c / d lambda_b
            Ae = g.adet[:, None, None, None] * _einsum("rsb,cbd->crsd", T, g.G)
            Be = np.einsum("q,qr,cqsd->crsd", self.w, aphi_r, agrad_c, optimize=True)
        Be = g.aadet[:, None, None, None] * Be
        rows, cols, val, (B,), cnt = _scatter(Ae, rd, cd, (nr, ncl), extra=(Be,))
        return Entries(rows, cols, val, B, cnt + chain("rect%d" % family, self.d, rdeg, cdeg), (nr, ncl))

    # -- vectors -----------------------------------------------------------------------------------------------------------
    def weights(self, which="v"):
        """int phi_i dx."""
        g = self.geo
        dofs, n, deg = self._space(which)
        aphi, _ = self._abs_tab(deg)
        be = g.adet[:, None] * self._ref("weights", deg)[None]
        Be = g.aadet[:, None] * np.einsum("q,qi->i", self.w, aphi)[None]
        val, (B,), cnt = _scatter_vec(be, dofs, n, extra=(Be,))
        return val, B, cnt + chain("weights", self.d, deg)

    def grad_vector(self, kind, p, base=None, scale=1.0):
        """kind 0: base + scale int p d_d(phi_r) (:487-497); kind 1: base + scale int d_d(p) phi_r (:618): (nv, d)."""
        g = self.geo
        aphi_v, agrad_v = self._abs_tab(self.u_deg)
        aphi_q, agrad_q = self._abs_tab(self.p_deg)
        pc, apc = self._e(p)[self.qd], np.abs(np.asarray(p, dtype=np.float64))[self.qd]
        if kind == 0:
            T = self._ref("val_grad", self.p_deg, self.u_deg)  # [s][r][b]
            be = _einsum("cs,srb,cbd->crd", pc, T, g.G)
            Be = np.einsum("q,cq,cqrd->crd", self.w, np.einsum("qs,cs->cq", aphi_q, apc), agrad_v, optimize=True)
        else:
            T = self._ref("val_grad", self.u_deg, self.p_deg)  # [r][s][b]
            be = _einsum("cs,rsb,cbd->crd", pc, T, g.G)
            Be = np.einsum("q,qr,cqd->crd", self.w, aphi_v, np.einsum("cqsd,cs->cqd", agrad_q, apc), optimize=True)
        be, Be = g.adet[:, None, None] * be, g.aadet[:, None, None] * Be
        val, (B,), cnt = _scatter_vec(be, self.vd, self.nv, extra=(Be,))
        sc = self._e(np.float64(scale))
        val, B = val * sc, B * abs(float(scale))
        if base is not None:
            val, B = val + self._e(base), B + np.abs(np.asarray(base, dtype=np.float64))
        return val, B, cnt[:, None] + chain("grad%d" % kind, self.d, self.u_deg, self.p_deg) + 0 * B.astype(np.int64)

    def div_vector(self, u, scale=1.0):
        """scale int div(u) psi_r (:328-330,538,546): (nq,)."""
        g = self.geo
        aphi_q, _ = self._abs_tab(self.p_deg)
        _, agrad_v = self._abs_tab(self.u_deg)
        T = self._ref("val_grad", self.p_deg, self.u_deg)  # [r][k][b]
        be = g.adet[:, None] * _einsum("rkb,cbd,ckd->cr", T, g.G, self._e(u)[self.vd])
        adiv = np.einsum("cqkd,ckd->cq", agrad_v, np.abs(np.asarray(u, dtype=np.float64))[self.vd], optimize=True)
        Be = g.aadet[:, None] * np.einsum("q,cq,qr->cr", self.w, adiv, aphi_q, optimize=True)
        val, (B,), cnt = _scatter_vec(be, self.qd, self.nq, extra=(Be,))
        return val * self._e(np.float64(scale)), B * abs(float(scale)), cnt + chain("div", self.d, self.p_deg, self.u_deg)

    def load_vector_table(self, wphi, fq, which="v"):
        """sum_e |det J_e| sum_q wphi[q][i] fq[e][q]: the kernel's sum over a given table, in the extended type."""
        g = self.geo
        dofs, n, _ = self._space(which)
        be = g.adet[:, None] * _einsum("qi,cq->ci", self._e(wphi), self._e(fq))
        Be = g.aadet[:, None] * np.einsum("qi,cq->ci", np.abs(wphi), np.abs(fq))
        val, (B,), cnt = _scatter_vec(be, dofs, n, extra=(Be,))
        return val, B, cnt + chain("load", self.d, 1, n_table=wphi.shape[0])

    def load_vector_poly(self, l1, l2, which="v"):
        """int (l1 . (1, x)) (l2 . (1, x)) phi_i dx, exact: the two affine factors by their vertex values ``l1``, ``l2``
        (nc, d + 1) (extended), the product integrated with int phi_i lambda_a lambda_b."""
        g = self.geo
        dofs, n, deg = self._space(which)
        be = g.adet[:, None] * _einsum("iab,ca,cb->ci", self._ref("tri", deg), l1, l2)
        val, _, _ = _scatter_vec(be, dofs, n)
        return val

    # -- the fused assemble_first (ox_assemble.hip:594-606) ------------------------------------------------------------
    def assemble_first(self, Mdev, Kdev, uab, u1, b0, dt, nu, nut=None, C=None):
        """From the device's own M and K (scipy, promoted exactly), with C = convection(uab[, nut]):
            A = M/dt + C/2 + nu K/2        (computed as 2 M/dt - ar,  ar = M/dt - C/2 - nu K/2: :594-603)
            b_first = ar u1 + b0           (:598,614)        a_u1 = A u1     (:606)
        Returns {"A": Entries, "b_first": (val, B, n), "a_u1": (val, B, n)}.  Epilogue operations: 1/dt (1), ar (2 fma),
        A (1 fma): + 4 on the convection chain; the row sums add the storage width of the row (<= 256) and the b0 add."""
        C = self.convection(uab, nut) if C is None else C  # (``C``: the same convection entries, computed before)
        x = self._e
        M, K = x(C.lookup(Mdev)), x(C.lookup(Kdev))
        aM, aK = np.abs(to_f64(M)), np.abs(to_f64(K))
        idt, hnu = 1 / x(np.float64(dt)), x(np.float64(nu)) / 2
        ar = idt * M - C.val / 2 - hnu * K
        Bar = aM / dt + C.B / 2 + nu / 2 * aK
        A = Entries(C.rows, C.cols, 2 * idt * M - ar, 2 * aM / dt + Bar, C.n + 4, C.shape)
        au1 = np.abs(np.asarray(u1, dtype=np.float64))
        width = np.bincount(C.rows, minlength=self.nv)
        width = (width + 1) // 2 * 2
        nrow = np.zeros(self.nv, dtype=np.int64)
        np.maximum.at(nrow, C.rows, C.n + 4)
        Bb = np.zeros((self.nv, self.d))
        np.add.at(Bb, C.rows, Bar[:, None] * au1[C.cols])
        Ba = np.zeros((self.nv, self.d))
        np.add.at(Ba, C.rows, A.B[:, None] * au1[C.cols])
        one = np.ones((1, self.d), dtype=np.int64)
        n_b, n_a = (nrow + width + 1)[:, None] * one, (nrow + width)[:, None] * one
        assert n_b.max() <= N_MAX
        return {"A": A, "b_first": (C.matvec(x(u1), ar) + x(b0), Bb + np.abs(np.asarray(b0, dtype=np.float64)), n_b),
                "a_u1": (A.matvec(x(u1)), Ba, n_a)}


    # -- the scalar row kernels (DESIGN.md sections 13, 25, 32) -----------------------------------------------------------
    def _pattern(self):
        """(rows, cols, cells per entry) of the velocity component space: every pair of dofs that share a cell."""
        if not hasattr(self, "_pat"):
            nd = self.vd.shape[1]
            rows, cols, _, _, cnt = _scatter(np.zeros((self.vd.shape[0], nd, nd)), self.vd, self.vd, (self.nv, self.nv))
            self._pat = (rows, cols, cnt)
        return self._pat

    def _supg_e(self, w, tau):
        """N_e[i][j] = |J| tau sum_a (w . G_a) int phi_j d(phi_i)/d(lambda_a),
        S_e[i][j] = |J| tau sum_ab (w . G_a)(w . G_b) int d(phi_i)/d(lambda_a) d(phi_j)/d(lambda_b), and their bounds."""
        g, deg = self.geo, self.u_deg
        aphi, agrad = self._abs_tab(deg)
        wa = _einsum("cd,cad->ca", self._e(w), g.G)
        s = (g.adet * self._e(tau))[:, None, None]
        T = self._ref("val_grad", deg, deg)  # [j][i][a] = int phi_j d(phi_i) / d(lambda_a)
        Ne = s * _einsum("ca,jia->cij", wa, T)
        Se = s * _einsum("ca,cjia->cij", wa, _einsum("cb,iajb->cjia", wa, self._ref("stiff", deg)))
        awg = np.einsum("cd,cqid->cqi", np.abs(np.asarray(w, dtype=np.float64)), agrad, optimize=True)
        sa = (g.aadet * np.abs(np.asarray(tau, dtype=np.float64)))[:, None, None]
        BN = sa * np.einsum("q,cqi,qj->cij", self.w, awg, aphi, optimize=True)
        BS = sa * np.einsum("q,cqi,cqj->cij", self.w, awg, awg, optimize=True)
        return Ne, BN, Se, BS

    def _rows(self, Adev, Mdev, Kdev, s, dt, c1, b0, a_c1, acc=None, n_acc=0, rs=None):
        """The epilogue shared by the three row kernels (k_scalar_rows :97-119, scalar_cellvisc_slice :1116-1142):
        A_c = A + s K [+ acc],  sa = A_c c_1,  sm = M c_1,  b_c = fma(2/dt, sm, -sa) + b0 [+ rs].
        ``acc`` (value, B) per entry of the pattern: what the LDS accumulator holds, scaled; ``n_acc`` (nnz,): its chain,
        the epilogue's operations on it included; ``rs`` (value, B, n) (n_dofs, NC): the register-summed right-hand side."""
        rows, cols, cnt = self._pattern()
        x = self._e
        look = lambda Mat: np.asarray(Mat.tocsr()[rows, cols]).ravel()  # noqa: E731
        A, M, K = x(look(Adev)), x(look(Mdev)), x(look(Kdev))
        aA, aM, aK = (np.abs(to_f64(v)) for v in (A, M, K))
        val, B = A + x(np.float64(s)) * K, aA + abs(float(s)) * aK
        n = np.ones_like(cnt)  # v = fma(s, k, a)
        if acc is not None:
            val, B, n = val + acc[0], B + acc[1], n + n_acc
        Ac = Entries(rows, cols, val, B, n, (self.nv, self.nv))
        c1 = np.asarray(c1, dtype=np.float64).reshape(self.nv, -1)
        b0 = np.asarray(b0, dtype=np.float64).reshape(self.nv, -1)
        ac1 = np.abs(c1)
        width = np.bincount(rows, minlength=self.nv)
        width = (width + 1) // 2 * 2  # the storage width of the row (OX_KV = 2)
        nrow = np.zeros(self.nv, dtype=np.int64)
        np.maximum.at(nrow, rows, n)
        Ba = np.zeros_like(ac1)
        np.add.at(Ba, rows, B[:, None] * ac1[cols])
        Bm = np.zeros_like(ac1)
        np.add.at(Bm, rows, aM[:, None] * ac1[cols])
        sa, sm = Ac.matvec(x(c1)), Ac.matvec(x(c1), M)
        two_idt = 2 / x(np.float64(dt))
        bval, bB = two_idt * sm - sa + x(b0), 2.0 / dt * Bm + Ba + np.abs(b0)
        # sa: the entry's chain + one fma per stored entry; sm: 2 / dt and one fma per stored entry; the fma, the b0 add
        n_b = nrow + width + 2
        if rs is not None:
            bval, bB, n_b = bval + rs[0], bB + rs[1], np.maximum(n_b, rs[2]) + 1
        one = np.ones((1, c1.shape[1]), dtype=np.int64)
        n_b, n_a = n_b[:, None] * one, (nrow + width)[:, None] * one
        assert n_b.max() <= N_MAX, int(n_b.max())
        out = {"A_c": Ac, "b_c": (bval, bB, n_b)}
        if a_c1:
            out["a_c1"] = (sa, Ba, n_a)
        return out

    def scalar_rows(self, Adev, Mdev, Kdev, s, dt, c1, b0, a_c1=True):
        """ox_scalar_rows from the device's own A, M, K (scipy, promoted exactly): A_c = A + s K,
        b_c = (2/dt) M c_1 - A_c c_1 + b0, a_c1 = A_c c_1; c_1, b0: (n_dofs, NC)."""
        return self._rows(Adev, Mdev, Kdev, s, dt, c1, b0, a_c1)

    def _acc_entries(self, Ae, Be):
        _, _, val, (B,), _ = _scatter(Ae, self.vd, self.vd, (self.nv, self.nv), extra=(Be,))
        return val, B

    def scalar_rows_cellvisc(self, Adev, Mdev, Kdev, s, dt, c1, b0, nut, t, a_c1=True):
        """ox_scalar_rows_cellvisc: A_c = A + s K + t K_t, K_t = sum_c nut_c K_c (v = fma(t, kt, fma(s, k, a)): + 1)."""
        Ke, BKe = self._stiff_e(self.u_deg)
        kt, Bkt = self._acc_entries(self._e(nut)[:, None, None] * Ke, np.abs(np.asarray(nut, dtype=np.float64))[:, None, None] * BKe)
        tx = self._e(np.float64(t))
        n_acc = self._pattern()[2] + chain("kt", self.d, self.u_deg) + 1
        return self._rows(Adev, Mdev, Kdev, s, dt, c1, b0, a_c1, acc=(tx * kt, abs(float(t)) * Bkt), n_acc=n_acc)

    def scalar_rows_supg(self, Adev, Mdev, Kdev, s, dt, c1, b0, nut, t, rec, fh, a_c1=True, mutate=None):
        """ox_scalar_rows_supg from the device's own records ``rec`` ((d + 1, n_cells): w_c, then tau_c; promoted exactly):
        A_c = A + s K + t K_t + N/dt + S/2 (the accumulator holds K_t + (N/dt + S/2)/t, v = fma(t, acc, fma(s, k, a)): + 1;
        without nut t = 1),  b_c += N ((2/dt) c_1 + f_h).  ``nut`` None: no K_t.
        ``mutate`` (host tests): called with the element tensors {"Kt", "N", "S"} before they are summed."""
        rec = np.asarray(rec, dtype=np.float64).reshape(self.d + 1, -1)
        w, tau = rec[: self.d].T, rec[self.d]
        x = self._e
        Ne, BN, Se, BS = self._supg_e(w, tau)
        idt = 1 / x(np.float64(dt))
        el = {"N": Ne, "S": Se, "Kt": None}
        Bacc = BN / dt + BS / 2
        if nut is not None:
            Ke, BKe = self._stiff_e(self.u_deg)
            el["Kt"] = x(np.float64(t)) * x(nut)[:, None, None] * Ke
            Bacc = Bacc + abs(float(t)) * np.abs(np.asarray(nut, dtype=np.float64))[:, None, None] * BKe
        if mutate is not None:
            mutate(el)
        acc_e = idt * el["N"] + el["S"] / 2
        if el["Kt"] is not None:
            acc_e = acc_e + el["Kt"]
        acc = self._acc_entries(acc_e, Bacc)
        n_acc = self._pattern()[2] + chain("supg", self.d, self.u_deg) + 1
        c1 = np.asarray(c1, dtype=np.float64).reshape(self.nv, -1)
        fh = np.asarray(fh, dtype=np.float64).reshape(self.nv, -1)
        rhs = 2 * idt * x(c1) + x(fh)
        arhs = 2.0 / dt * np.abs(c1) + np.abs(fh)
        re = _einsum("cij,cjk->cik", el["N"], rhs[self.vd])
        Bre = np.einsum("cij,cjk->cik", BN, arhs[self.vd], optimize=True)
        rval, (rB,), rcnt = _scatter_vec(re, self.vd, self.nv, extra=(Bre,))
        rs = (rval, rB, rcnt + chain("supg_rhs", self.d, self.u_deg))
        return self._rows(Adev, Mdev, Kdev, s, dt, c1, b0, a_c1, acc=acc, n_acc=n_acc, rs=rs)

    def supg_cells(self, uab, nut, kappa, inv_sct, dt, scale, time_term):
        """ox_supg_cells (k_supg_cells, csrc/ox_scalar.hip :572-612): {"w": (value (nc, d), B, n), "tau": (value (nc,), tol)}.
        w_c = sum_i phic_i u_i (phic: the basis at the centroid, exact): ND fma: n = ND, the criterion (n + 2) u B.
        tau_c = scale / sqrt(r), r = t2 + (k q)^2 + (2 k^2 kap g)^2: ``tol`` is the ABSOLUTE bound, propagated: q_c = sum_a
        |w . G_a| holds cancelling sums, so its error is bounded against sum_a sum_d |w_d| |G_ad| (and what the error of
        w itself does to it), not against q; g, kap, cq, cd, the two fma, the root and the division add one rounding each
        against their own (positive) terms; t2 = (2/dt)(2/dt) is formed on the host: 3."""
        d, deg, x = self.d, self.u_deg, self._e
        frac = Fraction(1, d + 1) if deg < 3 else mpmath.mpf(1) / (d + 1)
        phic = ext(np.array(basis_at(d, deg, [frac] * (d + 1)), dtype=object), self.x)
        nd = self.vd.shape[1]
        au = np.abs(np.asarray(uab, dtype=np.float64))
        w = _einsum("cid,i->cd", x(uab)[self.vd], phic)
        Bw = np.einsum("cid,i->cd", au[self.vd], np.abs(to_f64(phic)))
        # (``tab_err``: what someone else's tabulation of the centroid values adds to w, an absolute error)
        ew = np.einsum("cid,i->cd", au[self.vd], self.tab_err[deg][0]) if deg in self.tab_err else 0.0 * Bw
        G, aG = self.geo.G, self.geo.aG
        wa = _einsum("cd,cad->ca", w, G)
        q = absx(wa).sum(axis=1)
        g = (G * G).sum(axis=(1, 2))
        kap = x(np.float64(kappa)) + (x(np.float64(inv_sct)) * x(nut) if nut is not None else 0)
        k = deg
        t2 = (2 / x(np.float64(dt))) ** 2 if time_term else x(np.float64(0.0))
        cq, cd = k * q, 2 * k * k * kap * g
        r = t2 + cq * cq + cd * cd
        rf = to_f64(r)
        pos = rf > 0
        root = np.array([mpmath.sqrt(v) for v in r], dtype=object) if r.dtype == object else np.sqrt(r)
        tau = np.where(pos, x(np.float64(scale)) / np.where(pos, root, 1), 0 * r)
        # -- the bound, first order with the second-order terms kept on the safe side (float64) --
        dw = (nd + 2) * U * (Bw + ew) + ew
        Bwa = np.einsum("cd,cad->ca", np.abs(to_f64(w)) + dw, aG)  # sum_d |w_d| |G_ad|
        g0 = np.array([d] + [0] * d)  # G_0 = -sum_a G_a: d roundings against |G_0| := sum_a |G_a|
        dwa = np.einsum("cd,cad->ca", dw, aG) + (d + 1 + g0)[None] * U * Bwa
        dq = dwa.sum(axis=1) + (d + 1) * U * Bwa.sum(axis=1)
        Bg = (aG ** 2).sum(axis=(1, 2))
        dg = ((d + 1) * d + 2 * d + 1) * U * Bg
        kf, gf, qf = to_f64(kap) * np.ones(self.geo.nc), to_f64(g), to_f64(q)
        dk = U * kf if nut is not None else 0.0 * kf  # kap = fma(inv_sct, nut, kappa)
        cqf, dcq = k * qf, k * dq + U * k * (qf + dq)
        cdf = 2 * k * k * kf * gf
        dcd = 2 * k * k * ((kf + dk) * dg + dk * gf) + 2 * U * 2 * k * k * (kf + dk) * (gf + dg)
        dt2 = 3 * U * float(to_f64(t2))
        dr = (2 * cdf + dcd) * dcd + (2 * cqf + dcq) * dcq + dt2
        dr = dr + 2 * U * (rf + dr)  # the two fma
        assert (dr[pos] < 0.5 * rf[pos]).all(), "r has no correct digit: the first-order bound does not hold"
        tf = to_f64(tau)
        with np.errstate(divide="ignore", invalid="ignore"):
            grow = np.where(pos, np.expm1(-0.5 * np.log1p(-np.where(pos, dr / np.where(pos, rf, 1), 0.0))), 0.0)
        tol = tf * grow + 3 * U * tf * (1 + grow)  # the root, the division, and their second order
        return {"w": (w, Bw + ew, np.full(Bw.shape, nd, dtype=np.int64)), "tau": (tau, tol), "q": (q, Bwa.sum(axis=1)), "g": g}


def spmv_bound(A_csr, x):
    """(A x in the extended type, (row_len + 1) 2^-53 (|A| |x|)_i): the mat-vec criterion."""
    A = A_csr.tocsr()
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    xv = np.asarray(x, dtype=np.float64).reshape(A.shape[1], -1)
    prod = ext(A.data)[:, None] * ext(xv)[A.indices]
    val = np.zeros((A.shape[0], xv.shape[1]), dtype=prod.dtype) + prod.ravel()[0] * 0
    np.add.at(val, rows, prod)
    B = np.zeros((A.shape[0], xv.shape[1]))
    np.add.at(B, rows, np.abs(A.data)[:, None] * np.abs(xv)[A.indices])
    return val, (np.diff(A.indptr) + 1)[:, None] * U * B


# ---- the criterion -----------------------------------------------------------------------------------------------------
def ratio(dev, val, B):
    """max over the entries of |dev - val| / (2^-53 B) (entries with B == 0 must be exactly zero: they give inf if not)."""
    dev = np.asarray(dev, dtype=np.float64)
    err = to_f64(absx(ext(dev, val.dtype != object) - val))
    B = np.asarray(B, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(B > 0, err / (U * B), np.where((err == 0) & (dev == 0), 0.0, np.inf))
    return r


def check(dev, val, B, n, extra=None):
    """(ok, |dev - val| / (u B) of the entry that uses most of its allowance, that allowance n + 2): the criterion
    |dev - val| <= (n + 2) 2^-53 B per entry.
    ``extra`` (host comparisons with a reference that has errors of its own): an absolute allowance on top."""
    n = np.asarray(n)
    assert int(n.max()) <= N_MAX, int(n.max())
    r = ratio(dev, val, B)
    n = np.broadcast_to(n if n.ndim == r.ndim else n.reshape(n.shape + (1,) * (r.ndim - n.ndim)), r.shape)
    if extra is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            n = n + np.where(B > 0, np.asarray(extra) / (U * B), 0.0)
    bad = ~(r <= n + 2)  # (not ``r > n + 2``: a NaN entry -- a slot never written, a kernel that produced NaN -- is a violation)
    if not r.size:
        return True, 0.0, 0
    use = np.where(np.isnan(r), np.inf, r / (n + 2))
    k = int(np.argmax(use))  # the entry that uses most of ITS allowance (a NaN first): ratio and allowance of the same entry
    return (not bool(bad.any())), float(r.ravel()[k]), float(np.asarray(n, dtype=np.float64).ravel()[k]) + 2
