"""Extended-precision model of the cell locator and of point evaluation (csrc/ox_probe.hip), with counted bounds
(plain numpy: importable without a GPU).  The float64 model of tests/probe_model.py compares at a flat 1e-12; this one
states what the kernels may be off by on the meshes of tests/hard_meshes.py, and which points have an answer at all.

Barycentric coordinates.  ``lambda*`` of a point in a cell is computed in the extended type of tests/assembly_model.py
from the float64 coordinates taken as exact.  The device's chain (k_loc_geom, loc_bary), per lambda_a, a = 1..D:

* ``g_ak`` = grad lambda_a: the cofactor / determinant quotients of k_geometry -- the running bound ``tol_g[a][k]`` of
  ``assembly_model.geometry_from_coords`` applies entry by entry (2^-53 and the cancellation of the determinant included);
* ``r_k = x_k - x0_k``: one rounding, ``|dr_k| <= u |r_k|``;
* ``s = fma(g_a0, r_0, fma(...))``: D fmas, ``|ds| <= D u sum_k |g_ak| |r_k|`` (the standard forward bound, any order);

so ``|dlambda_a| <= sum_k tol_g[a][k] |r_k| + (D + 1) u sum_k |g_ak| |r_k|``.  ``lambda_0 = 1 - s_1 - ... - s_D`` adds the
errors of the s_a and D rounded subtractions of partial results no larger than ``1 + sum_a |lambda_a|``:
``|dlambda_0| <= sum_a |dlambda_a| + D u (1 + sum_a |lambda_a|)``.  ``fmin`` is exact, so the minimum is off by at most
the largest of these.  Every bound carries the factor 1.01 for the second-order terms and for the reference's own
rounding (2^-64 against 2^-53).  Nothing here is tuned.

Decisions.  The reference answer is the lowest cell with ``lambda*_min >= -tol``.  A point is DECIDED when
``|lambda*_min + tol|`` exceeds the bound on the minimum in EVERY cell of the tree (a superset of the cells whose padded
box holds the point -- the only ones the device can test): then no rounding of the device can change any of its
comparisons, and its answer must be the reference's.  The GPU tests feed decided points only.

Evaluation.  ``sum_a phi_a(bary) u_a`` in the extended type with ``bary`` the device's own float64 array promoted exactly
(as the assembly tests use the device's own geometry records).  The bound is ``(n + 2) 2^-53 B`` with ``B`` the same sum
over absolute values and ``n`` the longest rounded chain (probe_basis / probe_mono3 / probe_phi3, then the fma
accumulation over the nd dofs of k_eval_points):

* P1: phi_a = lambda_a, no rounding; B_a = |lambda_a|; n = nd;
* P2: vertices ``lambda (2 lambda - 1)``: the doubling is exact, one subtraction and one product: 2 roundings,
  B_a = |lambda| (2 |lambda| + 1); edges ``4 lambda_a lambda_b``: the product by 4 is exact, one rounding; n = 2 + nd;
* P3: powers ``l^2 = l l`` (1), ``l^3 = l^2 l`` (2); a monomial of total degree <= 3 is a product with factors 1.0 for
  the absent powers (exact): at most 2 roundings; phi_a = sum_q m_q C_qa: ND fmas over the coefficient table
  fe_tables_eval.h (read here from the same header, the literals converted as the compiler converts them: no rounding of
  the table enters); B_a = sum_q |m_q| |C_qa|; n = 2 + ND + nd.

The float64 transcriptions (``transcribe_*``) restate the kernels' arithmetic in numpy, operation by operation without
fma; the host tests hold them to the bounds and show that one product made wrong by 1e-9 breaks them.

Grid sizing.  ``grid_sizing`` emulates loc_create / k_loc_geom / k_loc_bins in float64 for both rules: ``isotropic``
(one length h = (vol / n)^(1/d), the rule before) and ``axis`` (bins proportional to extent / mean padded cell extent).
"""
from __future__ import annotations

import itertools
import os
import re

import numpy as np

from oracle import ipcs_oracle as O
from tests import assembly_model as AM
from tests.assembly_model import U, absx, ext, to_f64

TOL = 1e-10  # geometry.DEFAULT_TOL
SLACK = 1.01


# ---- barycentric coordinates -------------------------------------------------------------------------------------------
class CellGeometry:
    """grad lambda_1..d (m, d, d) in the extended type, its float64 bound, and x0 of the listed cells."""

    def __init__(self, points, cells, cell_ids=None):
        points, cells = np.asarray(points, dtype=np.float64), np.asarray(cells, dtype=np.int64)
        self.ids = np.arange(cells.shape[0]) if cell_ids is None else np.sort(np.asarray(cell_ids, dtype=np.int64))
        sel = cells[self.ids]
        self.d = d = points.shape[1]
        rec, tol, self.cancel = AM.geometry_from_coords(points, sel)
        self.G = rec[:, : d * d].reshape(-1, d, d)
        self.aG = np.abs(to_f64(self.G))
        self.tol_g = tol[:, : d * d].reshape(-1, d, d)
        self.x0 = ext(points[sel[:, 0]])


def barycentric(geo: CellGeometry, x, rows=None, shift=None):
    """(lam (m, n, d + 1) extended, bound (m, n, d + 1) float64) of every point in every cell of ``geo`` (``rows``: of
    point i in cell rows[i] only -- shapes (n, d + 1)).  ``shift`` (d,) or (n, d): the device's point may lie that far from
    ``x`` on every axis (a tracer's position against its closed form): sum_k |g_ak| shift_k is added to the bound."""
    d = geo.d
    X = ext(np.asarray(x, dtype=np.float64))
    if rows is None:
        G, aG, tg, r = geo.G[:, None], geo.aG[:, None], geo.tol_g[:, None], X[None, :, :] - geo.x0[:, None, :]
    else:
        G, aG, tg, r = geo.G[rows], geo.aG[rows], geo.tol_g[rows], X - geo.x0[rows]
    ar = np.abs(to_f64(r))
    if shift is not None:
        ar = ar + np.broadcast_to(np.asarray(shift, dtype=np.float64), ar.shape[-2:]) / ((d + 1) * U)
    lam, bnd = [], []
    for a in range(d):
        s = sum(G[..., a, k] * r[..., k] for k in range(d))
        lam.append(s)
        bnd.append(SLACK * sum(tg[..., a, k] * ar[..., k] + (d + 1) * U * aG[..., a, k] * ar[..., k] for k in range(d)))
    l0 = 1 - sum(lam)
    b0 = sum(bnd) + SLACK * d * U * (1.0 + sum(np.abs(to_f64(s)) for s in lam))
    return np.stack([l0] + lam, axis=-1), np.stack([b0] + bnd, axis=-1)


def locate(points, cells, x, tol=TOL, cell_ids=None, chunk=256, shift=None):
    """The reference answer and whether it is one: dict of
    ``cell`` (n,) lowest cell id with lambda*_min >= -tol, -1: none;  ``lam`` (n, d + 1) float64 rounding of lambda* there
    (NaN: none);  ``bound`` (n, d + 1) the counted bound on the device's value there;  ``decided`` (n,) bool;
    ``margin`` (n,) min over the cells of |lambda*_min + tol| - bound (> 0: decided);  ``worst_bound`` the largest bound on
    a minimum met in a cell within reach of a point (|lambda_min| <= 2)."""
    geo = CellGeometry(points, cells, cell_ids)
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    out = {"cell": np.full(n, -1, dtype=np.int64), "lam": np.full((n, d + 1), np.nan), "bound": np.full((n, d + 1), np.nan),
           "decided": np.zeros(n, dtype=bool), "margin": np.full(n, -np.inf), "worst_bound": 0.0}
    for p0 in range(0, n, chunk):
        xs = x[p0:p0 + chunk]
        fin = np.isfinite(xs).all(axis=1)
        sh = None if shift is None else np.broadcast_to(np.asarray(shift, dtype=np.float64), x.shape)[p0:p0 + chunk]
        lam, bnd = barycentric(geo, np.where(fin[:, None], xs, 0.0), shift=sh)
        lmin = lam.min(axis=2)  # (m, k)
        bmin = bnd.max(axis=2)
        inside = lmin >= -tol
        margin = (np.abs(to_f64(lmin + tol)) - bmin).min(axis=0)
        hit = inside.any(axis=0) & fin
        first = np.argmax(inside, axis=0)
        k = np.arange(xs.shape[0])
        out["cell"][p0:p0 + chunk] = np.where(hit, geo.ids[first], -1)
        out["lam"][p0:p0 + chunk] = np.where(hit[:, None], to_f64(lam[first, k]), np.nan)
        out["bound"][p0:p0 + chunk] = np.where(hit[:, None], bnd[first, k], np.nan)
        out["margin"][p0:p0 + chunk] = np.where(fin, margin, np.inf)  # (a NaN point fails every comparison: -1, decided)
        near = np.abs(to_f64(lmin)) <= 2.0
        if near.any():
            out["worst_bound"] = max(out["worst_bound"], float(bmin[near].max()))
    out["decided"] = out["margin"] > 0.0
    return out


def bary_in_cells(points, cells, x, cell, shift=None):
    """(lambda* (n, d + 1) extended, bound (n, d + 1)) of point i in the GIVEN cell[i] (all >= 0)."""
    geo = CellGeometry(points, cells)
    return barycentric(geo, x, rows=np.asarray(cell, dtype=np.int64), shift=shift)


def bary_ratio(dev, lam, bound):
    """|dev - lambda*| / bound per entry (a zero bound -- the point is the cell's first vertex -- wants a zero error)."""
    err = to_f64(absx(ext(np.asarray(dev, dtype=np.float64), lam.dtype != object) - lam))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))


def transcribe_bary(points, cells, x, cell, wrong=0.0):
    """float64 numpy restatement of k_loc_geom + loc_bary for point i in cell[i] (no fma).  ``wrong``: the relative error
    put on the first product of every lambda_1."""
    points, cells = np.asarray(points, dtype=np.float64), np.asarray(cells, dtype=np.int64)
    d = points.shape[1]
    xc = points[cells[np.asarray(cell)]]  # (n, d + 1, d)
    e = xc[:, 1:, :] - xc[:, :1, :]
    if d == 2:
        a, b, c2, dd = e[:, 0, 0], e[:, 1, 0], e[:, 0, 1], e[:, 1, 1]
        det = a * dd - b * c2
        g = np.stack([dd / det, -b / det, -c2 / det, a / det], axis=1).reshape(-1, 2, 2)
    else:
        def cross(p, q):
            return np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2],
                             p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], axis=1)
        e1, e2, e3 = e[:, 0], e[:, 1], e[:, 2]
        c23, c31, c12 = cross(e2, e3), cross(e3, e1), cross(e1, e2)
        det = e1[:, 0] * c23[:, 0] + e1[:, 1] * c23[:, 1] + e1[:, 2] * c23[:, 2]
        g = np.stack([c23 / det[:, None], c31 / det[:, None], c12 / det[:, None]], axis=1)
    r = np.asarray(x, dtype=np.float64) - xc[:, 0, :]
    lam = np.zeros((r.shape[0], d + 1))
    l0 = np.ones(r.shape[0])
    for a in range(d):
        s = np.zeros(r.shape[0])
        for k in range(d):
            p = g[:, a, k] * r[:, k]
            if a == 0 and k == 0:
                p = p * (1.0 + wrong)
            s = p + s
        lam[:, a + 1] = s
        l0 = l0 - s
    lam[:, 0] = l0
    return lam


# ---- point classes -----------------------------------------------------------------------------------------------------
def _facets(cells):
    """(facet vertices (nf, d), owner cell, local index of the opposite vertex, exterior mask): every facet once, with
    its lowest owner."""
    nv = cells.shape[1]
    rows = []
    for a in range(nv):
        keep = [b for b in range(nv) if b != a]
        f = np.sort(cells[:, keep], axis=1)
        rows.append(np.concatenate([f, np.arange(cells.shape[0])[:, None], np.full((cells.shape[0], 1), a)], axis=1))
    F = np.concatenate(rows)
    order = np.lexsort([F[:, nv - 1]] + [F[:, k] for k in range(nv - 2, -1, -1)])
    F = F[order]
    _, first, count = np.unique(F[:, : nv - 1], axis=0, return_index=True, return_counts=True)
    return F[first, : nv - 1], F[first, nv - 1], F[first, nv], count == 1


def _edges(cells):
    nv = cells.shape[1]
    E = np.concatenate([np.sort(cells[:, [a, b]], axis=1) for a, b in itertools.combinations(range(nv), 2)])
    return np.unique(E, axis=0)


INSIDE = ("random", "centroid", "facet_interior", "facet_exterior", "edge", "vertex", "within_tol")
OUTSIDE = ("pushed_out", "corner", "nan", "far")


def candidate_points(points, cells, seed=0, n_random=200, corners=False, tol=TOL):
    """name -> (n, d) candidate points of every class of the location tests (float64; whether they are decided and what
    they realise is for ``point_classes`` to say).  ``edge`` is listed on tetrahedra only (the edges of a triangle are its
    facets); ``corner``: the corners of the mesh's bounding box, for meshes that do not fill it."""
    points, cells = np.asarray(points, dtype=np.float64), np.asarray(cells, dtype=np.int64)
    d = points.shape[1]
    rng = np.random.default_rng(seed)
    out = {}
    c = rng.integers(0, cells.shape[0], n_random)
    w = rng.dirichlet(np.ones(d + 1) * 2.0, n_random)
    w = 0.02 + (1.0 - 0.02 * (d + 1)) * w  # every lambda >= 0.02
    out["random"] = np.einsum("na,nak->nk", w, points[cells[c]])
    out["centroid"] = points[cells].mean(axis=1)
    fv, owner, opp, exterior = _facets(cells)
    mid = points[fv].mean(axis=1)
    out["facet_interior"], out["facet_exterior"] = mid[~exterior], mid[exterior]
    if d == 3:
        out["edge"] = points[_edges(cells)].mean(axis=1)
    out["vertex"] = points.copy()
    # outward from an exterior facet: lambda of the opposite vertex is -t at m + t (m - x_opposite)
    m = mid[exterior]
    away = m - points[cells[owner[exterior], opp[exterior]]]
    out["pushed_out"] = m + 1e-6 * away
    out["within_tol"] = m + 0.5 * tol * away
    if corners:
        lo, hi = points.min(axis=0), points.max(axis=0)
        out["corner"] = np.array(list(itertools.product(*[(lo[k], hi[k]) for k in range(d)])))
    out["nan"] = np.full((1, d), np.nan)
    out["far"] = points.max(axis=0)[None, :] + 7.0 * (points.max(axis=0) - points.min(axis=0))[None, :]
    return out


def point_classes(points, cells, seed=0, n_random=200, corners=False, tol=TOL, cell_ids=None):
    """name -> dict(x, cell, lam, bound, dropped): the candidates of every class that are DECIDED and realise the class --
    an inside class: found; an outside class: -1; ``within_tol``: found with -0.9 tol <= lambda*_min <= -0.1 tol --
    with the reference answers, and the number of candidates dropped."""
    out = {}
    for name, x in candidate_points(points, cells, seed, n_random, corners, tol).items():
        R = locate(points, cells, x, tol, cell_ids)
        keep = R["decided"] & ((R["cell"] >= 0) if name in INSIDE else (R["cell"] < 0))
        if name == "within_tol":
            lmin = R["lam"].min(axis=1)
            with np.errstate(invalid="ignore"):
                keep &= (lmin >= -0.9 * tol) & (lmin <= -0.1 * tol)
        out[name] = {"x": x[keep], "cell": R["cell"][keep], "lam": R["lam"][keep], "bound": R["bound"][keep],
                     "dropped": int((~keep).sum()), "worst_bound": R["worst_bound"]}
    return out


# ---- evaluation --------------------------------------------------------------------------------------------------------
_COEF = {}


def p3_table(d: int) -> np.ndarray:
    """OX_P3_COEF<d>[q][a] as the kernel reads it: the literals of csrc/fe_tables_eval.h converted to float64."""
    if d not in _COEF:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        text = open(os.path.join(root, "oasisx_amd", "csrc", "fe_tables_eval.h")).read()
        m = re.search(r"OX_P3_COEF%d\[(\d+)\]\[(\d+)\]\s*=\s*\{(.*?)\};" % d, text, re.S)
        nums = re.findall(r"[-+]?\d+\.?\d*(?:[eE][-+]?\d+)?", m.group(3))
        nq, na = int(m.group(1)), int(m.group(2))
        assert len(nums) == nq * na == O.num_cell_dofs(d, 3) ** 2
        _COEF[d] = np.array([float(v) for v in nums]).reshape(nq, na)
    return _COEF[d]


def p3_exponents(d: int):
    """Exponents (i, j[, k]) of lambda_1..d in probe_mono3's order: i slowest."""
    if d == 2:
        return [(i, j) for i in range(4) for j in range(4 - i)]
    return [(i, j, k) for i in range(4) for j in range(4 - i) for k in range(4 - i - j)]


def basis(d: int, degree: int, lam):
    """(phi (n, nd) in the type of ``lam``, B_phi (n, nd) float64, rounded chain of one phi) at barycentric points."""
    al = np.abs(to_f64(lam))
    if degree == 1:
        return lam, al, 0
    if degree == 2:
        phi = [lam[:, a] * (2 * lam[:, a] - 1) for a in range(d + 1)] + [4 * lam[:, a] * lam[:, b] for a, b in O.local_edges(d)]
        B = [al[:, a] * (2 * al[:, a] + 1) for a in range(d + 1)] + [4 * al[:, a] * al[:, b] for a, b in O.local_edges(d)]
        return np.stack(phi, axis=1), np.stack(B, axis=1), 2
    C = p3_table(d)
    m = np.stack([np.prod([lam[:, v + 1] ** e for v, e in enumerate(ex)], axis=0) for ex in p3_exponents(d)], axis=1)
    am = np.abs(to_f64(m))
    Cx = ext(C, lam.dtype != object)
    phi = np.stack([sum(m[:, q] * Cx[q, a] for q in range(C.shape[0])) for a in range(C.shape[1])], axis=1)
    return phi, am @ np.abs(C), 2 + C.shape[0]


def evaluate(d: int, degree: int, bary, u_rows):
    """(value (n, k) extended, B (n, k) float64, n chain) of sum_a phi_a(bary_i) u_rows[i, a, :]; ``bary`` float64 (the
    device's), ``u_rows`` (n, nd, k) float64 dof values of the point's cell in local dof order."""
    lam = ext(np.asarray(bary, dtype=np.float64))
    u = np.asarray(u_rows, dtype=np.float64)
    phi, Bphi, n_phi = basis(d, degree, lam)
    ux = ext(u)
    val = sum(phi[:, a, None] * ux[:, a, :] for a in range(u.shape[1]))
    B = np.einsum("na,nak->nk", Bphi, np.abs(u))
    return val, B, n_phi + u.shape[1]


def transcribe_eval(d: int, degree: int, bary, u_rows, wrong=0.0):
    """float64 numpy restatement of probe_basis / probe_mono3 / probe_phi3 and the accumulation of k_eval_points (no
    fma).  ``wrong``: the relative error put on the product of the LAST dof's term."""
    lam = np.asarray(bary, dtype=np.float64)
    u = np.asarray(u_rows, dtype=np.float64)
    if degree == 1:
        phi = [lam[:, a] for a in range(d + 1)]
    elif degree == 2:
        phi = [lam[:, a] * (2.0 * lam[:, a] - 1.0) for a in range(d + 1)] + [4.0 * lam[:, a] * lam[:, b] for a, b in O.local_edges(d)]
    else:
        C = p3_table(d)
        p = [[np.ones(lam.shape[0]), lam[:, v + 1], lam[:, v + 1] * lam[:, v + 1], lam[:, v + 1] * lam[:, v + 1] * lam[:, v + 1]]
             for v in range(d)]
        ms = []
        for ex in p3_exponents(d):
            t = p[0][ex[0]] * p[1][ex[1]]
            ms.append(t if d == 2 else t * p[2][ex[2]])
        phi = []
        for a in range(C.shape[1]):
            s = np.zeros(lam.shape[0])
            for q in range(C.shape[0]):
                s = ms[q] * C[q, a] + s
            phi.append(s)
    acc = np.zeros((lam.shape[0], u.shape[2]))
    nd = len(phi)
    for a in range(nd):
        term = phi[a][:, None] * u[:, a, :]
        if a == nd - 1:
            term = term * (1.0 + wrong)
        acc = term + acc
    return acc


# ---- grid sizing -------------------------------------------------------------------------------------------------------
def grid_sizing(points, cells, tol=TOL, rule="axis", pad_abs=0.0, cell_ids=None):
    """float64 emulation of k_loc_geom's boxes, loc_create's bins per axis and k_loc_bins' counts: dict of ``nb`` (bins
    per axis), ``bins``, ``list`` (bin-list entries), ``span`` (the most bins one cell is listed in), ``frac`` (the
    distance of the unrounded bins per axis from the next integer below: how far ``nb`` is from changing)."""
    points, cells = np.asarray(points, dtype=np.float64), np.asarray(cells, dtype=np.int64)
    if cell_ids is not None:
        cells = cells[np.sort(np.asarray(cell_ids))]
    d = points.shape[1]
    n = cells.shape[0]
    x = points[cells]
    l, h = x.min(axis=1), x.max(axis=1)
    pad = (d + 2) * tol * (h - l) + 1e-15 * np.maximum(np.abs(l), np.abs(h)) + pad_abs
    l, h = l - pad, h + pad
    lo, hi = l.min(axis=0), h.max(axis=0)
    extent = hi - lo
    if rule == "isotropic":
        q = extent / (np.prod(extent) / n) ** (1.0 / d)
    else:
        r = extent / ((h - l).sum(axis=0) / n)
        q = r * (n / np.prod(r)) ** (1.0 / d)
    nb = np.minimum(np.maximum(np.ceil(q), 1.0), 1024.0).astype(np.int64)
    inv_h = nb / extent

    def bin_of(v):
        t = (v - lo) * inv_h
        return np.minimum(np.where(t > 0, np.minimum(t, 2.0e9), 0.0).astype(np.int64), nb - 1)
    per_cell = np.prod(bin_of(h) - bin_of(l) + 1, axis=1)
    return {"nb": [int(v) for v in nb], "bins": int(np.prod(nb)), "list": int(per_cell.sum()), "span": int(per_cell.max()),
            "frac": float((q - np.floor(q)).min()), "cells": n, "lo": lo, "hi": hi, "inv_h": inv_h}
