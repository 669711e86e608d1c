"""Reference of the flow diagnostics and running statistics (oasisx_amd/diagnostics.py, csrc/ox_diag.hip); no GPU.

* Centroid quantities: numpy on ``tests/viscosity_model.centroid_gradient`` (the contraction order of the kernel).
* Cell integrals: in the extended type of tests/assembly_model.py from ITS exact bases and reference tensors (the simplex
  formula), not from a quadrature rule -- each with the running bound ``B`` and the chain length ``n`` of that file's
  criterion ``|dev - value| <= (n + 2) 2^-53 B``.  ``B`` is the kernel's own computation with every factor replaced by its
  absolute value: |u|, |G| with |G_0| := sum_a |G_a|, the absolute mass table, the absolute derivatives at the points of
  the kernel's positive-weight rule (``kernel_rule``).  ``n`` is counted from the lines of ox_diag.hip (``chain``).
* Statistics: West's recurrence in the extended type with its running bound, and the two-pass moments.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import ipcs_oracle as O
from tests import assembly_model as AM
from tests import viscosity_model as VM

U = AM.U
COLUMNS = ("vol", "ke", "strain2", "diss", "ens", "div2", "div1")


# ---- centroid quantities ---------------------------------------------------------------------------------------------
def centroid_fields(F, u, dt):
    """{cfl, shear, divc, q, omega (nc, 1 | 3), gnorm = ||g||_F} per cell of the Forms ``F`` (float64)."""
    d = F.d
    g = VM.centroid_gradient(F, u)
    bary = np.full((1, d + 1), 1.0 / (d + 1))
    phi, _ = O.tabulate(d, F.u_deg, bary)
    uc = np.einsum("cid,i->cd", u[F.vd], phi[0])
    cfl = dt * np.abs(np.einsum("cd,cad->ca", uc, F.G)).max(axis=1)
    S = 0.5 * (g + np.swapaxes(g, 1, 2))
    W = 0.5 * (g - np.swapaxes(g, 1, 2))
    ss = np.einsum("cdk,cdk->c", S, S)
    ww = np.einsum("cdk,cdk->c", W, W)
    if d == 2:
        om = (g[:, 1, 0] - g[:, 0, 1])[:, None]
    else:
        om = np.stack([g[:, 2, 1] - g[:, 1, 2], g[:, 0, 2] - g[:, 2, 0], g[:, 1, 0] - g[:, 0, 1]], axis=1)
    return dict(cfl=cfl, shear=np.sqrt(2.0 * ss), divc=np.einsum("cdd->c", g), q=0.5 * (ww - ss), omega=om,
                gnorm=np.sqrt(np.einsum("cdk,cdk->c", g, g)))


# ---- the kernel's rule and chains ------------------------------------------------------------------------------------
def kernel_rule(d, deg):
    """(barycentric points, weights summing to 1) of the rule ox_diag.hip sums the gradient forms on
    (tools/gen_tables_diag.py: the centroid; the symmetric degree-2 rules; collapsed Gauss-Jacobi, 3 per direction)."""
    if deg == 1:
        return np.full((1, d + 1), 1.0 / (d + 1)), np.ones(1)
    if deg == 2:
        a, b = (1.0 / 6.0, 2.0 / 3.0) if d == 2 else ((5.0 - math.sqrt(5.0)) / 20.0, (5.0 + 3.0 * math.sqrt(5.0)) / 20.0)
        return np.full((d + 1, d + 1), a) + (b - a) * np.eye(d + 1), np.full(d + 1, 1.0 / (d + 1))
    bary, w = O.simplex_quadrature(d, 3)
    return bary, w * math.factorial(d)


def chain(form, d, deg):
    """Rounded operations in the longest chain that ends in one cell integral of k_flow_cells, tabulated constants
    included (one each).  A product of two computed gradients carries the chain of both."""
    nd = O.num_cell_dofs(d, deg)
    nq = kernel_rule(d, deg)[1].shape[0]
    nvol = 2  # vol = adet * (1 / 6): the constant and the product (0.5 * adet in 2-D is exact)
    if form == "vol":
        return nvol
    if form == "ke":  # r: the constant and ND fma; k2: GDIM ND fma; (0.5 vol) k2
        return 1 + nd + d * nd + nvol + 1
    ng = 1 + nd + (d + 1) + d  # t: the constant and ND fma; g: d + 1 fma with G_0 = -sum_a G_a (d subtractions)
    tail = 1 + nq + nvol + 1  # the weight, NQ fma, vol (or 0.5 vol, exact) times the sum
    if form == "strain2":  # s = 0.5 (g + g^T): 1; ss: d^2 fma of s s
        return 2 * (ng + 1) + d * d + tail
    if form == "diss":  # nu + nut, times strain2
        return chain("strain2", d, deg) + 2
    if form == "ens":  # om: 1 subtraction; om2: <= 3 operations
        return 2 * (ng + 1) + 3 + tail
    if form == "div2":  # tr: d - 1 additions; tr tr
        return 2 * (ng + d - 1) + 1 + tail
    if form == "div1":
        return ng + d - 1 + tail
    raise ValueError(form)


# ---- cell integrals in the extended type -----------------------------------------------------------------------------
def _first_moments(d, deg, extended):
    """D1[i][b] = int d(phi_i)/d(lambda_b) over the reference simplex per unit |det J|."""
    cols = [AM._tensor(d, [(deg, b)]) for b in range(d + 1)]
    return AM.ext(np.stack(cols, axis=-1), extended)


def cell_integrals(geo: AM.Geometry, vd, deg, u, nu, nut=None):
    """(value (nc, 7) extended, B (nc, 7) float64, n (7,) int) in the order of ``COLUMNS``; ``geo`` and ``vd`` in the
    kernel's cell order, ``u`` (n_u, d) float64, ``nut`` (nc,) float64 or None."""
    x, d = geo.extended, geo.d
    vd = np.asarray(vd, dtype=np.int64)
    u = np.asarray(u, dtype=np.float64)
    uc, auc = AM.ext(u, x)[vd], np.abs(u)[vd]  # (nc, nd, d)
    fact = math.factorial(d)
    adet, G = geo.adet, geo.G
    mass = AM.ref("mass", d, deg, extended=x)
    stiff = AM.ref("stiff", d, deg, extended=x)
    D1 = _first_moments(d, deg, x)
    ke = adet * AM._einsum("cid,ij,cjd->c", uc, mass, uc) / 2
    T = AM._einsum("cid,iajb,cje->cdaeb", uc, stiff, uc)
    P = adet[:, None, None, None, None] * AM._einsum("cdaeb,cak,cbl->cdkel", T, G, G)  # int g[d][k] g[e][l]
    sq = sum(P[:, a, b, a, b] for a in range(d) for b in range(d))  # int g:g
    tr = sum(P[:, a, b, b, a] for a in range(d) for b in range(d))  # int g:g^T
    strain2, ens = sq + tr, (sq - tr) / 2
    div2 = sum(P[:, a, a, b, b] for a in range(d) for b in range(d))
    div1 = adet * AM._einsum("cid,ib,cbd->c", uc, D1, G)
    nueff = AM.ext(np.float64(nu), x) + (0 if nut is None else AM.ext(np.asarray(nut, dtype=np.float64), x))
    val = np.stack([adet / fact, ke, strain2, nueff * strain2, ens, div2, div1], axis=1)
    # the bounds
    vol = geo.aadet / fact
    amass = np.abs(AM.to_f64(mass)) * fact  # the kernel's table: the mean of phi_i phi_j
    Bke = 0.5 * vol * np.einsum("cid,ij,cjd->c", auc, amass, auc, optimize=True)
    bary, w = kernel_rule(d, deg)
    _, dphi = O.tabulate(d, deg, bary)
    ag = np.einsum("cid,qib,cbk->cqdk", auc, np.abs(dphi), geo.aG, optimize=True)
    sym = 0.5 * (ag + np.swapaxes(ag, 2, 3))
    Bs2 = vol * np.einsum("q,cq->c", w, 2.0 * np.einsum("cqdk,cqdk->cq", sym, sym))
    pairs = [(1, 0)] if d == 2 else [(2, 1), (0, 2), (1, 0)]
    om2 = sum((ag[:, :, a, b] + ag[:, :, b, a]) ** 2 for a, b in pairs)
    Bens = 0.5 * vol * np.einsum("q,cq->c", w, om2)
    atr = np.einsum("cqdd->cq", ag)
    Bd2, Bd1 = vol * np.einsum("q,cq->c", w, atr * atr), vol * np.einsum("q,cq->c", w, atr)
    anu = float(nu) + (0.0 if nut is None else np.abs(np.asarray(nut, dtype=np.float64)))
    B = np.stack([vol, Bke, Bs2, anu * Bs2, Bens, Bd2, Bd1], axis=1)
    n = np.array([chain(f, d, deg) for f in COLUMNS], dtype=np.int64)
    assert int(n.max()) <= AM.N_MAX, n
    return val, B, n


def geometry_of_forms(F) -> AM.Geometry:
    """The extended geometry of the oracle's Forms (its own cell order) from the mesh coordinates."""
    rec, _, _ = AM.geometry_from_coords(F.coords, F.cells)
    d = F.d
    return AM.Geometry(rec[:, : d * d].reshape(-1, d, d), rec[:, d * d])


def extended_sum(a):
    """Column sums of a float64 array in the extended type, and sum |.| in float64."""
    a = np.asarray(a, dtype=np.float64)
    return AM.ext(a).sum(axis=0), np.abs(a).sum(axis=0)


# ---- statistics ------------------------------------------------------------------------------------------------------
C_MEAN, C_COV = 4, 9
"""Roundings per update of k_stats / west() in ox_diag.hip, with the float64 weight sums W handed to the model as data.
mean: a = w / W' (1), delta = x - mean (1), fma (1), and the rounding of the stored mean against its own bound (1): with
err_k <= (C_MEAN k + 2) u B_k and B_k = B_{k-1} + a (|x| + B_{k-1}):  err_k <= (1 + a) err_{k-1} + 3 u a (|x| + B_{k-1}) +
u B_k <= (C_MEAN (k - 1) + 2 + 4) u B_k.
cov: each delta carries the mean's error, (C_MEAN (k - 1) + 2 + 1) u (|x| + B_{k-1}); b = W a (2), b delta_i (1), the fma
(1):  err_k <= err_{k-1} + (2 (4 k - 1) + 3) u term_k + u Bc_k, summed over k <= K: (8 K + 1) u Bc_K + K u Bc_K = (C_COV K +
1) u Bc_K."""


def tri_pairs(nc):
    return [(i, j) for i in range(nc) for j in range(i, nc)]


def west(xs, ws, dtype=None):
    """West's recurrence over the levels ``xs`` ((n, nc) float64 each) with weights ``ws``; W accumulated in float64 as
    the caller of the kernel does.  Returns (mean, cov sums (n, nc (nc + 1) / 2)) in ``dtype`` (default: the extended
    type), and the running bounds (Bmean, Bcov) in float64."""
    dtype = np.longdouble if dtype is None else dtype
    nc = xs[0].shape[1]
    pr = tri_pairs(nc)
    W = 0.0
    mean = np.zeros(xs[0].shape, dtype=dtype)
    cov = np.zeros((xs[0].shape[0], len(pr)), dtype=dtype)
    Bm, Bc = np.zeros(xs[0].shape), np.zeros(cov.shape)
    for x64, w in zip(xs, ws):
        x, ax = x64.astype(dtype), np.abs(x64)
        if W == 0.0:
            mean, cov[:] = x.copy(), 0
            Bm, Bc[:] = ax.copy(), 0.0
        else:
            Wn = W + float(w)
            a = dtype(w) / dtype(Wn)
            b = dtype(W) * a
            dl, adl = x - mean, ax + Bm
            mean = mean + a * dl
            Bm = Bm + float(a) * adl
            for k, (i, j) in enumerate(pr):
                cov[:, k] += (b * dl[:, i]) * dl[:, j]
                Bc[:, k] += float(b) * adl[:, i] * adl[:, j]
        W = W + float(w)
    return mean, cov, Bm, Bc


def two_pass(xs, ws):
    """(mean, cov sums) in the extended type: the textbook moments about the final mean."""
    xe = [x.astype(np.longdouble) for x in xs]
    we = [np.longdouble(w) for w in ws]
    Wt = sum(we)
    mean = sum(w * x for w, x in zip(we, xe)) / Wt
    pr = tri_pairs(xs[0].shape[1])
    cov = np.zeros((xs[0].shape[0], len(pr)), dtype=np.longdouble)
    for w, x in zip(we, xe):
        dl = x - mean
        for k, (i, j) in enumerate(pr):
            cov[:, k] += w * dl[:, i] * dl[:, j]
    return mean, cov


def raw_sums(xs, ws):
    """(mean, cov sums) in float64 from sum w, sum w x, sum w x x: the formula the kernel must NOT use."""
    Wt = float(sum(ws))
    s1 = sum(w * x for w, x in zip(ws, xs))
    pr = tri_pairs(xs[0].shape[1])
    s2 = np.stack([sum(w * x[:, i] * x[:, j] for w, x in zip(ws, xs)) for i, j in pr], axis=1)
    mean = s1 / Wt
    return mean, s2 - Wt * np.stack([mean[:, i] * mean[:, j] for i, j in pr], axis=1)


STAT_WEIGHTS = [0.5, 0.25, 0.375, 1.0, 0.125, 0.75, 0.625, 0.25, 1.5, 0.875, 0.5, 0.3125]  # K = 12, unequal


def stat_levels(X, nc, offset=0.0, K=12):
    """K levels of ``nc`` components at the points X (3, n): the perturbed Taylor-Green of tests/test_gpu_viscosity.py at
    distinct t (nu = 0.01, amplitude 0.3), plus ``offset`` (the cancellation case: a mean flow of 1e6)."""
    fns = [O.tg_u, O.tg_v, O.tg_w]
    out = []
    for k in range(K):
        t = 0.05 * k + 0.01 * k * k
        cols = [fns[i](X, t, 0.01) + 0.3 * np.sin(1.3 * X[0] + 0.7 * X[1] - 0.9 * X[2] + 1.1 * i + 40.0 * t) for i in range(nc)]
        out.append(np.stack(cols, axis=1) + offset)
    return out
