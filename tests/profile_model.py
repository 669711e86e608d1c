"""Reference of the slab-averaged statistics (oasisx_amd/diagnostics.py ``ProfileStatistics``, ``ox_profile_cells`` /
``ox_profile_update`` of csrc/ox_diag.hip) in the extended type of tests/assembly_model.py; no GPU.

* Per cell: ``[vol, s1 (NQ), s2 (NQ (NQ + 1) / 2)]`` about a shift, from the exact mass tensor ``AM.ref("mass", ...)``, the
  geometry records, the dof table and the values, each with the running bound ``B`` (the kernel's own computation with
  every factor replaced by its absolute value) of the criterion ``|dev - value| <= (n + 2) 2^-53 B``.
* Sums over labelled groups of cells (chunks, bins): value, bound and the number of cells.
* The merge recurrence of ``ox_profile_update`` in ``np.longdouble`` (or any other type), fed the float64 weight sums
  ``W`` as data, with running bounds; and the space-time two-pass moments about the final mean.

Rounding counts
---------------
Per cell (``chain``; ND dofs, one rounding for each tabulated constant, as in tests/diagnostics_model.py):

* ``vol``: ``adet * (1 / 6)``, the constant and the product: 2 (``0.5 * adet`` in 2-D is exact).
* ``s1``: ``delta = q - shift`` (1);  ``m_i``, the row sum of the mean mass table, a constant and ND - 1 additions (ND);
  the ND fma of the sum over i (ND);  ``vol`` (2);  ``vol * s`` (1):  2 ND + 4.
* ``s2``: the two ``delta`` (2);  ``r = sum_j M_ij delta_j``, a constant and ND fma (ND + 1);  ``s2 += delta_i r``, ND fma
  (ND);  ``vol`` (2);  ``vol * s2`` (1):  2 ND + 6.

A sum of ``c`` cells through any tree adds ``c - 1``: ``n = chain + c - 1`` (``Slabs.sums`` returns it per bin).

Per update of lane 0 in ``k_profile_update`` (``C_MEAN``, ``C_COV`` and ``merge_counts``), with ``n1, n2, nV`` the counts of
the bin's ``S1, S2, V`` and their ``+ 2`` of the criterion kept:

* ``d = S1 * (1 / V)``: the error of ``S1`` (n1 + 2), the relative error of ``V`` (nV + 2, ``V`` is a sum of positive
  terms: its bound is itself), ``1 / V`` (1), the product (1):  ``n_d = n1 + nV + 6`` against ``Bd = B1 / V``.
* ``g = shift + d`` (1):  ``n_g = n_d + 1`` against ``Bg = |shift| + Bd``.  ``g`` is the sample West's update sees.
* mean: ``a = w / W'`` (1), ``dl = g - mean`` (1), the fma (1), the stored mean against its own bound (1).  With
  ``err_k <= (C_MEAN k + 2 + n_g) u Bm_k`` and ``Bm_k = Bm_{k-1} + a (Bg + Bm_{k-1})``:
  ``err_k <= (1 + a) err_{k-1} + a n_g u Bg + 3 u a (Bg + Bm_{k-1}) + u Bm_k <= (C_MEAN (k - 1) + 2 + n_g) u ((1 + a) Bm_{k-1}
  + a Bg) + 4 u Bm_k = (C_MEAN k + 2 + n_g) u Bm_k``,  ``C_MEAN = 4`` (n_g taken as its largest value over the samples).
* second moment, spatial part ``w (S2 / V - d_i d_j)``: ``S2 / V`` carries n2 + 2 + nV + 2 + 2, ``d_i d_j`` carries
  2 n_d + 1, the fma (1) and the product with w, folded into the accumulating fma (1):
  ``n_sp = (n2 + nV + 6) + (2 n_d + 1) + 2`` against ``w (B2 / V + Bd_i Bd_j)`` (the sum of the two chains bounds either).
* second moment, temporal part ``b dl_i dl_j``: each ``dl`` carries the error of g (n_g), of the mean
  (C_MEAN (k - 1) + 2 + n_g) and its own rounding (1); ``b = W a`` (2), ``b dl_i`` (1), the fma (1):
  ``2 (C_MEAN (k - 1) + 2 n_g + 3) + 4 = 8 k + 4 n_g + 2`` against ``b (Bg_i + Bm_i) (Bg_j + Bm_j)``.
* Each of the K accumulations rounds once against the running bound: summed over k <= K,
  ``err <= (8 K + 4 n_g + 2 + n_sp + K) u Bc_K = (C_COV K + 4 n_g + n_sp + 2) u Bc_K``,  ``C_COV = 9``.

The shift of a sample is the float64 running mean.  The model uses ITS OWN running mean, rounded to float64, where the
device uses the device's: exact sums do not depend on the shift, and the bounds change by a relative 2^-53 of |shift|.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import ipcs_oracle as O
from tests import assembly_model as AM

U = AM.U
C_MEAN, C_COV = 4, 9


def tri_pairs(nq):
    return [(i, j) for i in range(nq) for j in range(i, nq)]


def chain(what, d, deg):
    """Rounded operations in the longest chain that ends in one entry of a cell's row in k_profile_cells."""
    nd = O.num_cell_dofs(d, deg)
    n = {"vol": 2, "s1": 2 * nd + 4, "s2": 2 * nd + 6}[what]
    assert n <= AM.N_MAX
    return n


def row_chain(d, deg, nq):
    return np.array([chain("vol", d, deg)] + [chain("s1", d, deg)] * nq + [chain("s2", d, deg)] * (nq * (nq + 1) // 2))


def mean_mass(d, deg, extended=None):
    """The mean of phi_i phi_j over the cell (the kernel's OX_MASSD table) in the extended type."""
    return AM.ref("mass", d, deg, extended=extended) * math.factorial(d)


def cell_moments(geo: AM.Geometry, vd, deg, q, shift):
    """(value (nc, NR) extended, B (nc, NR) float64) per cell in the kernel's cell order: ``[vol, s1, s2]`` of the values
    ``q`` (n, NQ) float64 at the dofs ``vd`` about ``shift`` (nc, NQ), float64 or extended."""
    x, d = geo.extended, geo.d
    vd = np.asarray(vd, dtype=np.int64)
    q = np.asarray(q, dtype=np.float64)
    nq = q.shape[1]
    shift = np.asarray(shift)
    sh = AM.ext(shift, x) if shift.dtype == np.float64 else shift
    delta = AM.ext(q, x)[vd] - sh[:, None, :]  # (nc, nd, nq)
    adelta = np.abs(AM.to_f64(delta))
    fact = math.factorial(d)
    mass = mean_mass(d, deg, x)
    amass = np.abs(AM.to_f64(mass))
    vol, avol = geo.adet / fact, geo.aadet / fact
    s1 = vol[:, None] * AM._einsum("ij,cik->ck", mass, delta)
    B1 = avol[:, None] * np.einsum("ij,cik->ck", amass, adelta)
    Md = AM._einsum("ij,cjl->cil", mass, delta)
    aMd = np.einsum("ij,cjl->cil", amass, adelta)
    pr = tri_pairs(nq)
    s2 = np.stack([vol * (delta[:, :, k] * Md[:, :, l]).sum(axis=1) for k, l in pr], axis=1)
    B2 = np.stack([avol * (adelta[:, :, k] * aMd[:, :, l]).sum(axis=1) for k, l in pr], axis=1)
    val = np.concatenate([vol[:, None], s1, s2], axis=1)
    B = np.concatenate([avol[:, None], B1, B2], axis=1)
    return val, B


def label_sums(val, B, labels, n):
    """Sums over the cells of each label 0 .. n - 1 (-1: left out): (S (n, NR) in val's type, BS (n, NR) float64, count
    (n,))."""
    labels = np.asarray(labels, dtype=np.int64)
    S = np.zeros((n, val.shape[1]), dtype=val.dtype)
    if val.dtype == object:
        S = S * val.ravel()[0] * 0
    BS = np.zeros((n, val.shape[1]))
    keep = labels >= 0
    np.add.at(S, labels[keep], val[keep])
    np.add.at(BS, labels[keep], B[keep])
    return S, BS, np.bincount(labels[keep], minlength=n)


class Slabs:
    """The cells of a mesh (kernel cell order: geometry ``geo``, dof table ``vd`` of degree ``deg``) sorted into
    ``n_bins`` bins (``bins`` per cell, -1: left out)."""

    def __init__(self, geo, vd, deg, bins, n_bins=None):
        self.geo, self.vd, self.deg = geo, np.asarray(vd, dtype=np.int64), deg
        self.bins = np.asarray(bins, dtype=np.int64)
        self.n_bins = int(self.bins.max()) + 1 if n_bins is None else int(n_bins)

    def sums(self, q, shift, labels=None, n=None):
        """(S (n_bins, NR) extended, BS float64, n (n_bins, NR): the rounding count chain + cells - 1) about ``shift``
        (n_bins, NQ), or None for 0.  ``labels`` / ``n``: sum over other groups of cells (each inside ONE bin, which gives
        its shift), e.g. the chunks."""
        q = np.asarray(q, dtype=np.float64)
        nq = q.shape[1]
        shift = np.zeros((self.n_bins, nq)) if shift is None else np.asarray(shift)
        val, B = cell_moments(self.geo, self.vd, self.deg, q, shift[np.maximum(self.bins, 0)])
        if labels is None:
            labels, n = self.bins, self.n_bins
        else:
            labels = np.where(self.bins >= 0, labels, -1)
        S, BS, cnt = label_sums(val, B, labels, n)
        return S, BS, row_chain(self.geo.d, self.deg, nq)[None, :] + cnt[:, None] - 1


def chunk_labels(order, chunks, bin_chunk_ptr, n_cells):
    """The chunk of every cell (kernel order, -1: not sampled) from the set-up's tables ``order``, ``chunks``
    ({first entry of order, cells, bin, consecutive}) and ``bin_chunk_ptr`` (host arrays), which are checked on the way:
    the chunks tile ``order``, hold 1 .. 256 cells of ONE bin, the bins ascend, and ``consecutive`` says what it says."""
    order, ch, ptr = np.asarray(order), np.asarray(chunks), np.asarray(bin_chunk_ptr)
    assert ch.ndim == 2 and ch.shape[1] == 4 and ptr[0] == 0 and ptr[-1] == ch.shape[0] and (np.diff(ptr) >= 1).all()
    assert ch[0, 0] == 0 and np.array_equal(ch[1:, 0], ch[:-1, 0] + ch[:-1, 1]) and ch[-1, 0] + ch[-1, 1] == order.shape[0]
    assert ch[:, 1].min() >= 1 and ch[:, 1].max() <= 256 and np.unique(order).shape[0] == order.shape[0]
    assert order.min() >= 0 and order.max() < n_cells and (np.diff(ch[:, 2]) >= 0).all()
    lab = np.full(n_cells, -1, dtype=np.int64)
    for c, (off, ln, b, consecutive) in enumerate(ch):
        cells = order[off:off + ln]
        lab[cells] = c
        assert ptr[b] <= c < ptr[b + 1] and bool(consecutive) == bool((np.diff(cells) == 1).all())
    return lab


def merge_counts(n1, n2, nV):
    """(n_g, n_sp) of the module docstring from the counts of S1, S2 and V (integers or arrays)."""
    n_d = n1 + nV + 6
    return n_d + 1, (n2 + nV + 6) + (2 * n_d + 1) + 2


def recurrence(slabs: Slabs, levels, ws, dtype=None, seed=True):
    """The running state of ProfileStatistics over the ``levels`` ((n, NQ) float64 each) with weights ``ws``: every sample
    is summed about the float64 running mean (the first one about its own slab means when ``seed``, about 0 otherwise) and
    merged as ox_profile_update does, in ``dtype`` (default: the extended type; the bin sums are rounded to it first).
    Returns dict(mean, m2, vol, Bm, Bc (float64 running bounds), n_mean, n_cov (the counts for AM.check), W)."""
    dtype = np.longdouble if dtype is None else dtype
    nq = levels[0].shape[1]
    pr = tri_pairs(nq)
    nb = slabs.n_bins
    W = 0.0
    mean, m2 = np.zeros((nb, nq), dtype=dtype), np.zeros((nb, len(pr)), dtype=dtype)
    Bm, Bc = np.zeros((nb, nq)), np.zeros((nb, len(pr)))
    n_g, n_sp, vol = 0, 0, None
    for x, w in zip(levels, ws):
        if W == 0.0:
            if seed:
                S, _, _ = slabs.sums(x, None)
                S = AM.to_f64(S).astype(dtype) if dtype != np.longdouble else S
                mean = (S[:, 1:1 + nq] / S[:, :1]).astype(np.float64).astype(dtype)
            Bm = np.abs(mean.astype(np.float64))
        shift = mean.astype(np.float64)
        S, BS, n = slabs.sums(x, shift)
        S = AM.to_f64(S).astype(dtype) if dtype != np.longdouble else S
        g_cnt, sp_cnt = merge_counts(n[:, 1:1 + nq].max(), n[:, 1 + nq:].max(), n[:, 0].max())
        n_g, n_sp = max(n_g, int(g_cnt)), max(n_sp, int(sp_cnt))
        V, aV = S[:, :1], AM.to_f64(S[:, :1])
        vol = V[:, 0]
        a = dtype(w) / dtype(W + float(w))
        b = dtype(W) * a
        d, Bd = S[:, 1:1 + nq] / V, BS[:, 1:1 + nq] / aV
        g, Bg = shift.astype(dtype) + d, np.abs(shift) + Bd
        dl, adl = g - mean, Bg + Bm
        mean = mean + a * dl
        Bm = Bm + float(a) * adl
        for m, (i, j) in enumerate(pr):
            c = S[:, 1 + nq + m] / V[:, 0] - d[:, i] * d[:, j]
            m2[:, m] = m2[:, m] + dtype(w) * c + (b * dl[:, i]) * dl[:, j]
            Bc[:, m] += float(w) * (BS[:, 1 + nq + m] / aV[:, 0] + Bd[:, i] * Bd[:, j]) + float(b) * adl[:, i] * adl[:, j]
        W = W + float(w)
    K = len(ws)
    return dict(mean=mean, m2=m2, vol=vol, Bm=Bm, Bc=Bc, n_mean=C_MEAN * K + n_g, n_cov=C_COV * K + 4 * n_g + n_sp, W=W)


def two_pass(slabs: Slabs, levels, ws):
    """(mean (n_bins, NQ), m2 (n_bins, NV)) in the extended type: ``sum_k w_k int_b q / V_b / W`` and ``sum_k w_k int_b
    (q - mean)(q - mean)^T / V_b`` about that final mean."""
    nq = levels[0].shape[1]
    we = [np.longdouble(w) for w in ws]
    Wt = sum(we)
    acc = 0
    for x, w in zip(levels, we):
        S, _, _ = slabs.sums(x, None)
        acc = acc + w * S[:, 1:1 + nq] / S[:, :1]
    mean = acc / Wt
    m2 = 0
    for x, w in zip(levels, we):
        S, _, _ = slabs.sums(x, mean)
        m2 = m2 + w * S[:, 1 + nq:] / S[:, :1]
    return mean, m2
