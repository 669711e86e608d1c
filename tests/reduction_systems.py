"""The mesh-free test systems of tests/test_gpu_reduction_sizes.py and the partial-row counts of the library's reductions
(plain numpy / scipy: importable without a GPU)."""
from __future__ import annotations

import numpy as np

# ---- the mesh-free systems ------------------------------------------------------------------------------------------
KINDS = ("sym", "nonsym", "dict")
# the dictionary system's values: 4 off-diagonal and 8 diagonal values (<= 256 distinct bit patterns in the matrix and in
# its inverse diagonal: la.SellMatrix.freeze builds the value dictionary, KSPSolver the dictionary of dinv)
DICT_OFF = np.array([-0.25, -0.3125, -0.375, -0.5])
DICT_DIAG = np.array([2.5, 2.625, 2.75, 3.0, 3.25, 3.5, 3.75, 4.0])


def band_offset(n: int) -> int:
    """The far band's offset m: odd, no multiple of 64, a few slices away from the diagonal."""
    return int(min(1021, max(3, (n // 3) | 1)))


def banded_system(n: int, kind: str, seed: int = 0):
    """scipy CSR (sorted indices) with the bands 0, +-1, +-m, strictly diagonally dominant with a positive diagonal.
    "sym": symmetric, every value its own random number (more than 256 distinct diagonal values); "nonsym": upper and
    lower bands drawn independently; "dict": symmetric, values from DICT_OFF / DICT_DIAG."""
    import scipy.sparse as sp

    assert kind in KINDS and n >= 8
    m = band_offset(n)
    rng = np.random.default_rng(1000 + seed)
    if kind == "dict":
        u1, um = DICT_OFF[rng.integers(0, 4, n - 1)], DICT_OFF[rng.integers(0, 4, n - m)]
        l1, lm = u1, um
        d = DICT_DIAG[rng.integers(0, 8, n)]
    else:
        u1, um = -(0.3 + 0.2 * rng.random(n - 1)), -(0.2 + 0.2 * rng.random(n - m))
        if kind == "sym":
            l1, lm = u1, um
        else:
            l1, lm = -(0.3 + 0.2 * rng.random(n - 1)), 0.1 + 0.3 * rng.random(n - m)  # (mixed signs below the diagonal)
        s = np.zeros(n)
        s[:-1] += np.abs(u1)
        s[:-m] += np.abs(um)
        s[1:] += np.abs(l1)
        s[m:] += np.abs(lm)
        d = s * (1.5 + 0.5 * rng.random(n)) + 0.1
    A = sp.diags([lm, l1, d, u1, um], [-m, -1, 0, 1, m], format="csr")
    A.sort_indices()
    return A


def dominance(A) -> float:
    """min over rows of (|a_ii| - sum_{j != i} |a_ij|) / |a_ii|: positive for a strictly diagonally dominant matrix."""
    d = np.abs(A.diagonal())
    off = np.asarray(abs(A).sum(axis=1)).ravel() - d
    return float(((d - off) / d).min())


def signed_unit_vectors(n: int, nc: int, seed: int):
    """(n, nc) entries of magnitude in [0.5, 1.5] with mixed signs: every block's share of a dot product has the same
    order of magnitude, so a partial row lost or read twice moves the sum by about 1 / nparts relative."""
    rng = np.random.default_rng(2000 + seed)
    return (0.5 + rng.random((n, nc))) * np.where(rng.random((n, nc)) < 0.5, -1.0, 1.0)


# ---- the same systems as the local matrix of a one-rank plan whose only peer is the rank itself -----------------------
def ghosted(Acsr, r0: int, perm_seed: int, m: int | None = None):
    """(A_loc, send): ``Acsr`` (n x n, far lower band at offset ``m``, default ``band_offset(n)``) as the n x (n + ng)
    local matrix of a partitioned operator, ng = n - r0.  In every row r >= r0 the entry of column r - m moves to ghost
    column n + j, j a fixed pseudo-random permutation of r - r0 (the send list is not monotone: a pack-order error
    shows), and ``send[j] = r - m``: with ghost j receiving owned row send[j] the matrix acts on owned vectors as
    ``folded(A_loc, send)``, which is ``Acsr`` entry for entry.  r0 > m (every row from r0 on has the band entry) and
    r0 % 64 not in (0, 63): the slice of r0 mixes rows with and without ghost columns and must count as a boundary
    slice.  scipy CSR with sorted indices."""
    import scipy.sparse as sp

    n = Acsr.shape[0]
    m = band_offset(n) if m is None else int(m)
    assert Acsr.shape == (n, n) and m < r0 < n and r0 % 64 not in (0, 63)
    ng = n - r0
    perm = np.random.default_rng(4000 + perm_seed).permutation(ng)
    assert ng < 3 or (np.diff(perm) < 0).any()
    coo = Acsr.tocoo()
    row, col = coo.row.astype(np.int64), coo.col.astype(np.int64)
    move = (row >= r0) & (col == row - m)
    col[move] = n + perm[row[move] - r0]
    send = np.empty(ng, dtype=np.int64)
    send[perm] = np.arange(r0, n) - m
    A_loc = sp.csr_matrix((coo.data, (row, col)), shape=(n, n + ng))
    A_loc.sort_indices()
    assert A_loc.nnz == Acsr.nnz
    return A_loc, send


def folded(A_loc, send):
    """A_eff = A_loc[:, :n] + A_loc[:, n:] S with S[j, send[j]] = 1: what the ghosted matrix does to owned vectors."""
    import scipy.sparse as sp

    n, ng = A_loc.shape[0], A_loc.shape[1] - A_loc.shape[0]
    S = sp.csr_matrix((np.ones(ng), (np.arange(ng), np.asarray(send))), shape=(ng, n))
    A = sp.csr_matrix(A_loc[:, :n] + A_loc[:, n:] @ S)
    A.sort_indices()
    return A


def slice_kinds(A_loc):
    """(interior, boundary) 64-row slices of a ghosted matrix: boundary = some row of the slice has a ghost column (as
    SellPattern.split_interior lists them)."""
    n = A_loc.shape[0]
    coo = A_loc.tocoo()
    boundary = np.unique(coo.row[coo.col >= n] // 64).size
    return (n + 63) // 64 - boundary, boundary


def ghost_start(n: int, m: int | None = None) -> int:
    """r0 of the larger cases: about n / 3 and beyond the far band, r0 % 64 == 21, with a number of interior slices that
    is 2 or 3 mod 4 (n_slices % 4 == 1 in these systems: the boundary slices are then no multiple of 4 either, and both
    grids end in a partly filled block)."""
    m = band_offset(n) if m is None else m
    ni = max(n // 3, m) // 64
    while ni % 4 not in (2, 3) or ni * 64 + 21 <= m:
        ni += 1
    return ni * 64 + 21


# ---- partial-row counts (the formulas of csrc/ox_kernels.h) --------------------------------------------------------
def spmv_parts(n_rows: int) -> int:
    """Partial rows the lane = row mat-vec writes: round8(ceil(n_slices / 4)) (ox_spmv_blocks_n)."""
    n_slices = (n_rows + 63) // 64
    return (((n_slices + 3) // 4) + 7) & ~7


def vec_blocks(n: int, cap_small: int = 2048, cap_large: int = 1024) -> int:
    """ox_vec_blocks(n): blocks of a BLAS-1 launch over n elements, two per thread, capped by ox_vec_cap(n)."""
    b = max((n // 2 + 255) // 256, 1)
    return min(b, cap_large if n >= (1 << 24) else cap_small)


def vec_parts(n_rows: int) -> int:
    """Partial rows the Krylov vector kernels write: ox_vec_blocks(2 n_rows) (one row per thread)."""
    return vec_blocks(2 * max(n_rows, 1))


def split_parts(n_interior_slices: int, n_boundary_slices: int) -> int:
    """Partial rows the overlapped mat-vec of a partitioned operator writes: the interior and the boundary launch each
    round their own grid to 8 (ox_spmv_dist_nparts)."""
    r8 = lambda n_slices: (((n_slices + 3) // 4) + 7) & ~7
    return r8(n_interior_slices) + r8(n_boundary_slices)


def rows_for_parts(nparts: int) -> int:
    """The n_rows with spmv_parts(n_rows) == nparts (a multiple of 8), n_rows % 64 == 37 and n_slices % 4 == 1."""
    assert nparts % 8 == 0 and nparts >= 8
    n_slices = 4 * (nparts - 1) + 1
    n = (n_slices - 1) * 64 + 37
    assert spmv_parts(n) == nparts and n % 64 != 0 and ((n + 63) // 64) % 4 != 0
    return n
