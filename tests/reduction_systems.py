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


def rows_for_parts(nparts: int) -> int:
    """The n_rows with spmv_parts(n_rows) == nparts (a multiple of 8), n_rows % 64 == 37 and n_slices % 4 == 1."""
    assert nparts % 8 == 0 and nparts >= 8
    n_slices = 4 * (nparts - 1) + 1
    n = (n_slices - 1) * 64 + 37
    assert spmv_parts(n) == nparts and n % 64 != 0 and ((n + 63) // 64) % 4 != 0
    return n
