"""GPU: the small vector and row kernels next to the BLAS-1 code, called directly through the C ABI and compared with
numpy / ``math.fsum`` on the host: ``ox_dot``, ``ox_axpby``, ``ox_remove_mean``, ``ox_scatter_add``, ``ox_zero_rows``,
``ox_zero_rows_au``, ``ox_zero_rows_cols`` and ``ox_jacobi_setup``.  Inside full steps they are only ever seen at the
sizes and arguments the solver happens to use; here each meets its own edges: n = 0 / 1 / odd, the ``double2`` tail
element, sizes above the grid cap (a thread takes more than one pair) and past the 2^24 cap change, ``b == 0`` with
``y == NULL``, ``n_apply > n``, a diagonal in either slot of a storage pair, a stored zero diagonal and a tail slice.

Every case passes legal arguments only; the error-path cases are the ones the library rejects on the host before any
launch.

Bounds.  ``ox_dot``: a thread's fma chain, the 256-thread block tree and the ordered reduction of <= 2048 block sums
are a summation tree of depth under 40 over the exact products, so |result - exact| <= 40 * (eps / 2) * sum|x_i y_i| in
the worst case and far less on random data; 8 * eps * sum|x_i y_i| holds with room while one lost element of magnitude
about 1 in 10^6..10^7 (>= 1e-7 relative) does not.  ``ox_axpby``: ``a * x + b * y`` may contract to one fma, i.e. one of
the two products is not rounded; where a x and b y have the same sign that product is no larger than the result, so the
contracted and the uncontracted result round values that differ by at most half an ulp of the result: they are at
most one ulp apart.  With mixed signs (cancellation) the two forms may differ by more; there the result is held to
the exact value within the roundings either form may make: (ulp(a x) + ulp(b y) + ulp(z)) / 2.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import krylov_steps_model as K
from tests import reduction_systems as RS

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
VEC_CAP, PAIR_BLOCK = 2048, 512  # ox_vec_cap below 2^24 elements; elements a block of the pair kernels covers per sweep


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ulps(a, b):
    """Distance in units in the last place between float64 arrays of equal sign pattern (or zero)."""
    ia, ib = np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64)
    return np.abs(ia - ib)


def _signed(n, seed, nc=None):
    v = RS.signed_unit_vectors(max(n, 1), nc or 1, seed)[:n]
    return v if nc else v[:, 0]


# ---- ox_dot -----------------------------------------------------------------------------------------------------
DOT_SIZES = [0, 1, 255, 256, 257, 1048577 + VEC_CAP * PAIR_BLOCK]


@pytest.mark.parametrize("ncomp,n", [(c, n) for n in DOT_SIZES for c in (1, 2, 3)] + [(1, (1 << 24) + 3)])
def test_dot_against_the_exact_sum(hip, ncomp, n):
    from oasisx_amd import _lib

    x, y = _signed(n, 11, ncomp), _signed(n, 12, ncomp)
    if n > (1 << 20):  # 24-bit mantissas: the products are exact in float64 and math.fsum alone is the exact sum
        x, y = x.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)
    xd, yd = _dev(x if n else np.zeros((1, ncomp))), _dev(y if n else np.zeros((1, ncomp)))
    out = [(C.c_double * 3)(7.0, 7.0, 7.0) for _ in range(2)]
    for o in out:
        _lib.check(hip.ox_dot(n, ncomp, _lib.ptr(xd), _lib.ptr(yd), o, None, _lib.current_stream()), "ox_dot")
    for c in range(ncomp):
        ref = K.exact_dot(x[:, c], y[:, c]) if n else 0.0
        bound = 8.0 * EPS * (math.fsum(np.abs(x[:, c] * y[:, c])) if n else 0.0)
        err = abs(out[0][c] - ref)
        print(f"ox_dot n={n} ncomp={ncomp} c={c}: |dev - exact| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (n, ncomp, c, out[0][c], ref)
        assert np.float64(out[0][c]).view(np.int64) == np.float64(out[1][c]).view(np.int64)  # run to run: the same bits
    assert all(out[0][c] == 7.0 for c in range(ncomp, 3))  # only ncomp sums are written


def test_dot_sizes_cross_the_grid_cap_and_the_cap_change():
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oasisx_amd", "csrc", "ox_kernels.h")).read()
    m = re.search(r"return n >= \(\(int64_t\)1 << (\d+)\) \? (\d+) : (\d+);", src)
    assert m, "ox_vec_cap no longer reads as it did: choose the sizes of this module again"
    shift, cap_large, cap_small = (int(g) for g in m.groups())
    assert (cap_small, cap_large) == (VEC_CAP, 1024)
    # k_dot: one row per thread, ox_vec_blocks(n) blocks: above the cap a thread takes several rows, and the last size's
    # last row wraps once more than the others'
    assert RS.vec_blocks(DOT_SIZES[-1]) == cap_small and DOT_SIZES[-1] > cap_small * 256 * 4
    assert (1 << 24) + 3 >= (1 << shift) > DOT_SIZES[-1]
    # the reduction of these block sums is where ox_gather_partials keeps 4 rows in flight (more than 3 x 256 rows)
    small = int(re.search(r"#define OX_RED_THREADS_SMALL (\d+)", src).group(1))
    assert cap_small > 3 * small and re.search(r"p \+ 3 \* T < nparts", src)


# ---- ox_axpby ---------------------------------------------------------------------------------------------------
AXPBY_SIZES = [1, 2, 7, 1000, VEC_CAP * PAIR_BLOCK + 513]


@pytest.mark.parametrize("n", AXPBY_SIZES)
@pytest.mark.parametrize("alias", ["none", "x", "y"])
def test_axpby_same_sign_terms_within_one_ulp_of_numpy(hip, n, alias):
    from oasisx_amd import _lib

    rng = np.random.default_rng(n)
    x, y = 0.5 + rng.random(n), 0.5 + rng.random(n)
    a, b = 0.7, 1.3
    ref = a * x + b * y
    xd, yd = _dev(x), _dev(y)
    zd = {"none": torch.full((n + 2,), -3.0, dtype=torch.float64, device="cuda"), "x": xd, "y": yd}[alias]
    _lib.check(hip.ox_axpby(n, a, _lib.ptr(xd), b, _lib.ptr(yd), _lib.ptr(zd), _lib.current_stream()), "ox_axpby")
    z = zd.cpu().numpy()
    assert _ulps(z[:n], ref).max() <= 1, (n, alias, int(_ulps(z[:n], ref).max()))
    if alias == "none":
        assert (z[n:] == -3.0).all()  # nothing past n (the tail element of an odd n is one 8-byte store)
        assert np.array_equal(xd.cpu().numpy(), x) and np.array_equal(yd.cpu().numpy(), y)
    elif alias == "x":
        assert np.array_equal(yd.cpu().numpy(), y)
    else:
        assert np.array_equal(xd.cpu().numpy(), x)


@pytest.mark.parametrize("n", AXPBY_SIZES)
@pytest.mark.parametrize("alias", ["none", "x", "y"])
def test_axpby_mixed_signs_against_the_exact_value(hip, n, alias):
    from oasisx_amd import _lib

    x, y = _signed(n, 21), _signed(n, 22)
    a, b = -0.7, 1.3
    xd, yd = _dev(x), _dev(y)
    zd = {"none": torch.zeros(n, dtype=torch.float64, device="cuda"), "x": xd, "y": yd}[alias]
    _lib.check(hip.ox_axpby(n, a, _lib.ptr(xd), b, _lib.ptr(yd), _lib.ptr(zd), _lib.current_stream()), "ox_axpby")
    z = zd.cpu().numpy()
    L = np.longdouble
    exact = L(a) * x.astype(L) + L(b) * y.astype(L)  # (64-bit mantissas: the 53 x 53-bit products lose < 2^-63 relative)
    bound = 0.5 * (np.spacing(np.abs(a * x)) + np.spacing(np.abs(b * y)) + np.spacing(np.abs(z))) * (1.0 + 1e-3)
    assert (np.abs(z.astype(L) - exact) <= bound).all()


@pytest.mark.parametrize("n", AXPBY_SIZES)
def test_axpby_b_zero_takes_no_y(hip, n):
    from oasisx_amd import _lib

    x = _signed(n, 23)
    xd = _dev(x)
    zd = torch.full((n + 1,), -3.0, dtype=torch.float64, device="cuda")
    _lib.check(hip.ox_axpby(n, 0.3, _lib.ptr(xd), 0.0, None, _lib.ptr(zd), _lib.current_stream()), "ox_axpby")
    z = zd.cpu().numpy()
    assert np.array_equal(z[:n], 0.3 * x) and z[n] == -3.0  # one product, one rounding: the same bits
    # b != 0 without y: rejected on the host, nothing is launched
    zd.fill_(-5.0)
    assert hip.ox_axpby(n, 0.3, _lib.ptr(xd), 1.0, None, _lib.ptr(zd), _lib.current_stream()) != 0
    assert b"ox_axpby" in hip.ox_last_error()
    torch.cuda.synchronize()
    assert (zd.cpu().numpy() == -5.0).all()
    # n <= 0: nothing to do, no error
    assert hip.ox_axpby(0, 0.3, _lib.ptr(xd), 0.0, None, _lib.ptr(zd), _lib.current_stream()) == 0
    torch.cuda.synchronize()
    assert (zd.cpu().numpy() == -5.0).all()


# ---- ox_remove_mean ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ghosts", [(1, 0), (257, 0), (257, 100), (1000003, 777)])
@pytest.mark.parametrize("weights", [False, True])
def test_remove_mean(hip, n, ghosts, weights):
    """x -= (sum_i<n w_i x_i) / wsum on n_apply = n + ghosts rows: the ghost rows are shifted by the same mean and do not
    enter it (they hold values near 1000: one of them in the sum would move the mean by >= 1e-3)."""
    from oasisx_amd import _lib

    rng = np.random.default_rng(n + ghosts)
    x = np.concatenate([0.25 + _signed(n, 31), 1000.0 + rng.random(ghosts)])
    w = 0.5 + rng.random(n) if weights else None
    L = np.longdouble
    wsum = float(np.sum(w.astype(L))) if weights else float(n)
    mean = np.sum((w.astype(L) if weights else L(1)) * x[:n].astype(L)) / L(wsum)
    xd = torch.cat([_dev(x), torch.full((3,), -3.0, dtype=torch.float64, device="cuda")])
    wd = _dev(w) if weights else None
    _lib.check(hip.ox_remove_mean(n, n + ghosts, _lib.ptr(xd), _lib.ptr(wd), wsum, None, _lib.current_stream()),
               "ox_remove_mean")
    out = xd.cpu().numpy()
    assert (out[n + ghosts:] == -3.0).all()
    xs = out[: n + ghosts]
    tol = 8.0 * EPS * np.abs(x[:n]).max()
    left = abs(float(np.sum((w.astype(L) if weights else L(1)) * xs[:n].astype(L)) / L(wsum)))
    print(f"ox_remove_mean n={n} ghosts={ghosts} weights={weights}: mean left {left:.3e}, bound {tol:.3e}")
    assert left <= tol
    # every row, ghosts included, moved by the one mean (a ghost's own rounding is an ulp of 1000)
    assert np.abs(xs[:n] - (x[:n] - float(mean))).max() <= tol
    if ghosts:
        assert np.abs(xs[n:] - (x[n:] - float(mean))).max() <= tol + np.spacing(1000.0)
    # n_apply < n means n
    xd2 = _dev(x[:n].copy())
    _lib.check(hip.ox_remove_mean(n, 0, _lib.ptr(xd2), _lib.ptr(wd), wsum, None, _lib.current_stream()), "ox_remove_mean")
    assert np.array_equal(xd2.cpu().numpy(), xs[:n])
    # wsum == 0: an error, x is left alone
    before = xd2.clone()
    assert hip.ox_remove_mean(n, n, _lib.ptr(xd2), _lib.ptr(wd), 0.0, None, _lib.current_stream()) != 0
    assert b"wsum" in hip.ox_last_error()
    torch.cuda.synchronize()
    assert torch.equal(before, xd2)


# ---- ox_scatter_add ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncomp", [1, 2, 3])
def test_scatter_add_unique_rows(hip, ncomp):
    from oasisx_amd import _lib

    nb, n = 1531, 777  # rows of b, listed rows: more than one 256-thread block, a partial last one
    rng = np.random.default_rng(ncomp)
    rows = rng.permutation(nb)[:n].astype(np.int32)
    st = _lib.current_stream()
    for comp in range(ncomp):
        b0, y = 0.5 + rng.random((nb, ncomp)), 0.5 + rng.random(n)
        for scale, ulp in ((0.5, 0), (-2.0, 0), (0.3, 1)):  # a power of two: scale * y is exact, fma or not; else <= 1 ulp
            bd, yd, rd = _dev(b0), _dev(y), _dev(rows)
            _lib.check(hip.ox_scatter_add(_lib.ptr(bd), _lib.ptr(rd), _lib.ptr(yd), n, ncomp, comp, scale, st), "ox_scatter_add")
            ref = b0.copy()
            ref[rows, comp] += scale * y
            got = bd.cpu().numpy()
            touched = np.zeros((nb, ncomp), dtype=bool)
            touched[rows, comp] = True
            assert np.array_equal(got[~touched], b0[~touched])  # other rows and other components: untouched
            if ulp == 0:
                assert np.array_equal(got[touched], ref[touched])
            else:
                assert _ulps(got[touched], ref[touched]).max() <= ulp
        # n == 0: nothing happens (the row and value arrays are not read)
        bd = _dev(b0)
        assert hip.ox_scatter_add(_lib.ptr(bd), _lib.ptr(rd), _lib.ptr(yd), 0, ncomp, comp, 1.0, st) == 0
        torch.cuda.synchronize()
        assert np.array_equal(bd.cpu().numpy(), b0)
    # a component outside 0..ncomp-1: rejected on the host
    for comp in (-1, ncomp):
        assert hip.ox_scatter_add(_lib.ptr(bd), _lib.ptr(rd), _lib.ptr(yd), n, ncomp, comp, 1.0, st) != 0
        assert b"ox_scatter_add" in hip.ox_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(bd.cpu().numpy(), b0)


# ---- the row kernels on a small SELL pattern --------------------------------------------------------------------
N_ROWS = 64 * 3 + 21  # a tail slice of 21 rows
ZERO_DIAG_ROW = 70


def _row_system():
    """(SellMatrix, scipy CSR) with n_rows % 64 != 0: row r holds its diagonal and up to three columns on either side, so
    the diagonal sits in slot 0, 1, 2 or 3 of the row (either half of a storage pair); rows differ in length (padding
    slots); ZERO_DIAG_ROW stores a zero on its diagonal."""
    import scipy.sparse as sp

    from oasisx_amd import fem
    from oasisx_amd.la import SellMatrix

    n = N_ROWS
    rng = np.random.default_rng(5)
    rr, cc = [], []
    for r in range(n):
        below = [c for c in range(r - 3, r) if c >= 0][: r % 4]  # 0..3 columns before the diagonal
        above = [c for c in range(r + 1, r + 4) if c < n][: (r // 4) % 4]
        cs = sorted(set(below + [r] + above + ([n - 1 - r] if r % 5 == 0 else [])))
        rr += [r] * len(cs)
        cc += cs
    rr, cc = np.array(rr), np.array(cc)
    vals = np.where(rr == cc, 2.0 + rng.random(rr.size), -0.25 - 0.5 * rng.random(rr.size))
    vals[(rr == ZERO_DIAG_ROW) & (cc == ZERO_DIAG_ROW)] = 0.0
    Acsr = sp.csr_matrix((vals, (rr, cc)), shape=(n, n))  # (explicit zeros are kept)
    Acsr.sort_indices()
    keys = torch.from_numpy(rr.astype(np.int64) * n + cc).cuda()
    row_len = torch.from_numpy(np.diff(Acsr.indptr).astype(np.int64)).cuda()
    row_ptr = torch.from_numpy(Acsr.indptr.astype(np.int64)).cuda()
    P = fem.build_sell(n, n, keys, row_len, row_ptr)
    A = SellMatrix(P)
    A.vals.copy_(P.values_from_csr(Acsr))
    A.version += 1
    slot = np.array([(Acsr.indices[Acsr.indptr[r]:Acsr.indptr[r + 1]] < r).sum() for r in range(n)])
    assert {0, 1, 2, 3} <= set(slot.tolist()) and len(set(np.diff(Acsr.indptr).tolist())) > 3
    return A, Acsr


def _padding_is_zero(A):
    P = A.pattern
    rows, k = P.slot_rows_k()
    rl = np.zeros(P.n_slices * 64, dtype=np.int64)
    rl[: P.n_rows] = P.row_len.cpu().numpy()
    return bool((A.vals.cpu().numpy()[k >= rl[rows]] == 0.0).all())


def _zeroed(Acsr, rows, diag, cols=()):
    ref = Acsr.toarray()
    ref[rows, :] = 0.0
    ref[:, list(cols)] = 0.0
    ref[rows, rows] = diag
    return ref


BC_ROWS = np.array([0, 1, 2, 3, 5, 63, 64, ZERO_DIAG_ROW, 127, 130, 191, 192, 200, N_ROWS - 1], dtype=np.int32)


def test_jacobi_setup_finds_the_diagonal_in_either_slot_of_a_pair(hip):
    from oasisx_amd import _lib

    A, Acsr = _row_system()
    dinv = torch.full((N_ROWS + 64,), -3.0, dtype=torch.float64, device="cuda")
    _lib.check(hip.ox_jacobi_setup(A.ref(), _lib.ptr(dinv), _lib.current_stream()), "ox_jacobi_setup")
    got = dinv.cpu().numpy()
    d = Acsr.diagonal()
    ref = np.where(d != 0.0, 1.0 / np.where(d != 0.0, d, 1.0), 1.0)
    assert ref[ZERO_DIAG_ROW] == 1.0
    assert np.array_equal(got[:N_ROWS], ref)  # IEEE division: entry by entry the same bits
    assert (got[N_ROWS:] == -3.0).all()  # the lanes of the tail slice past n_rows write nothing


def test_zero_rows_keeps_the_pattern_and_places_the_diagonal(hip):
    from oasisx_amd import _lib

    A, Acsr = _row_system()
    before = A.vals.clone()
    rows = _dev(BC_ROWS)
    _lib.check(hip.ox_zero_rows(A.ref(), _lib.ptr(rows), len(BC_ROWS), 1.5, _lib.current_stream()), "ox_zero_rows")
    assert np.array_equal(A.to_scipy().toarray(), _zeroed(Acsr, BC_ROWS, 1.5))
    assert _padding_is_zero(A)
    # n == 0: nothing
    A.vals.copy_(before)
    assert hip.ox_zero_rows(A.ref(), _lib.ptr(rows), 0, 1.5, _lib.current_stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(A.vals, before)
    # the Jacobi diagonal of the result: 1 / diag on the listed rows
    A.zero_rows(rows, 4.0)
    dinv = torch.empty(N_ROWS, dtype=torch.float64, device="cuda")
    _lib.check(hip.ox_jacobi_setup(A.ref(), _lib.ptr(dinv), _lib.current_stream()), "ox_jacobi_setup")
    assert (dinv.cpu().numpy()[BC_ROWS] == 0.25).all()


@pytest.mark.parametrize("ncomp", [1, 2, 3])
def test_zero_rows_au_sets_the_identity_rows_of_the_product(hip, ncomp):
    from oasisx_amd import _lib

    A, Acsr = _row_system()
    rng = np.random.default_rng(ncomp)
    u1, au0 = rng.standard_normal((N_ROWS, ncomp)), rng.standard_normal((N_ROWS, ncomp))
    u1d, aud, rows = _dev(u1), _dev(au0), _dev(BC_ROWS)
    diag = 0.75  # (a power of two times 3: diag * u1 is one rounding on the device and in numpy alike)
    _lib.check(hip.ox_zero_rows_au(A.ref(), _lib.ptr(rows), len(BC_ROWS), diag, _lib.ptr(aud), _lib.ptr(u1d), ncomp,
                                   _lib.current_stream()), "ox_zero_rows_au")
    assert np.array_equal(A.to_scipy().toarray(), _zeroed(Acsr, BC_ROWS, diag))
    assert _padding_is_zero(A)
    ref = au0.copy()
    ref[BC_ROWS] = diag * u1[BC_ROWS]
    assert np.array_equal(aud.cpu().numpy(), ref)  # diag * u1 on the listed rows, untouched elsewhere
    assert np.array_equal(u1d.cpu().numpy(), u1)
    # au without u1, or a column count outside 1..3: rejected on the host
    assert hip.ox_zero_rows_au(A.ref(), _lib.ptr(rows), len(BC_ROWS), diag, _lib.ptr(aud), None, ncomp, _lib.current_stream()) != 0
    assert hip.ox_zero_rows_au(A.ref(), _lib.ptr(rows), len(BC_ROWS), diag, _lib.ptr(aud), _lib.ptr(u1d), 4, _lib.current_stream()) != 0
    torch.cuda.synchronize()
    assert np.array_equal(aud.cpu().numpy(), ref)


def test_zero_rows_cols_zeroes_rows_and_columns(hip):
    from oasisx_amd import _lib

    A, Acsr = _row_system()
    flag = np.zeros(N_ROWS, dtype=np.uint8)
    flag[BC_ROWS] = 1
    fd = _dev(flag)
    _lib.check(hip.ox_zero_rows_cols(A.ref(), _lib.ptr(fd), 1.0, _lib.current_stream()), "ox_zero_rows_cols")
    got = A.to_scipy().toarray()
    assert np.array_equal(got, _zeroed(Acsr, BC_ROWS, 1.0, cols=BC_ROWS))
    assert _padding_is_zero(A)
    # no row flagged: the matrix is left as it is
    A2, _ = _row_system()
    before = A2.vals.clone()
    fd.zero_()
    _lib.check(hip.ox_zero_rows_cols(A2.ref(), _lib.ptr(fd), 1.0, _lib.current_stream()), "ox_zero_rows_cols")
    assert torch.equal(A2.vals, before)
