"""k-step reference of the Jacobi-preconditioned Krylov solvers in extended precision (plain numpy / scipy: importable
without a GPU; the test systems it is run on are in tests/reduction_systems.py).

``jacobi_cg_steps`` / ``jacobi_bicgstab_steps`` run exactly k iterations of left-Jacobi-preconditioned CG / BiCGStab in
PETSc's conventions -- the algorithm of ``oracle.ipcs_oracle.jacobi_cg`` / ``jacobi_bicgstab`` -- in ``np.longdouble``
(x87 extended: eps 1.1e-19) and return the k-th iterate, |D^-1 b| and |D^-1 (b - A x_k)|.  In exact arithmetic every
device variant (standard, single-reduction, merged, folded and folded merged CG; BiCGStab and merged BiCGStab) produces
these iterates, so one reference serves all of them; run in float64 (``dtype=np.float64``) the same code is the
"does the system itself allow 1e-13" precondition of the device tests.

Where ``np.longdouble`` is no wider than float64 the dot products are summed exactly instead (``math.fsum`` over
error-free products); ``DOT_EPS`` says which precision the sums have.
"""
from __future__ import annotations

import math

import numpy as np

EXTENDED = bool(np.finfo(np.longdouble).eps < 1e-18)
# relative precision of the model's dot products: the extended format's, or float64's last rounding of an exact sum
DOT_EPS = float(np.finfo(np.longdouble).eps) if EXTENDED else float(np.finfo(np.float64).eps)
assert EXTENDED or DOT_EPS < 3e-16


def two_product(x, y):
    """Error-free product of float64 arrays: x * y = p + e exactly (Veltkamp / Dekker; |x|, |y| far from overflow)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    p = x * y
    c = 134217729.0  # 2^27 + 1
    xh = c * x
    xh = xh - (xh - x)
    xl = x - xh
    yh = c * y
    yh = yh - (yh - y)
    yl = y - yh
    e = ((xh * yh - p) + xh * yl + xl * yh) + xl * yl
    return p, e


def exact_dot(x, y) -> float:
    """sum x_i y_i of float64 arrays, rounded once (``math.fsum`` over the error-free products)."""
    p, e = two_product(np.ravel(x), np.ravel(y))
    e = e[e != 0.0]
    return math.fsum(p) if e.size == 0 else math.fsum(np.concatenate([p, e]))


def _dot(x, y, dtype):
    if dtype == np.longdouble and not EXTENDED:
        return np.longdouble(exact_dot(x, y))
    return np.dot(x, y)


def _prep(A, b, x0, dtype):
    Aw = A.tocsr().astype(dtype)
    d = Aw.diagonal()
    dinv = np.where(d != 0, dtype(1) / np.where(d != 0, d, dtype(1)), dtype(1))  # (a stored zero diagonal: 1, as the device)
    bw = np.asarray(b).astype(dtype)
    xw = np.zeros(bw.shape[0], dtype=dtype) if x0 is None else np.asarray(x0).astype(dtype)
    return Aw, dinv, bw, xw


def jacobi_cg_trace(A, b, x0, kmax, dtype=np.longdouble):
    """[(x_k, |D^-1 b|, |D^-1 (b - A x_k)|) for k = 0..kmax] of Jacobi-CG (the true residual, not the recurrence's)."""
    Aw, dinv, b, x = _prep(A, b, x0, dtype)
    sq = lambda v: np.sqrt(_dot(v, v, dtype))
    bn = sq(dinv * b)
    r = b - Aw @ x if x0 is not None else b.copy()
    z = dinv * r
    out = [(x.copy(), bn, sq(dinv * (b - Aw @ x)))]
    p = z.copy()
    rz = _dot(r, z, dtype)
    for _ in range(kmax):
        q = Aw @ p
        alpha = rz / _dot(p, q, dtype)
        x = x + alpha * p
        r = r - alpha * q
        z = dinv * r
        rz_new = _dot(r, z, dtype)
        p = z + (rz_new / rz) * p
        rz = rz_new
        out.append((x.copy(), bn, sq(dinv * (b - Aw @ x))))
    return out


def jacobi_bicgstab_trace(A, b, x0, kmax, dtype=np.longdouble):
    """[(x_k, |D^-1 b|, |D^-1 (b - A x_k)|, recurrence norm) for k = 0..kmax] of left-Jacobi-preconditioned BiCGStab.
    The fourth entry is sqrt(s.s - 2 omega t.s + omega^2 t.t), the norm the merged-reduction form tests: equal to the
    third in exact arithmetic."""
    Aw, dinv, b, x = _prep(A, b, x0, dtype)
    sq = lambda v: np.sqrt(_dot(v, v, dtype))
    bn = sq(dinv * b)
    r = dinv * (b - Aw @ x) if x0 is not None else dinv * b
    true = lambda: sq(dinv * (b - Aw @ x))
    out = [(x.copy(), bn, true(), sq(r))]
    rhat = r.copy()
    rho = alpha = omega = dtype(1)
    v = np.zeros_like(r)
    p = np.zeros_like(r)
    for _ in range(kmax):
        rho_new = _dot(rhat, r, dtype)
        beta = (rho_new / rho) * (alpha / omega)
        rho = rho_new
        p = r + beta * (p - omega * v)
        v = dinv * (Aw @ p)
        alpha = rho / _dot(rhat, v, dtype)
        s = r - alpha * v
        t = dinv * (Aw @ s)
        tt, ts, ss = _dot(t, t, dtype), _dot(t, s, dtype), _dot(s, s, dtype)
        omega = ts / tt
        x = x + alpha * p + omega * s
        r = s - omega * t
        rec = np.sqrt(max(ss - 2 * omega * ts + omega * omega * tt, dtype(0)))
        out.append((x.copy(), bn, true(), rec))
    return out


def jacobi_cg_steps(A, b, x0, k, dtype=np.longdouble):
    """(x_k, |D^-1 b|, |D^-1 (b - A x_k)|) after exactly k iterations of Jacobi-CG from x0 (None: zero)."""
    return jacobi_cg_trace(A, b, x0, k, dtype)[k]


def jacobi_bicgstab_steps(A, b, x0, k, dtype=np.longdouble):
    """(x_k, |D^-1 b|, |D^-1 (b - A x_k)|) after exactly k iterations of left-Jacobi-preconditioned BiCGStab."""
    return jacobi_bicgstab_trace(A, b, x0, k, dtype)[k][:3]
