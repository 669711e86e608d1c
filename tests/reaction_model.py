"""numpy model of the reacting-scalar kernels (oasisx_amd/reaction.py, csrc/ox_reaction.hip: ox_scalar_react,
ox_reaction_rates): the same formulas, the same pivot rule and the same order of operations, vectorised over the dofs, in
float64 or in ``numpy.longdouble`` (the project's extended model).  Per dof::

    k_j  = rate_j [exp(-Ta_j / c_T)]
    r_j  = ((k_j p_j0) p_j1) ...,    p_js = c_s^o_js by repeated multiplication (1, c, c c, (c c) c)
    f_s  = sum_j nu_sj r_j           (j ascending, from 0)
    J_st = sum_j nu_sj d_jt,  d_jt = k_j prod_s (s == t ? o_js c_s^(o_js - 1) : p_js)  [+ (r_j Ta_j) / (c_T c_T) at t = T]

ROS2 with g = 1 + 1/sqrt(2), h = H / substeps, W = I - (g h) J::

    W k1 = f(y);   W k2 = f(y + h k1) - 2 k1;   y <- (y + (1.5 h) k1) + (0.5 h) k2

W = P^T L U with partial pivoting (largest |.|, ties to the lower row), the pivots kept as reciprocals.  The device differs
from the float64 model by fused multiply-adds, its ``exp`` and, at near ties, the pivot row.

``whole_step`` composes the kinetics with the transport step of tests/scalar_model.py (Strang or Lie splitting).
"""
import numpy as np


class ReactionModel:
    """``nu``: (S, R); ``orders``: (R, S) integers 0..3; ``k``: per reaction a float or an (n,) array; ``arr``: per reaction
    the index of the Arrhenius temperature or -1; ``Ta``: per reaction."""

    def __init__(self, nu, orders, k, arr=None, Ta=None, dtype=np.float64):
        self.dt = dtype
        self.nu = np.asarray(nu, dtype=np.float64)
        self.S, self.R = self.nu.shape
        self.orders = np.asarray(orders, dtype=np.int64).reshape(self.R, self.S)
        assert ((self.orders >= 0) & (self.orders <= 3)).all()
        self.k = [np.asarray(v, dtype=np.float64).astype(dtype) for v in k]
        self.arr = [-1] * self.R if arr is None else [int(a) for a in arr]
        self.Ta = [0.0] * self.R if Ta is None else [float(t) for t in Ta]
        self.gamma = dtype(1) + dtype(1) / np.sqrt(dtype(2))

    @classmethod
    def from_network(cls, network, X=None, dtype=np.float64):
        """The model of an ``oasisx_amd.ReactionNetwork``; callable rates are evaluated at ``X: (3, n)``."""
        k = []
        for r in network.reactions:
            k.append(np.asarray(r.rate(X), dtype=np.float64) if callable(r.rate) else r.rate)
        a = network.arrhenius()
        return cls(network.stoichiometry(), network.orders(), k, [i for i, _ in a], [t for _, t in a], dtype)

    # ---- the rate function -----------------------------------------------------------------------------------------------
    def _power(self, o, c):
        one = np.ones_like(c)
        c2 = c * c
        p = (one, c, c2, c2 * c)[o]
        q = (np.zeros_like(c), one, self.dt(2) * c, self.dt(3) * c2)[o]
        return p, q

    def _rate(self, j, y):
        ka = self.k[j] * np.ones_like(y[0])
        cT = None
        if self.arr[j] >= 0:
            cT = y[self.arr[j]]
            with np.errstate(all="ignore"):
                ka = ka * np.exp(-self.dt(self.Ta[j]) / cT)
        r = ka
        p, q = [], []
        for s in range(self.S):
            ps, qs = self._power(int(self.orders[j, s]), y[s])
            p.append(ps)
            q.append(qs)
            r = r * ps
        return ka, r, p, q, cT

    def rates(self, y):
        """(R, n): r_j at the state y: (S, n)."""
        y = [np.asarray(v, dtype=self.dt) for v in y]
        with np.errstate(all="ignore"):
            return np.stack([self._rate(j, y)[1] for j in range(self.R)])

    def rhs(self, y, jac=True):
        S = self.S
        f = [np.zeros_like(y[0]) for _ in range(S)]
        J = [[np.zeros_like(y[0]) for _ in range(S)] for _ in range(S)] if jac else None
        for j in range(self.R):
            ka, r, p, q, cT = self._rate(j, y)
            nu = [self.dt(self.nu[s, j]) for s in range(S)]
            for s in range(S):
                f[s] = f[s] + nu[s] * r
            if jac:
                for t in range(S):
                    d = ka
                    for s in range(S):
                        d = d * (q[s] if s == t else p[s])
                    if self.arr[j] == t:
                        d = d + (r * self.dt(self.Ta[j])) / (cT * cT)
                    for s in range(S):
                        J[s][t] = J[s][t] + nu[s] * d
        return f, J

    # ---- LU with partial pivoting, rows exchanged through selects ----------------------------------------------------------
    def lu(self, W):
        S = self.S
        piv = []
        for c in range(S):
            pr = np.full(W[0][0].shape, c, dtype=np.int64)
            best = np.abs(W[c][c])
            for r in range(c + 1, S):
                v = np.abs(W[r][c])
                g = v > best
                pr = np.where(g, r, pr)
                best = np.where(g, v, best)
            piv.append(pr)
            for r in range(c + 1, S):
                sw = pr == r
                for t in range(S):
                    a, b = W[c][t], W[r][t]
                    W[c][t], W[r][t] = np.where(sw, b, a), np.where(sw, a, b)
            inv = self.dt(1) / W[c][c]
            W[c][c] = inv
            for r in range(c + 1, S):
                m = W[r][c] * inv
                W[r][c] = m
                for t in range(c + 1, S):
                    W[r][t] = W[r][t] - m * W[c][t]
        return piv

    def lu_solve(self, W, piv, x):
        S = self.S
        x = list(x)
        for c in range(S):
            for r in range(c + 1, S):
                sw = piv[c] == r
                a, b = x[c], x[r]
                x[c], x[r] = np.where(sw, b, a), np.where(sw, a, b)
            for r in range(c + 1, S):
                x[r] = x[r] - W[r][c] * x[c]
        for c in range(S - 1, -1, -1):
            acc = x[c]
            for t in range(c + 1, S):
                acc = acc - W[c][t] * x[t]
            x[c] = acc * W[c][c]
        return x

    # ---- ROS2 --------------------------------------------------------------------------------------------------------------
    def step(self, y, H, substeps=1, held=None):
        """``substeps`` steps over H from y: (S, n); ``held``: (S, n) bool, values written back as they were read."""
        dt = self.dt
        y0 = [np.asarray(v, dtype=dt).copy() for v in y]
        y = [v.copy() for v in y0]
        S = self.S
        h = dt(H) / dt(substeps)
        gh = self.gamma * h
        h15, h05 = dt(1.5) * h, dt(0.5) * h
        with np.errstate(all="ignore"):
            for _ in range(int(substeps)):
                k1, W = self.rhs(y, True)
                for s in range(S):
                    for t in range(S):
                        W[s][t] = dt(1.0 if s == t else 0.0) - gh * W[s][t]
                piv = self.lu(W)
                k1 = self.lu_solve(W, piv, k1)
                y1 = [y[s] + h * k1[s] for s in range(S)]
                f, _ = self.rhs(y1, False)
                k2 = self.lu_solve(W, piv, [f[s] - dt(2) * k1[s] for s in range(S)])
                y = [(y[s] + h15 * k1[s]) + h05 * k2[s] for s in range(S)]
        out = np.stack(y)
        if held is not None:
            out = np.where(held, np.stack(y0), out)
        return out


def distance(a, b):
    """Per species: max |a_s - b_s| relative to max |b_s| (at least the smallest normal number), in longdouble; NaN counts
    as equal to NaN at the same dof."""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    both = np.isnan(a) & np.isnan(b)
    d = np.where(both, 0, np.abs(a - b))
    scale = np.maximum(np.nanmax(np.abs(b), axis=1), np.finfo(np.float64).tiny)
    return np.asarray(d.max(axis=1) / scale, dtype=np.float64)


def yardstick(dev, m64, mld):
    """(device's distance, bound) per species: the bound is 8 x the float64 model's own distance from the longdouble model
    plus 64 eps."""
    return distance(dev, mld), 8.0 * distance(m64, mld) + 64.0 * np.finfo(np.float64).eps


def whole_step(rm, models, uab, dt, splitting="strang", substeps=1, held=None):
    """One step of the device's ``solve`` on the float64 models: ``models`` are the ``ScalarModel`` of the species, in the
    network's order (a scalar in no reaction is stepped by the caller)."""
    if splitting == "strang":
        y = rm.step(np.stack([m.c1 for m in models]), 0.5 * dt, substeps, held)
        for m, v in zip(models, y):
            m.c1 = np.asarray(v, dtype=np.float64).copy()
    for m in models:
        m.step(uab, dt)
    y = rm.step(np.stack([m.c for m in models]), 0.5 * dt if splitting == "strang" else dt, substeps, held)
    for m, v in zip(models, y):
        m.c = np.asarray(v, dtype=np.float64).copy()
        m.c1 = m.c.copy()
