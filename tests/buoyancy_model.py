"""numpy model of scalars that drive the flow (Boussinesq forces) and of the scalar flux through exterior facets
(oasisx_amd/scalar.py, csrc/ox_scalar.hip: ox_buoyancy_rows, ox_scalar_flux), built on the oracle's fractional step and
forms and on tests/scalar_model.ScalarModel (no GPU).  Per step, with c_1, c_2 of every coupled scalar at its start:

    d      = (c_1 + 0.5 (c_1 - c_2)) - reference            (c_1 - reference without extrapolation)
    b0_i   = b0_i(body force) + sum_scalars b_i M d         the oracle's b_first = (M/dt - C/2 - nu K/2) u_1 + b0
    the oracle's velocity / pressure step;  every scalar's step with the u_ab of this step;  c_2 <- c_1, c_1 <- c

Facet flux: q_f = -kappa n . mean_f(grad c), the facet mean by a 3-point Gauss rule on an edge and the triangle rule of
Forms.pressure_surface_vec on a face (exact: grad c has degree <= 2).
"""
import math

import numpy as np
import scipy.sparse.linalg as spla

from oracle import ipcs_oracle as O
from tests.scalar_model import ScalarModel


def midpoint_deviation(c1, c2, reference, extrapolate=True):
    """d of the module docstring, in the device's order of operations."""
    return ((c1 + 0.5 * (c1 - c2)) if extrapolate else c1) - reference


def buoyancy_rows(M, b, terms):
    """b + sum_t coef_t (M d_t): ``terms`` is a list of (c1, c2 or None, reference, coef (gdim,))."""
    out = np.array(b, dtype=np.float64, copy=True)
    for c1, c2, ref, coef in terms:
        y = M @ midpoint_deviation(c1, c1 if c2 is None else c2, ref, c2 is not None)
        out += np.outer(y, np.asarray(coef, dtype=np.float64))
    return out


class CoupledScalar:
    """A ScalarModel with its Boussinesq coefficients, reference and second time level."""

    def __init__(self, model: ScalarModel, buoyancy=None, reference=0.0, extrapolate=True):
        self.m = model
        self.buoyancy = None if buoyancy is None else np.asarray(buoyancy, dtype=np.float64)
        self.reference, self.extrapolate = float(reference), bool(extrapolate)
        self.c2 = model.c1.copy()

    def interpolate(self, f):
        self.m.interpolate(f)
        self.c2 = self.m.c1.copy()

    def solve(self, uab, dt, direct=False):
        """One scalar step; c_2 <- c_1 before c_1 <- c."""
        m = self.m
        if direct:
            A, b = m.assemble(uab, dt)
            m.c = spla.splu(A.tocsc()).solve(b)
            m.reason, m.its = O.CONVERGED_ITS, 1
            c1_new = m.c.copy()
            self.c2 = m.c1.copy()
            m.c1 = c1_new
        else:
            old = m.c1.copy()
            m.step(uab, dt)
            self.c2 = old
        return m.c


class CoupledStep:
    """OracleFractionalStep with scalars that force it."""

    def __init__(self, step: O.OracleFractionalStep, scalars, direct_scalars=False):
        self.S, self.scalars, self.direct = step, list(scalars), direct_scalars
        self.b0_body = step.b0.copy()

    def force(self):
        """sum_scalars b_i M d, (nv, d)."""
        terms = [(s.m.c1, s.c2 if s.extrapolate else None, s.reference, s.buoyancy) for s in self.scalars
                 if s.buoyancy is not None]
        return buoyancy_rows(self.S.M, np.zeros_like(self.b0_body), terms)

    def solve(self, dt, nu, max_iter=1):
        S = self.S
        S.b0 = self.b0_body + self.force()
        S.solve(dt, nu, max_iter=max_iter)
        for s in self.scalars:
            s.solve(S.uab, dt, self.direct)


# ---- facet flux ----------------------------------------------------------------------------------------------------------
def _facet_rule(d):
    if d == 2:
        from numpy.polynomial.legendre import leggauss

        s, w = leggauss(3)
        return np.stack([(1 - s) / 2, (1 + s) / 2], axis=1), w / 2
    bf, wf = O.simplex_quadrature(2, 3)
    return bf, wf * math.factorial(2)  # the weights of a mean: they sum to 1


def facet_flux(F: O.Forms, fc, fa, c, kappa):
    """(q, |f|, cbar, n) per facet (cell fc, opposite local vertex fa): q = -kappa n . mean_f(grad c), cbar = mean_f(c)."""
    d = F.d
    bf, wf = _facet_rule(d)
    assert abs(wf.sum() - 1.0) < 1e-14
    nf = len(fc)
    q, area, cbar, normals = np.zeros(nf), np.zeros(nf), np.zeros(nf), np.zeros((nf, d))
    for f in range(nf):
        cell, a = int(fc[f]), int(fa[f])
        others = [b for b in range(d + 1) if b != a]
        bary = np.zeros((bf.shape[0], d + 1))
        bary[:, others] = bf
        phi, dphi = O.tabulate(d, F.u_deg, bary)
        G = F.G[cell]
        gnorm = np.linalg.norm(G[a])
        n = -G[a] / gnorm
        cc = c[F.vd[cell]]
        grad = np.einsum("q,qib,bk,i->k", wf, dphi, G, cc)
        q[f] = -kappa * float(n @ grad)
        area[f] = F.adet[cell] * gnorm / math.factorial(d - 1)
        cbar[f] = float(wf @ (phi @ cc))
        normals[f] = n
    return q, area, cbar, normals


# ---- the de Vahl Davis differentially heated square ----------------------------------------------------------------------
BENCHMARK = {"Ra": 1e3, "Nu": 1.118, "umax": 3.649, "vmax": 3.697}  # de Vahl Davis (1983), Ra = 1e3, Pr = 0.71


def cavity_walls(x, tol=1e-10):
    """Boolean masks of the points x (n, 2) on the hot (x = 0), cold (x = 1) and adiabatic (y = 0, 1) walls."""
    hot, cold = np.abs(x[:, 0]) < tol, np.abs(x[:, 0] - 1.0) < tol
    return hot, cold, (np.abs(x[:, 1]) < tol) | (np.abs(x[:, 1] - 1.0) < tol)


class HeatedCavity:
    """T = 1 at x = 0, T = 0 at x = 1, adiabatic top and bottom, no-slip walls on the unit square, in diffusion units:
    nu = Pr, kappa = 1, buoyancy (0, Ra Pr), reference 0.5; the run starts from rest and the conduction profile 1 - x.
    ``forms`` / ``x_v`` / ``x_q``: the device's numbering (default: the oracle's own on an N x N mesh)."""

    def __init__(self, N=8, Ra=1e3, Pr=0.71, solver_options=None, scalar_options=None, forms=None, x_v=None, x_q=None,
                 extrapolate=True):
        if forms is None:
            coords, cells = O.create_rectangle_mesh([0.0, 0.0], [1.0, 1.0], [N, N])
            forms = O.Forms(coords, cells, 2, 1)
            x_v, x_q = forms.x_v, forms.x_q
        self.F, self.x_v, self.Pr, self.Ra = forms, x_v, float(Pr), float(Ra)
        hot, cold, adiabatic = cavity_walls(x_v)
        wall = np.nonzero(hot | cold | adiabatic)[0]
        bcs_u = [[O.DirichletData(wall, 0.0)] for _ in range(2)]
        step = O.OracleFractionalStep(forms, x_v, x_q, bcs_u, solver_options=solver_options)
        self.direct = scalar_options is None
        T = ScalarModel(forms, x_v, 1.0, dofs=np.nonzero(hot | cold)[0], value=lambda x: 1.0 - x[0],
                        options=scalar_options, M=step.M, K=step.K)
        self.T = CoupledScalar(T, buoyancy=(0.0, self.Ra * self.Pr), reference=0.5, extrapolate=extrapolate)
        self.T.interpolate(lambda x: 1.0 - x[0])
        self.step = CoupledStep(step, [self.T], direct_scalars=self.direct)
        fc, fa = forms.exterior_facets()
        mid = forms.facet_midpoints(fc, fa)
        self.fc, self.fa = fc, fa
        self.hot, self.cold, self.adiabatic = cavity_walls(mid)

    def solve(self, dt):
        self.step.solve(dt, self.Pr, max_iter=1)

    def domain_nusselt(self):
        """The domain mean of u T - dT/dx: u_x . M T + 1."""
        S = self.step.S
        return float(S.u1[:, 0] @ (S.M @ self.T.m.c)) + 1.0

    def wall_totals(self):
        """sum |f| q over the hot, the cold and the adiabatic facets (positive: out of the domain)."""
        q, area, _, _ = facet_flux(self.F, self.fc, self.fa, self.T.m.c, 1.0)
        fq = area * q
        return float(fq[self.hot].sum()), float(fq[self.cold].sum()), float(fq[self.adiabatic].sum())

    def extrema(self):
        u = self.step.S.u1
        return float(np.abs(u[:, 0]).max()), float(np.abs(u[:, 1]).max())
