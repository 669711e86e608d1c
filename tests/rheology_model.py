"""numpy model of the generalised-Newtonian laws and of the full stress form of FractionalStep_AB_CN
(oasisx_amd/viscosity.py, csrc/ox_viscosity.hip and k_stress_transpose of csrc/ox_assemble.hip), on top of
tests/viscosity_model.py and the oracle's forms (no GPU).

    gd_c        = sqrt(2 S:S), S = sym(grad u_ab) at the centroid of cell c
    nut_c       = max(nu(gd_c) - base, 0)             Carreau-Yasuda, Cross, power law
    T[r][i]     = sum_c nut_c int_c sum_j d(u_ab)_j/dx_i d(phi_r)/dx_j           stress_form="full":  b_first -= T

A law is a tuple: ``("carreau_yasuda", (nu0, nu_inf, lam, n, a))``, ``("cross", (nu0, nu_inf, lam, m))`` or
``("power_law", (k, n, nu_min, nu_max))``; every other model tuple is that of tests/viscosity_model.py.  The laws are
written in the kernel's expression order, with ``np.power``.
"""
import numpy as np

from oracle import ipcs_oracle as O
from tests import viscosity_model as VM

LAWS = ("carreau_yasuda", "cross", "power_law")


def shear_rate(F, uab):
    """gd = sqrt(2 S:S) per cell, from the centroid gradient of tests/viscosity_model.py."""
    g = VM.centroid_gradient(F, uab)
    S = 0.5 * (g + np.swapaxes(g, 1, 2))
    return np.sqrt(2.0 * np.einsum("cdk,cdk->c", S, S))


def base_viscosity(model):
    kind, par = model
    if kind == "power_law":
        return float(par[2])
    return min(float(par[0]), float(par[1]))


def law_viscosity(model, gd):
    """nu(gd) of a law, elementwise."""
    kind, par = model
    gd = np.asarray(gd, dtype=np.float64)
    if kind == "carreau_yasuda":
        nu0, nu_inf, lam, n, a = (float(v) for v in par)
        return nu_inf + (nu0 - nu_inf) * np.power(1.0 + np.power(lam * gd, a), (n - 1.0) / a)
    if kind == "cross":
        nu0, nu_inf, lam, m = (float(v) for v in par)
        return nu_inf + (nu0 - nu_inf) / (1.0 + np.power(lam * gd, m))
    if kind != "power_law":
        raise ValueError(kind)
    k, n, nu_min, nu_max = (float(v) for v in par)
    at_rest = nu_max if n < 1.0 else (nu_min if n > 1.0 else k)
    nu = np.full(gd.shape, at_rest)
    pos = gd > 0.0
    with np.errstate(over="ignore"):
        nu[pos] = k * np.power(gd[pos], n - 1.0)
    return np.minimum(np.maximum(nu, nu_min), nu_max)


def nut_cells(F, uab, model):
    """nut per cell: the laws here, every other model from tests/viscosity_model.py."""
    if model[0] not in LAWS:
        return VM.nut_cells(F, uab, model)
    return np.maximum(law_viscosity(model, shear_rate(F, uab)) - base_viscosity(model), 0.0)


def transposed_term(F, uab, nut):
    """T[r, i] = sum_c nut_c |J_c| sum_q w_q sum_j d(u_ab)_j/dx_i (x_q) d(phi_r)/dx_j (x_q), an (nv, d) array."""
    gu = np.einsum("cmj,cqmi->cqji", uab[F.vd], F.grad_v, optimize=True)  # d(u_ab)_j / dx_i at the points
    Te = np.einsum("q,cqji,cqrj->cri", F.w, gu, F.grad_v, optimize=True)
    Te *= (F.adet * np.asarray(nut, dtype=np.float64))[:, None, None]
    out = np.zeros((F.nv, F.d))
    for i in range(F.d):
        np.add.at(out[:, i], F.vd.ravel(), Te[:, :, i].ravel())
    return out


class _FormsWithLaw:
    """The oracle's forms with ``convection`` returning C + K_w(nut(u_ab)), ``nut`` from :func:`nut_cells` of this file."""

    def __init__(self, forms, owner):
        self._F, self._owner = forms, owner

    def __getattr__(self, name):
        return getattr(self._F, name)

    def convection(self, uab):
        nut = nut_cells(self._F, uab, self._owner.model)
        self._owner.nut = nut
        return self._F.convection(uab) + VM.weighted_stiffness(self._F, nut)


class RheologyOracleStep(VM.ViscosityOracleStep):
    """``ViscosityOracleStep`` that knows the laws and subtracts ``T`` from ``b_first`` when ``stress_form == "full"``."""

    def __init__(self, *args, stress_form="laplacian", **kw):
        super().__init__(*args, **kw)
        if stress_form not in ("laplacian", "full"):
            raise ValueError(stress_form)
        self.stress_form = stress_form
        self.T = None

    def assemble_first(self, dt, nu):
        if self.model is None:
            return O.OracleFractionalStep.assemble_first(self, dt, nu)
        plain = self.F
        self.F = _FormsWithLaw(plain, self)
        try:
            O.OracleFractionalStep.assemble_first(self, dt, nu)
        finally:
            self.F = plain
        if self.stress_form == "full":
            self.T = transposed_term(plain, self.uab, self.nut)
            self.b_first -= self.T


def tg_step_model(F, x_v, x_q, model, stress_form="laplacian", nu=0.01, dt=0.005, t0=0.0, solver_options=None,
                  low_memory=True):
    """``tests.viscosity_model.tg_step_model`` around a :class:`RheologyOracleStep`."""
    d = F.d
    clock = {"t": t0}
    fns = [O.tg_u, O.tg_v, O.tg_w][:d]
    bd = O.boundary_dofs(x_v, F.coords.min(axis=0), F.coords.max(axis=0))
    bcs_u = [[O.DirichletData(bd, (lambda x, f=f: f(x, clock["t"], nu)))] for f in fns]
    S = RheologyOracleStep(F, x_v, x_q, bcs_u, solver_options=solver_options, low_memory=low_memory, model=model,
                           stress_form=stress_form)
    X = np.zeros((3, x_v.shape[0]))
    X[:d] = x_v.T
    Xq = np.zeros((3, x_q.shape[0]))
    Xq[:d] = x_q.T
    for i, f in enumerate(fns):
        S.u2[:, i] = f(X, t0 - dt, nu)
        S.u1[:, i] = f(X, t0, nu)
    S.p[:] = O.tg_p(Xq, t0 - dt / 2.0, nu)
    return S, clock


def rigid_rotation(x):
    """u = omega x x on (n, d) points: (-y, x) in 2-D, omega = (0.3, -0.5, 0.8) in 3-D."""
    if x.shape[1] == 2:
        return np.stack([-x[:, 1], x[:, 0]], axis=1)
    return np.cross(np.array([0.3, -0.5, 0.8])[None], x)
