"""numpy model of the eddy-viscosity step of FractionalStep_AB_CN (oasisx_amd/viscosity.py, csrc/ox_viscosity.hip and
the NUT form of csrc/ox_assemble.hip), built on the oracle's forms (no GPU).

    nut_c       from grad u_ab at the centroid of cell c  (Smagorinsky, WALE) or fixed per cell
    K_w(nut)  = sum_c nut_c K_c          the per-cell ``Ae`` of ``Forms.stiffness_v`` scaled before ``_csr``
    A         = M/dt + (C + K_w)/2 + nu K/2,   b = (M/dt - (C + K_w)/2 - nu K/2) u_1 + b0

A model is a tuple: ``("smagorinsky", Cs)``, ``("wale", Cw)`` or ``("cell", values)`` with one value per cell in the
cell order of the ``Forms`` object.  The powers of WALE are written as products and square roots, as the kernel does.
"""
import math

import numpy as np

from oracle import ipcs_oracle as O


def centroid_gradient(F, uab):
    """g[c, d, k] = d(u_ab)_d / dx_k at the centroid of every cell: the barycentric derivatives of the velocity basis at
    the centroid, contracted with the cell's dofs first and with grad lambda second (the kernel's order)."""
    d = F.d
    bary = np.full((1, d + 1), 1.0 / (d + 1))
    _, dphi = O.tabulate(d, F.u_deg, bary)  # (1, nd, d + 1)
    t = np.einsum("cid,ib->cdb", uab[F.vd], dphi[0])
    return np.einsum("cdb,cbk->cdk", t, F.G)


def delta2(F):
    """Delta_c^2 = |cell|^(2/gdim), |cell| = |det J| / gdim!."""
    if F.d == 2:
        return 0.5 * F.adet
    h = np.cbrt(F.adet * (1.0 / 6.0))
    return h * h


def nut_cells(F, uab, model):
    kind, par = model
    if kind == "cell":
        v = np.asarray(par, dtype=np.float64)
        return np.full(F.cells.shape[0], float(v)) if v.ndim == 0 else v.copy()
    g = centroid_gradient(F, uab)
    S = 0.5 * (g + np.swapaxes(g, 1, 2))
    ss = np.einsum("cdk,cdk->c", S, S)
    c2 = float(par) ** 2
    if kind == "smagorinsky":
        return c2 * delta2(F) * np.sqrt(2.0 * ss)
    if kind != "wale":
        raise ValueError(kind)
    if F.d != 3:
        raise ValueError("WALE is defined in three dimensions")
    g2 = np.einsum("cdm,cmk->cdk", g, g)
    tr3 = np.einsum("cdd->c", g2) * (1.0 / 3.0)
    Sd = 0.5 * (g2 + np.swapaxes(g2, 1, 2)) - tr3[:, None, None] * np.eye(3)[None]
    x = np.einsum("cdk,cdk->c", Sd, Sd)
    num = x * np.sqrt(x)
    den = ss * ss * np.sqrt(ss) + x * np.sqrt(np.sqrt(x))
    out = np.zeros_like(x)
    ok = den > 0.0
    out[ok] = c2 * delta2(F)[ok] * (num[ok] / den[ok])
    return out


def weighted_stiffness(F, w):
    """K_w = sum_c w_c K_c on the velocity component space."""
    Ae = np.einsum("q,cqik,cqjk->cij", F.w, F.grad_v, F.grad_v, optimize=True)
    Ae *= (F.adet * np.asarray(w, dtype=np.float64))[:, None, None]
    return F._csr(Ae, F.vd, F.vd, (F.nv, F.nv))


class _FormsWithNut:
    """The oracle's forms with ``convection`` returning C + K_w(nut(u_ab)): what the fused kernel accumulates as "C"."""

    def __init__(self, forms, owner):
        self._F, self._owner = forms, owner

    def __getattr__(self, name):
        return getattr(self._F, name)

    def convection(self, uab):
        nut = nut_cells(self._F, uab, self._owner.model)
        self._owner.nut = nut
        return self._F.convection(uab) + weighted_stiffness(self._F, nut)


class ViscosityOracleStep(O.OracleFractionalStep):
    """``OracleFractionalStep`` whose ``assemble_first`` uses C + K_w(nut) where the oracle uses C."""

    def __init__(self, *args, model=None, **kw):
        super().__init__(*args, **kw)
        self.model = model
        self.nut = None

    def assemble_first(self, dt, nu):
        if self.model is None:
            return super().assemble_first(dt, nu)
        plain = self.F
        self.F = _FormsWithNut(plain, self)
        try:
            super().assemble_first(dt, nu)
        finally:
            self.F = plain

    def kinetic_energy(self):
        """(1/2) sum_d u_d^T M u_d of the last completed step."""
        return 0.5 * float(sum(self.u1[:, i] @ (self.M @ self.u1[:, i]) for i in range(self.d)))


def tg_step_model(F, x_v, x_q, model, nu=0.01, dt=0.005, t0=0.0, solver_options=None, low_memory=True):
    """The Taylor-Green set-up of ``oracle.ipcs_oracle.taylor_green_problem`` around a ``ViscosityOracleStep``: exact
    Dirichlet velocity on the boundary of the box, no pressure condition, u2(t0 - dt), u1(t0), p(t0 - dt/2)."""
    d = F.d
    clock = {"t": t0}
    fns = [O.tg_u, O.tg_v, O.tg_w][:d]
    bd = O.boundary_dofs(x_v, F.coords.min(axis=0), F.coords.max(axis=0))
    bcs_u = [[O.DirichletData(bd, (lambda x, f=f: f(x, clock["t"], nu)))] for f in fns]
    S = ViscosityOracleStep(F, x_v, x_q, bcs_u, solver_options=solver_options, low_memory=low_memory, model=model)
    X = np.zeros((3, x_v.shape[0]))
    X[:d] = x_v.T
    Xq = np.zeros((3, x_q.shape[0]))
    Xq[:d] = x_q.T
    for i, f in enumerate(fns):
        S.u2[:, i] = f(X, t0 - dt, nu)
        S.u1[:, i] = f(X, t0, nu)
    S.p[:] = O.tg_p(Xq, t0 - dt / 2.0, nu)
    return S, clock


def tg_forms(dim, N, deg, p_deg=1):
    """The oracle's own Taylor-Green mesh and numbering on [-1, 1]^dim."""
    if dim == 2:
        coords, cells = O.create_rectangle_mesh([-1, -1], [1, 1], [N, N])
    else:
        coords, cells = O.create_box_mesh([-1, -1, -1], [1, 1, 1], [N, N, N])
    return O.Forms(coords, cells, deg, p_deg)


# the dissipation check, asserted in this model (CPU) and on the device (GPU) on the same mesh
DISSIPATION = dict(dim=3, N=3, deg=2, steps=5, nu=0.01, dt=0.005, Cs=0.1677)


def run_energy(F, x_v, x_q, model, steps, nu=0.01, dt=0.005, solver_options=None):
    """Kinetic energy after ``steps`` Taylor-Green steps of the model."""
    S, clock = tg_step_model(F, x_v, x_q, model, nu=nu, dt=dt, solver_options=solver_options)
    for k in range(steps):
        clock["t"] = (k + 1) * dt
        S.solve(dt, nu, max_iter=1)
    return S.kinetic_energy(), S


def smagorinsky_closed_form(F, A, Cs):
    """nut per cell for u = A x: (Cs Delta)^2 sqrt(2 S:S) with S = sym(A)."""
    S = 0.5 * (A + A.T)
    return Cs ** 2 * delta2(F) * math.sqrt(2.0 * float(np.sum(S * S)))
