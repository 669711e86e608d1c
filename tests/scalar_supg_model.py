"""numpy model of a scalar with SUPG stabilisation (oasisx_amd/scalar.py with ``stabilization=SUPG(...)``, ``ox_supg_cells``
of csrc/ox_scalar.hip and ``ox_scalar_rows_supg`` of csrc/ox_assemble.hip), built on
tests/scalar_model.ScalarModel, the oracle's forms and tests/viscosity_model.weighted_stiffness / nut_cells (no GPU).

Per cell c, with k the element degree and G[a] = grad lambda_a:

    w_c = u_ab at the centroid,   q_c = sum_a |w_c . G[a]|,   g_c = sum_a |G[a]|^2,   kappa_c = kappa + nut_c / Sc_t
    tau_c = scale ([time_term] (2/dt)^2 + (k q_c)^2 + (2 k^2 kappa_c g_c)^2)^(-1/2)
    N_ij = sum_c tau_c int_c (w_c . grad phi_i) phi_j,   S_ij = sum_c tau_c int_c (w_c . grad phi_i)(w_c . grad phi_j)
    A_c = M/dt + C(u_ab)/2 + kappa K/2 + K_w(nut)/(2 Sc_t) + N/dt + S/2
    b_c = (2/dt) M c_1 - A_c c_1 + b0_c + N ((2/dt) c_1 + f_h)            f_h: the source at the dofs
    the scalar's own Dirichlet rows -> identity in A_c, boundary value in b_c, as in ``ScalarModel.assemble``.

N and S are formed cell by cell on the quadrature rule of the ``Forms`` object (degree 7 for P1 / P2, 9 for P3; the
integrands have degree 2k - 1 and 2k - 2).  ``model``: a tuple of tests/viscosity_model.py, or ``None`` with ``nut`` handed
to ``assemble`` / ``step`` (the device's own array, kernel cell order), or no ``nut`` at all (no viscosity model).
"""
import numpy as np

from oracle import ipcs_oracle as O
from tests.scalar_model import ScalarModel
from tests.viscosity_model import nut_cells, weighted_stiffness


def centroid_velocity(F, uab):
    """w[c, d]: u_ab at the centroid of every cell."""
    bary = np.full((1, F.d + 1), 1.0 / (F.d + 1))
    phi, _ = O.tabulate(F.d, F.u_deg, bary)  # (1, nd)
    return np.einsum("cid,i->cd", uab[F.vd], phi[0])


def tau_cells(w, G, kappa_c, dt, degree, scale=1.0, time_term=True):
    """Shakib's parameter from w: (nc, d), G: (nc, d + 1, d) and kappa_c (a float or (nc,)); any d >= 1.  Where every term
    under the root is zero tau is 0."""
    k = float(degree)
    q = np.abs(np.einsum("cd,cad->ca", w, G)).sum(axis=1)
    g = np.einsum("cad,cad->c", G, G)
    r = (k * q) ** 2 + (2.0 * k * k * np.asarray(kappa_c, dtype=np.float64) * g) ** 2
    if time_term:
        r = r + (2.0 / dt) ** 2
    out = np.zeros_like(r)
    ok = r > 0.0
    out[ok] = scale / np.sqrt(r[ok])
    out[~np.isfinite(r)] = np.nan
    return out


def supg_element_matrices(F, w, tau):
    """(Ne, Se): (nc, nd, nd) each, tau_c int_c (w_c . grad phi_i) phi_j and tau_c int_c (w_c . grad phi_i)(w_c . grad phi_j)."""
    wg = np.einsum("cd,cqid->cqi", w, F.grad_v, optimize=True)
    Ne = np.einsum("q,cqi,qj->cij", F.w, wg, F.phi_v, optimize=True)
    Se = np.einsum("q,cqi,cqj->cij", F.w, wg, wg, optimize=True)
    s = (F.adet * tau)[:, None, None]
    return s * Ne, s * Se


def supg_matrices(F, w, tau):
    """(N, S) assembled on the velocity component space."""
    Ne, Se = supg_element_matrices(F, w, tau)
    shape = (F.nv, F.nv)
    return F._csr(Ne, F.vd, F.vd, shape), F._csr(Se, F.vd, F.vd, shape)


class _FormsWithSupg:
    """The oracle's forms with ``convection`` returning C + extra: with extra = K_w/Sc_t + 2 N/dt + S,
    ``ScalarModel.assemble`` forms M/dt + C/2 + kappa K/2 + K_w/(2 Sc_t) + N/dt + S/2."""

    def __init__(self, forms, extra):
        self._F, self._extra = forms, extra

    def __getattr__(self, name):
        return getattr(self._F, name)

    def convection(self, uab):
        return self._F.convection(uab) + self._extra


class ScalarSupgModel(ScalarModel):
    """``turbulent_schmidt``: ``None`` (no viscosity model) or Sc_t > 0 (``inf``: none of nut reaches the scalar).
    ``source`` (a float or a callable) is also interpolated at the dofs: f_h.  ``galerkin_source_only=True`` leaves
    N f_h out of b_c -- a streamline-diffusion-like scheme that is NOT consistent (tests/test_scalar_supg_host.py)."""

    def __init__(self, forms, x_v, kappa, scale=1.0, time_term=True, turbulent_schmidt=None, model=None, source=0.0,
                 stabilize=True, galerkin_source_only=False, **kw):
        super().__init__(forms, x_v, kappa, source=source, **kw)
        self.scale, self.time_term, self.stabilize = float(scale), bool(time_term), bool(stabilize)
        self.sct = None if turbulent_schmidt is None else float(turbulent_schmidt)
        self.model = model
        self.galerkin_source_only = galerkin_source_only
        X = np.zeros((3, x_v.shape[0]))
        X[: x_v.shape[1]] = x_v.T
        self.fh = np.broadcast_to(np.asarray(source(X) if callable(source) else float(source), dtype=np.float64),
                                  (forms.nv,)).copy()
        self.nut = self.Kw = self.w = self.tau = self.N = self.S = None

    def assemble(self, uab, dt, nut=None):
        plain, b0 = self.F, self.b0
        extra = 0.0 * self.M
        kappa_c = self.kappa
        self.nut = None
        if self.sct is not None:
            self.nut = nut_cells(plain, uab, self.model) if nut is None else np.asarray(nut, dtype=np.float64)
            self.Kw = weighted_stiffness(plain, self.nut)
            extra = extra + (1.0 / self.sct) * self.Kw
            kappa_c = self.kappa + self.nut / self.sct
        if self.stabilize:
            self.w = centroid_velocity(plain, uab)
            self.tau = tau_cells(self.w, plain.G, kappa_c, dt, plain.u_deg, self.scale, self.time_term)
            self.N, self.S = supg_matrices(plain, self.w, self.tau)
            extra = extra + (2.0 / dt) * self.N + self.S
            rhs = (2.0 / dt) * self.c1 + (0.0 if self.galerkin_source_only else self.fh)
            self.b0 = b0 + self.N @ rhs
        self.F = _FormsWithSupg(plain, extra)
        try:
            return super().assemble(uab, dt)
        finally:
            self.F, self.b0 = plain, b0

    def step(self, uab, dt, nut=None):
        self.assemble(uab, dt, nut)
        x0 = self.c1.copy() if self.guess else None
        self.c, self.reason, self.its, _ = O.jacobi_bicgstab(self.A, self.b, x0, self.rtol, self.atol, self.max_it)
        self.c1 = self.c.copy()
        return self.c


# ---- the skew step of demo/supg_front_hip.py and of the overshoot tests ---------------------------------------------------
SKEW_Y0 = -0.3  # the step of the inflow profile on the face x = -1


def skew_velocity(angle_deg, speed=1.0):
    a = np.deg2rad(angle_deg)
    return speed * np.cos(a), speed * np.sin(a)


def skew_profile(x):
    """The data of the skew step on [-1, 1]^2: 1 on the inflow face x = -1 above y = SKEW_Y0, 0 elsewhere -- the Dirichlet
    value on the inflow faces x = -1 and y = -1 and, inside, the initial state."""
    return np.where(np.isclose(x[0], -1.0) & (x[1] > SKEW_Y0), 1.0, 0.0)


def skew_inflow_dofs(x_v):
    return np.nonzero(np.isclose(x_v[:, 0], -1.0) | np.isclose(x_v[:, 1], -1.0))[0]


def run_skew(F, x_v, kappa, dt, steps, angle_deg, stabilize, scale=1.0, options=None):
    """The skew step on the model: uniform velocity at ``angle_deg`` to the x axis, c = skew_profile on the inflow faces
    (Dirichlet), insulated outflow faces, c(0) = skew_profile.  Returns the model after ``steps`` steps."""
    ux, uy = skew_velocity(angle_deg)
    uab = np.zeros((F.nv, F.d))
    uab[:, 0], uab[:, 1] = ux, uy
    m = ScalarSupgModel(F, x_v, kappa, scale=scale, stabilize=stabilize, dofs=skew_inflow_dofs(x_v), value=skew_profile,
                        options=options or {"ksp_rtol": 1e-11, "ksp_atol": 1e-30})
    m.interpolate(skew_profile)
    for _ in range(steps):
        m.step(uab, dt)
        assert m.reason > 0
    return m
