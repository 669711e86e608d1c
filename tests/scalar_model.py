"""numpy model of the passive scalar step of FractionalStep_AB_CN (oasisx_amd/scalar.py, csrc/ox_scalar.hip), built on
the oracle's forms and Krylov solver (no GPU).  Per step, with the extrapolated velocity u_ab:

    A_c = M/dt + C(u_ab)/2 + kappa K/2
    b_c = (M/dt - C/2 - kappa K/2) c_1 + b0_c
    the scalar's own Dirichlet rows -> identity in A_c, boundary value in b_c;  solve;  c_1 <- c
"""
import numpy as np

from oracle import ipcs_oracle as O


def exact_c(x, t, kappa):
    """cos(pi x) cos(pi y) exp(-2 kappa pi^2 t): a function of the Taylor-Green stream function, so u . grad c = 0 and
    the advection-diffusion equation holds for ANY kappa."""
    return np.cos(np.pi * x[0]) * np.cos(np.pi * x[1]) * np.exp(-2.0 * kappa * np.pi ** 2 * t)


class ScalarModel:
    """One scalar on the oracle's velocity component space.  ``dofs`` / ``value``: Dirichlet rows and their value (float
    or callable on x:(3, npts)); ``source``: float or callable; ``options``: PETSc-style dict (bcgs + jacobi)."""

    def __init__(self, forms, x_v, kappa, dofs=None, value=0.0, source=0.0, options=None, M=None, K=None):
        self.F, self.x_v, self.kappa = forms, x_v, float(kappa)
        self.M = forms.mass_v() if M is None else M
        self.K = forms.stiffness_v() if K is None else K
        self.bc = None if dofs is None or len(dofs) == 0 else O.DirichletData(np.unique(dofs), value)
        if self.bc is not None:
            self.bc.update(x_v)
        self.b0 = forms.load_vec(source) if callable(source) else forms.body_force_vec(float(source))
        o = dict(options or {})
        self.rtol, self.atol = float(o.get("ksp_rtol", 1e-5)), float(o.get("ksp_atol", 1e-50))
        self.max_it = int(o.get("ksp_max_it", 10000))
        self.guess = bool(o.get("ksp_initial_guess_nonzero", False))
        self.c1 = np.zeros(forms.nv)
        self.c = np.zeros(forms.nv)
        self.A = self.b = None
        self.its = self.reason = None

    def interpolate(self, f):
        X = np.zeros((3, self.x_v.shape[0]))
        X[: self.x_v.shape[1]] = self.x_v.T
        self.c1[:] = f(X)
        self.c[:] = self.c1

    def assemble(self, uab, dt):
        """A_c (identity Dirichlet rows, columns kept) and b_c (boundary values in)."""
        C = self.F.convection(uab)
        Ac = (1.0 / dt) * self.M + 0.5 * C + (0.5 * self.kappa) * self.K
        self.b = (2.0 / dt) * (self.M @ self.c1) - Ac @ self.c1 + self.b0
        if self.bc is not None:
            self.bc.update(self.x_v)
            keep = np.ones(self.F.nv)
            keep[self.bc.dofs] = 0.0
            import scipy.sparse as sp

            Ac = sp.diags(keep) @ Ac + sp.diags(1.0 - keep)
            self.bc.apply(self.b)
        self.A = Ac.tocsr()
        return self.A, self.b

    def step(self, uab, dt):
        self.assemble(uab, dt)
        x0 = self.c1.copy() if self.guess else None
        self.c, self.reason, self.its, _ = O.jacobi_bicgstab(self.A, self.b, x0, self.rtol, self.atol, self.max_it)
        self.c1 = self.c.copy()
        return self.c


def tg_uab(x_v, t, dt, nu):
    """1.5 u(t - dt) - 0.5 u(t - 2 dt) of the Taylor-Green velocity at the dofs: what the step towards t extrapolates."""
    d = x_v.shape[1]
    X = np.zeros((3, x_v.shape[0]))
    X[:d] = x_v.T
    fns = [O.tg_u, O.tg_v, O.tg_w][:d]
    u1 = np.stack([f(X, t - dt, nu) for f in fns], axis=1)
    u2 = np.stack([f(X, t - 2 * dt, nu) for f in fns], axis=1)
    return 1.5 * u1 - 0.5 * u2


def exact_solution_error(N, kappa=0.05, nu=0.01, dt=0.005, steps=10, deg=2, options=None):
    """L2 error at t = steps * dt of the model on the N x N Taylor-Green square with exact Dirichlet data."""
    coords, cells = O.create_rectangle_mesh([-1, -1], [1, 1], [N, N])
    F = O.Forms(coords, cells, deg, 1)
    clock = {"t": 0.0}
    bd = O.boundary_dofs(F.x_v, coords.min(axis=0), coords.max(axis=0))
    m = ScalarModel(F, F.x_v, kappa, dofs=bd, value=lambda x: exact_c(x, clock["t"], kappa),
                    options=options or {"ksp_rtol": 1e-12, "ksp_atol": 1e-30})
    m.interpolate(lambda x: exact_c(x, 0.0, kappa))
    for k in range(steps):
        clock["t"] = (k + 1) * dt
        m.step(tg_uab(F.x_v, clock["t"], dt, nu), dt)
    return float(np.sqrt(F.l2_error_sq(m.c, lambda x: exact_c(x, clock["t"], kappa))))
