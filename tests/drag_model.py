"""numpy model of the drag zones of FractionalStep_AB_CN (oasisx_amd/drag.py, csrc/ox_drag.hip), built on the oracle's
forms (no GPU, no generated tables).

    sigma_c = alpha_c + beta_c |w(x_c)|,  w = u_ab - u_t at the centroid (the velocity basis tabulated there)
    D       = sum_c sigma_c M_c           ``adet * sigma`` times the reference mass matrix of ``Forms.mass_v``, by ``F._csr``
    A       = M/dt + C/2 + nu K/2 + theta D
    b       = (M/dt - C/2 - nu K/2) u_1 + b0 - (1 - theta) D u_1 + D u_t

A zone is a :class:`Zone`: the cells in the cell order of the ``Forms`` object, ``alpha`` and ``beta`` per cell of the zone
(or floats) and the target as an ``(nv, d)`` field in the numbering of ``F.vd`` (``None``: zero).
"""
import numpy as np

from oracle import ipcs_oracle as O
from tests import viscosity_model as VM


class Zone:
    def __init__(self, cells, alpha=0.0, beta=0.0, ut=None, rho=1.0):
        self.cells = np.asarray(cells, dtype=np.int64)
        n = self.cells.shape[0]
        self.alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (n,)).copy()
        self.beta = np.broadcast_to(np.asarray(beta, dtype=np.float64), (n,)).copy()
        self.ut, self.rho = ut, float(rho)


def centroid_value(F, u, cells=None):
    """u at the centroids, (n, d): the velocity basis at the centroid contracted with the cells' dofs."""
    d = F.d
    bary = np.full((1, d + 1), 1.0 / (d + 1))
    phi, _ = O.tabulate(d, F.u_deg, bary)  # (1, nd)
    vd = F.vd if cells is None else F.vd[cells]
    return np.einsum("i,cid->cd", phi[0], u[vd])


_OWN = object()


def sigma_cells(F, uab, zone, ut=_OWN):
    """sigma per cell of the ZONE (in the order of ``zone.cells``); ``ut``: the target field (default: the zone's own)."""
    ut = zone.ut if ut is _OWN else ut
    w = uab if ut is None else uab - ut
    mag = np.linalg.norm(centroid_value(F, w, zone.cells), axis=1)
    return zone.alpha + zone.beta * mag


def sigma_field(F, uab, zones):
    """sigma per cell of the mesh, zero outside the zones.  The target is ONE field of the velocity space
    (``merged_target``): a dof that cells of two zones share carries one value."""
    out = np.zeros(F.cells.shape[0])
    ut = merged_target(F, zones)
    for z in zones:
        out[z.cells] = sigma_cells(F, uab, z, ut)
    return out


def weighted_mass(F, w):
    """sum_c w_c M_c on the velocity component space."""
    w = np.broadcast_to(np.asarray(w, dtype=np.float64), F.adet.shape)
    Mref = np.einsum("q,qi,qj->ij", F.w, F.phi_v, F.phi_v)
    Ae = (F.adet * w)[:, None, None] * Mref[None]
    return F._csr(Ae, F.vd, F.vd, (F.nv, F.nv))


def weighted_load(F, w):
    """sum_c w_c int_c phi_i dx: the row sums of ``weighted_mass(F, w)``."""
    w = np.broadcast_to(np.asarray(w, dtype=np.float64), F.adet.shape)
    be = (F.adet * w)[:, None] * np.einsum("q,qi->i", F.w, F.phi_v)[None]
    return F._vec(be, F.vd, F.nv)


def zone_force(F, u, sigma, zone, ut=_OWN):
    """rho sum_c sigma_c int_c (u - u_t) dx over the cells of the zone, (d,), and the sum of the magnitudes of its terms;
    ``sigma``: per cell of the mesh; ``ut``: the target field (default: the zone's own)."""
    ut = zone.ut if ut is _OWN else ut
    w = u if ut is None else u - ut
    mean = np.einsum("q,qi->i", F.w, F.phi_v)  # int phi_i over the reference cell
    t = (sigma[zone.cells] * F.adet[zone.cells])[:, None] * np.einsum("i,cid->cd", mean, w[F.vd[zone.cells]])
    return zone.rho * t.sum(axis=0), zone.rho * np.abs(t).sum(axis=0)


def merged_target(F, zones):
    """One (nv, d) field from the zones' targets, in the order of the zones, on the dofs of their cells (zero where
    none), or None: what the solver keeps.  On a dof shared by cells of two zones the later zone's target holds."""
    if all(z.ut is None for z in zones):
        return None
    ut = np.zeros((F.nv, F.d))
    for z in zones:
        if z.ut is not None:
            dofs = np.unique(F.vd[z.cells])
            ut[dofs] = z.ut[dofs]
    return ut


class DragOracleStep(VM.ViscosityOracleStep):
    """``OracleFractionalStep`` (with the eddy-viscosity models of ``ViscosityOracleStep``) whose ``assemble_first``
    inserts ``theta D`` and the two vector terms before the identity rows -- it restates the oracle's lines
    (oracle/ipcs_oracle.py, ``OracleFractionalStep.assemble_first``), which cannot be split from outside."""

    def __init__(self, *args, zones=(), theta=1.0, **kw):
        super().__init__(*args, **kw)
        self.zones, self.theta = list(zones), float(theta)
        self.sigma = None
        self.drag_matrix = None

    def assemble_first(self, dt, nu):
        plain = self.F
        F = VM._FormsWithNut(plain, self) if self.model is not None else plain
        self.uab[:] = 1.5 * self.u1 - 0.5 * self.u2
        Cm = F.convection(self.uab)
        A = -0.5 * Cm + (1.0 / dt) * self.M + (-0.5 * nu) * self.K
        for bp in self.bcs_p:
            bp.update(self.x_q)
        for i in range(self.d):
            self.b_first[:, i] = A @ self.u1[:, i] + self.b0[:, i]
            for bp in self.bcs_p:
                self.b_first[:, i] += plain.pressure_surface_vec(bp.fc, bp.fa, bp.h, i)
        A = -A + (2.0 / dt) * self.M
        if self.zones:
            self.sigma = sigma_field(plain, self.uab, self.zones)
            self.drag_matrix = weighted_mass(plain, self.sigma)
            A = A + self.theta * self.drag_matrix
            if self.theta != 1.0:
                self.b_first -= (1.0 - self.theta) * (self.drag_matrix @ self.u1)
            ut = merged_target(plain, self.zones)
            if ut is not None:
                self.b_first += self.drag_matrix @ ut
        A = A.tolil()
        for bc in self.bcs_u[0]:
            for r in np.unique(bc.dofs):
                A.rows[r] = list(A.rows[r])
                A.data[r] = [1.0 if c == r else 0.0 for c in A.rows[r]]
        self.A = A.tocsr()
        self.solver_u.set_operator(self.A)


# ---- the Brinkman channel: -nu u'' + sigma u = f on (-1, 1), u(+-1) = 0 -------------------------------------------------
BRINKMAN = dict(nu=0.5, sigma=2.0, f=1.0)
# max |u_h - u| / u(0) of the direct solve nu K + sigma M on the oracle's forms, measured on the CPU with this set-up
BRINKMAN_MEASURED = {(1, 8): 6.1e-3, (2, 4): 1.0e-3, (2, 8): 7.5e-5, (3, 4): 2.8e-4}


def brinkman_exact(y, nu=BRINKMAN["nu"], sigma=BRINKMAN["sigma"], f=BRINKMAN["f"]):
    m = np.sqrt(sigma / nu)
    return (f / sigma) * (1.0 - np.cosh(m * y) / np.cosh(m))


def brinkman_direct(deg, N):
    """The discrete steady state of the Brinkman channel on [-1, 1]^2 (sigma everywhere, body force f along x, exact
    Dirichlet data on the whole boundary): one linear solve with nu K + sigma M on the oracle's forms.  Returns
    (max |u_h - u| / u(0), u_h, forms)."""
    import scipy.sparse.linalg as spla

    nu, sigma, f = BRINKMAN["nu"], BRINKMAN["sigma"], BRINKMAN["f"]
    F = VM.tg_forms(2, N, deg, 2 if deg == 3 else 1)
    x = F.x_v
    D = weighted_mass(F, sigma)
    L = (nu * F.stiffness_v() + D).tocsr()
    b = F.body_force_vec(f)
    bd = O.boundary_dofs(x, F.coords.min(axis=0), F.coords.max(axis=0))
    exact = brinkman_exact(x[:, 1])
    u = np.zeros(F.nv)
    u[bd] = exact[bd]
    free = np.setdiff1d(np.arange(F.nv), bd)
    rhs = b - L @ u
    u[free] = spla.spsolve(L[free][:, free].tocsc(), rhs[free])
    return float(np.abs(u - exact).max() / brinkman_exact(0.0)), u, F
