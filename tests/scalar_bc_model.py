"""numpy model of the flux and Robin conditions of a scalar (oasisx_amd/scalar.py ``flux_bcs=``, ``ox_scalar_boundary`` of
csrc/ox_scalar.hip), built on tests/scalar_model.ScalarModel, on the facet rule of tests/outlet_model.py and on the oracle's
forms fed the device's numbering (no GPU).  With n outward, on the facets of a condition:

    flux:    kappa_eff dc/dn = q                                              q > 0 enters the domain
    Robin:  -kappa_eff dc/dn = hq (c - c_inf),   hq = h + beta max(-u_ab . n, 0)

    H_rs   = sum_f |f| sum_k w_k hq(x_k) phi_r(x_k) phi_s(x_k)
    load_r = sum_f |f| sum_k w_k (q(x_k) + hq(x_k) c_inf(x_k)) phi_r(x_k)
    A_c = M/dt + C(u_ab)/2 + kappa K/2 + H/2
    b_c = (2/dt) M c_1 - A_c c_1 + b0_c + load          (Crank-Nicolson in c: the -H/2 c_1 is in A_c c_1)
    the scalar's own Dirichlet rows last, as in ``ScalarModel.assemble``: they win on rim dofs.

q, h and c_inf are NODAL: a float or a callable evaluated at the dof coordinates ``x_v`` and interpolated on the facet with
the cell's basis (the basis functions of dofs off the facet vanish there).  The conditions of one facet add.
"""
import numpy as np
import scipy.sparse as sp

from oasisx_amd import fem
from tests import outlet_model as OM
from tests import wall_stress_model as WM
from tests.scalar_model import ScalarModel


def nodal(f, x_v):
    """The datum at every dof: (n_dofs,)."""
    X = np.zeros((3, x_v.shape[0]))
    X[: x_v.shape[1]] = x_v.T
    return np.broadcast_to(np.asarray(f(X) if callable(f) else float(f), dtype=np.float64), (x_v.shape[0],)).copy()


class Flux:
    """``FluxBC(q, facets)``: facets as (cell in the forms' order, opposite local vertex)."""

    def __init__(self, fc, fa, q):
        self.fc, self.fa, self.q = np.asarray(fc), np.asarray(fa), q
        self.h, self.c_inf, self.beta = 0.0, 0.0, 0.0


class Robin:
    """``RobinBC(h, c_inf, facets, advective=beta)``."""

    def __init__(self, fc, fa, h, c_inf, beta=0.0):
        self.fc, self.fa, self.q = np.asarray(fc), np.asarray(fa), 0.0
        self.h, self.c_inf, self.beta = h, c_inf, float(beta)


def surface_terms(F, x_v, cond, uab):
    """(H as CSR, load, advective part of H as CSR) of one condition."""
    d, deg, n = F.d, F.u_deg, F.nv
    normals, meas, _ = WM.facet_geometry(F.coords, F.cells, cond.fc, cond.fa)
    qn, hn, cn = nodal(cond.q, x_v), nodal(cond.h, x_v), nodal(cond.c_inf, x_v)
    assert (hn >= 0.0).all()
    rows, cols, vals, avals = [], [], [], []
    load = np.zeros(n)
    for a in range(d + 1):
        sel = np.nonzero(cond.fa == a)[0]
        if sel.size == 0:
            continue
        pts, w = OM.facet_points(d, deg, a)
        phi = fem.lagrange_basis(d, deg, pts)  # (nq, nd)
        dofs = F.vd[cond.fc[sel]]  # (m, nd)
        un = np.einsum("qn,fnk,fk->fq", phi, uab[dofs], normals[sel])
        adv = cond.beta * np.maximum(-un, 0.0)
        hq = np.einsum("qn,fn->fq", phi, hn[dofs]) + adv
        g = np.einsum("qn,fn->fq", phi, qn[dofs]) + hq * np.einsum("qn,fn->fq", phi, cn[dofs])
        He = np.einsum("f,q,fq,qr,qs->frs", meas[sel], w, hq, phi, phi)
        Ae = np.einsum("f,q,fq,qr,qs->frs", meas[sel], w, adv, phi, phi)
        np.add.at(load, dofs.ravel(), np.einsum("f,q,fq,qr->fr", meas[sel], w, g, phi).ravel())
        nd = dofs.shape[1]
        rows.append(np.repeat(dofs, nd, axis=1).ravel())
        cols.append(np.tile(dofs, (1, nd)).ravel())
        vals.append(He.ravel())
        avals.append(Ae.ravel())
    if not rows:
        return sp.csr_matrix((n, n)), load, sp.csr_matrix((n, n))
    r, c = np.concatenate(rows), np.concatenate(cols)
    H = sp.coo_matrix((np.concatenate(vals), (r, c)), shape=(n, n)).tocsr()
    Hadv = sp.coo_matrix((np.concatenate(avals), (r, c)), shape=(n, n)).tocsr()
    return H, load, Hadv


def boundary_terms(F, x_v, conditions, uab):
    """(H, load) summed over the conditions."""
    n = F.nv
    H, load = sp.csr_matrix((n, n)), np.zeros(n)
    for cond in conditions:
        Hc, lc, _ = surface_terms(F, x_v, cond, uab)
        H, load = H + Hc, load + lc
    return H.tocsr(), load


def boundary_measure(F, cond):
    return float(WM.facet_geometry(F.coords, F.cells, cond.fc, cond.fa)[1].sum())


class _FormsWithSurfaceTerm:
    """The forms with ``convection`` returning C + H: with it ``ScalarModel.assemble`` forms M/dt + (C + H)/2 + kappa K/2
    and takes (C + H)/2 c_1 from the right-hand side (the trick of tests/scalar_les_model.py)."""

    def __init__(self, forms, H):
        self._F, self._H = forms, H

    def __getattr__(self, name):
        return getattr(self._F, name)

    def convection(self, uab):
        return self._F.convection(uab) + self._H


def with_conditions(base=ScalarModel):
    """``base`` (ScalarModel or a model built on it) with ``conditions=[Flux | Robin, ...]``."""

    class Conditioned(base):
        def __init__(self, *a, conditions=(), **kw):
            super().__init__(*a, **kw)
            self.conditions = list(conditions)
            self.H = self.load = None

        def assemble(self, uab, dt, *a, **kw):
            plain, b0 = self.F, self.b0
            self.H, self.load = boundary_terms(plain, self.x_v, self.conditions, uab)
            self.F, self.b0 = _FormsWithSurfaceTerm(plain, self.H), b0 + self.load
            try:
                return super().assemble(uab, dt, *a, **kw)
            finally:
                self.F, self.b0 = plain, b0

    Conditioned.__name__ = base.__name__ + "WithConditions"
    return Conditioned


ScalarBCModel = with_conditions(ScalarModel)
