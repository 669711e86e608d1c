"""numpy model of the wall-stress evaluation on exterior facets (no GPU, no generated tables).

On facet f of cell c, opposite local vertex a, with outward unit normal n and measure |f|:

    t_f   = -pbar n + nu_eff (gbar + gbar^T) n     gbar, pbar: facet means of grad u and p
    wss_f = t_f - (t_f . n) n
    F_tag = -rho sum_{f in tag} |f| t_f

The facet means are taken with a quadrature on the facet that is exact to degree 5 (three Gauss points on an edge,
``fem._simplex_rule(2, 3)`` on a triangle) of ``fem.lagrange_basis`` / ``lagrange_basis_derivs``; normals, measures
and midpoints come from the vertex coordinates alone (edge vectors and cross products), not from grad(lambda).
"""
import numpy as np

from oasisx_amd import fem


def exterior_facets(cells):
    """(cell, opposite local vertex) of every facet that belongs to one cell only, sorted by (cell, vertex)."""
    nc, nv = cells.shape
    keys = {}
    for a in range(nv):
        others = np.sort(np.delete(cells, a, axis=1), axis=1)
        for c in range(nc):
            keys.setdefault(tuple(others[c]), []).append((c, a))
    out = sorted(v[0] for v in keys.values() if len(v) == 1)
    return np.array([c for c, _ in out]), np.array([a for _, a in out])


def facet_rule(d):
    """Points (nq, d) in the facet's own barycentric coordinates and weights summing to 1; exact to degree 5."""
    if d == 2:
        from numpy.polynomial.legendre import leggauss

        s, w = leggauss(3)
        return np.stack([(1 - s) / 2, (1 + s) / 2], axis=1), w / 2
    b, w = fem._simplex_rule(2, 3)
    return b, w * 2.0


def facet_points(d, a):
    """The rule of ``facet_rule`` on local facet a, as barycentric points (nq, d + 1) of the cell (lambda_a = 0)."""
    b, w = facet_rule(d)
    p = np.zeros((b.shape[0], d + 1))
    p[:, [k for k in range(d + 1) if k != a]] = b
    return p, w


def facet_means(d, degree, a):
    """(mean of phi_i (nd,), mean of dphi_i/dlambda_b (nd, d + 1), sum_q w_q |dphi| (nd, d + 1)) over local facet a."""
    p, w = facet_points(d, a)
    phi = fem.lagrange_basis(d, degree, p)
    dphi = fem.lagrange_basis_derivs(d, degree, p)
    return w @ phi, np.einsum("q,qib->ib", w, dphi), np.einsum("q,qib->ib", w, np.abs(dphi))


def facet_geometry(coords, cells, fcell, fopp):
    """(normals (nf, d), measures (nf,), midpoints (nf, d)) from the vertex coordinates: the normal points away from
    the opposite vertex."""
    d = coords.shape[1]
    x = coords[cells[fcell]]  # (nf, d + 1, d)
    nf = x.shape[0]
    idx = np.array([[k for k in range(d + 1) if k != a] for a in fopp])
    xf = x[np.arange(nf)[:, None], idx]  # (nf, d, d): the facet's vertices
    xo = x[np.arange(nf), fopp]
    mid = xf.mean(axis=1)
    if d == 2:
        e = xf[:, 1] - xf[:, 0]
        nrm = np.stack([e[:, 1], -e[:, 0]], axis=1)
        meas = np.linalg.norm(e, axis=1)
    else:
        nrm = np.cross(xf[:, 1] - xf[:, 0], xf[:, 2] - xf[:, 0])
        meas = 0.5 * np.linalg.norm(nrm, axis=1)
    nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    sign = np.sign(np.einsum("fk,fk->f", nrm, mid - xo))
    return nrm * sign[:, None], meas, mid


def barycentric_gradients(coords, cells, fcell):
    """grad lambda_b (nf, d + 1, d) of the facets' cells."""
    x = coords[cells[fcell]]
    J = np.swapaxes(x[:, 1:, :] - x[:, :1, :], 1, 2)
    Ginv = np.linalg.inv(J)
    return np.concatenate([-Ginv.sum(axis=1, keepdims=True), Ginv], axis=1)


def facet_mean_fields(coords, cells, fcell, fopp, vd, qd, u, p, deg_u, deg_p):
    """(gbar (nf, d, d) with gbar[f, i, k] = mean of d u_i / d x_k, pbar (nf,))."""
    d = coords.shape[1]
    G = barycentric_gradients(coords, cells, fcell)
    nf = fcell.shape[0]
    gbar, pbar = np.zeros((nf, d, d)), np.zeros(nf)
    for a in range(d + 1):
        sel = np.nonzero(fopp == a)[0]
        if sel.size == 0:
            continue
        pts, w = facet_points(d, a)
        dphi = fem.lagrange_basis_derivs(d, deg_u, pts)  # (nq, nd, d + 1)
        psi = fem.lagrange_basis(d, deg_p, pts)  # (nq, ndq)
        uc = u[vd[fcell[sel]]]  # (m, nd, d)
        gq = np.einsum("fni,qnb,fbk->fqik", uc, dphi, G[sel])
        gbar[sel] = np.einsum("q,fqik->fik", w, gq)
        pbar[sel] = np.einsum("q,qn,fn->f", w, psi, p[qd[fcell[sel]]])
    return gbar, pbar


def traction(gbar, pbar, normals, nu_eff):
    """(t (nf, d), wss (nf, d)) from the facet means; nu_eff a scalar or one value per facet."""
    sym = gbar + np.swapaxes(gbar, 1, 2)
    nu_eff = np.broadcast_to(np.asarray(nu_eff, dtype=np.float64), pbar.shape)
    t = -pbar[:, None] * normals + nu_eff[:, None] * np.einsum("fik,fk->fi", sym, normals)
    wss = t - np.einsum("fi,fi->f", t, normals)[:, None] * normals
    return t, wss


def wall_stress(coords, cells, fcell, fopp, vd, qd, u, p, deg_u, deg_p, nu_eff):
    normals, meas, _ = facet_geometry(coords, cells, fcell, fopp)
    gbar, pbar = facet_mean_fields(coords, cells, fcell, fopp, vd, qd, u, p, deg_u, deg_p)
    return traction(gbar, pbar, normals, nu_eff)


def forces(t, measures, tag_of_facet, tags, rho=1.0):
    """F[k] = -rho sum_{f: tag_of_facet[f] == tags[k]} |f| t_f, shape (n_tags, d)."""
    return np.stack([-rho * (measures[tag_of_facet == g, None] * t[tag_of_facet == g]).sum(axis=0) for g in tags])
