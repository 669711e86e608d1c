"""numpy model of the wall-distance query (oasisx_amd.geometry.WallDistance, ox_walldist_* of csrc/ox_probe.hip) and of
the van Driest damping of the Smagorinsky model (oasisx_amd.VanDriest, the damping of ox_cell_viscosity).  No GPU, no
grid: every point is tested against every facet.

    2-D   closest point of the segment (a, b): the projection t = (x - a).(b - a) / |b - a|^2 clamped to [0, 1]
    3-D   closest point of the triangle (a, b, c) by its seven regions: three vertices, three edges, the face
    both  q first, then d = |x - q| from the difference vector

    D = 1 - exp(-y+ / A+),   y+ = d u_tau / nu,   u_tau = sqrt(|wss|) of the nearest facet
    nut = (Cs Delta D)^2 sqrt(2 S:S)
"""
import itertools

import numpy as np

EPS = np.finfo(np.float64).eps


def closest_points(xyz, x):
    """q[i, f, :]: the closest point of facet f (xyz: (nf, d, d) vertices) to point x[i] ((n, d))."""
    xyz, x = np.asarray(xyz, dtype=np.float64), np.asarray(x, dtype=np.float64)
    d = xyz.shape[1]
    P = x[:, None, :]
    a, b = xyz[None, :, 0, :], xyz[None, :, 1, :]
    ab = b - a
    ap = P - a
    if d == 2:
        num, den = np.sum(ap * ab, axis=2), np.sum(ab * ab, axis=2)
        with np.errstate(invalid="ignore", divide="ignore"):
            t = num / den
        q = a + t[..., None] * ab
        q = np.where((num >= den)[..., None], b, q)
        return np.where(~(num > 0.0)[..., None], a, q)
    c = xyz[None, :, 2, :]
    ac, bp, cp = c - a, P - b, P - c
    dot = lambda u, v: np.sum(u * v, axis=2)  # noqa: E731
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(invalid="ignore", divide="ignore"):
        t_ab, t_ac = d1 / (d1 - d3), d2 / (d2 - d6)
        t_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = 1.0 / (va + vb + vc)
    conds = [(d1 <= 0.0) & (d2 <= 0.0), (d3 >= 0.0) & (d4 <= d3), (d6 >= 0.0) & (d5 <= d6),
             (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0), (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0),
             (va <= 0.0) & ((d4 - d3) >= 0.0) & ((d5 - d6) >= 0.0)]
    shape = np.broadcast_shapes(P.shape, a.shape)
    full = lambda v: np.broadcast_to(v, shape)  # noqa: E731
    choices = [full(a), full(b), full(c), a + t_ab[..., None] * ab, a + t_ac[..., None] * ac, b + t_bc[..., None] * (c - b)]
    q = a + (vb * den)[..., None] * ab + (vc * den)[..., None] * ac
    for cond, ch in zip(reversed(conds), reversed(choices)):  # (the first condition that holds wins)
        q = np.where(cond[..., None], ch, q)
    return q


def distances(xyz, x):
    """D[i, f] = distance of x[i] to facet f."""
    q = closest_points(xyz, x)
    r = np.asarray(x, dtype=np.float64)[:, None, :] - q
    return np.sqrt(np.sum(r * r, axis=2))


def nearest(xyz, x, shifts=None):
    """(dist (n,), nearest (n,), D (n, nf)): the minimum over the facets -- and over the images x + s of ``shifts`` -- the
    lowest facet that attains it, and the whole table of (image-minimal) distances."""
    x = np.asarray(x, dtype=np.float64)
    D = distances(xyz, x)
    for s in ([] if shifts is None else shifts):
        D = np.minimum(D, distances(xyz, x + np.asarray(s, dtype=np.float64)[None, : x.shape[1]]))
    return D.min(axis=1), D.argmin(axis=1), D


def image_shifts(period, axes):
    """The non-zero translations s * period, s in {-1, 0, 1} per periodic axis."""
    out = []
    for s in itertools.product((0, -1, 1), repeat=len(axes)):
        if any(s):
            v = np.zeros(3)
            for k, sk in zip(axes, s):
                v[k] = sk * period[k]
            out.append(v)
    return out


def shape_factor(xyz):
    """kappa = max_f (longest edge)^2 / (2 |f|) of triangles (>= 2 / sqrt(3)); 1 for segments."""
    xyz = np.asarray(xyz, dtype=np.float64)
    if xyz.shape[1] == 2:
        return 1.0, float(np.linalg.norm(xyz[:, 1] - xyz[:, 0], axis=1).min())
    e = np.stack([xyz[:, 1] - xyz[:, 0], xyz[:, 2] - xyz[:, 0], xyz[:, 2] - xyz[:, 1]], axis=1)
    ell = np.linalg.norm(e, axis=2).max(axis=1)
    area2 = np.linalg.norm(np.cross(e[:, 0], e[:, 1]), axis=1)
    return float((ell * ell / area2).max()), float(ell.min())


def distance_bound(xyz, x):
    """(C, L): |d_computed - d_model| <= C eps L for two evaluations of the formulas above in IEEE double arithmetic, in any
    order of the sums and with or without fused multiply-adds.

    L is the diagonal of the box of facets and queries: every difference vector is shorter.  One evaluation:

    * x - a, b - a, ...: one rounding each, eps/2 relative.  A dot product of two such vectors u, v of dimension d: at
      most (d + 2) (eps/2) |u| |v| off, i.e. <= 3 eps |u| |v|.
    * 2-D: t = num / den with |num| <= |ap| |ab|: |dt| |ab| <= (3 + 3 + 1/2) eps |ap| <= 7 eps L; q = a + t ab adds two
      roundings of numbers <= L: the computed q lies within 8 eps L of a point of the segment that is the exact
      minimiser up to the same amount.  x - q and the norm: (1 + (d + 2)/2) eps L more.  The distance is 1-Lipschitz in
      q, so one evaluation is within 11 eps L and two differ by at most C = 22.
    * 3-D, edge regions: as 2-D with d1 - d3 = |ab|^2 formed from two numbers <= l L (l: the edge): the quotient is
      off by 7 eps L / l, times |ab| = l: the same 7 eps L.  Face region: va, vb, vc are differences of products of the
      dot products, each product <= l^2 L^2 with (2 * 3 + 1/2) eps relative error: |d vc| <= 14 eps l^2 L^2, while
      va + vb + vc = (2 |f|)^2.  The barycentric weights are off by 14 eps l^2 L^2 / (2 |f|)^2 (and the same again for
      the sum and the division: 3 times), times the edge l: |dq| <= 42 kappa^2 (L / l) eps L with kappa = l^2 / (2 |f|),
      the facet's shape factor.  A region chosen differently near a region's border moves q by no more than that.
      With the roundings of q (3 terms), of x - q and of the norm: C = 2 (42 kappa^2 L / l_min + 8).

    The 3-D constant is an a-priori bound: q's error in the face region is tangential and enters the distance only to
    second order for points off the plane, so the measured differences are far below it."""
    xyz, x = np.asarray(xyz, dtype=np.float64), np.asarray(x, dtype=np.float64)
    d = xyz.shape[1]
    pts = np.concatenate([xyz.reshape(-1, d), x[np.isfinite(x).all(axis=1)].reshape(-1, d)])
    L = float(np.linalg.norm(pts.max(axis=0) - pts.min(axis=0)))
    if d == 2:
        return 22.0, L
    kappa, lmin = shape_factor(xyz)
    return 2.0 * (42.0 * kappa * kappa * L / lmin + 8.0), L


# ---- van Driest ------------------------------------------------------------------------------------------------------
def damping(dist, u_tau, nu, a_plus):
    """(y+, D): y+ = d u_tau / nu, D = 1 - exp(-y+ / A+) (as -expm1: no cancellation at the wall)."""
    yp = np.asarray(dist, dtype=np.float64) * np.asarray(u_tau, dtype=np.float64) / float(nu)
    return yp, -np.expm1(-yp / float(a_plus))


def friction_velocity(wss):
    """u_tau = sqrt(|wss|) per facet, wss (nf, d) kinematic."""
    return np.sqrt(np.sqrt(np.sum(np.asarray(wss, dtype=np.float64) ** 2, axis=1)))


def damped_smagorinsky(F, uab, Cs, D):
    """nut per cell (the cell order of the Forms object F): (Cs Delta D)^2 sqrt(2 S:S)."""
    from tests import viscosity_model as VM

    return VM.nut_cells(F, uab, ("smagorinsky", Cs)) * np.asarray(D, dtype=np.float64) ** 2


def poiseuille_nut(Cs, cell_area, y_c, H, G, nu, a_plus):
    """Closed form for u_x = G y (H - y) / (2 nu) between walls at y = 0 and y = H (2-D): |wss| = G H / 2 on both walls,
    gd = G |H - 2 y| / (2 nu), Delta^2 = |cell|:  nut_c = Cs^2 |cell| D(y_c)^2 G |H - 2 y_c| / (2 nu)."""
    y_c = np.asarray(y_c, dtype=np.float64)
    u_tau = np.sqrt(G * H / 2.0)
    _, D = damping(np.minimum(y_c, H - y_c), u_tau, nu, a_plus)
    return Cs ** 2 * np.asarray(cell_area) * D ** 2 * G * np.abs(H - 2.0 * y_c) / (2.0 * nu)
