"""numpy model of the Lagrangian average of the dynamic Smagorinsky model (oasisx_amd.DynamicSmagorinsky with
``average="lagrangian"``, ``ox_dynamic_lagrangian`` in csrc/ox_probe.hip), built on
tests/dynamic_model.py (no GPU).  Per vertex class v, with ``(.)_v`` the patch mean of dynamic_model.Patches:

    sources      s_LM = -2 (LM)_v,  s_MM = 4 (MM)_v                     Delta_v = ((|c|)_v)^(1/gdim)
    velocity     u_v = the patch mean of the centroid values of u_ab
    first update F_MM = s_MM,  F_LM = max(cs2_initial s_MM, cs2_floor s_MM)
    later        x' = x_v - h u_v, folded into the box on periodic axes; its cell: the hint (the first cell of the vertex's
                 patch) if all barycentric coordinates are >= 0, else the lowest MESH cell id with min lambda >= -tol;
                 B = the P1 interpolant of the old fields at x' (status 0), F_old(v) (status 1: no cell), NaN (status 2:
                 x' not finite);  T = time_scale Delta_v (F_LM F_MM)_old^(-1/8),  eps = (h/T) / (1 + h/T), 0 where the
                 product is not positive and finite;  F_MM = eps s_MM + (1 - eps) B_MM,
                 F_LM = max(eps s_LM + (1 - eps) B_LM, cs2_floor F_MM)
    coefficient  Cs2_v = clip(F_LM / F_MM, 0, cs2_max), 0 where F_MM is not positive;  Cs2_c = the mean over the cell's
                 vertices;  nut_c = Cs2_c D_c s_c

``Geometry`` takes the cells in the order the patches were built in (the kernels' order on the device) and, where that is
not the mesh's order, ``cell_ids``: the mesh cell id of every position -- "lowest containing cell" is by mesh id.
Every update also returns the magnitude sums ``eps |s| + (1 - eps) sum_j |lambda_j| |F_old,j|`` of both fields -- the
basis of the tests' bounds, as kappa is in section 26 -- and the smallest barycentric coordinate at the departure point.
"""
import numpy as np

from oracle import ipcs_oracle as O
from tests import dynamic_model as DM
from tests import viscosity_model as VM

DEFAULT = dict(filter_ratio=2.0, cs2_max=0.09, cs2_initial=0.0256, time_scale=1.5, cs2_floor=1e-24)


def nanmax(a, b):
    """max(a, b) that lets a NaN of either side through."""
    return np.where(a >= b, a, np.where(np.isnan(a), a, b))


def clip(f_lm, f_mm, cs2_max):
    """F_LM / F_MM clipped to [0, cs2_max]; 0 where F_MM is not positive; NaN stays NaN (dynamic_model.clip's forms)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        c = f_lm / f_mm
    out = np.where(c < 0.0, 0.0, np.where(c > cs2_max, cs2_max, c))
    out = np.where(f_mm > 0.0, out, 0.0)
    return np.where(np.isnan(f_lm) | np.isnan(f_mm), np.nan, out)


class Geometry:
    """What the back-trace needs of a mesh: ``coords`` (nv_geo, d), ``cells`` (nc, d + 1) geometric vertex ids, ``P`` the
    dynamic_model.Patches on them (its ``verts`` are the vertex classes), ``x_v`` (n_classes, d) the master vertex of every
    class, ``periodic``: None or ``(axes, lo, hi, period)``."""

    def __init__(self, coords, cells, P, x_v=None, cell_ids=None, periodic=None, tol=1e-10):
        self.coords, self.cells, self.P = np.asarray(coords, dtype=np.float64), np.asarray(cells, dtype=np.int64), P
        self.d = d = self.coords.shape[1]
        self.n = P.n_vertices
        self.x_v = self.coords if x_v is None else np.asarray(x_v, dtype=np.float64)
        assert self.x_v.shape == (self.n, d), (self.x_v.shape, self.n, d)
        nc = self.cells.shape[0]
        self.cell_ids = np.arange(nc) if cell_ids is None else np.asarray(cell_ids, dtype=np.int64)
        self.order = np.argsort(self.cell_ids, kind="stable")  # positions in ascending mesh cell id
        self.periodic, self.tol = periodic, float(tol)
        xc = self.coords[self.cells]  # (nc, d + 1, d)
        self.x0 = xc[:, 0]
        T = np.swapaxes(xc[:, 1:] - xc[:, :1], 1, 2)  # columns x_a - x_0
        self.grad = np.linalg.inv(T)  # rows: grad(lambda_1..d)
        # the hint: the lowest position among the cells of the class's patch
        hint = np.full(self.n, nc, dtype=np.int64)
        for a in range(d + 1):
            np.minimum.at(hint, P.verts[:, a], np.arange(nc))
        assert hint.max() < nc
        self.hint = hint
        self.delta = P.to_vertices(P.vol) ** (1.0 / d)
        self.altitude = 1.0 / np.sqrt(np.concatenate([(self.grad ** 2).sum(axis=2),
                                                      ((self.grad.sum(axis=1)) ** 2).sum(axis=1)[:, None]], axis=1))

    def bary(self, x, c):
        """lambda (d + 1,) of the point x in the cell at position c."""
        l = self.grad[c] @ (x - self.x0[c])
        return np.concatenate([[1.0 - l.sum()], l])

    def bary_all(self, x):
        """lambda (nc, d + 1) of one point in every cell."""
        l = np.einsum("cak,ck->ca", self.grad, x[None, :] - self.x0)
        return np.concatenate([1.0 - l.sum(axis=1, keepdims=True), l], axis=1)

    def fold(self, x):
        x = np.array(x, dtype=np.float64)
        if self.periodic is not None:
            axes, lo, hi, period = self.periodic
            for k in axes:
                x[..., k] -= period[k] * np.floor((x[..., k] - lo[k]) / period[k])
                x[..., k] = np.where(x[..., k] >= hi[k], x[..., k] - period[k], x[..., k])
        return x

    def locate(self, x, hint):
        """(position of the cell or -1, lambda, the min lambda that decided)."""
        lam = self.bary(x, hint)
        if lam.min() >= 0.0:
            return hint, lam, lam.min()
        la = self.bary_all(x)
        mins = la.min(axis=1)
        ok = np.nonzero(mins[self.order] >= -self.tol)[0]
        if ok.shape[0] == 0:
            return -1, None, mins.max()
        c = self.order[ok[0]]
        return c, la[c], mins[c]

    def backtrace(self, u_v, h, f_old):
        """(B (n, 2), |B| (n, 2), status (n,), min lambda (n,), x' (n, d)) of the old fields f_old (n, 2)."""
        with np.errstate(invalid="ignore"):
            xp = self.fold(self.x_v - h * u_v)
        B, Bm = np.array(f_old, dtype=np.float64), np.abs(f_old)
        status = np.zeros(self.n, dtype=np.int32)
        minlam = np.full(self.n, np.nan)
        for v in range(self.n):
            if not np.isfinite(xp[v]).all():
                status[v] = 2
                continue
            c, lam, minlam[v] = self.locate(xp[v], self.hint[v])
            if c < 0:
                status[v] = 1
                continue
            w = self.P.verts[c]
            a, am = np.zeros(2), np.zeros(2)
            for j in range(self.d + 1):  # local vertex order
                a = a + lam[j] * f_old[w[j]]
                am = am + abs(lam[j]) * np.abs(f_old[w[j]])
            B[v], Bm[v] = a, am
        return B, Bm, status, minlam, xp


def update(geo, s_lm, s_mm, u_v, h, f_old, first, cs2_max=0.09, cs2_initial=0.0256, time_scale=1.5, cs2_floor=1e-24,
           filter_ratio=None):
    """One update of the fields from the sources per vertex.  Returns a dict: ``F`` (n, 2) = {F_LM, F_MM}, ``cs2v``,
    ``status``, ``mag`` (n, 2) the magnitude sums, ``minlam``, ``eps``, ``unfloored`` (F_LM before the floor), ``xp``."""
    n = geo.n
    s = np.stack([s_lm, s_mm], axis=1)
    if first:
        f_mm = s_mm.copy()
        unfl = cs2_initial * s_mm
        f_lm = nanmax(unfl, cs2_floor * s_mm)
        return dict(F=np.stack([f_lm, f_mm], axis=1), cs2v=clip(f_lm, f_mm, cs2_max), status=np.zeros(n, dtype=np.int32),
                    mag=np.abs(np.stack([f_lm, f_mm], axis=1)), minlam=np.full(n, np.nan), eps=np.ones(n), unfloored=unfl,
                    xp=geo.x_v.copy())
    B, Bm, status, minlam, xp = geo.backtrace(u_v, h, f_old)
    p = f_old[:, 0] * f_old[:, 1]
    good = np.isfinite(p) & (p > 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        T = time_scale * geo.delta * np.where(good, p, 1.0) ** (-0.125)
        r = h / T
        eps = np.where(good, r / (1.0 + r), 0.0)
    eps = np.where(np.isnan(p), np.nan, eps)
    f_mm = eps * s_mm + (1.0 - eps) * B[:, 1]
    unfl = eps * s_lm + (1.0 - eps) * B[:, 0]
    f_lm = nanmax(unfl, cs2_floor * f_mm)
    bad = status == 2
    f_lm, f_mm = np.where(bad, np.nan, f_lm), np.where(bad, np.nan, f_mm)
    mag = eps[:, None] * np.abs(s) + (1.0 - eps)[:, None] * Bm
    return dict(F=np.stack([f_lm, f_mm], axis=1), cs2v=clip(f_lm, f_mm, cs2_max), status=status, mag=mag, minlam=minlam,
                eps=eps, unfloored=unfl, xp=xp)


def cs2_bound(res, rel=1e-12):
    """The bound on Cs2_v that follows from ``rel`` times the magnitude sums of the two fields:
    d(a / b) <= (da + |a / b| db) / b."""
    F, mag = res["F"], res["mag"]
    with np.errstate(divide="ignore", invalid="ignore"):
        return rel * (mag[:, 0] + np.abs(F[:, 0] / F[:, 1]) * mag[:, 1]) / np.abs(F[:, 1])


def near_floor(res, cs2_floor, rel=1e-12):
    """Vertices whose unfloored F_LM lies within its bound of the floor: there the max may pick either side."""
    return np.abs(res["unfloored"] - cs2_floor * res["F"][:, 1]) <= rel * res["mag"][:, 0] + cs2_floor * rel * res["mag"][:, 1]


def sources(F, uab, P, filter_ratio=2.0):
    """(s_LM, s_MM, u_v) per vertex class from u_ab."""
    LM, MM = DM.products(F, uab, P, filter_ratio)
    u_v = DM.vertex_moments(F, uab, P)[:, : F.d]
    return -2.0 * P.to_vertices(LM), 4.0 * P.to_vertices(MM), u_v


class Lagrangian:
    """The model with its memory: ``evaluate(F, uab, dt)`` returns (nut, Cs2 per cell) as the device's ``evaluate`` does."""

    def __init__(self, geo, update_every=1, **params):
        self.geo, self.update_every = geo, int(update_every)
        self.params = dict(DEFAULT)
        self.params.update(params)
        self.n_evaluations = self.n_updates = 0
        self.fields = np.zeros((geo.n, 2))
        self.res = self.cs2 = None

    def step_fields(self, F, uab, dt):
        s_lm, s_mm, u_v = sources(F, uab, self.geo.P, self.params["filter_ratio"])
        self.res = update(self.geo, s_lm, s_mm, u_v, self.update_every * dt, self.fields, self.n_updates == 0, **self.params)
        self.fields = self.res["F"]
        self.cs2 = self.geo.P.to_cells(self.res["cs2v"])
        self.n_updates += 1

    def evaluate(self, F, uab, dt):
        if self.n_evaluations % self.update_every == 0:
            self.step_fields(F, uab, dt)
        self.n_evaluations += 1
        _, _, ds, _ = DM.cell_record(F, uab)
        return self.cs2 * ds, self.cs2


class _FormsWithLagrangianNut:
    def __init__(self, forms, owner, dt):
        self._F, self._owner, self._dt = forms, owner, dt

    def __getattr__(self, name):
        return getattr(self._F, name)

    def convection(self, uab):
        o = self._owner
        o.nut, o.cs2 = o.lagrangian.evaluate(self._F, uab, self._dt)
        return self._F.convection(uab) + VM.weighted_stiffness(self._F, o.nut)


class LagrangianOracleStep(VM.ViscosityOracleStep):
    """``ViscosityOracleStep`` whose ``nut`` comes from the Lagrangian model: the fields and ``Cs2`` are updated in the
    first ``assemble_first`` and every ``update_every``-th after it, ``nut = Cs2 D s`` in every one."""

    def __init__(self, *args, geometry=None, update_every=1, lagrangian=None, **kw):
        super().__init__(*args, **kw)
        self.model = "lagrangian"
        self.lagrangian = Lagrangian(geometry, update_every=update_every, **(lagrangian or {}))
        self.nut = self.cs2 = None

    @property
    def n_evaluations(self):
        return self.lagrangian.n_evaluations

    @property
    def n_updates(self):
        return self.lagrangian.n_updates

    def assemble_first(self, dt, nu):
        plain = self.F
        self.F = _FormsWithLagrangianNut(plain, self, dt)
        try:
            O.OracleFractionalStep.assemble_first(self, dt, nu)
        finally:
            self.F = plain


def step_model(F, x_v, x_q, geometry, update_every=1, nu=0.01, dt=0.005, solver_options=None, low_memory=True,
               lagrangian=None):
    """dynamic_model.tg_step_model around a ``LagrangianOracleStep``: the (steady) Dirichlet values of ``input_field`` on
    the box's boundary."""
    d = F.d
    bd = O.boundary_dofs(x_v, F.coords.min(axis=0), F.coords.max(axis=0))
    bcs_u = [[O.DirichletData(bd, (lambda x, i=i: input_field(np.asarray(x)[:d].T, d)[:, i]))] for i in range(d)]
    return LagrangianOracleStep(F, x_v, x_q, bcs_u, solver_options=solver_options, low_memory=low_memory,
                                geometry=geometry, update_every=update_every, lagrangian=lagrangian)


# ---- the inputs the host and the GPU tests share ------------------------------------------------------------------------
DRIFT = (0.21, -0.13, 0.17)


def input_field(x_v, d):
    """The wave (2-D) / shear (3-D) field of section 26 plus a small drift: on the symmetric lattices the patch mean of
    the plain fields vanishes exactly in one component at some vertices, which puts their departure points on a facet."""
    return DM.field("wave" if d == 2 else "shear", x_v, d) + np.array(DRIFT)[:d]


def periodic_field(x_v, d):
    """A field of period 2 along every axis with a mean flow, at the points x_v (n, d) -> (n, d)."""
    x = np.zeros((x_v.shape[0], 3))
    x[:, :d] = x_v
    return np.stack([(0.9 - 0.5 * i) * (1.0 + 0.4 * np.sin(np.pi * x[:, 0] + 0.5 + i))
                     * (1.0 + 0.3 * np.cos(np.pi * x[:, 1] + 1.0 + 0.2 * i)) * (1.0 + 0.3 * np.sin(np.pi * x[:, 2] + 0.7 * i))
                     for i in range(d)], axis=1)


def channel_field(x_v, d):
    """Period 2 along x (and z), sheared across y: the input of the channel that is periodic in x only."""
    x = np.zeros((x_v.shape[0], 3))
    x[:, :d] = x_v
    return np.stack([np.sin(1.3 * x[:, 1] + 1.1 * i + 2.0) * (1.0 + 0.4 * np.sin(np.pi * x[:, 0] + 0.5 + i)
                                                             + 0.3 * np.cos(np.pi * x[:, 2] + 0.2 * i)) for i in range(d)],
                    axis=1)


def walled_dt(geo, u_v, fraction=0.45):
    """The step at which max |u_v| h is ``fraction`` (< 1/2) of the smallest cell altitude: a path line that starts at an
    interior vertex then ends inside that vertex's patch."""
    return fraction * float(geo.altitude.min()) / float(np.sqrt((u_v ** 2).sum(axis=1)).max())


def mesh_geometry(mesh, cells=None, cell_ids=None, tol=1e-10):
    """(Geometry, vertex classes or None) of an oasisx_amd mesh; ``cells`` / ``cell_ids``: the cells in another order (the
    kernels') and the mesh cell id of every position."""
    coords = mesh.coords.cpu().numpy()
    cells = mesh.cells.cpu().numpy().astype(np.int64) if cells is None else np.asarray(cells, dtype=np.int64)
    per = getattr(mesh, "periodic", None)

    class _F:  # what dynamic_model.Patches reads of a Forms object
        pass

    f = _F()
    f.cells, f.d = cells, coords.shape[1]
    xc = coords[cells]
    f.adet = np.abs(np.linalg.det(xc[:, 1:] - xc[:, :1]))
    if per is None:
        P = DM.Patches(f)
        return Geometry(coords, cells, P, cell_ids=cell_ids, tol=tol), None
    vt = np.asarray(per.vertex_topo)
    vm = np.asarray(per.vertex_master)
    P = DM.Patches(f, vertex_class=vt)
    free = np.nonzero(vm == np.arange(vm.shape[0]))[0]
    periodic = (tuple(per.axes), np.asarray(per.lo, dtype=np.float64), np.asarray(per.hi, dtype=np.float64),
                np.asarray(per.period, dtype=np.float64))
    return Geometry(coords, cells, P, x_v=coords[free], cell_ids=cell_ids, periodic=periodic, tol=tol), vt
