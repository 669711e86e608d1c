"""GPU: slab-averaged running statistics (oasisx_amd.ProfileStatistics, ox_profile_cells / ox_profile_update of
csrc/ox_diag.hip) against the extended-precision reference of tests/profile_model.py, which tests/test_profile_host.py pins
to closed forms.  The reference is fed the device's own numbering, geometry records and field blocks.  Cases, meshes and
the perturbed Taylor-Green field are those of tests/test_gpu_viscosity.py.

Observed on one MI355X: chunk rows and bin sums use at most 0.33 of their allowance (n + 2) on the six elements and 0.21
at the chunk boundaries; means and second moments of the recurrence at most 0.03 u B of allowances of 87 to 1001; with
1e6 added to u the second moments are within 3.1e-10 (2-D P2) and 2.6e-10 (3-D P1) of the two-pass value."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.test_gpu_diagnostics import DT, NU, _setup  # noqa: E402
from tests.test_gpu_viscosity import CASES  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bins_in_kernel_order(P, S):
    return P._bins[S._Vi[0][0].local_cells.cpu().numpy()]


def _chunk_labels(P, n_cells):
    """The chunk of every cell (kernel order), -1 for cells that are not sampled, from the device's own tables, which
    profile_model.chunk_labels checks on the way."""
    from tests import profile_model as PM

    assert P._chunks.shape == (P.n_chunks, 4) and P._bin_chunk_ptr.shape == (P.n_bins + 1,)
    return PM.chunk_labels(P._order.cpu().numpy(), P._chunks.cpu().numpy(), P._bin_chunk_ptr.cpu().numpy(), n_cells)


def _launch_once(P, g, shift):
    """One ox_profile_cells / ox_profile_update pair of the group ``g`` about ``shift`` into scratch arrays: (chunk
    partial rows, bin sums [V, S1, S2], mean, m2, vol) on the host."""
    import torch

    nr = 1 + g.nq + g.nv
    dev = P._vol.device
    sums = torch.full((P.n_bins, nr), -7.0, dtype=torch.float64, device=dev)
    mean = torch.zeros((P.n_bins, g.nq), dtype=torch.float64, device=dev)
    m2 = torch.zeros((P.n_bins, g.nv), dtype=torch.float64, device=dev)
    vol = torch.zeros(P.n_bins, dtype=torch.float64, device=dev)
    sh = None if shift is None else torch.from_numpy(np.ascontiguousarray(shift)).to(dev)
    P._launch(g, g.sources, sh, 1.0, 0.0, False, mean, m2, vol, sums)
    torch.cuda.synchronize()
    rows = P._partials.reshape(-1)[: P.n_chunks * nr].reshape(P.n_chunks, nr).cpu().numpy().copy()
    return rows, sums.cpu().numpy(), mean.cpu().numpy(), m2.cpu().numpy(), vol.cpu().numpy()


def _values(g):
    """The joint vector of a group as the device holds it, (n, nq) on the host."""
    cols = []
    for k, (st, col) in enumerate(g.sources):
        nc = g.members[0][2] if k == 0 else 1
        cols.append(st.rhost()[:, col:col + nc])
    return np.concatenate(cols, axis=1)


def _within(dev, val, B, n):
    """The criterion of tests/assembly_model.py without its cap on n (the sums over a whole mesh exceed it, as in
    test_ring_reduction): (ok, largest ratio / allowance)."""
    from tests import assembly_model as AM

    r = AM.ratio(dev, val, B) / (np.asarray(n, dtype=np.float64) + 2.0)
    return bool((r <= 1.0).all()), float(np.nanmax(r)) if r.size else 0.0


# ---- 1. partial rows and bin sums ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lattice", "delaunay"])
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_partial_rows_and_bin_sums_match_the_model(hip, dim, N, deg, kind):
    """After one launch pair about a nonzero shift: every chunk row and every bin's V, S1, S2 against the model under
    (n + 2) u B, n = the per-cell count + the cells summed - 1; for u (NQ = d, the velocity space) and p (NQ = 1, the
    pressure space).  sum_b V_b is the volume of the box under the same bound, n = the count of vol + all cells - 1."""
    import oasisx_amd as ox
    from tests import assembly_model as AM
    from tests import profile_model as PM

    S, _, mesh = _setup(dim, N, deg, kind)
    kw = dict(axis=1) if kind == "lattice" else dict(axis=1, edges=np.linspace(-1.0, 1.0, 4))
    P = ox.ProfileStatistics(S, fields=("u", "p"), **kw)
    assert P.n_bins == (N if kind == "lattice" else 3) and [g.nq for g in P._groups] == [dim, 1]
    assert P.n_sampled == int(mesh.num_cells) and np.allclose(P.coordinates(), 0.5 * (P.edges[1:] + P.edges[:-1]))
    geo = AM.geometry_from_records(S._geom.cpu().numpy())
    nc = int(S._geom.shape[0])
    bins = _bins_in_kernel_order(P, S)
    lab = _chunk_labels(P, nc)
    for g in P._groups:
        slabs = PM.Slabs(geo, g.cell_dofs.cpu().numpy(), g.degree, bins, P.n_bins)
        q = _values(g)
        shift = 0.05 + 0.1 * np.arange(P.n_bins)[:, None] - 0.07 * np.arange(g.nq)[None, :]
        rows, sums, _, _, vol = _launch_once(P, g, shift)
        for what, dev, (val, B, n) in (("chunk rows", rows, slabs.sums(q, shift, lab, P.n_chunks)),
                                       ("bin sums", sums, slabs.sums(q, shift))):
            ok, r, allow = AM.check(dev, val, B, n)
            print(f"{kind} ({dim},{N},{deg}) nq {g.nq} {what}: |dev - value| / (u B) = {r:.2f} of {allow:.0f}")
            assert ok, (what, r, allow)
        assert np.array_equal(vol, sums[:, 0])
        total = float(np.sum(vol.astype(np.longdouble)))
        allow = (PM.chain("vol", dim, g.degree) + nc - 1 + 2) * PM.U * total
        print(f"    sum V_b - |box| = {total - 2.0 ** dim:.3e}, allowed {allow:.3e}")
        assert abs(total - 2.0 ** dim) <= allow


# ---- 2. chunk boundaries -------------------------------------------------------------------------------------------------
def _mixed_bins(nc):
    """Bins of 1, 255, 256 and 257 cells, some cells left out, the rest in a fifth bin -- scattered over the mesh."""
    rng = np.random.default_rng(11)
    perm = rng.permutation(nc)
    b = np.full(nc, 4, dtype=np.int64)
    at = 0
    for k, size in enumerate((1, 255, 256, 257)):
        b[perm[at:at + size]] = k
        at += size
    b[perm[at:at + 300]] = -1
    return b


@pytest.mark.parametrize("N,layout,chunks", [(6, "one", 1), (12, "one", 2), (192, "one", 288), (6, "holes", 1),
                                             (192, "mixed", 1 + 1 + 1 + 2 + 284)])
def test_chunk_boundaries(hip, N, layout, chunks):
    """cell_bins on the 2-D P1 lattices of test_ring_reduction (72 / 288 / 73 728 cells): one partly filled chunk, two
    chunks, 288 chunk rows in one bin (a lane of the update takes several), bins of 1 / 255 / 256 / 257 cells and cells at
    -1, which reach no sum.  Bin sums under the forward bound (n + 2) u B, n = per-cell count + cells - 1.  With one bin,
    V (1/2) (tr cov + |mean|^2) of one sample is the kinetic energy of FlowDiagnostics within the sum of the two bounds."""
    import oasisx_amd as ox
    from tests import assembly_model as AM
    from tests import diagnostics_model as DM
    from tests import profile_model as PM

    S, _, mesh = _setup(2, N, 1)
    ncm = int(mesh.num_cells)
    assert ncm == {6: 72, 12: 288, 192: 73728}[N]
    if layout == "one":
        cb = np.zeros(ncm, dtype=np.int64)
    elif layout == "holes":
        cb = np.zeros(ncm, dtype=np.int64)
        cb[[0, 5, 17, 40, 71]] = -1
    else:
        cb = _mixed_bins(ncm)
    P = ox.ProfileStatistics(S, cell_bins=cb, fields=("u",))
    assert P.n_chunks == chunks and P.n_bins == int(cb.max()) + 1 and P.n_sampled == int((cb >= 0).sum())
    assert P.coordinates() is None and P.edges is None
    ptr = P._bin_chunk_ptr.cpu().numpy()
    if layout == "mixed":
        assert np.diff(ptr).tolist() == [1, 1, 1, 2, 284]
    geo = AM.geometry_from_records(S._geom.cpu().numpy())
    bins = _bins_in_kernel_order(P, S)
    lab = _chunk_labels(P, int(S._geom.shape[0]))
    assert np.array_equal(lab >= 0, bins >= 0)
    g = P._groups[0]
    slabs = PM.Slabs(geo, g.cell_dofs.cpu().numpy(), g.degree, bins, P.n_bins)
    q = _values(g)
    shift = np.full((P.n_bins, 2), 0.125)
    rows, sums, _, _, vol = _launch_once(P, g, shift)
    for what, dev, (val, B, n) in (("chunk rows", rows, slabs.sums(q, shift, lab, P.n_chunks)), ("bin sums", sums, slabs.sums(q, shift))):
        ok, r = _within(dev, val, B, n)
        print(f"N {N} {layout} {what}: largest |dev - value| / ((n + 2) u B) = {r:.3f}, n up to {int(n.max())}")
        assert ok, (what, r)
    left_out = float(np.sum(AM.to_f64(geo.adet)[bins < 0])) / 2.0
    assert abs(float(vol.sum()) - (4.0 - left_out)) <= (int(S._geom.shape[0]) + 4) * PM.U * 4.0 and (left_out > 0) == (layout != "one")
    if P.n_bins == 1:
        P.sample(0.5)
        D = ox.FlowDiagnostics(S)
        D.sample(0.0, DT, NU)
        ke_ring = float(D.latest().cpu().numpy()[1])
        r = PM.recurrence(slabs, [q], [0.5])
        V = float(P.volume().cpu().numpy()[0])
        mean, cov = P.mean("u").cpu().numpy()[0].astype(np.longdouble), P.covariance("u").cpu().numpy()[0].astype(np.longdouble)
        ke_prof = np.longdouble(V) * (cov[0] + cov[2] + mean[0] ** 2 + mean[1] ** 2) / 2
        # the bounds: the ring's, any tree over the cells' ke; the profile's, its counted bounds carried through the formula
        _, Bk, nk = DM.cell_integrals(geo, g.cell_dofs.cpu().numpy(), 1, q, NU)
        sel = bins >= 0
        b_ring = (nk[1] + int(sel.sum()) - 1 + 2) * PM.U * float(Bk[sel, 1].sum())
        Bm, Bc, W = r["Bm"][0], r["Bc"][0] / r["W"], r["W"]
        absm = np.abs(AM.to_f64(r["mean"][0]))
        b_prof = 0.5 * V * PM.U * ((r["n_cov"] + 3) * (Bc[0] + Bc[2]) + 2.0 * (r["n_mean"] + 2) * float((absm * Bm).sum())
                                   + (int(sel.sum()) + 8) * (Bc[0] + Bc[2] + float((Bm * Bm).sum())))
        print(f"    ke: ring {ke_ring:.15e}, profile {float(ke_prof):.15e}, |d| = {abs(float(ke_prof - ke_ring)):.3e}, "
              f"bounds {b_ring:.3e} + {b_prof:.3e}")
        assert layout != "one" or abs(float(ke_prof - ke_ring)) <= b_ring + b_prof
        if layout == "holes":  # the ring sums every cell: the profile's energy is smaller by the cells left out
            assert float(ke_prof) < ke_ring


# ---- 3. the recurrence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N,deg", [(2, 5, 2), (3, 3, 1)])
def test_profile_statistics_object(hip, dim, N, deg, tmp_path):
    """K = 12 levels with DM.STAT_WEIGHTS written into u, p and, in 2-D, two scalars of equal diffusivity, which share ONE
    storage block of two columns (asserted): in the joint vector they are further sources read with stride 2, the second
    from an address one column in; in a second object without "u" each stands alone, a source 0 whose stride is not its
    width.  Means and M2 of every group against the extended recurrence under its counted bound; flux() and tke() are
    entries of the joint covariance; save after six samples, load, carry on: the bits of the uninterrupted run; reset();
    with 1e6 added to u the covariance is within 1e-8 of the extended two-pass value, relative to its largest entry."""
    import torch

    import oasisx_amd as ox
    from oracle import ipcs_oracle as O
    from tests import assembly_model as AM
    from tests import diagnostics_model as DM
    from tests import profile_model as PM
    from tests import test_gpu_viscosity as V

    kw = dict(scalars=[ox.ScalarTransport("T", diffusivity=0.1), ox.ScalarTransport("C", diffusivity=0.1)]) if dim == 2 else {}
    S, _, _ = V._problem(dim, N, deg, None, nu=NU, dt=DT, **kw)
    names = ("T", "C") if dim == 2 else ()
    P = ox.ProfileStatistics(S, axis=1, scalars=names)
    assert P.names == ("u",) + names + ("p",) and [g.nq for g in P._groups] == [dim + len(names), 1] and P.n_bins == N
    with pytest.raises(RuntimeError, match="ProfileStatistics"):
        P.mean("u")
    alone = None
    if names:
        st = S.scalar("T")._storage
        assert S.scalar("C")._storage is st and st.nc == 2 and (S.scalar("T")._comp, S.scalar("C")._comp) == (0, 1)
        addr, ld = P._source_args(P._groups[0].sources)
        base = st.rdev().data_ptr()
        assert ld == [dim, 2, 2] and addr[1:] == [base, base + 8] and addr[0] == S._U.rdev().data_ptr()
        alone = ox.ProfileStatistics(S, axis=1, fields=(), scalars=names)
        assert [g.nq for g in alone._groups] == [1, 1]
        assert [alone._source_args(g.sources) for g in alone._groups] == [([base], [2]), ([base + 8], [2])]
    ws = DM.STAT_WEIGHTS
    K = len(ws)
    levels = [[], []]
    half = None
    for k, w in enumerate(ws):
        t = 0.05 * k + 0.01 * k * k
        for i, f in enumerate([O.tg_u, O.tg_v, O.tg_w][:dim]):
            S._u[i].interpolate(V._perturbed(f, i, t, NU, 0.3))
        S._p.interpolate(lambda x: O.tg_p(x, t, NU) + 0.1 * np.sin(x[0] + 30.0 * t))
        for j, s in enumerate(names):
            S.scalar(s).interpolate(lambda x: np.cos(x[0] * (j + 1) + 20.0 * t) + x[1])
        P.sample(w)
        if alone is not None:
            alone.sample(w)
        for g, lv in zip(P._groups, levels):
            lv.append(_values(g))
        if k == 5:
            P.save(tmp_path / "half.npz")
            half = ox.ProfileStatistics.load(S, tmp_path / "half.npz")
            assert half.total_weight == P.total_weight and half.n_samples == 6 and np.array_equal(half.edges, P.edges)
        elif k > 5:
            half.sample(w)
    assert P.total_weight == sum(ws) and P.n_samples == K
    geo = AM.geometry_from_records(S._geom.cpu().numpy())
    bins = _bins_in_kernel_order(P, S)
    for g, xs, h in zip(P._groups, levels, half._groups):
        slabs = PM.Slabs(geo, g.cell_dofs.cpu().numpy(), g.degree, bins, P.n_bins)
        r = PM.recurrence(slabs, xs, ws)
        for name, dev, val, B, n in (("mean", g.mean, r["mean"], r["Bm"], r["n_mean"]), ("m2", g.m2, r["m2"], r["Bc"], r["n_cov"])):
            ok, ratio, allow = AM.check(dev.cpu().numpy(), val, B, np.full(B.shape, n))
            print(f"({dim},{N},{deg}) nq {g.nq} {name}: |dev - value| / (u B) = {ratio:.2f} of {allow:.0f}")
            assert ok, (name, ratio, allow)
        assert torch.equal(h.mean, g.mean) and torch.equal(h.m2, g.m2)  # the restart
        vol = P.volume().cpu().numpy()
        ok, ratio, allow = AM.check(vol, r["vol"], AM.to_f64(r["vol"]), np.full(vol.shape, PM.chain("vol", dim, g.degree) + (bins == 0).sum() - 1))
        assert ok, ("vol", ratio, allow)
    assert torch.equal(half.volume(), P.volume())
    for j, g in enumerate(alone._groups if alone is not None else ()):  # each scalar alone: column j of the shared block
        slabs = PM.Slabs(geo, g.cell_dofs.cpu().numpy(), g.degree, bins, P.n_bins)
        r = PM.recurrence(slabs, [x[:, dim + j:dim + j + 1] for x in levels[0]], ws)
        for name, dev, val, B, n in (("mean", g.mean, r["mean"], r["Bm"], r["n_mean"]), ("m2", g.m2, r["m2"], r["Bc"], r["n_cov"])):
            ok, ratio, allow = AM.check(dev.cpu().numpy(), val, B, np.full(B.shape, n))
            print(f"({dim},{N},{deg}) {names[j]} alone, {name}: |dev - value| / (u B) = {ratio:.2f} of {allow:.0f}")
            assert ok, (names[j], name, ratio, allow)
        assert not torch.equal(g.mean, alone._groups[1 - j].mean)  # (the two columns hold different fields)
    # the surface
    J = P.joint_covariance("u")
    nq = dim + len(names)
    tri = [(i, j) for i in range(nq) for j in range(i, nq)]
    assert J.shape == (N, len(tri)) and torch.equal(J, P._groups[0].m2 / P.total_weight)
    cu = P.covariance("u")
    assert torch.equal(cu, J[:, [tri.index((i, j)) for i in range(dim) for j in range(i, dim)]])
    diag = [tri.index((i, i)) for i in range(dim)]
    trace = J[:, diag[0]].clone()
    for m in diag[1:]:
        trace = trace + J[:, m]
    assert torch.equal(P.tke(), 0.5 * trace)
    assert float(P.tke().min()) > 0.0 and P.mean("u").shape == (N, dim) and P.mean("p").shape == (N, 1)
    assert torch.equal(P.variance("p"), P.covariance("p")[:, 0]) and float(P.variance("p").min()) > 0.0
    for j, s in enumerate(names):
        assert torch.equal(P.flux(s), J[:, [tri.index((i, dim + j)) for i in range(dim)]]) and P.flux(s).shape == (N, dim)
        assert torch.equal(P.variance(s), J[:, tri.index((dim + j, dim + j))]) and P.mean(s).shape == (N, 1)
    with pytest.raises(ValueError, match="ProfileStatistics"):
        P.flux("p")
    with pytest.raises(ValueError, match="ProfileStatistics"):
        P.variance("u")
    # reset
    P.reset()
    assert P.total_weight == 0.0 and P.n_samples == 0 and not bool(P._groups[0].m2.any())
    with pytest.raises(RuntimeError, match="ProfileStatistics"):
        P.covariance("u")
    # a mean flow of 1e6: the seeded first sample keeps the variance
    B6 = ox.ProfileStatistics(S, axis=1, fields=("u",))
    xo = [x[:, :dim] + 1.0e6 for x in levels[0]]
    for x, w in zip(xo, ws):
        S._U.host()[:, :] = x
        B6.sample(w)
    g = B6._groups[0]
    slabs = PM.Slabs(geo, g.cell_dofs.cpu().numpy(), g.degree, bins, N)
    ref = AM.to_f64(PM.two_pass(slabs, xo, ws)[1])
    rel = (np.abs(g.m2.cpu().numpy() - ref).max(axis=0) / np.abs(ref).max(axis=0)).max()
    print(f"({dim},{N},{deg}) mean 1e6: relative error of the second moments {rel:.2e}")
    assert rel <= 1e-8


# ---- 4. periodic ---------------------------------------------------------------------------------------------------------
def test_periodic_channel_profiles(hip):
    """make_periodic(create_box N = 4, axes (0, 2)), P2-P1, walls in y: the bin sums against the model on the reduced
    numbering; the same field moved by one cell along the periodic axis x (a permutation of the dof values) gives the
    same sums up to the two summation bounds."""
    import oasisx_amd as ox
    from oasisx_amd import mesh as M
    from tests import assembly_model as AM
    from tests import profile_model as PM
    from tests.helpers import KRYLOV

    L, Wd, N = 3.0, 2.0, 4
    mesh = M.make_periodic(M.create_box(None, [[0.0, -1.0, 0.0], [L, 1.0, Wd]], [N, N, N]), (0, 2))
    walls = lambda x: np.isclose(np.abs(x[1]), 1.0)  # noqa: E731
    noslip = [[ox.DirichletBC(0.0, ox.LocatorMethod.GEOMETRICAL, walls)] for _ in range(3)]
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_u=noslip, bcs_p=[], solver_options=KRYLOV)
    kx, kz = 2.0 * np.pi / L, 2.0 * np.pi / Wd
    for i in range(3):
        S._u[i].interpolate(lambda x, i=i: (1.0 - x[1] ** 2) * (1.0 + 0.5 * i + np.sin(kx * x[0] + 0.4 * i) * np.cos(kz * x[2]))
                            + 0.2 * x[1] * np.cos(2.0 * kx * x[0] + i))
    P = ox.ProfileStatistics(S, axis=1, fields=("u",))
    assert P.n_bins == N and P.n_sampled == 6 * N ** 3
    Vi = S._Vi[0][0]
    assert Vi.num_dofs < (2 * N + 1) ** 3  # the reduced numbering
    geo = AM.geometry_from_records(S._geom.cpu().numpy())
    bins = _bins_in_kernel_order(P, S)
    g = P._groups[0]
    slabs = PM.Slabs(geo, g.cell_dofs.cpu().numpy(), 2, bins, N)
    U0 = S._U.rhost().copy()
    shift = np.full((N, 3), 0.25)
    _, sums0, _, _, _ = _launch_once(P, g, shift)
    val, B, n = slabs.sums(U0, shift)
    ok, r, allow = AM.check(sums0, val, B, n)
    print(f"periodic: |dev - value| / (u B) = {r:.2f} of {allow:.0f}")
    assert ok, (r, allow)
    # move the field by one cell along x: the dof at x + h (mod L) takes the value of the dof at x
    X = Vi.x.cpu().numpy()[: U0.shape[0]]
    h = L / N

    def key(x):
        t = x[:, 0] / L
        t = t - np.floor(t + 1e-9)
        s = x[:, 2] / Wd
        s = s - np.floor(s + 1e-9)
        return np.round(np.stack([t * 2 * N, (x[:, 1] + 1.0) * N, s * 2 * N], axis=1)).astype(np.int64) % np.array([2 * N, 10 ** 6, 2 * N])

    k0 = key(X)
    Xs = X.copy()
    Xs[:, 0] += h
    k1 = key(Xs)
    code = lambda k: (k[:, 0] * (2 * N + 1) + k[:, 1]) * (2 * N) + k[:, 2]  # noqa: E731
    c0, c1 = code(k0), code(k1)
    assert np.unique(c0).shape[0] == c0.shape[0]
    srt = np.argsort(c0)
    target = srt[np.searchsorted(c0[srt], c1)]
    assert np.array_equal(c0[target], c1) and np.array_equal(np.sort(target), np.arange(c0.shape[0]))
    U1 = np.empty_like(U0)
    U1[target] = U0
    assert not np.array_equal(U1, U0)
    S._U.host()[:, :] = U1
    _, sums1, _, _, _ = _launch_once(P, g, shift)
    ok, r = _within(sums1, AM.ext(sums0), 2.0 * B, n)
    print(f"periodic, moved by one cell: |d sums| / (2 (n + 2) u B) = {r:.3f}")
    assert ok, r


# ---- 5. invisible and reproducible ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N,deg", [(2, 5, 2), (3, 3, 1)])
def test_samples_are_reproducible_and_invisible_to_the_step(hip, dim, N, deg):
    """Two identical runs of (sample, step, sample, step) give equal bits in the profile state and in u, p; a run without
    sampling gives the same u, p; sample() and slab_mean() leave the write stamps of the solver's blocks and the running
    state as they were."""
    import torch

    import oasisx_amd as ox
    from oasisx_amd.fem import Function
    from tests import test_gpu_viscosity as V

    out = []
    for sampling in (True, True, False):
        S, clock, _ = V._problem(dim, N, deg, None, nu=0.01, dt=0.005)
        state = None
        if sampling:
            P, T = ox.ProfileStatistics(S, axis=1), ox.FlowStatistics(S)
            for b in (S._U, S._U1, S._U2, S._P):
                b.rdev()
            stamps = [b.generation for b in (S._U, S._U1, S._U2, S._P)]
        for k in (1, 2):
            if sampling:
                P.sample(0.005)
                T.sample(0.005)
                if k == 1:
                    assert stamps == [b.generation for b in (S._U, S._U1, S._U2, S._P)]
            clock["t"] = 0.005 * k
            S.solve(0.005, 0.01, max_iter=1)
        if sampling:
            before = [t.clone() for g in P._groups for t in (g.mean, g.m2)] + [P._vol.clone()]
            sm = P.slab_mean(T.mean("u"))
            sp = P.slab_mean(T.mean("p"))
            s0 = P.slab_mean(S._u[0])
            # one component read out of the block (source 0 with a stride that is not its width) is that column of the
            # blocked slab mean, bit for bit: the same sums in the same order
            sb = P.slab_mean(S.u)
            for i in range(dim):
                assert torch.equal(P.slab_mean(S._u[i])[:, 0], sb[:, i])
                assert torch.equal(P.slab_mean(Function(S._Vi[0][0], "c", T.mean("u")._storage, i))[:, 0], sm[:, i])
            after = [t for g in P._groups for t in (g.mean, g.m2)] + [P._vol]
            assert all(torch.equal(a, b) for a, b in zip(before, after))
            assert sm.shape == (N, dim) and sp.shape == (N, 1) and s0.shape == (N, 1)
            # the slab mean of the time mean is the time mean of the slab means (both linear): the two ways agree
            assert torch.allclose(sm, P.mean("u"), rtol=0.0, atol=1e-13) and torch.allclose(sp, P.mean("p"), rtol=0.0, atol=1e-13)
            state = before + [sm, sp]
        out.append((S._U.rdev().clone(), S._P.rdev().clone(), state))
    for a, b in ((0, 1), (0, 2)):
        assert torch.equal(out[a][0], out[b][0]) and torch.equal(out[a][1], out[b][1])
    assert all(torch.equal(a, b) for a, b in zip(out[0][2], out[1][2]))


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    import oasisx_amd as ox
    from oasisx_amd.parallel import Comm
    from tests import test_gpu_viscosity as V

    S, _, mesh = V._problem(2, 4, 2, None, scalars=[ox.ScalarTransport(n, diffusivity=0.1) for n in ("A", "B", "C")])
    nc = int(mesh.num_cells)
    with pytest.raises(ValueError, match="ProfileStatistics.*exactly one"):
        ox.ProfileStatistics(S)
    with pytest.raises(ValueError, match="ProfileStatistics.*exactly one"):
        ox.ProfileStatistics(S, axis=1, cell_bins=np.zeros(nc, dtype=np.int64))
    with pytest.raises(ValueError, match="ProfileStatistics: unknown field 'w'"):
        ox.ProfileStatistics(S, axis=1, fields=("u", "w"))
    with pytest.raises(ValueError, match="ProfileStatistics: 3 scalars"):
        ox.ProfileStatistics(S, axis=1, scalars=("A", "B", "C"))
    with pytest.raises(ValueError, match="ProfileStatistics: no scalar named"):
        ox.ProfileStatistics(S, axis=1, scalars=("Z",))
    with pytest.raises(ValueError, match="ProfileStatistics: cell_bins"):
        ox.ProfileStatistics(S, cell_bins=np.zeros(nc + 1, dtype=np.int64))
    with pytest.raises(ValueError, match="ProfileStatistics: bin 1 holds no cell"):
        ox.ProfileStatistics(S, cell_bins=np.where(np.arange(nc) < 3, 2, 0))
    with pytest.raises(ValueError, match="dt"):
        ox.ProfileStatistics(S, axis=1).sample(0.0)
    ok = ox.ProfileStatistics(S, axis=0, fields=("p",), scalars=("A", "B"))  # without u every scalar stands alone
    assert [g.nq for g in ok._groups] == [1, 1, 1]
    with pytest.raises(ValueError, match="ProfileStatistics.flux"):
        ok.flux("A")
    comm = mesh.comm
    try:
        mesh.comm = Comm(0, 2, None, transport="host")
        with pytest.raises(NotImplementedError, match=r"ProfileStatistics.*comm.size > 1"):
            ox.ProfileStatistics(S, axis=1)
    finally:
        mesh.comm = comm


# ---- 7. the demo ---------------------------------------------------------------------------------------------------------
def test_demo_runs_in_a_fresh_process(hip):
    """demo/channel_profiles_hip.py at N = 4 in a child process: the profile of u_x is the slab means of the parabola
    and the Reynolds stresses vanish, both within the tolerance the demo prints."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "demo", "channel_profiles_hip.py"), "-N", "4", "--steps", "200",
                        "--samples", "5"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    m = re.search(r"max \|<u_x> - parabola\| / peak = (\S+) \(tolerance (\S+)\)", r.stdout)
    s = re.search(r"largest Reynolds stress .* = (\S+) \(tolerance (\S+)\)", r.stdout)
    assert m and s, r.stdout[-2000:]
    assert float(m.group(1)) <= float(m.group(2)) <= 1e-6 and float(s.group(1)) <= float(s.group(2)) <= 1e-6
    rows = [ln.split() for ln in r.stdout.splitlines() if re.match(r"\s*-?0\.\d+\s", ln)]
    assert len(rows) == 4 and all(float(c[1]) > 0.0 for c in rows)
    assert "4 slabs along y" in r.stdout and "over 5 samples" in r.stdout
