"""GPU: flow diagnostics and running statistics (oasisx_amd/diagnostics.py, csrc/ox_diag.hip) against the reference of
tests/diagnostics_model.py, which tests/test_diagnostics_host.py pins to closed forms.  The reference is fed the device's
own numbering, geometry records and velocity block, so fields and integrals compare cell by cell.  Cases, meshes and the
perturbed Taylor-Green field (neither solenoidal nor symmetric) are those of tests/test_gpu_viscosity.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.test_gpu_viscosity import CASES  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, NU = 0.1, 0.5


def _setup(dim, N, deg, kind="lattice", model=None, **kw):
    """The problem of tests/test_gpu_viscosity.py with the perturbed field in the CURRENT velocity too (what a sample
    reads) and, with a model, ``nut`` evaluated once."""
    from oracle import ipcs_oracle as O
    from tests import test_gpu_viscosity as V

    mesh = V._delaunay(dim, N) if kind == "delaunay" else None
    S, clock, mesh = V._problem(dim, N, deg, model, nu=NU, dt=DT, mesh=mesh, perturb=0.3, **kw)
    for i, f in enumerate([O.tg_u, O.tg_v, O.tg_w][:dim]):
        S._u[i].interpolate(V._perturbed(f, i, 0.02, NU, 0.3))
    if model is not None:
        V._assemble_first(S, clock, DT, NU)
    return S, clock, mesh


def _reference(S, mesh):
    from tests import assembly_model as AM
    from tests import test_gpu_viscosity as V

    F, _, _ = V._forms(S, mesh)
    geo = AM.geometry_from_records(S._geom.cpu().numpy())
    return F, geo, S._Vi[0][0].cell_dofs.cpu().numpy(), S._U.rhost()


ALL_FIELDS = ("cfl", "shear_rate", "divergence", "q_criterion", "vorticity")


# ---- 1. centroid fields ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lattice", "delaunay"])
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_centroid_fields_match_the_model(hip, dim, N, deg, kind):
    """max |dev - model| <= 1e-12 scale (the bound of tests/test_gpu_viscosity.py): scale = max |model| for cfl, shear and
    the vorticity; max ||g||_F^2 for q and max ||g||_F for the divergence, which cancel.  cell_field() is the kernel-order
    array permuted by local_cells."""
    import oasisx_amd as ox
    from tests import diagnostics_model as DM

    S, _, mesh = _setup(dim, N, deg, kind)
    D = ox.FlowDiagnostics(S, fields=ALL_FIELDS)
    D.sample(0.0, DT, NU)
    F, _, _, u = _reference(S, mesh)
    ref = DM.centroid_fields(F, u, DT)
    dev = D._fields.cpu().numpy()
    g1 = ref["gnorm"].max()
    cmp = [("cfl", dev[:, 0], ref["cfl"], np.abs(ref["cfl"]).max()), ("shear", dev[:, 1], ref["shear"], ref["shear"].max()),
           ("divc", dev[:, 2], ref["divc"], g1), ("q", dev[:, 3], ref["q"], g1 * g1),
           ("omega", dev[:, 4:], ref["omega"], np.abs(ref["omega"]).max())]
    for name, a, b, scale in cmp:
        d = float(np.abs(a - b).max())
        print(f"{kind} ({dim},{N},{deg}) {name}: max |d| = {d:.3e}, scale {scale:.3e}, ratio {d / scale:.3e}")
        assert scale > 0.0 and d <= 1e-12 * scale, (name, d, scale)
    lc = S._Vi[0][0].local_cells.cpu().numpy()
    for k, name in enumerate(ALL_FIELDS):
        mo = D.cell_field(name).cpu().numpy()
        want = dev[:, 4:] if (name == "vorticity" and dim == 3) else dev[:, k]
        assert mo.shape[0] == int(mesh.num_cells) and np.array_equal(mo[lc], want), name


# ---- 2. cell integrals -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lattice", "delaunay"])
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_cell_integrals_entry_by_entry(hip, dim, N, deg, kind):
    """Each of the seven integrals per cell against the extended-precision model: |dev - value| <= (n + 2) 2^-53 B, n
    counted from the kernel (diagnostics_model.chain), n <= 1024."""
    import oasisx_amd as ox
    from tests import assembly_model as AM
    from tests import diagnostics_model as DM

    S, _, mesh = _setup(dim, N, deg, kind)
    D = ox.FlowDiagnostics(S, cell_integrals=True)
    D.sample(0.0, DT, NU)
    _, geo, vd, u = _reference(S, mesh)
    val, B, n = DM.cell_integrals(geo, vd, deg, u, NU)
    assert int(n.max()) <= 1024
    dev = D._cint.cpu().numpy()
    for k, name in enumerate(DM.COLUMNS):
        ok, r, allow = AM.check(dev[:, k], val[:, k], B[:, k], np.full(dev.shape[0], n[k]))
        print(f"{kind} ({dim},{N},{deg}) {name}: |dev - value| / (u B) = {r:.2f} of {allow:.0f}")
        assert ok, (name, r, allow)
    lc = S._Vi[0][0].local_cells.cpu().numpy()
    assert np.array_equal(D.cell_integrals().cpu().numpy()[lc], dev)


# ---- 3. the ring reduction ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N,deg,kind", [(2, 6, 1, "lattice"), (2, 12, 1, "lattice"), (2, 192, 1, "lattice"),
                                            (3, 3, 2, "delaunay")])
def test_ring_reduction(hip, dim, N, deg, kind):
    """The ring row against the extended-precision sum of the device's own cell integrals: <= (n_cells - 1) 2^-53 sum |v|
    (the forward bound of any summation tree); cfl_max is the maximum of the field, exactly.  72 cells (one partly filled
    block), 288 (two blocks, the second partly filled), 73 728 (288 partial rows: a lane of the second stage takes two),
    and tetrahedra.  On the lattice meshes the volume column is the volume of the box under the same bound."""
    import oasisx_amd as ox
    from tests import assembly_model as AM
    from tests import diagnostics_model as DM

    S, _, mesh = _setup(dim, N, deg, kind)
    D = ox.FlowDiagnostics(S, fields=("cfl",), cell_integrals=True, capacity=1)
    D.sample(0.0, DT, NU)
    D.sample(1.0, DT, NU)  # (the ring doubles)
    nc = D.n_cells
    assert nc == {6: 72, 12: 288, 192: 73728}.get(N, nc) and D.capacity == 2
    cint = D._cint.cpu().numpy()
    row = D.latest().cpu().numpy()
    tot, asum = DM.extended_sum(cint)
    for k in range(7):
        err = float(abs(AM.ext(row[k:k + 1])[0] - tot[k]))
        print(f"({dim},{N},{deg}) {DM.COLUMNS[k]}: |ring - sum| = {err:.3e}, bound {(nc - 1) * DM.U * asum[k]:.3e}")
        assert err <= (nc - 1) * DM.U * asum[k], (DM.COLUMNS[k], err)
    cfl = D._fields[:, 0].cpu().numpy()
    assert row[7] == cfl.max() and row[7] > 0.0
    if kind == "lattice":
        assert abs(row[0] - 2.0 ** dim) <= (nc - 1) * DM.U * asum[0]
    h = D.history()
    assert h["t"].tolist() == [0.0, 1.0] and h["div_l2"][1] == np.sqrt(row[5]) and h["kinetic_energy"][0] == row[1]
    assert np.array_equal(D._ring[0].cpu().numpy(), row)  # equal state, equal bits


# ---- 4. with nut -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N,deg", [(2, 5, 2), (3, 3, 1), (3, 2, 3)])
def test_dissipation_uses_the_eddy_viscosity(hip, dim, N, deg):
    """Smagorinsky: diss per cell is (nu + S._nut[c]) strain2[c] to 2 ulp; without a model nu strain2, bitwise."""
    import oasisx_amd as ox

    for model in (ox.Smagorinsky(), None):
        S, _, _ = _setup(dim, N, deg, model=model)
        D = ox.FlowDiagnostics(S, cell_integrals=True)
        D.sample(0.0, DT, NU)
        c = D._cint.cpu().numpy()
        if model is None:
            assert np.array_equal(c[:, 3], NU * c[:, 2])
        else:
            nut = S._nut.cpu().numpy()
            ref = (NU + nut) * c[:, 2]
            assert nut.max() > 0.0 and (np.abs(c[:, 3] - ref) <= 2.0 * np.spacing(np.abs(ref))).all()
            assert (c[:, 3] > NU * c[:, 2]).any()


# ---- 5. NaN and reproducibility ----------------------------------------------------------------------------------------
def test_nan_shows_in_the_ring(hip):
    """One velocity dof of a scratch copy of the state set to NaN: cfl_max and the sums over u are NaN (the volume is
    not), where fmax would have returned the largest finite value."""
    import oasisx_amd as ox

    S, _, _ = _setup(2, 12, 2)  # a scratch state of its own: nothing else reads it
    D = ox.FlowDiagnostics(S, fields=("cfl",))
    D.sample(0.0, DT, NU)
    assert np.isfinite(D.latest().cpu().numpy()).all()
    S._U.host()[S._n_u // 2, 0] = np.nan
    D.sample(1.0, DT, NU)
    row = D.latest().cpu().numpy()
    assert np.isnan(row[7]) and np.isnan(row[[1, 2, 3, 4, 5, 6]]).all() and np.isfinite(row[0])
    cfl = D.cell_field("cfl").cpu().numpy()
    assert np.isnan(cfl).any() and np.isfinite(cfl).any()


@pytest.mark.parametrize("dim,N,deg", [(2, 5, 2), (3, 3, 1)])
def test_samples_are_reproducible_and_invisible_to_the_step(hip, dim, N, deg):
    """Two sample() calls on equal state give equal bits in ring and fields; sample() leaves the write stamps of the
    solver's blocks as they were; a solve after sampling gives the bits of a solve without."""
    import torch

    import oasisx_amd as ox
    from tests import test_gpu_viscosity as V

    out = []
    for sampling in (True, False):
        S, clock, _ = V._problem(dim, N, deg, None, nu=0.01, dt=0.005)
        if sampling:
            D, T = ox.FlowDiagnostics(S, fields=ALL_FIELDS, cell_integrals=True), ox.FlowStatistics(S)
            for b in (S._U, S._U1, S._U2, S._P):
                b.rdev()  # (the initial data was written on the host: the first device read of any kind copies it over)
            stamps = [b.generation for b in (S._U, S._U1, S._U2, S._P)]
            D.sample(0.0, 0.005, 0.01)
            f0 = D._fields.clone()
            D.sample(0.0, 0.005, 0.01)
            T.sample(0.005)
            assert torch.equal(D._ring[0], D._ring[1]) and torch.equal(f0, D._fields)
            assert stamps == [b.generation for b in (S._U, S._U1, S._U2, S._P)]
        clock["t"] = 0.005
        S.solve(0.005, 0.01, max_iter=1)
        out.append((S._U.rdev().clone(), S._P.rdev().clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ---- 6. statistics -----------------------------------------------------------------------------------------------------
def _accumulate(xs, ws, ncomp, strided=False):
    """ox_stats_accumulate over the levels; ``strided``: x is a column block of a wider, misaligned array."""
    import torch

    from oasisx_amd import _lib

    lib, st = _lib.load(), _lib.current_stream()
    n = xs[0].shape[0]
    mean = torch.full((n, ncomp), 7.0, dtype=torch.float64, device="cuda")  # (W = 0 overwrites whatever is there)
    cov = torch.full((n, ncomp * (ncomp + 1) // 2), -3.0, dtype=torch.float64, device="cuda")
    W = 0.0
    keep = []
    for x, w in zip(xs, ws):
        if strided:
            wide = torch.zeros((n, ncomp + 2), dtype=torch.float64, device="cuda")
            wide[:, 1:1 + ncomp] = torch.from_numpy(x).cuda()
            ptr, ldx = _lib.C.c_void_p(wide.data_ptr() + 8), ncomp + 2
        else:
            wide = torch.from_numpy(np.ascontiguousarray(x)).cuda()
            ptr, ldx = _lib.ptr(wide), ncomp
        keep.append(wide)
        _lib.check(lib.ox_stats_accumulate(ncomp, n, ptr, ldx, float(w), W, _lib.ptr(mean), _lib.ptr(cov), st), "ox_stats_accumulate")
        W += float(w)
    torch.cuda.synchronize()
    return mean.cpu().numpy(), cov.cpu().numpy()


@pytest.fixture(scope="module")
def stat_points():
    rng = np.random.default_rng(5)
    return rng.uniform(-1.0, 1.0, size=(3, 1037))  # n = 4 blocks + 13: not a multiple of the block, odd


@pytest.mark.parametrize("ncomp", [1, 2, 3])
def test_stats_kernel_against_the_extended_recurrence(hip, stat_points, ncomp):
    """K = 12 levels, unequal weights: mean and cov sums against the extended West recurrence under its running bound
    (c K + 2) 2^-53 B, c = 4 (mean), 9 (cov) counted in diagnostics_model; the strided instantiation gives the same bits.
    On a mean of 1e6 the covariance is within 1e-8 (relative to its largest entry) of the extended two-pass value -- raw
    sums would sit near 2e-4, West's update carries about 1e-9 (tests/test_diagnostics_host.py shows the gap on the CPU)."""
    from tests import assembly_model as AM
    from tests import diagnostics_model as DM

    ws = DM.STAT_WEIGHTS
    K = len(ws)
    xs = DM.stat_levels(stat_points, ncomp)
    mean, cov = _accumulate(xs, ws, ncomp)
    mx, cx, Bm, Bc = DM.west(xs, ws)
    rm = np.abs(AM.to_f64(mean.astype(np.longdouble) - mx)) / (DM.U * Bm)
    rc = np.abs(AM.to_f64(cov.astype(np.longdouble) - cx)) / (DM.U * Bc)
    print(f"ncomp {ncomp}: mean {rm.max():.2f} of {DM.C_MEAN * K + 2}, cov {rc.max():.2f} of {DM.C_COV * K + 2}")
    assert (rm <= DM.C_MEAN * K + 2).all() and (rc <= DM.C_COV * K + 2).all()
    ms, cs = _accumulate(xs, ws, ncomp, strided=True)
    assert np.array_equal(ms, mean) and np.array_equal(cs, cov)
    m1, c1 = _accumulate(xs[:1], ws[:1], ncomp)
    assert np.array_equal(m1, xs[0]) and not c1.any()  # W = 0: mean = x, cov = 0
    xo = DM.stat_levels(stat_points, ncomp, offset=1.0e6)
    _, co = _accumulate(xo, ws, ncomp)
    ref = AM.to_f64(DM.two_pass(xo, ws)[1])
    rel = (np.abs(co - ref).max(axis=0) / np.abs(ref).max(axis=0)).max()
    print(f"ncomp {ncomp}, mean 1e6: relative covariance error {rel:.2e}")
    assert rel <= 1e-8


@pytest.mark.parametrize("dim,N,deg", [(2, 5, 2), (3, 3, 1)])
def test_flow_statistics_object(hip, dim, N, deg, tmp_path):
    """FlowStatistics over K = 12 levels of u, p (and, in 2-D, two scalars that share a block: a strided read) written
    into the solver's fields: mean and covariance against the extended recurrence of the levels the device held;
    tke() == 1/2 tr covariance; save / load round trip bitwise, and sampling goes on after it; reset()."""
    import torch

    import oasisx_amd as ox
    from oracle import ipcs_oracle as O
    from tests import assembly_model as AM
    from tests import diagnostics_model as DM
    from tests import test_gpu_viscosity as V

    kw = dict(scalars=[ox.ScalarTransport("T", diffusivity=0.1), ox.ScalarTransport("C", diffusivity=0.2)]) if dim == 2 else {}
    S, _, _ = V._problem(dim, N, deg, None, nu=NU, dt=DT, **kw)
    names = ("T", "C") if dim == 2 else ()
    T = ox.FlowStatistics(S, scalars=names)
    ws = DM.STAT_WEIGHTS
    K = len(ws)
    levels = {k: [] for k in ("u", "p") + names}
    half = None
    for k, w in enumerate(ws):
        t = 0.05 * k + 0.01 * k * k
        for i, f in enumerate([O.tg_u, O.tg_v, O.tg_w][:dim]):
            S._u[i].interpolate(V._perturbed(f, i, t, NU, 0.3))
        S._p.interpolate(lambda x: O.tg_p(x, t, NU) + 0.1 * np.sin(x[0] + 30.0 * t))
        for j, s in enumerate(names):
            S.scalar(s).interpolate(lambda x: np.cos(x[0] * (j + 1) + 20.0 * t) + x[1])
        T.sample(w)
        levels["u"].append(S._U.rhost())
        levels["p"].append(S._P.rhost())
        for s in names:
            c = S.scalar(s)
            levels[s].append(c._storage.rhost()[:, c._comp:c._comp + 1])
        if k == 5:
            T.save(tmp_path / "half.npz")
            half = ox.FlowStatistics.load(S, tmp_path / "half.npz")
        elif k > 5:
            half.sample(w)
    assert T.total_weight == sum(ws) and T.n_samples == K
    assert S._n_u % 256 != 0
    for name, xs in levels.items():
        mx, cx, Bm, Bc = DM.west(xs, ws)
        mean = T.mean(name)._storage.rhost()
        cov = T._m[name].cov[: xs[0].shape[0]].cpu().numpy()
        rm = np.abs(AM.to_f64(mean.astype(np.longdouble) - mx)) / (DM.U * Bm)
        rc = np.abs(AM.to_f64(cov.astype(np.longdouble) - cx)) / (DM.U * Bc)
        print(f"{name}: mean {rm.max():.2f} of {DM.C_MEAN * K + 2}, cov {rc.max():.2f} of {DM.C_COV * K + 2}")
        assert (rm <= DM.C_MEAN * K + 2).all() and (rc <= DM.C_COV * K + 2).all(), name
        want = cov / T.total_weight  # (the device's division is not numpy's to the last bit: one ulp)
        assert (np.abs(T.covariance(name).cpu().numpy() - want) <= np.spacing(np.abs(want))).all()
        # the restart: statistics saved after six samples and carried on are the bits of the uninterrupted ones
        assert np.array_equal(half.mean(name)._storage.rhost(), mean)
        assert np.array_equal(half._m[name].cov.cpu().numpy(), T._m[name].cov.cpu().numpy())
    assert half.total_weight == T.total_weight
    cu = T.covariance("u")
    tr = cu[:, 0] + cu[:, 2] if dim == 2 else cu[:, 0] + cu[:, 3] + cu[:, 5]
    assert torch.equal(T.tke()._storage.rdev()[: S._n_u, 0], 0.5 * tr) and float(tr.min()) > 0.0
    assert torch.equal(T.variance("p"), T.covariance("p")[:, 0])
    T.save(tmp_path / "full.npz")
    L = ox.FlowStatistics.load(S, tmp_path / "full.npz")
    for name in levels:
        assert torch.equal(L._m[name].cov, T._m[name].cov) and torch.equal(L.mean(name)._storage.rdev(), T.mean(name)._storage.rdev())
    T.reset()
    assert T.total_weight == 0.0 and not bool(T._m["u"].cov.any())
    with pytest.raises(RuntimeError):
        T.mean("u")
    T.sample(0.25)
    assert np.array_equal(T.mean("u")._storage.rhost(), S._U.rhost())


# ---- 7. the surface ----------------------------------------------------------------------------------------------------
def test_means_and_cell_fields_can_be_written_and_evaluated(hip, tmp_path):
    """mean("u") goes through VTXWriter and Function.eval; write_cell_vtu -> read_vtu returns the cell arrays bitwise."""
    import oasisx_amd as ox

    S, _, mesh = _setup(2, 5, 2)
    T = ox.FlowStatistics(S)
    T.sample(0.5)
    um = T.mean("u")
    assert um.function_space is S._V
    with ox.io.VTXWriter(None, str(tmp_path / "mean.bp"), [um, T.tke()]) as w:
        w.write(0.5)
    back = ox.io.read_vtu(str(tmp_path / "mean_000000.vtu"))
    assert np.array_equal(back["point_data"]["mean_u"][:, :2], S._U.rhost())
    x = np.array([[0.1, -0.3, 0.0], [-0.7, 0.55, 0.0]])
    assert np.array_equal(um.eval(x), S.u.eval(x)) and np.isfinite(um.eval(x)).all()
    D = ox.FlowDiagnostics(S, fields=ALL_FIELDS, cell_integrals=True)
    D.sample(0.0, DT, NU)
    data = {n: D.cell_field(n) for n in ALL_FIELDS}
    data["energy"] = D.cell_integrals()[:, 1]
    ox.io.write_cell_vtu(str(tmp_path / "cells.vtu"), mesh, data, time=0.25)
    back = ox.io.read_vtu(str(tmp_path / "cells.vtu"))
    assert back["time"] == 0.25 and back["types"].tolist() == [5] * int(mesh.num_cells)
    assert np.array_equal(back["connectivity"].reshape(-1, 3), mesh.cells.cpu().numpy())
    for n, a in data.items():
        assert np.array_equal(back["cell_data"][n], a.cpu().numpy()), n
    D.save(tmp_path / "diag.npz")
    with np.load(tmp_path / "diag.npz") as z:
        assert np.array_equal(z["q_criterion"], data["q_criterion"].cpu().numpy()) and z["t"].tolist() == [0.0]
    with pytest.raises(ValueError):
        ox.io.write_cell_vtu(str(tmp_path / "bad.vtu"), mesh, {"x": np.zeros(3)})


def test_demo_runs_in_a_fresh_process(hip, tmp_path):
    """demo/turbulence_statistics_hip.py at N = 8 in a child process: it prints the table from the ring and writes the
    means, the TKE and the Q-criterion file."""
    import oasisx_amd as ox

    out = tmp_path / "stats"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "demo", "turbulence_statistics_hip.py"), "-N", "8", "--steps", "3",
                        "--out", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "-dissipation" in r.stdout and "max CFL" in r.stdout and "max TKE" in r.stdout
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.strip()[:1].isdigit()]
    assert [int(c[0]) for c in rows] == [1, 2, 3]
    e = [float(c[1]) for c in rows]
    assert all(b < a for a, b in zip(e, e[1:])) and all(float(c[3]) < 0.0 for c in rows)  # the energy decays; -diss < 0
    q = ox.io.read_vtu(str(out / "q_criterion.vtu"))
    assert set(q["cell_data"]) == {"q_criterion", "vorticity", "cfl", "nut"} and q["cell_data"]["vorticity"].shape[1] == 3
    assert np.isfinite(q["cell_data"]["q_criterion"]).all()
    m = ox.io.read_vtu(str(out / "mean_u_000000.vtu"))
    assert set(m["point_data"]) == {"mean_u", "tke"}
    with np.load(out / "statistics.npz") as z:
        assert float(z["total_weight"]) == pytest.approx(3 * 0.005)
