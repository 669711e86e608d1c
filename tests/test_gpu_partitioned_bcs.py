"""GPU: pressure outlets (``PressureBC``), boundaries located through mesh tags and the rotational pressure update on the
rank-local data of a mesh partition, and the serial combination of the three against the oracle.

Rank by rank, no collectives (the pattern of tests/test_gpu_partition.py): one process builds the serial channel of
tests/channel_problem.py, then the channel of every rank in turn on a bare rank/size communicator -- no halo plan exists,
no thread waits on another -- and holds the owned rows of every operator and vector, and what the conditions do to ghost
entries, to the serial run through the dof coordinates.  The bounds are those of tests/test_gpu_partition.py for the same
kind of comparison (matrices 1e-12 max|ref|, vectors 1e-11 max|ref|: the same cell terms summed in another order); whatever
a condition writes -- identity rows, zeroed columns, ``b2`` on outlet dofs, the term of a rank without outlet facets -- is
exact."""
import numpy as np
import pytest

from tests import channel_problem as CP

pytestmark = pytest.mark.gpu

MAT, VEC = 1e-12, 1e-11


# ---- 1. the serial combination PressureBC + rotational=True against the oracle ---------------------------------------------
@pytest.mark.parametrize("kind,N", [("rect", 8), ("box", 4)])
def test_serial_outlet_with_the_rotational_form_against_the_oracle(hip, kind, N):
    """Two whole ``solve()`` steps of the P2-P1 channel with an outlet AND the rotational pressure update -- tested apart
    so far (test_gpu_parity: rotational without outlets; test_gpu_pressure_bc: outlets without it).  Bounds: those of
    ``test_tentative_with_outlet`` for its fields after a step."""
    prob = CP.build(kind, N, None, (2, 1), "float", True, rotational=True)
    R = CP.oracle_twin(prob)
    CP.run_steps(prob, 2, twin=R)
    S, dim = prob.S, prob.dim
    u = S.u.x.array.reshape(-1, dim)
    du, dp = float(np.abs(u - R.u).max()), float(np.abs(S._p.x.array - R.p).max())
    print(f"\n{kind} {N}: max|u - oracle| = {du:.3e} (max|u| = {np.abs(R.u).max():.3f}), max|p - oracle| = {dp:.3e} "
          f"(max|p| = {np.abs(R.p).max():.3f})")
    assert np.abs(R.u).max() > 0.5 and np.abs(R.p).max() > 1.0
    assert du < 1e-8 and dp < 1e-7


# ---- 2. rank by rank ---------------------------------------------------------------------------------------------------------
def _smooth(dim):
    return lambda x: np.sin(1.3 * x[0] + 0.2) * np.cos(0.7 * x[1]) + 0.4 * x[dim - 1] ** 2 + 0.25


def _collect(prob):
    """Everything the checks read of one solver (serial or one rank's), on the host."""
    import torch

    from oasisx_amd import fem
    from oasisx_amd.la import SellMatrix

    S, dim, bcp = prob.S, prob.dim, prob.bcp
    Vi, Q = S._Vi[0][0], S._Q
    out = {"xu": Vi.x.cpu().numpy(), "xq": Q.x.cpu().numpy(), "no": int(Vi.n_owned), "nqo": int(Q.n_owned)}
    out["surf"] = np.stack([bcp.surface_vector_host(i) for i in range(dim)], axis=1)
    prob.clock["t"] = 0.25  # the inlet moves: its values are re-evaluated at the LOCAL dof coordinates
    for bcl in S._bcs_u:
        for bc in bcl:
            bc.update_bc()
    S.assemble_first(CP.DT, CP.NU)
    S.velocity_tentative_assemble()
    out["A"] = S._A.to_scipy()
    out["bfirst"] = S._BFIRST.dev().cpu().numpy().copy()
    for i in range(dim):
        for bc in S._bcs_u[i]:
            bc.apply(S._rhs1[i].x)
    out["rhs1"] = S._RHS1.dev().cpu().numpy().copy()
    S._B2.dev().fill_(7.0)  # what the kernels do not write stays 7: the outlet's ghost entries must be WRITTEN, to 0
    S.pressure_assemble(CP.DT)
    out["b2"] = S._B2.dev().cpu().numpy()[:, 0].copy()
    out["Ap"] = S._Ap.to_scipy()
    Kq = SellMatrix(Q.pattern, symmetric=True, name="Kq")  # the pressure Laplacian before the outlet's rows and columns go
    S._assemble_matrix(1, Q, Kq)
    out["Kq"] = Kq.to_scipy()
    # the frozen Ap's product, default storage levels and the plain stream plus the value codes (7)
    x = fem.Function(Q, "x")
    x.interpolate(_smooth(dim))
    xd = x._storage.dev()
    ys = []
    for levels in (None, 7):
        S._Ap.set_levels(levels)
        y = torch.full((Q.n_local, 1), 3.0, dtype=torch.float64, device=xd.device)
        S._Ap.mult(xd, y, 1)
        ys.append(y[: Q.n_owned, 0].cpu().numpy().copy())
    S._Ap.set_levels(None)
    out["x"], out["Apx"], out["Apx7"] = xd[:, 0].cpu().numpy().copy(), ys[0], ys[1]
    out["Ap_frozen"] = S._Ap.vcode is not None
    # the rotational update's linear form on the interpolated p, dp, u (it uses the block of b2 as its work space)
    S._nu = CP.NU
    assert S._projector_p._function.s is S
    S._projector_p._function.assemble_rhs_into(S._projector_p._B)
    out["rot"] = S._projector_p._B.dev().cpu().numpy()[:, 0].copy()
    torch.cuda.synchronize()
    return out


CASES = [  # kind, N, (u, p) degree, ranks, a rank without outlet facets exists
    ("box", 4, (2, 1), 8, True),
    ("box", 4, (2, 1), 3, False),
    ("rect", 8, (2, 1), 4, True),
    ("box", 5, (1, 1), 2, False),
    ("box", 3, (3, 2), 2, False),
    ("delaunay", 4, (2, 1), 8, True),
]
PARAMS = [c + (h, True) for c in CASES for h in ("float", "callable")] + [CASES[0] + ("float", False)]


@pytest.mark.parametrize("kind,N,degrees,P,has_empty,h,low_memory", PARAMS)
def test_owned_rows_of_the_partitioned_channel_match_serial(hip, kind, N, degrees, P, has_empty, h, low_memory):
    """On every rank of the partition:

    1. the outlet term ``int h n_i dv/dx_i ds`` of every component: owned rows equal the serial ones (a facet of a
       ghost-layer cell is seen by several ranks and must count once per row), ghost rows hold nothing, and a rank without
       outlet facets gets exactly zero;
    2. ``A`` (identity rows on the topologically located Dirichlet dofs), ``b_first`` and ``rhs1`` after ``bc.apply`` with
       the clock moved (owned AND ghost Dirichlet entries: the inlet is evaluated at local coordinates);
    3. ``Ap`` entry by entry: every entry in an outlet column, ghost column or not, is exactly 0 but the 1 on the diagonal
       of an owned outlet row;
    4. the product of the frozen ``Ap``: bit-identical between storage levels, equal to ``Ap.to_scipy() @ x``;
    5. ``b2``: exactly 0 on every outlet dof, owned and ghost;
    6. the linear form of the rotational update.

    The case's own edges are asserted, not assumed: a rank without outlet facets (where the cut allows one), a rank with
    ghost outlet dofs, facets seen by more than one rank, and the owned outlet dofs adding up to the serial count."""
    dim = 2 if kind == "rect" else 3
    Gp = CP.build(kind, N, None, degrees, h, low_memory, rotational=True)
    g = _collect(Gp)
    tu, tq = CP.lookup(g["xu"]), CP.lookup(g["xq"])
    n_out_serial = int(np.isclose(g["xq"][:, 0], 1.0).sum())
    assert sorted(Gp.bcp._dofs.tolist()) == np.nonzero(np.isclose(g["xq"][:, 0], 1.0))[0].tolist()
    assert Gp.bcp._n_facets == Gp.outlet.shape[0] > 0
    frozen = kind != "delaunay" and degrees[1] == 1  # the P1 operator of a lattice mesh carries the value dictionary
    assert g["Ap_frozen"] or not frozen
    scale = {k: float(np.abs(g[k]).max()) for k in ("surf", "bfirst", "rhs1", "b2", "rot", "Apx")}
    scale["A"], scale["Ap"] = float(abs(g["A"]).max()), float(abs(g["Ap"]).max())
    assert min(scale.values()) > 1e-3, scale
    facets, owned_out, ghost_out, owned_u, ghost_cols, live_ghost_cols = [], [], [], 0, 0, 0
    for r in range(P):
        Sp = CP.build(kind, N, CP.FakeComm(r, P), degrees, h, low_memory, rotational=True)
        S, bcp = Sp.S, Sp.bcp
        Vi, Q = S._Vi[0][0], S._Q
        assert Vi.n_local > Vi.n_owned > 0 and Q.n_local > Q.n_owned > 0
        s = _collect(Sp)
        no, nqo = s["no"], s["nqo"]
        owned_u += no
        iu, iq = CP.to_serial(tu, s["xu"]), CP.to_serial(tq, s["xq"])
        # the outlet's facets and dofs, independently of the product: from the coordinates
        cells = Sp.mesh.cells[Vi.local_cells].cpu().numpy()
        on_plane = np.isclose(Sp.mesh.coords.cpu().numpy()[:, 0], 1.0)
        n_f = int((on_plane[cells].sum(axis=1) == dim).sum())
        out_q = np.isclose(s["xq"][:, 0], 1.0)
        assert bcp._n_facets == n_f and sorted(bcp._dofs.tolist()) == np.nonzero(out_q)[0].tolist()
        facets.append(n_f)
        owned_out.append(int(out_q[:nqo].sum()))
        ghost_out.append(int(out_q[nqo:].sum()))
        # 1. surface vectors
        assert s["surf"].shape == (Vi.n_local, dim)
        assert np.abs(s["surf"][:no] - g["surf"][iu[:no]]).max() <= VEC * scale["surf"], r
        assert (s["surf"][no:] == 0.0).all(), r  # rows exist for owned dofs only
        if n_f == 0:
            assert (s["surf"] == 0.0).all() and bcp._S == [], r
        # 2. the tentative system
        loc = s["A"].tocoo()
        assert np.abs(loc.data - np.asarray(g["A"][iu[loc.row], iu[loc.col]]).ravel()).max() <= MAT * scale["A"], r
        assert s["A"].nnz == g["A"][iu[:no]].nnz
        xu = s["xu"]
        dirichlet = np.isclose(xu[:, 0], -1.0) | np.isclose(np.abs(xu[:, 1:]), 1.0).any(axis=1)  # inlet and walls
        rows_d = dirichlet[loc.row]
        assert dirichlet[:no].any() and (loc.data[rows_d] == (loc.row == loc.col)[rows_d].astype(float)).all(), r
        assert np.abs(s["bfirst"][:no] - g["bfirst"][iu[:no]]).max() <= VEC * scale["bfirst"], r
        assert np.abs(s["rhs1"][:no] - g["rhs1"][iu[:no]]).max() <= VEC * scale["rhs1"], r
        assert np.abs(s["rhs1"][dirichlet] - g["rhs1"][iu[dirichlet]]).max() <= VEC * scale["rhs1"], r  # ghosts too
        # 3. Ap entry by entry
        loc = s["Ap"].tocoo()
        assert s["Ap"].shape == (nqo, Q.n_local)
        assert np.abs(loc.data - np.asarray(g["Ap"][iq[loc.row], iq[loc.col]]).ravel()).max() <= MAT * scale["Ap"], r
        assert s["Ap"].nnz == g["Ap"][iq[:nqo]].nnz
        touched = out_q[loc.row] | out_q[loc.col]
        diag = (loc.row == loc.col) & out_q[loc.row]
        assert (loc.data[touched & ~diag] == 0.0).all() and (loc.data[diag] == 1.0).all(), r
        assert int(diag.sum()) == owned_out[-1]
        raw = s["Kq"].tocoo()  # (the same pattern in the same order)
        assert (raw.row == loc.row).all() and (raw.col == loc.col).all() and (loc.data[~touched] == raw.data[~touched]).all(), r
        in_ghost_col = out_q[loc.col] & (loc.col >= nqo) & ~out_q[loc.row]
        ghost_cols += int(in_ghost_col.sum())
        live_ghost_cols += int((in_ghost_col & (raw.data != 0.0)).sum())
        # 4. the frozen Ap's product
        assert s["Ap_frozen"] or not frozen
        assert (s["Apx"] == s["Apx7"]).all(), r
        host = s["Ap"] @ s["x"]
        assert np.abs(s["Apx"] - host).max() <= VEC * scale["Apx"], r
        assert np.abs(s["Apx"] - g["Apx"][iq[:nqo]]).max() <= VEC * scale["Apx"], r
        # 5. b2
        assert (s["b2"][out_q] == 0.0).all(), r
        assert np.abs(s["b2"][:nqo] - g["b2"][iq[:nqo]]).max() <= VEC * scale["b2"], r
        # 6. the rotational update's right-hand side
        assert np.abs(s["rot"][:nqo] - g["rot"][iq[:nqo]]).max() <= VEC * scale["rot"], r
    print(f"\n{kind} N={N} P{degrees[0]}-P{degrees[1]} on {P} ranks, h {h}: outlet facets per rank {facets} (mesh: "
          f"{Gp.outlet.shape[0]}), owned outlet dofs {owned_out} (serial: {n_out_serial}), ghost outlet dofs {ghost_out}, "
          f"entries of owned rows in ghost outlet columns {ghost_cols}, nonzero before the condition {live_ghost_cols}")
    assert owned_u == Gp.S._Vi[0][0].num_dofs
    assert sum(owned_out) == n_out_serial
    assert max(ghost_out) > 0 and ghost_cols > 0
    # (P2-P1 on the lattice meshes cut along lattice planes: a ghost outlet column of a P1 row outside the outlet belongs to a
    # diagonal of the lattice, whose stiffness entry is zero anyway; every other case has columns that would show if they stayed)
    assert live_ghost_cols > 0 or (kind != "delaunay" and degrees == (2, 1))
    assert sum(facets) > Gp.outlet.shape[0]  # facets of ghost-layer cells are seen by more than one rank
    assert (min(facets) == 0) == has_empty
    if (kind, N, P) == ("box", 4, 8):  # the figures of the 2 x 2 x 2 split
        assert [f == 0 for f in facets] == [True, False] * 4 and sum(facets) == 48
        assert all(gh >= 5 for gh, f in zip(ghost_out, facets) if f) and all(o == 0 for o, f in zip(owned_out, facets) if not f)


@pytest.mark.parametrize("kind,N,P", [("box", 4, 8), ("rect", 8, 4)])
def test_projector_with_a_tagged_dirichlet_condition_on_partitioned_spaces(hip, kind, N, P):
    """``Projector(f, V, bcs=[DirichletBC(g, TOPOLOGICAL, (tags, walls))])`` on the partitioned P1 and P2 spaces of the
    channel: the right-hand side after the lifting through the unconstrained matrix (a product over owned and ghost
    columns of the Dirichlet values) and the constrained matrix, owned rows against the serial ones."""
    import torch

    import oasisx_amd as ox
    from oasisx_amd.function import Projector
    from tests.helpers import KRYLOV

    dim = 2 if kind == "rect" else 3
    f, gval = _smooth(dim), (lambda x: 1.0 + x[0] * x[1] - 0.5 * x[dim - 1])

    def project(prob, V):
        bc = ox.DirichletBC(gval, ox.LocatorMethod.TOPOLOGICAL, (prob.tags, CP.WALLS))
        proj = Projector(f, V, bcs=[bc], petsc_options=KRYLOV["scalar"])
        proj.assemble_rhs()
        torch.cuda.synchronize()
        return proj._A.to_scipy(), proj._B.dev().cpu().numpy()[:, 0].copy(), V.x.cpu().numpy(), int(V.n_owned)

    def spaces(prob):
        return {1: prob.S._Q, 2: prob.S._Vi[0][0]}

    Gp = CP.build(kind, N, None, (2, 1), "float", True, fields=False)
    ref = {deg: project(Gp, V) for deg, V in spaces(Gp).items()}
    for r in range(P):
        Sp = CP.build(kind, N, CP.FakeComm(r, P), (2, 1), "float", True, fields=False)
        for deg, V in spaces(Sp).items():
            Ag, Bg, xg, _ = ref[deg]
            A, B, x, no = project(Sp, V)
            assert V.n_local > no
            ix = CP.to_serial(CP.lookup(xg), x)
            walls = np.isclose(np.abs(x[:, 1:]), 1.0).any(axis=1)
            assert walls[:no].any() or r > 0
            assert np.abs(B[:no] - Bg[ix[:no]]).max() <= VEC * np.abs(Bg).max(), (deg, r)
            X = np.zeros((3, x.shape[0]))
            X[:dim] = x.T
            assert (B[walls] == gval(X)[walls]).all(), (deg, r)  # the Dirichlet values, owned and ghost entries
            loc = A.tocoo()
            assert np.abs(loc.data - np.asarray(Ag[ix[loc.row], ix[loc.col]]).ravel()).max() <= MAT * abs(Ag).max(), (deg, r)
            assert A.nnz == Ag[ix[:no]].nnz
            touched = walls[loc.row] | walls[loc.col]
            diag = (loc.row == loc.col) & walls[loc.row]
            assert (loc.data[touched & ~diag] == 0.0).all() and (loc.data[diag] == 1.0).all(), (deg, r)
            assert int(diag.sum()) == int(walls[:no].sum())


# ---- 4. features that refuse partitions refuse at construction, before any collective ----------------------------------------
class _NoCollectives(CP.FakeComm):
    """Rank 0 of 2: any collective call is an error (a rank that refuses must not have entered one before)."""

    def allreduce(self, v, op=None):
        raise AssertionError("a collective was entered before the feature refused the partition")

    Barrier = _all_ok = allreduce


REFUSALS = ["scalars", "viscosity_model", "resistance", "windkessel", "backflow", "WallStress", "ScalarFlux", "FlowRate",
            "FlowDiagnostics", "FlowStatistics", "Tracers"]


@pytest.mark.parametrize("feature", REFUSALS)
def test_one_gpu_features_refuse_a_partition_at_construction(hip, feature):
    import oasisx_amd as ox

    comm = _NoCollectives(0, 2)
    mesh = CP.make_mesh("rect", 4, comm)
    tags, *_ = CP.make_tags(mesh)
    clock = {"t": 0.0}

    def solver(bcs_p=(), **kw):
        from tests.helpers import KRYLOV

        return ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_u=CP.velocity_bcs(tags, 2, clock),
                                       bcs_p=list(bcs_p), solver_options=KRYLOV, options={"sell_window": 128}, **kw)

    in_constructor = {
        "scalars": lambda: solver(scalars=[ox.ScalarTransport("T", diffusivity=0.1)]),
        "viscosity_model": lambda: solver(viscosity_model=ox.Smagorinsky()),
        "resistance": lambda: solver([ox.PressureBC(ox.Resistance(1.0), (tags, CP.OUTLET))]),
        "windkessel": lambda: solver([ox.PressureBC(ox.Windkessel(1.0, 0.5, 2.0), (tags, CP.OUTLET))]),
        "backflow": lambda: solver([ox.PressureBC(4.0, (tags, CP.OUTLET), backflow=0.5)]),
    }
    if feature in in_constructor:
        with pytest.raises(NotImplementedError, match="partition"):
            in_constructor[feature]()
        return
    # attached to a solver: the solver of rank 0 of 2 itself is built without a collective (the volume's all-reduce aside)
    comm.allreduce = lambda v, op=None: v
    S = solver([ox.PressureBC(4.0, (tags, CP.OUTLET))])
    del comm.allreduce
    assert S._Vi[0][0].part is not None
    attach = {
        "WallStress": lambda: ox.WallStress(S, (tags, CP.WALLS)),
        "ScalarFlux": lambda: ox.ScalarFlux(S, "T", (tags, CP.WALLS)),
        "FlowRate": lambda: ox.FlowRate(S, (tags, CP.OUTLET)),
        "FlowDiagnostics": lambda: ox.FlowDiagnostics(S),
        "FlowStatistics": lambda: ox.FlowStatistics(S),
        "Tracers": lambda: ox.Tracers(S, np.zeros((4, 3))),
    }
    with pytest.raises(NotImplementedError, match="partition"):
        attach[feature]()
