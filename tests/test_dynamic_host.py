"""Host (no GPU): the numpy model of the dynamic Smagorinsky procedure (tests/dynamic_model.py) against the properties
the procedure must have, the conditions the GPU tests put on their input fields, and the construction-time guards and
the update_every bookkeeping of oasisx_amd.DynamicSmagorinsky."""
import numpy as np
import pytest

from tests import dynamic_model as DM
from tests import viscosity_model as VM

CASES = [(2, 6, 1), (2, 5, 2), (3, 3, 1), (3, 3, 2), (2, 4, 3), (3, 2, 3)]
# the ratio tests' inputs: (field, dim, N, deg)
RATIO_INPUTS = [("wave", 2, 6, 1), ("wave", 2, 5, 2), ("wave", 2, 4, 3), ("shear", 3, 3, 1), ("shear", 3, 3, 2),
                ("shear", 3, 2, 3)]
CLIP_INPUTS = [("shifted_tg", 2, 6, 1), ("shifted_tg", 2, 5, 2), ("shifted_tg", 2, 4, 3)]


def _setup(name, dim, N, deg):
    F = VM.tg_forms(dim, N, deg, 2 if deg == 3 else 1)
    return F, DM.field(name, F.x_v, dim), DM.Patches(F)


# ---- the filter --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,N,deg", CASES)
def test_filter_preserves_constants_with_positive_weights(dim, N, deg):
    F = VM.tg_forms(dim, N, deg, 2 if deg == 3 else 1)
    P = DM.Patches(F)
    nc = F.cells.shape[0]
    c = P.filter(np.full((nc, 2), [3.25, -7.5]))
    assert np.abs(c - [3.25, -7.5]).max() <= 8 * np.finfo(float).eps * 7.5
    W = P.weights()
    assert W.min() >= 0.0 and np.abs(W.sum(axis=1) - 1.0).max() <= 1e-14
    q = np.random.default_rng(3).standard_normal((nc, 3))
    assert np.abs(W @ q - P.filter(q)).max() <= 1e-14 * np.abs(q).max() * 8


@pytest.mark.parametrize("name,dim,N,deg", RATIO_INPUTS + CLIP_INPUTS)
def test_leonard_tensor_is_positive_semidefinite(name, dim, N, deg):
    """L = (u u^T)^ - u^ u^^T is a covariance under positive weights that sum to one."""
    F, u, P = _setup(name, dim, N, deg)
    L, Ld, M = DM.tensors(F, u, P)
    ev = np.linalg.eigvalsh(L)
    assert ev.min() >= -1e-14 * np.abs(u).max() ** 2
    assert np.abs(np.einsum("cii->c", Ld)).max() <= 1e-14 * np.abs(L).max()


# ---- invariances -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dim,N,deg", RATIO_INPUTS)
def test_scaling(name, dim, N, deg):
    """u -> a u: LM, MM -> a^4 ., Cs2 unchanged, nut -> a nut, to 1e-12 relative."""
    F, u, P = _setup(name, dim, N, deg)
    a = 1.7
    bins = DM.slab_bins_of(F, 1)
    for kw in ({}, {"bins": bins}, {"average": "local"}):
        n1, c1, i1 = DM.nut_cells(F, u, P, **kw)
        n2, c2, i2 = DM.nut_cells(F, a * u, P, **kw)
        assert np.abs(i2["LM"] - a ** 4 * i1["LM"]).max() <= 1e-12 * a ** 4 * np.abs(i1["LM"]).max()
        assert np.abs(i2["MM"] - a ** 4 * i1["MM"]).max() <= 1e-12 * a ** 4 * np.abs(i1["MM"]).max()
        assert np.abs(c2 - c1).max() <= 1e-12 * np.abs(c1).max()
        assert np.abs(n2 - a * n1).max() <= 1e-12 * a * np.abs(n1).max()


@pytest.mark.parametrize("name,dim,N,deg", RATIO_INPUTS)
def test_galilean_invariance(name, dim, N, deg):
    """u -> u + U, |U| ~ 3: LM unchanged within 1e-12 gdim max|u + U|^2 max|M| (the cancellation in (uu)^ - u^u^)."""
    F, u, P = _setup(name, dim, N, deg)
    U = np.array([2.0, -1.8, 1.3])[:dim]
    LM1, MM1 = DM.products(F, u, P)
    LM2, MM2 = DM.products(F, u + U, P)
    _, _, M = DM.tensors(F, u, P)
    bound = 1e-12 * dim * np.abs(u + U).max() ** 2 * np.abs(M).max()
    assert np.abs(LM2 - LM1).max() <= bound
    assert np.abs(MM2 - MM1).max() <= 1e-12 * np.abs(MM1).max()


@pytest.mark.parametrize("dim,N,deg", CASES)
def test_zero_field_and_nan(dim, N, deg):
    F, u, P = _setup("wave" if dim == 2 else "shear", dim, N, deg)
    for kw in ({}, {"bins": DM.slab_bins_of(F, 1)}, {"average": "local"}):
        nut, cs2, _ = DM.nut_cells(F, np.zeros_like(u), P, **kw)
        assert np.array_equal(nut, np.zeros_like(nut)) and np.array_equal(cs2, np.zeros_like(cs2))
        bad = u.copy()
        bad[F.vd[0, 0], 0] = np.nan
        nut, _, _ = DM.nut_cells(F, bad, P, **kw)
        assert np.isnan(nut[0])  # the clip does not turn a NaN into a number
        if kw.get("average") != "local":  # a NaN in one cell of a bin is a NaN in the whole bin
            b = kw.get("bins", np.zeros(nut.shape[0], dtype=np.int64))
            assert np.isnan(nut[b == b[0]]).all()


def test_clip_keeps_nan_and_zeroes_nonpositive_denominators():
    c = DM.clip(np.array([-1.0, 1.0, -1.0, np.nan, -1.0, 0.0, -1.0]), np.array([1.0, 1.0, 0.01, 1.0, np.nan, 0.0, -2.0]), 0.09)
    assert c[0] == 0.09 and c[1] == 0.0 and c[2] == 0.09 and np.isnan(c[3]) and np.isnan(c[4]) and c[5] == 0.0 and c[6] == 0.0
    assert DM.clip(np.array([-0.1]), np.array([1.0]), 0.09)[0] == 0.05


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------------
def test_symmetric_taylor_green_is_no_ratio_input():
    """On the symmetric Taylor-Green field the global sums cancel to rounding: kappa ~ 1e15."""
    F, u, P = _setup("tg", 2, 6, 1)
    _, info = DM.coefficient(F, u, P)
    assert info["kappa"][0] > 1e12


@pytest.mark.parametrize("name,dim,N,deg", RATIO_INPUTS)
def test_ratio_inputs_are_well_conditioned(name, dim, N, deg):
    """The conditions the GPU ratio tests rely on: kappa <= 100 per bin, a positive coefficient, and in local mode at
    least 30 % of the cells positive."""
    F, u, P = _setup(name, dim, N, deg)
    _, g = DM.coefficient(F, u, P)
    _, s = DM.coefficient(F, u, P, bins=DM.slab_bins_of(F, 1))
    cl, _ = DM.coefficient(F, u, P, average="local")
    print(f"{name} ({dim},{N},{deg}): global Cs2 {g['raw'][0]:.4f} kappa {g['kappa'][0]:.3g}; slabs "
          f"{np.round(s['raw'], 4)} kappa <= {s['kappa'].max():.3g}; local share {(cl > 0).mean():.2f}")
    assert g["kappa"][0] <= 100.0 and s["kappa"].max() <= 100.0
    assert g["raw"][0] > 0.0 and (s["raw"] > 0.0).all()
    assert (cl > 0.0).mean() >= 0.30


def test_model_reproduces_the_recorded_values():
    """Drift of the model shows here: the global Cs2 of the input fields, recorded to four decimals."""
    want = {("wave", 2, 6, 1): 0.054, ("wave", 2, 5, 2): 0.054, ("wave", 2, 4, 3): 0.048, ("shear", 3, 3, 1): 0.031,
            ("shear", 3, 3, 2): 0.023, ("shear", 3, 2, 3): 0.051, ("shifted_tg", 2, 6, 1): 0.0017,
            ("shifted_tg", 2, 5, 2): 0.0060, ("shifted_tg", 2, 4, 3): 0.0106}
    for key, v in want.items():
        F, u, P = _setup(*key)
        _, g = DM.coefficient(F, u, P)
        assert abs(g["raw"][0] - v) <= (5e-4 if v > 0.02 else 5e-5), (key, g["raw"][0])


@pytest.mark.parametrize("name,dim,N,deg", CLIP_INPUTS)
def test_clip_inputs_have_bins_on_both_sides(name, dim, N, deg):
    F, u, P = _setup(name, dim, N, deg)
    c, s = DM.coefficient(F, u, P, bins=DM.slab_bins_of(F, 1))
    assert (s["raw"] > 0.0).any() and (s["raw"] < 0.0).any() and s["kappa"].max() <= 100.0
    assert np.array_equal(s["clipped"] == 0.0, s["raw"] <= 0.0) and c.min() >= 0.0 and c.max() <= 0.09


@pytest.mark.parametrize("dim,N,deg", CASES)
def test_delaunay_inputs_are_well_conditioned(dim, N, deg):
    """The same conditions on the Delaunay meshes of the GPU tests (seed 2), with centroid bins along axis 1."""
    from oracle import ipcs_oracle as O
    from tests.helpers import delaunay_box_mesh

    pts, cells = delaunay_box_mesh(N, dim, seed=2)
    F = O.Forms(pts, cells, deg, 2 if deg == 3 else 1)
    u = DM.field("wave" if dim == 2 else "shear", F.x_v, dim)
    P = DM.Patches(F)
    _, g = DM.coefficient(F, u, P)
    _, s = DM.coefficient(F, u, P, bins=DM.slab_bins_of(F, 1, [-1.0, -0.3, 0.4, 1.0]))
    cl, _ = DM.coefficient(F, u, P, average="local")
    assert g["kappa"][0] <= 100.0 and s["kappa"].max() <= 100.0 and g["raw"][0] > 0.0 and (s["raw"] > 0.0).any()
    assert (cl > 0.0).mean() >= 0.30


def test_slab_bins_of_matches_the_package():
    import types

    import torch

    from oasisx_amd.diagnostics import slab_bins

    F = VM.tg_forms(3, 3, 1)
    mesh = types.SimpleNamespace(gdim=3, coords=torch.from_numpy(F.coords), cells=torch.from_numpy(F.cells))
    for axis in (0, 1, 2):
        assert np.array_equal(slab_bins(mesh, axis)[0], DM.slab_bins_of(F, axis))
    e = [-1.0, -0.2, 0.5, 0.9]
    assert np.array_equal(slab_bins(mesh, 1, edges=e)[0], DM.slab_bins_of(F, 1, edges=e))


# ---- update_every and the guards ---------------------------------------------------------------------------------------
def test_update_every_in_the_model():
    F = VM.tg_forms(2, 4, 2)
    R, rc = DM.tg_step_model(F, F.x_v, F.x_q, {}, update_every=2)
    seen = []
    for k in range(4):
        rc["t"] = (k + 1) * 0.005
        R.solve(0.005, 0.01, max_iter=1)
        seen.append((R.n_evaluations, R.n_updates))
    assert seen == [(1, 1), (2, 1), (3, 2), (4, 2)]


def test_guards_at_construction():
    import oasisx_amd as ox

    with pytest.raises(ValueError, match="local"):
        ox.DynamicSmagorinsky(average="local", axis=1)
    with pytest.raises(ValueError, match="local"):
        ox.DynamicSmagorinsky(average="local", cell_bins=np.zeros(4, dtype=np.int64))
    with pytest.raises(ValueError, match="at most one"):
        ox.DynamicSmagorinsky(axis=1, cell_bins=np.zeros(4, dtype=np.int64))
    with pytest.raises(ValueError, match="average"):
        ox.DynamicSmagorinsky(average="plane")
    for r in (1.0, 0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="filter_ratio"):
            ox.DynamicSmagorinsky(filter_ratio=r)
    for c in (-0.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cs2_max"):
            ox.DynamicSmagorinsky(cs2_max=c)
    for n in (0, -1, 1.5):
        with pytest.raises(ValueError, match="update_every"):
            ox.DynamicSmagorinsky(update_every=n)
    with pytest.raises(TypeError):
        ox.DynamicSmagorinsky(damping=ox.VanDriest())
    m = ox.DynamicSmagorinsky()
    assert m.diffuses_scalars and m.update_every == 1 and m.filter_ratio == 2.0 and m.cs2_max == 0.09
    with pytest.raises(RuntimeError):
        m.products()


def test_check_model_guards_before_the_library():
    """rotational, partitions, bins that do not fit the mesh and the TypeError text: check_model alone, no solver."""
    import oasisx_amd as ox
    from oasisx_amd.parallel import Comm
    from oasisx_amd.viscosity import check_model
    from tests.helpers import tg_mesh

    mesh = tg_mesh(2, 4)
    check_model(ox.DynamicSmagorinsky(), mesh, False, None)
    check_model(ox.DynamicSmagorinsky(axis=1), mesh, False, None)
    with pytest.raises(NotImplementedError, match="rotational"):
        check_model(ox.DynamicSmagorinsky(), mesh, True, None)
    with pytest.raises(ValueError, match="cell_bins"):
        check_model(ox.DynamicSmagorinsky(cell_bins=np.zeros(3, dtype=np.int64)), mesh, False, None)
    with pytest.raises(ValueError, match="holds no cell"):
        check_model(ox.DynamicSmagorinsky(axis=1, edges=[-1.0, 0.0, 1.0, 2.0]), mesh, False, None)
    with pytest.raises(ValueError, match="axis"):
        check_model(ox.DynamicSmagorinsky(axis=2), mesh, False, None)
    with pytest.raises(TypeError, match="DynamicSmagorinsky"):
        check_model(object(), mesh, False, None)
    pmesh = tg_mesh(2, 4)
    pmesh.comm = Comm(0, 2, None, transport="host")
    with pytest.raises(NotImplementedError, match="partition"):
        check_model(ox.DynamicSmagorinsky(), pmesh, False, None)
