"""GPU: Lagrangian tracers (``ox_tracer_advance``, csrc/ox_probe.hip) in a constant velocity field on the meshes of
tests/hard_meshes.py, against the closed form ``x0 + t v`` under the counted bounds of tests/tracer_zoo.py -- through the
253-valent centre of the fan and the axis of the spindle, across slivers and cells of both orientations, at 1e-3 per unit
time a kilometre from the origin.

The chain (tracer_zoo's docstring derives it): per completed substep and axis, u (max |x_k| + (3 D + 8) h |v_k|) -- one
rounding of the update on |x|, the partition of unity in D + 1 fmas and the D subtractions behind lambda_0 on |v|, four
fmas of the stage sum, two roundings of the step length; n substeps add.  The bound is of the order of 1e-15 on the
fan and 1e-11 on the 2-D slivers (|x| = 1e4), not 1e-12.  Every located point of every closed-form path is decided
(asserted here on the host), so status, exit time and the substep a particle freezes in must be the model's."""
import numpy as np
import pytest

from tests import assembly_model as AM
from tests import locator_model as LM
from tests import tracer_zoo as TZ

pytestmark = pytest.mark.gpu


def _field(C):
    from oasisx_amd import fem
    from oasisx_amd import mesh as M

    mesh = M.from_arrays(C["points"], C["cells"])
    V = fem.FunctionSpace(mesh, 1, window=256)
    w = fem.Function(fem.VectorFunctionSpace(V, C["d"]))
    w._storage.host()[:, :] = C["v"][None, :]  # a constant: exact in P1
    w._storage.rdev()
    return mesh, w


def _err(dev, val):
    return AM.to_f64(AM.absx(AM.ext(np.asarray(dev, dtype=np.float64)) - val))


@pytest.mark.parametrize("d,name", [c for c in TZ.CASES if c[1] != "tiny_far"])
def test_the_hint_and_the_search_agree_within_the_tolerance_band(hip, d, name):
    """The hint accepts its cell at lambda >= 0, the search at lambda >= -tol.  Seeds half a tolerance OUTSIDE an exterior
    facet (decided: the search must find them) in a field at rest: the end point of every substep is the seed itself, the
    hint refuses it, the search takes it -- the particle stays alive in the model's cell, with and without the hint, and
    does not move by a bit.  (Not on tiny_far: float64 cannot place a point there, tests/locator_model.py.)"""
    import oasisx_amd as ox

    C = dict(TZ.case(d, name), v=np.zeros(d))
    mesh, w = _field(C)
    coords, cells = mesh.coords.cpu().numpy(), mesh.cells.cpu().numpy()
    classes = LM.point_classes(coords, cells, seed=d)
    P = classes["within_tol"]
    x0 = np.concatenate([P["x"], classes["vertex"]["x"]])  # (the vertices: lambda = 0 to rounding, the other edge of the band)
    want = np.concatenate([P["cell"], classes["vertex"]["cell"]])
    assert P["dropped"] == 0 and P["x"].shape[0] >= 24 and (P["lam"].min(axis=1) < -0.1 * LM.TOL).all()
    for scheme in TZ.SCHEMES:
        for hint in (True, False):
            T = ox.Tracers(w, x0, scheme=scheme, substeps=3, hint=hint, sort_every=0)
            T.advance(0.25)
            T.advance(0.25)
            assert (T.status() == 0).all() and np.array_equal(T.positions(), x0) and np.array_equal(T.cells(), want), (scheme, hint)
            assert (T.path_length() == 0.0).all() and np.isnan(T.exit_time()).all()


@pytest.mark.parametrize("d,name", TZ.CASES)
def test_constant_field_on_the_zoo_follows_the_closed_form(hip, d, name):
    import oasisx_amd as ox

    C = TZ.case(d, name)
    mesh, w = _field(C)
    coords, cells = mesh.coords.cpu().numpy(), mesh.cells.cpu().numpy()
    x0 = C["seeds"]
    S0 = LM.locate(coords, cells, x0)
    assert S0["decided"].all() and (S0["cell"] >= 0).all()  # every seed has a cell, and the device must find it
    worst = {"x": 0.0, "age": 0.0, "path": 0.0}
    for m in TZ.SUBSTEPS:
        h = TZ.DT / m
        E = TZ.expectation(C, m)
        for scheme in TZ.SCHEMES:
            e = E[scheme]
            assert e["decided"].all(), (name, scheme, m, np.nonzero(~e["decided"])[0][:10])  # the host's side of the bargain
            gone = e["status"] == 1
            assert 10 <= gone.sum() <= x0.shape[0] - 100  # some leave, most stay
            bx, ba, bp = TZ.position_bound(C, h, e["n"]), TZ.age_bound(e["n"]), TZ.path_bound(C, h, e["n"])
            runs = {}
            for hint in (True, False):
                T = ox.Tracers(w, x0, scheme=scheme, substeps=m, hint=hint, sort_every=0)
                assert np.array_equal(T.cells(), S0["cell"])
                for _ in range(TZ.ADVANCES):
                    T.advance(TZ.DT)
                X, st, age, path, te, cell = T.positions(), T.status(), T.age(), T.path_length(), T.exit_time(), T.cells()
                runs[hint] = (X, cell)
                assert np.array_equal(st, e["status"]), (name, scheme, m, hint, np.nonzero(st != e["status"])[0][:10])
                assert np.array_equal(te, e["t_exit"], equal_nan=True), (name, scheme, m, hint)
                ex, ea, ep = _err(X, e["x"]), np.abs(age - e["age"]), np.abs(path - e["path"])
                with np.errstate(divide="ignore", invalid="ignore"):
                    rx = float(np.where(bx > 0, ex / bx, np.where(ex == 0, 0.0, np.inf)).max())
                    ra = float((ea / ba).max())
                    rp = float(np.where(bp > 0, ep / bp, np.where(ep == 0, 0.0, np.inf)).max())
                worst = {"x": max(worst["x"], rx), "age": max(worst["age"], ra), "path": max(worst["path"], rp)}
                assert rx <= 1.0 and ra <= 1.0 and rp <= 1.0, (name, scheme, m, hint, rx, ra, rp)
                assert np.array_equal(X[e["n"] == 0], x0[e["n"] == 0])  # frozen in the first substep: the seed itself
                assert (cell[gone] == -1).all() and (cell[~gone] >= 0).all() and (cell < mesh.num_cells).all()
                # the cached cell holds the end point (lambda* of the closed form there, within tolerance and bounds)
                lam, bnd = LM.bary_in_cells(coords, cells, AM.to_f64(e["x"])[~gone], cell[~gone], shift=2.0 * bx[~gone])
                assert (AM.to_f64(lam.min(axis=1)) >= -T.tol - bnd.max(axis=1)).all(), (name, scheme, m, hint)
                if not hint:  # the search: the model's lowest containing cell
                    assert np.array_equal(cell, e["cells_end"]), (name, scheme, m)
            # hint on and off: the same path within twice the bound; other cells only on shared facets (both cells hold
            # the end point, and it is within tolerance and bounds of a facet of the hinted one)
            (Xh, ch), (Xs, cs) = runs[True], runs[False]
            assert (np.abs(Xh - Xs) <= 2.0 * bx).all(), (name, scheme, m)
            diff = np.nonzero(ch != cs)[0]
            if diff.size:
                lam, bnd = LM.bary_in_cells(coords, cells, AM.to_f64(e["x"])[diff], ch[diff], shift=2.0 * bx[diff])
                assert (np.abs(AM.to_f64(lam.min(axis=1))) <= T.tol + bnd.max(axis=1)).all(), (name, scheme, m, diff[:10])
    print(f"RATIO tracers {d}-D {name}: worst |x - closed form| / bound = {worst['x']:.3f}, age {worst['age']:.3f}, path {worst['path']:.3f} "
          f"(allowance 1; the largest position bound {float(TZ.position_bound(C, TZ.DT / 4, np.full(x0.shape[0], 8)).max()):.2e})")
