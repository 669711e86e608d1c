"""CPU: the scalar-row and SUPG-cell forms of the extended-precision model (tests/assembly_model.py: ``scalar_rows``,
``scalar_rows_cellvisc``, ``scalar_rows_supg``, ``supg_cells``) -- what tests/test_gpu_scalar_rows_entries.py holds the
device to.

* the forms against the float64 models the suite already has (tests/scalar_model.py, tests/scalar_les_model.py,
  tests/scalar_supg_model.py on ``oracle.ipcs_oracle.Forms``) on an ordinary lattice and on every zoo mesh, entry by entry
  under the criterion.  The oracle's results are rounded evaluations of the same sums (by chains no longer than the
  kernels'): they get the same bound once more as the allowance of a reference with errors of its own (P3: over the
  absolute tables widened by the measured error of the oracle's coefficient table), and ``10 u`` of the absolute sum
  ``|M|/dt + |C|/2 + ...`` for forming ``A`` and ``A_c`` in float64;
* identities of the model itself;
* the criterion can fail where ``1e-12 * max`` cannot: four mutations, each flagged;
* the input conditions of the device test (``UAB_SCALE`` of that file), on the model alone."""
import numpy as np
import pytest

from oracle import ipcs_oracle as O
from tests import assembly_model as AM
from tests import hard_meshes as H
from tests.scalar_les_model import ScalarLesModel
from tests.scalar_model import ScalarModel
from tests.scalar_supg_model import ScalarSupgModel
from tests.test_assembly_model_host import X_EPS, _oracle_and_model
from tests.test_gpu_scalar_rows_entries import PARAMS, SC_T, SHIFT, SUPG_FORMS, T_FACTOR, UAB_SCALE, _switch_cases, switch_widths
from tests.viscosity_model import weighted_stiffness

ELEMENTS = {2: [(1, 1), (2, 1), (3, 2)], 3: [(1, 1), (2, 1), (3, 2)]}
CASES = [(d, u, p, name) for d in (2, 3) for u, p in ELEMENTS[d] for name in ["ordinary"] + list(H.zoo(d, u))]


def _scale(d, name):
    return UAB_SCALE[(d, "lattice" if name == "ordinary" else name)]


def _inputs(F, d, name, seed=7):
    rng = np.random.default_rng(seed)
    uab = _scale(d, name) * rng.standard_normal((F.nv, d))
    cols = []
    for _ in range(3):  # c_1, b0, f_h: every column drawn separately, column 1 shifted
        x = rng.standard_normal((F.nv, 3))
        x[:, 1] += SHIFT
        cols.append(x)
    nut = 0.02 + 0.1 * rng.random(F.vd.shape[0])
    return uab, cols[0], cols[1], cols[2], nut


def _abs_lookup(E, mats):
    """sum |coefficient| |matrix| at the pattern: what forming A and A_c in float64 is rounded against."""
    return sum(abs(c) * np.abs(E.lookup(m)) for c, m in mats)


@pytest.mark.parametrize("d,u_deg,p_deg,name", CASES)
def test_scalar_forms_match_the_float64_models_entry_by_entry(d, u_deg, p_deg, name):
    F, Mo = _oracle_and_model(d, u_deg, p_deg, name)
    Me = Mo.with_oracle_error or Mo
    uab, c1, b0, fh, nut = _inputs(F, d, name)
    M, K, C = F.mass_v(), F.stiffness_v(), F.convection(uab)
    Kw = weighted_stiffness(F, nut)
    worst = {}

    def hold(what, dev, ref, ref_e, extra_abs):
        val, B, n = (ref.val, ref.B, ref.n) if isinstance(ref, AM.Entries) else ref
        Be = ref_e.B if isinstance(ref_e, AM.Entries) else ref_e[1]
        n2 = np.asarray(n).reshape(np.asarray(n).shape + (1,) * (Be.ndim - np.asarray(n).ndim))
        ok, r, allow = AM.check(dev, val, B, n, (Be - B) + (n2 + 2) * AM.U * Be + extra_abs)
        worst[what] = max(worst.get(what, 0.0), r)
        assert ok, (what, r, allow)

    for ip, (dt, nu, kappa) in enumerate(PARAMS):
        s = 0.5 * (kappa - nu)
        for with_nut in (False, True):
            A = (M / dt + C / 2 + nu / 2 * K + (Kw / 2 if with_nut else 0 * K)).tocsr()
            mats = [(1 / dt, M), (0.5, C), (nu / 2, K), (abs(s), K)] + ([(0.5 + abs(T_FACTOR), Kw)] if with_nut else [])
            forms = []
            if not with_nut:
                forms.append(("rows", lambda m: m.scalar_rows(A, M, K, s, dt, c1, b0),
                              lambda j: ScalarModel(F, F.x_v, kappa, M=M, K=K), {}, None, None))
            else:
                forms.append(("cellvisc", lambda m: m.scalar_rows_cellvisc(A, M, K, s, dt, c1, b0, nut, T_FACTOR),
                              lambda j: ScalarLesModel(F, F.x_v, kappa, SC_T, M=M, K=K), {"nut": nut}, None, None))
            for wn, scale, tt in SUPG_FORMS[ip]:
                if wn != with_nut:
                    continue
                mk = lambda j, scale=scale, tt=tt, wn=wn: ScalarSupgModel(F, F.x_v, kappa, scale=scale, time_term=tt,  # noqa: E731
                                                                           turbulent_schmidt=SC_T if wn else None, M=M, K=K)
                forms.append(("supg", None, mk, {"nut": nut} if wn else {}, scale, tt))
            for kind, model, oracle, kw, scale, tt in forms:
                got_A, got_b = None, []
                for j in range(3):
                    o = oracle(j)
                    o.c1[:], o.b0 = c1[:, j], b0[:, j].copy()
                    if kind == "supg":
                        o.fh = fh[:, j].copy()
                    Ao, bo = o.assemble(uab, dt, **kw)
                    got_A = Ao
                    got_b.append(bo)
                if kind == "supg":
                    rec = np.concatenate([o.w.T, o.tau[None]], axis=0)
                    cl = Mo.supg_cells(uab, nut if kw else None, kappa, 1 / SC_T, dt, scale, tt)
                    cle = Me.supg_cells(uab, nut if kw else None, kappa, 1 / SC_T, dt, scale, tt)
                    hold("w", o.w, cl["w"], cle["w"], 0.0)
                    err = np.abs(AM.to_f64(AM.ext(o.tau) - cl["tau"][0]))
                    # the oracle's tau is a float64 evaluation under the same propagated bound (P3: from its own table)
                    assert (err <= cl["tau"][1] + cle["tau"][1]).all(), ("tau", float((err / cle["tau"][1]).max()))
                    worst["tau/bound"] = max(worst.get("tau/bound", 0.0), float((err / cl["tau"][1]).max()))
                    model = lambda m: m.scalar_rows_supg(A, M, K, s, dt, c1, b0, nut if kw else None, T_FACTOR, rec, fh)  # noqa: E731
                ref, ref_e = model(Mo), (model(Me) if Me is not Mo else None)
                ref_e = ref if ref_e is None else ref_e
                E = ref["A_c"]
                aA = _abs_lookup(E, mats)
                hold("A_c " + kind, E.lookup(got_A), E, ref_e["A_c"], 10 * AM.U * aA)
                ab = np.zeros((F.nv, 3))
                np.add.at(ab, E.rows, aA[:, None] * np.abs(c1)[E.cols])
                hold("b_c " + kind, np.stack(got_b, axis=1), ref["b_c"], ref_e["b_c"], 10 * AM.U * ab)
                assert "a_c1" in ref and ref["a_c1"][0].shape == (F.nv, 3)
    print(f"scalar model vs float64 models {d}-D P{u_deg} {name}: max err / (u B) " + " ".join(f"{k}={v:.1f}" for k, v in worst.items()))


@pytest.mark.parametrize("d,u_deg,p_deg,name", [(2, 1, 1, "ordinary"), (2, 2, 1, "stretched"), (3, 2, 1, "flipped"), (2, 3, 2, "fan254")])
def test_identities_of_the_scalar_forms(d, u_deg, p_deg, name):
    F, Mo = _oracle_and_model(d, u_deg, p_deg, name)
    uab, c1, b0, fh, nut = _inputs(F, d, name)
    dt, nu, kappa = PARAMS[0]
    s = 0.5 * (kappa - nu)
    M, K = F.mass_v(), F.stiffness_v()
    A = (M / dt + F.convection(uab) / 2 + nu / 2 * K).tocsr()
    nc = F.vd.shape[0]
    # w = 0: N = S = 0 exactly, tau finite and positive
    cl = Mo.supg_cells(0.0 * uab, nut, kappa, 1 / SC_T, dt, 1.0, True)
    w0, tau0 = AM.to_f64(cl["w"][0]), AM.to_f64(cl["tau"][0])
    assert (w0 == 0).all() and np.isfinite(tau0).all() and (tau0 > 0).all() and (cl["w"][1] == 0).all()
    Ne, BN, Se, BS = Mo._supg_e(w0, tau0)
    assert all((AM.to_f64(AM.absx(v)) == 0).all() for v in (Ne, Se)) and (BN == 0).all() and (BS == 0).all()
    # t = 0 and no SUPG reproduce scalar_rows, value by value
    plain = Mo.scalar_rows(A, M, K, s, dt, c1, b0)
    rec0 = np.concatenate([w0.T, tau0[None]], axis=0)
    for other in (Mo.scalar_rows_cellvisc(A, M, K, s, dt, c1, b0, nut, 0.0), Mo.scalar_rows_supg(A, M, K, s, dt, c1, b0, None, 0.0, rec0, fh)):
        assert (AM.to_f64(AM.absx(other["A_c"].val - plain["A_c"].val)) == 0).all()
        for what in ("b_c", "a_c1"):
            assert (AM.to_f64(AM.absx(other[what][0] - plain[what][0])) == 0).all()
        assert (other["A_c"].n >= plain["A_c"].n).all() and (other["b_c"][2] >= plain["b_c"][2]).all()
    # a velocity field: rows of N over a constant c are tau |J| int w . grad phi_i; S symmetric
    cl = Mo.supg_cells(uab, nut, kappa, 1 / SC_T, dt, 1.0, True)
    w, tau = AM.to_f64(cl["w"][0]), AM.to_f64(cl["tau"][0])
    Ne, BN, Se, BS = Mo._supg_e(w, tau)
    nchain = AM.chain("supg", d, u_deg) + 2
    grad_int = AM.ext(np.stack([AM._tensor(d, [(u_deg, a)]) for a in range(d + 1)], axis=1), Mo.x)  # [i][a] = int d(phi_i)/d(lambda_a)
    wa = AM._einsum("cd,cad->ca", Mo._e(w), Mo.geo.G)
    want = (Mo.geo.adet * Mo._e(tau))[:, None] * AM._einsum("ca,ia->ci", wa, grad_int)
    assert (AM.to_f64(AM.absx(Ne.sum(axis=2) - want)) <= X_EPS * nchain * BN.sum(axis=2) + 1e-300).all()
    assert (AM.to_f64(AM.absx(Se - np.swapaxes(Se, 1, 2))) <= X_EPS * nchain * BS + 1e-300).all()
    # N + N^T is the boundary term tau oint (w . n) phi_i phi_j: with one w and one tau for every cell it vanishes wherever
    # phi_i phi_j vanishes on the boundary, and its entries sum to 2 tau int w . grad(1) = 0.  On the lattice with h = 1/2 the
    # records are exact, so the cancellation between neighbouring cells is exact to the extended type.
    pts, cells = H.lattice(d, 4)
    F2 = O.Forms(pts, cells, u_deg, p_deg)
    rec = np.concatenate([F2.G[:, 1:, :].reshape(F2.G.shape[0], -1), F2.adet[:, None]], axis=1)
    rec = np.concatenate([rec, np.zeros((rec.shape[0], (6 if d == 2 else 10) - rec.shape[1]))], axis=1)
    M2 = AM.Model(AM.geometry_from_records(rec), F2.vd, F2.nv, u_deg)
    nc = cells.shape[0]
    N1, BN1, _, _ = M2._supg_e(np.tile(np.linspace(0.75, -0.5, d)[None], (nc, 1)), np.full(nc, 0.25))
    rows, cols, val, (B,), cnt = AM._scatter(N1 + np.swapaxes(N1, 1, 2), F2.vd, F2.vd, (F2.nv, F2.nv),
                                             extra=(BN1 + np.swapaxes(BN1, 1, 2),))
    on_rim = np.zeros(F2.nv, dtype=bool)
    on_rim[O.boundary_dofs(F2.x_v, pts.min(axis=0), pts.max(axis=0))] = True
    inner = ~(on_rim[rows] & on_rim[cols])
    assert inner.any() and (~inner).any()
    assert (AM.to_f64(AM.absx(val[inner])) <= X_EPS * (cnt[inner] + nchain) * B[inner]).all()
    assert AM.to_f64(AM.absx(val[~inner])).max() > 1e-3 * B.max()  # and it is there on the boundary
    assert abs(float(val.sum())) <= X_EPS * float(((cnt + nchain) * B).sum())


def _mutation_case(d, u_deg, p_deg, name, ip=0):
    F, Mo = _oracle_and_model(d, u_deg, p_deg, name)
    uab, c1, b0, fh, nut = _inputs(F, d, name)
    dt, nu, kappa = PARAMS[ip]
    M, K = F.mass_v(), F.stiffness_v()
    A = (M / dt + F.convection(uab) / 2 + nu / 2 * K + weighted_stiffness(F, nut) / 2).tocsr()
    cl = Mo.supg_cells(uab, nut, kappa, 1 / SC_T, dt, 1.0, True)
    rec = np.concatenate([AM.to_f64(cl["w"][0]).T, AM.to_f64(cl["tau"][0])[None]], axis=0)
    run = lambda rec=rec, mutate=None: Mo.scalar_rows_supg(A, M, K, 0.5 * (kappa - nu), dt, c1, b0, nut, T_FACTOR, rec, fh,  # noqa: E731
                                                          mutate=mutate)
    return F, Mo, run, rec


def test_the_criterion_flags_four_mutations_of_the_supg_rows():
    """A correctly rounded result passes; each mutation is flagged entry-wise.  What ``1e-12 * max`` (the criterion of
    tests/test_gpu_scalar_supg.py) says to each is asserted beside it."""
    F, Mo, run, rec = _mutation_case(2, 2, 1, "stretched")
    ref = run()
    E = ref["A_c"]
    dev = AM.to_f64(E.val)
    dev_b = AM.to_f64(ref["b_c"][0])
    assert AM.check(dev, E.val, E.B, E.n)[0] and AM.check(dev_b, *ref["b_c"])[0]
    old = lambda a, b: np.abs(a - b).max() <= 1e-12 * np.abs(b).max()  # noqa: E731
    flagged = lambda a: not AM.check(a, E.val, E.B, E.n)[0]  # noqa: E731 (E: the case at hand)
    # 1. one (row, cell) contribution of S dropped: of the pairs whose loss the max-norm does not see, the one the
    #    entry-wise criterion sees best
    _, _, Se, _ = Mo._supg_e(rec[:2].T, rec[2])
    lost = AM.to_f64(AM.absx(Se)) / 2  # (cell, i, j): what the entry (dof_i, dof_j) loses
    idx = {(int(r), int(c)): k for k, (r, c) in enumerate(zip(E.rows, E.cols))}
    slot = np.array([[[idx[(int(F.vd[e, i]), int(F.vd[e, j]))] for j in range(F.vd.shape[1])] for i in range(F.vd.shape[1])]
                     for e in range(F.vd.shape[0])])
    seen = (lost / (AM.U * (E.n[slot] + 2) * E.B[slot])).max(axis=2)
    cell, i = np.unravel_index(np.argmin(np.where(seen > 1.0, lost.max(axis=2), np.inf)), seen.shape)  # the smallest loss it sees

    def drop(el):
        el["S"] = el["S"].copy()
        el["S"][cell, i, :] = 0
    dropped = AM.to_f64(run(mutate=drop)["A_c"].val)
    print(f"mutation 1: S of (cell {cell}, row dof {i}) dropped: loses {lost[cell, i].max() / np.abs(dev).max():.2e} max|A_c|, "
          f"{seen[cell, i]:.1f} allowances of its entry; max-norm accepts: {old(dropped, dev)}")
    assert flagged(dropped)
    assert not old(dropped, dev)  # with this velocity even the smallest S contribution is 1.7e-9 of the maximum: REJECTED too
    # 3. column 2 of the right-hand side taken from column 1 (shifted by 1e6)
    wrong = dev_b.copy()
    wrong[:, 2] = dev_b[:, 1]
    assert not AM.check(wrong, *ref["b_c"])[0] and not old(wrong, dev_b)  # the max-norm REJECTS it too
    # 2. (the P1 fan) one tau_c changed by a relative 1e-10: of the cells whose N/dt + S/2 is at most 1e-3 max|A_c| -- 1e-10
    #    of it is below what the max-norm resolves -- the one that weighs most in one of its entries
    F, Mo, run, rec = _mutation_case(2, 1, 1, "fan254")
    ref = run()
    E = ref["A_c"]
    dev = AM.to_f64(E.val)
    Ne, _, Se, _ = Mo._supg_e(rec[:2].T, rec[2])
    idx = {(int(r), int(c)): k for k, (r, c) in enumerate(zip(E.rows, E.cols))}
    slot = np.array([[[idx[(int(F.vd[e, i]), int(F.vd[e, j]))] for j in range(3)] for i in range(3)] for e in range(F.vd.shape[0])])
    part = AM.to_f64(AM.absx(Ne)) / PARAMS[0][0] + AM.to_f64(AM.absx(Se)) / 2
    small = part.max(axis=(1, 2)) <= 1e-3 * np.abs(dev).max()
    assert small.any()
    cell = int(np.argmax(np.where(small, (part / E.B[slot]).max(axis=(1, 2)), 0.0)))
    rec2 = rec.copy()
    rec2[2, cell] *= 1.0 + 1e-10
    assert rec2[2, cell] != rec[2, cell]
    nudged = AM.to_f64(run(rec=rec2)["A_c"].val)
    print(f"mutation 2: tau of cell {cell} times 1 + 1e-10: max-norm accepts: {old(nudged, dev)}")
    assert flagged(nudged) and old(nudged, dev)  # the max-norm ACCEPTS it: the gap
    # 4. the last entry pair of the widest row swapped (the 254-wide centre row of the P1 fan)
    row = int(np.argmax(np.bincount(E.rows)))
    k = np.nonzero(E.rows == row)[0]
    assert k.shape[0] == 254
    swapped = dev.copy()
    swapped[k[-2]], swapped[k[-1]] = dev[k[-1]], dev[k[-2]]
    flag = not AM.check(swapped, E.val, E.B, E.n)[0]
    print(f"mutation 4: the last pair of the 254-wide row: {dev[k[-2]]:.6e} <-> {dev[k[-1]]:.6e}; max-norm accepts: {old(swapped, dev)}")
    assert flag and not old(swapped, dev)  # entries of the size of the maximum: the max-norm REJECTS it too


def test_the_switch_meshes_reach_every_epilogue_tail():
    for table in (H.FAN_K, H.SPINDLE_K):
        for deg in (1, 2, 3):
            w = [e[1] for e in switch_widths(table[deg])]
            assert w[0] <= 67 < w[1] <= 134 and w[2] <= 134 < w[3], w
    assert {(w // 2) % 4 for _, _, _, w in _switch_cases()} | {(254 // 2) % 4} == {0, 1, 2, 3}


# ---- the input conditions of the device test ---------------------------------------------------------------------------
def _terms(F, Mo, d, name, ip, wn, scale, tt, factor=1.0):
    uab, c1, b0, fh, nut = _inputs(F, d, name)
    uab = factor * uab
    dt, nu, kappa = PARAMS[ip]
    M, K = F.mass_v(), F.stiffness_v()
    A = (M / dt + F.convection(uab) / 2 + nu / 2 * K + weighted_stiffness(F, nut) / 2).tocsr()
    cl = Mo.supg_cells(uab, nut, kappa, 1 / SC_T, dt, scale, tt)
    w, tau = AM.to_f64(cl["w"][0]), AM.to_f64(cl["tau"][0])
    Ne, BN, Se, BS = Mo._supg_e(w, tau)
    Ke, BKe = Mo._stiff_e(Mo.u_deg)
    z = np.zeros_like(BN)
    rows, cols, _ = Mo._pattern()
    sK = 0.5 * (kappa - nu) * np.asarray(K.tocsr()[rows, cols]).ravel()
    tKt = AM.to_f64(Mo._acc_entries(T_FACTOR * nut[:, None, None] * Ke, z)[0])
    Ndt = AM.to_f64(Mo._acc_entries(Ne / dt, z)[0])
    S2 = AM.to_f64(Mo._acc_entries(Se / 2, z)[0])
    Ac = np.asarray(A[rows, cols]).ravel() + sK + tKt + Ndt + S2
    mx = np.abs(Ac).max()
    return {"s K": np.abs(sK).max() / mx, "t K_t": np.abs(tKt).max() / mx, "N/dt": np.abs(Ndt).max() / mx, "S/2": np.abs(S2).max() / mx}


@pytest.mark.parametrize("d,u_deg,p_deg,name", CASES)
def test_input_conditions_of_the_device_test(d, u_deg, p_deg, name):
    """With ``UAB_SCALE`` each of s K, t K_t, N/dt and S/2 has a largest entry of at least 1e-6 max|A_c| -- except N/dt where
    no scaling of the velocity brings it there.  Why there is such a limit: tau k q <= scale whatever u_ab is, so
    |N_ij / dt| <= sum_c |J_c| max_a |int phi_j d(phi_i)/d(lambda_a)| / (k dt), a mass-like size, while max|A_c| holds
    kappa K / 2 of the size kappa g |J| / 2; and a velocity large enough to leave the diffusive limit of tau
    (k q ~ 2 k^2 kappa g) raises max|A_c| through C/2 and S/2 with it.  On the cells with |G| of 1e3 and more (tiny_far, the
    3-D stretched and flipped lattices, squashed) the ratio therefore has a maximum below 1e-6 over the scale of u_ab.  For
    those the test scans the scale over four decades around ``UAB_SCALE`` and asserts that (a) no scale reaches 1e-6 and
    (b) the chosen one is within a decade of the best; the other three terms are held to 1e-6 there as everywhere."""
    F, Mo = _oracle_and_model(d, u_deg, p_deg, name)
    for ip in range(len(PARAMS)):
        for wn, scale, tt in SUPG_FORMS[ip]:
            r = _terms(F, Mo, d, name, ip, wn, scale, tt)
            print(f"INPUT {d}-D P{u_deg} {name:<10s} dt={PARAMS[ip][0]} scale={scale:g} time_term={tt}: "
                  + " ".join(f"{k} {v:.1e}" for k, v in r.items()))
            for k, v in r.items():
                if k != "N/dt" or v >= 1e-6:
                    assert v >= 1e-6, (k, v)
                    continue
                scan = {f: _terms(F, Mo, d, name, ip, wn, scale, tt, f)["N/dt"] for f in (1e-2, 1e-1, 10.0, 1e2)}
                best = max(max(scan.values()), v)
                print(f"INPUT {d}-D P{u_deg} {name:<10s}   N/dt over u_ab * (1e-2, 1e-1, 1, 10, 1e2): "
                      + " ".join(f"{x:.1e}" for x in (scan[1e-2], scan[1e-1], v, scan[10.0], scan[1e2])))
                assert best < 1e-6 and v >= 0.1 * best, (k, v, scan)
