"""GPU: the scalar row kernels and the SUPG cell kernel held ENTRY BY ENTRY to the extended-precision model of
tests/assembly_model.py, on the meshes of tests/hard_meshes.py -- ``ox_scalar_rows`` (csrc/ox_scalar.hip),
``ox_scalar_rows_cellvisc`` and ``ox_scalar_rows_supg`` (csrc/ox_assemble.hip) and ``ox_supg_cells``, driven through the
bindings as ``Problem.first`` of tests/test_gpu_assembly_entries.py drives ``ox_assemble_first``; no solver.

Criterion: ``|dev - ref| <= (n + 2) 2^-53 B`` for every entry of ``A_c``, ``b_c`` and ``A_c c_1`` (assembly_model: B = the
same assembly over absolute values, n = the longest rounded chain, counted); entries with ``B == 0`` must be exactly zero;
``tau_c`` under its propagated absolute bound; everything else is bit equality (width bins = row blocks = the dictionary
instantiation; ``a_c1`` = ``Ac.mult(c1)``).  ``A`` is what ``ox_assemble_first`` left for a random ``u_ab``; ``Ac``, ``b`` and
``a_c1`` are NaN before every launch.  Column 1 of ``c_1``, ``b0`` and ``f_h`` is shifted by 1e6: a cross-column index
shows as a miss of that size.  Every check prints its figure (``-s``); DESIGN.md section 5.1 quotes them.

``UAB_SCALE``: the factor on the random ``u_ab`` per mesh, chosen on the model (tests/test_scalar_rows_model_host.py checks
the input conditions with it): ``tau`` leaves its diffusive limit where ``k q ~ 2 k^2 kappa g``, i.e. ``|u| ~ kappa |G|``, so the
meshes with large ``|G|`` need a large velocity for ``S/2`` and ``N/dt`` to be seen beside ``kappa K / 2``."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import assembly_model as AM
from tests import hard_meshes as H
from tests.test_gpu_assembly_entries import (ELEMENTS, _MISSES, Problem, _designed_width, _fresh_list_of_misses,  # noqa: F401
                                             _report, _verdict)

pytestmark = pytest.mark.gpu

PARAMS = ((0.005, 0.01, 1e-3), (0.1, 0.5, 0.2))  # (dt, nu, kappa)
SC_T = 0.7
T_FACTOR = (1.0 / SC_T - 1.0) / 2.0
# (with nut, scale, time_term) of the SUPG launches per parameter set: every value of each, with and without a model
SUPG_FORMS = (((True, 1.0, True), (False, 0.5, False)), ((True, 0.5, False), (False, 1.0, True)))
UAB_SCALE = {(2, "lattice"): 10.0, (2, "fan254"): 10.0, (2, "stretched"): 10.0, (2, "flipped"): 10.0, (2, "tiny_far"): 1.0e3,
             (3, "lattice"): 10.0, (3, "spindle254"): 10.0, (3, "stretched"): 1.0e4, (3, "flipped"): 1.0e4,
             (3, "squashed"): 1.0e6, (3, "tiny_far"): 1.0e3}
SWITCH_UAB_SCALE = 10.0  # the fans and spindles on either side of a launch switch: the shapes of fan254 / spindle254
SHIFT = 1.0e6

CASES = [(d, u, p, name) for d in (2, 3) for u, p in ELEMENTS[d] for name in H.zoo(d, u)]
# the cases in which M.freeze() and K.freeze() both build a value dictionary (at most 256 distinct stored values: the
# lattice-derived meshes of congruent cells, mostly P1), so that the DICT instantiations run; the others run the plain ones
DICTIONARY_CASES = {(2, 1, "stretched"), (2, 1, "tiny_far"), (2, 1, "flipped"), (2, 2, "tiny_far"),
                    (3, 1, "stretched"), (3, 1, "squashed"), (3, 1, "tiny_far"), (3, 1, "flipped")}
assert {c[0] for c in DICTIONARY_CASES} == {2, 3}  # the dictionary path is reached in both dimensions


def switch_widths(table):
    """The entries of FAN_K / SPINDLE_K on either side of 67 and of 134: [(k, width)] x 4."""
    out = []
    for lim in (67, 134):
        below = max((e for e in table if e[1] <= lim), key=lambda e: e[1])
        above = min((e for e in table if e[1] > lim), key=lambda e: e[1])
        out += [below, above]
    return out


def _switch_cases():
    return [(kind, deg, k, w) for kind, table in (("fan", H.FAN_K), ("spindle", H.SPINDLE_K)) for deg in (1, 2, 3)
            for k, w in switch_widths(table[deg])]


def test_switch_widths_reach_every_epilogue_tail():
    """(no device) The epilogue streams four entry pairs per turn: between the switch meshes and the 254-wide ones the
    widths reach all four values of npair % 4, on either side of 67 and of 134, per degree."""
    for table in (H.FAN_K, H.SPINDLE_K):
        for deg in (1, 2, 3):
            w = [e[1] for e in switch_widths(table[deg])]
            assert w[0] <= 67 < w[1] <= 134 and w[1] <= 134 and w[2] <= 134 < w[3], w
    tails = {(w // 2) % 4 for _, _, _, w in _switch_cases()} | {(254 // 2) % 4}
    assert tails == {0, 1, 2, 3}, tails
    assert {(w // 2) % 4 for w in (66, 68, 136, 254)} == {0, 1, 2, 3}
    assert all(w in [c[3] for c in _switch_cases()] for w in (66, 68, 134, 136))


class ScalarProblem(Problem):
    """``Problem`` with the scalar group's arrays: A_c on the shared pattern and the launches of the four entries."""

    def __init__(self, pts, cells, u_deg, p_deg):
        from oasisx_amd.la import SellMatrix

        super().__init__(pts, cells, u_deg, p_deg)
        self.Ac = SellMatrix(self.Vi.pattern, name="Ac")
        self.ncells = int(self.geom.shape[0])

    def supg_cells(self, uab, nut, kappa, inv_sct, dt, scale, time_term):
        from oasisx_amd import _lib

        rec = torch.full((self.d + 1, self.ncells), float("nan"), dtype=torch.float64, device="cuda")
        _lib.check(self.lib.ox_supg_cells(self.Vi.degree, C.byref(self.cells), _lib.ptr(self.Vi.cell_dofs), _lib.ptr(uab),
                                          _lib.ptr(nut), float(kappa), float(inv_sct), float(dt), float(scale), int(time_term),
                                          _lib.ptr(rec), _lib.current_stream()), "ox_supg_cells")
        return rec

    def rows(self, kind, A_vals, s, t, dt, c1, b0, fh=None, nut=None, rec=None, row_blocks=0):
        """One launch of ``kind`` in ("rows", "cellvisc", "supg") on NaN-filled outputs: (A_c values, b, a_c1)."""
        from oasisx_amd import _lib

        n, nc = self.Vi.n_local, int(c1.shape[1])
        self.mass_and_stiffness()
        self.A.vals.copy_(A_vals)
        self.A.version += 1
        self.Ac.vals.fill_(float("nan"))
        b = torch.full((n, nc), float("nan"), dtype=torch.float64, device="cuda")
        a_c1 = torch.full((n, nc), float("nan"), dtype=torch.float64, device="cuda")
        st, lib = _lib.current_stream(), self.lib
        refs = (self.A.ref(), self.M.ref(), self.K.ref(), self.Ac.ref())
        if kind == "rows":
            _lib.check(lib.ox_scalar_rows(*refs, float(s), float(dt), nc, _lib.ptr(c1), _lib.ptr(b0), _lib.ptr(b), _lib.ptr(a_c1), st),
                       "ox_scalar_rows")
        elif kind == "cellvisc":
            _lib.check(lib.ox_scalar_rows_cellvisc(C.byref(self.cells), C.byref(self.Vi.assembly_info()), *refs, _lib.ptr(nut),
                                                   float(s), float(t), float(dt), nc, _lib.ptr(c1), _lib.ptr(b0), _lib.ptr(b),
                                                   _lib.ptr(a_c1), int(row_blocks), st), "ox_scalar_rows_cellvisc")
        else:
            _lib.check(lib.ox_scalar_rows_supg(C.byref(self.cells), C.byref(self.Vi.assembly_info()), *refs, _lib.ptr(nut),
                                               _lib.ptr(rec), float(s), float(t), float(dt), nc, _lib.ptr(c1), _lib.ptr(b0),
                                               _lib.ptr(fh), _lib.ptr(b), _lib.ptr(a_c1), int(row_blocks), st),
                       "ox_scalar_rows_supg")
        self.Ac.version += 1
        return self.Ac.vals.clone(), b, a_c1

    def freeze(self):
        """Value dictionaries of M and K (the DICT instantiations read them): whether both exist."""
        self.mass_and_stiffness()
        fm, fk = self.M.freeze(), self.K.freeze()
        if not (fm and fk):
            self.thaw()
        return fm and fk

    def thaw(self):
        self.M._drop_codes()
        self.K._drop_codes()


@functools.lru_cache(maxsize=None)
def _problem(d, u_deg, p_deg, name):
    return ScalarProblem(*H.zoo(d, u_deg)[name], u_deg, p_deg)


def _columns(n, g, ncol=3):
    """(n, 3) with every column drawn separately and column 1 shifted."""
    x = torch.stack([torch.randn(n, dtype=torch.float64, device="cuda", generator=g) for _ in range(ncol)], dim=1)
    x[:, 1] += SHIFT
    return x.contiguous()


def _report_tau(d, u_deg, mesh, what, dev, val, tol):
    err = AM.to_f64(AM.absx(AM.ext(dev) - val))
    ok = bool((err <= tol).all()) and bool(np.isfinite(dev).all())
    with np.errstate(divide="ignore", invalid="ignore"):
        r = float(np.nanmax(np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))))
        rel = float(np.max(tol / np.abs(dev)) / AM.U)
    print(f"RATIO {what:<22s} {d}-D P{u_deg} {mesh:<12s} err/bound  = {r:8.3f}   bound <= {rel:6.0f} u tau   {'ok' if ok else 'MISS'}")
    if not ok:
        _MISSES.append((what, d, u_deg, mesh, round(r, 3), 1))


def _launches(Pb, ncs, kind, A_vals, s, t, dt, c1, b0, fh, nut, rec):
    """The launch in every form the pattern has, per number of columns: {nc: (A_c values, b, a_c1)}, bins = row blocks."""
    out = {}
    for nc in ncs:
        cols = [x[:, :nc].contiguous() if x is not None else None for x in (c1, b0, fh)]
        got = Pb.rows(kind, A_vals, s, t, dt, cols[0], cols[1], cols[2], nut, rec, 0)
        if kind != "rows" and Pb.Vi.pattern.n_row_blocks > 0:
            blk = Pb.rows(kind, A_vals, s, t, dt, cols[0], cols[1], cols[2], nut, rec, 1)
            for a, b in zip(got, blk):
                assert torch.equal(a, b), (kind, nc, "row blocks and width bins differ")
        y = torch.full_like(got[2], float("nan"))
        Pb.Ac.mult(cols[0], y, nc)
        assert torch.equal(y, got[2]), (kind, nc, "a_c1 is not the bits of Ac.mult(c1)")
        out[nc] = got
    return out


def _hold(Pb, d, u_deg, name, tag, got, ref):
    """The device results of every column count against one model evaluation with three columns."""
    E = ref["A_c"]
    for nc, (vals, b, a_c1) in got.items():
        A = Pb.Vi.pattern.to_csr(vals)
        sfx = f"{tag} x{nc}"
        _report("A_c " + sfx, d, u_deg, name, E.lookup(A), E.val, E.B, E.n)
        for what, dev in (("b_c", b), ("a_c1", a_c1)):
            val, B, n = ref[what]
            _report(f"{what} {sfx}", d, u_deg, name, dev.cpu().numpy(), val[:, :nc], B[:, :nc], n[:, :nc])


def _check_scalar_rows(Pb, d, u_deg, name, uab_scale, params=PARAMS, kinds=("rows", "cellvisc", "supg"), ncs=(1, 2, 3), dictionary=True):
    Mo = Pb.model
    n = Pb.Vi.n_local
    g = torch.Generator(device="cuda").manual_seed(17)
    uab = uab_scale * torch.randn(n, d, dtype=torch.float64, device="cuda", generator=g)
    u1, bv = (torch.randn(n, d, dtype=torch.float64, device="cuda", generator=g) for _ in range(2))
    c1, b0, fh = (_columns(n, g) for _ in range(3))
    nut = 0.02 + 0.1 * torch.rand(Pb.ncells, dtype=torch.float64, device="cuda", generator=g)
    Md, Kd = (m.to_scipy() for m in Pb.mass_and_stiffness())
    h = lambda x: None if x is None else x.cpu().numpy()  # noqa: E731
    jobs = []  # (kind, arguments of _launches, results): run again with the value dictionaries at the end
    for ip, (dt, nu, kappa) in enumerate(params):
        s = 0.5 * (kappa - nu)
        for with_nut in (False, True):
            A, _, _ = Pb.first(uab, u1, bv, dt, nu, nut if with_nut else None)
            A_vals = Pb.A.vals.clone()
            todo = []
            if not with_nut and "rows" in kinds:
                todo.append(("rows", f"dt={dt}", 0.0, None, None, lambda: Mo.scalar_rows(A, Md, Kd, s, dt, h(c1), h(b0))))
            if with_nut and "cellvisc" in kinds:
                todo.append(("cellvisc", f"+nut dt={dt}", T_FACTOR, nut, None,
                             lambda: Mo.scalar_rows_cellvisc(A, Md, Kd, s, dt, h(c1), h(b0), h(nut), T_FACTOR)))
            for wn, scale, time_term in (SUPG_FORMS[ip] if "supg" in kinds else ()):
                if wn != with_nut:
                    continue
                nu_t = nut if wn else None
                rec = Pb.supg_cells(uab, nu_t, kappa, 1.0 / SC_T, dt, scale, time_term)
                cl = Mo.supg_cells(h(uab), h(nu_t), kappa, 1.0 / SC_T, dt, scale, time_term)
                tag = f"supg{'+nut' if wn else ''} {scale:g}{'t' if time_term else ''} dt={dt}"
                _report("w " + tag, d, u_deg, name, h(rec)[:d].T, *cl["w"])
                _report_tau(d, u_deg, name, "tau " + tag, h(rec)[d], *cl["tau"])
                todo.append(("supg", tag[4:], T_FACTOR if wn else 0.0, nu_t, rec,
                             lambda nu_t=nu_t, rec=rec: Mo.scalar_rows_supg(A, Md, Kd, s, dt, h(c1), h(b0), h(nu_t), T_FACTOR, h(rec), h(fh))))
            for kind, tag, t, nu_t, rec, model in todo:
                args = (kind, A_vals, s, t, dt, c1, b0, fh if kind == "supg" else None, nu_t, rec)
                got = _launches(Pb, ncs, *args)
                _hold(Pb, d, u_deg, name, f"{kind} {tag}", got, model())
                jobs.append((args, got))
    froze = False
    if dictionary:
        froze = Pb.freeze()
        if froze:
            try:
                for args, got in jobs:
                    again = _launches(Pb, ncs, *args)
                    for nc in ncs:
                        for a, b in zip(got[nc], again[nc]):
                            assert torch.equal(a, b), (args[0], nc, "the dictionary instantiation and the plain one differ")
            finally:
                Pb.thaw()
        print(f"DICTIONARY {d}-D P{u_deg} {name}: M and K froze: {froze} ({len(jobs)} launches x {len(ncs)} column counts compared)")
    return froze


# ---- every mesh of the zoo -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,u_deg,p_deg,name", CASES)
def test_scalar_rows_cellvisc_supg_and_supg_cells_entry_by_entry(hip, d, u_deg, p_deg, name):
    Pb = _problem(d, u_deg, p_deg, name)
    if name in ("fan254", "spindle254"):
        width = _designed_width(Pb.Vi.pattern, name[:-3], H.WIDEST[(name[:-3], u_deg)], u_deg)
        assert width in (252, 254) and int(Pb.Vi.pattern.bin_width.max()) == width  # one wave per block, 127 KB of accumulator
    froze = _check_scalar_rows(Pb, d, u_deg, name, UAB_SCALE[(d, name)])
    assert froze == ((d, u_deg, name) in DICTIONARY_CASES), (d, u_deg, name, froze)
    _verdict()


# ---- rows on either side of the launch switches of launch_scalar_cellvisc_t ----------------------------------------------
@pytest.mark.parametrize("kind,u_deg,k,width", _switch_cases())
def test_scalar_rows_on_either_side_of_the_launch_switches(hip, kind, u_deg, k, width):
    """launch_scalar_cellvisc_t: 4 waves per block while 4 * width * 512 B fit in OX_ROW_BLOCK_LDS (width <= 67), 2 up to
    134, then 1; hipFuncSetAttribute above 32 KB.  The epilogue tail is npair % 4 pairs long."""
    d = 2 if kind == "fan" else 3
    Pb = ScalarProblem(*(H.fan(k, 3.0, 1.0) if kind == "fan" else H.spindle(k)), u_deg, 1 if u_deg < 3 else 2)
    assert _designed_width(Pb.Vi.pattern, kind, k, u_deg) == width
    assert int(Pb.Vi.pattern.bin_width.max()) == width  # the launch is sized for it
    _check_scalar_rows(Pb, d, u_deg, f"{kind}{width}", SWITCH_UAB_SCALE, params=PARAMS[:1], kinds=("cellvisc", "supg"),
                       ncs=(1, 3), dictionary=False)
    _verdict()


# ---- the fluid at rest ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,u_deg,p_deg,name", CASES)
def test_at_rest_the_supg_rows_are_the_rows_without_stabilisation(hip, d, u_deg, p_deg, name):
    """u_ab = 0: w is exactly 0 and tau finite and positive; without a model the SUPG rows are the bits of ox_scalar_rows,
    with nut and t the bits of ox_scalar_rows_cellvisc (the SUPG accumulator holds K_t + (N/dt + S/2)/t and the epilogue is
    the sibling's fma(t, acc, .): with the accumulator t nut K_c + ... of the first version the rows differed from the
    sibling's in the last bits, up to 4.7e-14 of an entry of A_c)."""
    Pb = _problem(d, u_deg, p_deg, name)
    n = Pb.Vi.n_local
    g = torch.Generator(device="cuda").manual_seed(23)
    uab = torch.zeros(n, d, dtype=torch.float64, device="cuda")
    u1, bv = (torch.randn(n, d, dtype=torch.float64, device="cuda", generator=g) for _ in range(2))
    c1, b0, fh = (_columns(n, g) for _ in range(3))
    nut = 0.02 + 0.1 * torch.rand(Pb.ncells, dtype=torch.float64, device="cuda", generator=g)
    dt, nu, kappa = PARAMS[0]
    s = 0.5 * (kappa - nu)
    worst = 0.0
    for nu_t, t, sibling in ((None, 0.0, "rows"), (nut, T_FACTOR, "cellvisc")):
        Pb.first(uab, u1, bv, dt, nu, nu_t)
        A_vals = Pb.A.vals.clone()
        rec = Pb.supg_cells(uab, nu_t, kappa, 1.0 / SC_T, dt, 1.0, True)
        assert bool((rec[:d] == 0).all()), "w is not exactly zero"
        assert bool(torch.isfinite(rec[d]).all()) and bool((rec[d] > 0).all()), "tau is not finite and positive"
        for nc in (1, 2, 3):
            cols = [x[:, :nc].contiguous() for x in (c1, b0, fh)]
            got = Pb.rows("supg", A_vals, s, t, dt, cols[0], cols[1], cols[2], nu_t, rec)
            want = Pb.rows(sibling, A_vals, s, t, dt, cols[0], cols[1], None, nu_t, None)
            for what, a, b in zip(("A_c", "b_c", "a_c1"), got, want):
                same = torch.equal(a, b)
                fin = torch.isfinite(b)
                diff = float(((a - b)[fin].abs() / b[fin].abs().clamp_min(1e-300)).max()) if bool(fin.any()) else 0.0
                worst = max(worst, diff)
                print(f"AT REST {d}-D P{u_deg} {name:<12s} supg vs {sibling:<8s} x{nc} {what:<5s} bit-identical: {same}; "
                      f"max relative difference {diff:.3e}")
                if not same:
                    _MISSES.append((f"at rest {what} x{nc} vs {sibling}", d, u_deg, name, diff, 0))
    _verdict()
