"""GPU: ``ox_assemble_first`` called directly, in all eight combinations of its launch form (``row_blocks`` 0 / 1) and its two
optional arguments (``ox_first_args.a_u1``, ``ox_first_args.nut``): the form and the by-product change no bit, ``nut = 0``
gives the bits of ``nut == NULL`` (which selects the constant-viscosity kernels), and a viscosity that is not zero changes
the result the same way in both forms."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _box():
    from oasisx_amd import mesh as M

    # P2, sort window 256: several row lengths, two row blocks, the last one partial (3 of 8 slices)
    return M.create_box(None, [[-1.0] * 3, [1.0] * 3], [4, 5, 3]), {"sell_window": 256}


def _delaunay():
    from oasisx_amd import mesh as M

    return M.create_delaunay_box(None, [[-1.0] * 2, [1.0] * 2], 8), {}  # P2: a dozen row lengths


@pytest.mark.parametrize("make", [_box, _delaunay])
def test_launch_form_and_optional_arguments_change_no_bit(hip, make):
    import oasisx_amd as ox
    from oasisx_amd import _lib
    from tests.helpers import KRYLOV

    mesh, options = make()
    dim = mesh.gdim
    bcs = [[ox.DirichletBC(0.0, ox.LocatorMethod.GEOMETRICAL, lambda x: np.isclose(np.abs(x[0]), 1.0))] for _ in range(dim)]
    S = ox.FractionalStep_AB_CN(mesh, ("Lagrange", 2), ("Lagrange", 1), bcs_u=bcs, bcs_p=[], solver_options=KRYLOV,
                                options=options)
    Vi, P, lib = S._Vi[0][0], S._A.pattern, _lib.load()
    lens = np.unique(P.row_len.cpu().numpy())
    bp = P.row_blk_ptr.cpu().numpy()
    if make is _box:
        assert len(lens) >= 3 and P.n_row_blocks >= 2 and bp[-1] - bp[-2] < 8, (lens, bp)
    else:
        assert len(lens) > 3 and P.n_row_blocks >= 1, (lens, bp)
    n, ncells = Vi.n_local, int(S._geom.shape[0])
    g = torch.Generator(device="cuda").manual_seed(11)
    u1, u2, b0 = (torch.randn(n, dim, dtype=torch.float64, device="cuda", generator=g) for _ in range(3))
    uab = 1.5 * u1 - 0.5 * u2
    dt, nu = 0.01, 0.02

    def run(row_blocks, want_au, nut):
        S._A.vals.fill_(float("nan"))
        b_first = torch.full((n, dim), float("nan"), dtype=torch.float64, device="cuda")
        a_u1 = torch.full((n, dim), float("nan"), dtype=torch.float64, device="cuda") if want_au else None
        args = _lib.ox_first_args(uab.data_ptr(), u1.data_ptr(), b0.data_ptr(), b_first.data_ptr(), dt, nu, _lib.ptr(a_u1),
                                  _lib.ptr(nut))
        _lib.check(lib.ox_assemble_first(C.byref(S._cells), C.byref(Vi.assembly_info()), S._A.ref(), S._M.ref(), S._K.ref(),
                                         C.byref(args), row_blocks, _lib.current_stream()), "ox_assemble_first")
        S._A.version += 1
        y = None
        if want_au:
            y = torch.zeros(n, dim, dtype=torch.float64, device="cuda")
            S._A.mult(u1, y, dim)  # ox_spmv(A, u1)
        return S._A.vals.clone(), b_first, a_u1, y

    zeros = torch.zeros(ncells, dtype=torch.float64, device="cuda")
    got = {(rb, au, z): run(rb, au, zeros if z else None) for rb, au, z in itertools.product((0, 1), (False, True), (False, True))}
    A0, b0_first = got[(0, False, False)][:2]
    assert bool(torch.isfinite(A0).all()) and bool(torch.isfinite(b0_first).all()) and float(A0.abs().sum()) > 0
    for key, (A, b_first, a_u1, y) in got.items():
        assert torch.equal(A, A0) and torch.equal(b_first, b0_first), key
        if key[1]:
            assert torch.equal(a_u1, got[(0, True, False)][2]) and torch.equal(a_u1, y), key
    # a viscosity that is not zero: the two forms agree with each other, not with nut == NULL
    const = torch.full((ncells,), 0.05, dtype=torch.float64, device="cuda")
    bins, blocks = run(0, True, const), run(1, True, const)
    for a, b in zip(bins, blocks):
        assert torch.equal(a, b)
    assert torch.equal(bins[2], bins[3])
    assert not torch.equal(bins[0], A0) and not torch.equal(bins[1], b0_first)
