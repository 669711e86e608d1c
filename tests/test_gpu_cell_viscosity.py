"""GPU: the one entry point of the per-cell viscosities, ox_cell_viscosity (csrc/ox_viscosity.hip):
what its argument check refuses, and that its table form with a constant table is its constant form, bit for bit.  The
models themselves are held to their numpy models by tests/test_gpu_viscosity.py, test_gpu_rheology.py,
test_gpu_vandriest.py and test_gpu_dynamic.py."""
import ctypes as C

import pytest

from tests.test_gpu_viscosity import _assemble_first, _problem

pytestmark = pytest.mark.gpu

CS = 0.1677


def _block(S, nut, **kw):
    """An ox_viscosity_args on the solver's u_ab; the keywords replace fields."""
    from oasisx_amd import _lib

    Vi = S._Vi[0][0]
    f = dict(model=0, degree=Vi.degree, cell_dofs=_lib.ptr(Vi.cell_dofs), uab=S._UAB.rptr(), nut=_lib.ptr(nut),
             coefficient=0.0, params=None, n_params=0, damping=None, cs2=None, cs2_stride=0, n_coef=0, cell_bin=None)
    f.update(kw)
    return _lib.ox_viscosity_args(**f)


def test_refused_combinations_write_nothing(hip):
    """Every combination the checker refuses returns non-zero with a message that names ox_cell_viscosity and the field,
    and leaves nut as it was."""
    import torch

    from oasisx_amd import _lib

    S, clock, _ = _problem(2, 5, 2, None, perturb=0.05)
    _assemble_first(S, clock, 0.005, 0.01)
    nc, dev = int(S._cells.n_cells), S._UAB.dev().device
    nut = torch.full((nc,), -7.0, dtype=torch.float64, device=dev)
    dist = torch.ones(nc, dtype=torch.float64, device=dev)
    nearest = torch.zeros(nc, dtype=torch.int32, device=dev)
    cs2 = torch.full((nc,), CS * CS, dtype=torch.float64, device=dev)
    vd = C.pointer(_lib.ox_vandriest(dist.data_ptr(), nearest.data_ptr(), None, 0.05, 0.01, 26.0, 1))
    table = dict(cs2=_lib.ptr(cs2), cs2_stride=1, n_coef=nc)
    law = (C.c_double * 4)(0.16, 0.01, 3.313, 0.3568)  # Cross
    refused = [
        ("damping with cs2", dict(damping=vd, **table), b"damping"),
        ("WALE with damping", dict(model=1, coefficient=0.325, damping=vd), b"damping"),
        ("a law with a coefficient", dict(model=3, params=law, n_params=4, coefficient=0.1), b"coefficient"),
        ("model 5", dict(model=5, coefficient=CS), b"model"),
        ("degree 4", dict(degree=4, coefficient=CS), b"degree"),
        ("NULL nut", dict(coefficient=CS), b"nut"),
    ]
    for what, kw, field in refused:
        args = _block(S, None if what == "NULL nut" else nut, **kw)
        assert hip.ox_cell_viscosity(C.byref(S._cells), C.byref(args), None) != 0, what
        msg = hip.ox_last_error()
        assert b"ox_cell_viscosity" in msg and field in msg, (what, msg)
    assert hip.ox_cell_viscosity(C.byref(S._cells), None, None) != 0
    assert b"ox_cell_viscosity" in hip.ox_last_error() and b"args" in hip.ox_last_error()
    assert torch.equal(nut, torch.full_like(nut, -7.0))
    # (the blocks above are refused for the named reason alone: each form goes through once the extra field is gone)
    for kw in (dict(damping=vd, coefficient=CS), table, dict(model=3, params=law, n_params=4), dict(coefficient=CS)):
        assert hip.ox_cell_viscosity(C.byref(S._cells), C.byref(_block(S, nut, **kw)), None) == 0, hip.ox_last_error()
    assert bool(torch.isfinite(nut).all()) and float(nut.min()) >= 0.0 and float(nut.max()) > 0.0


# 2-D n = 5: 50 cells, one partial block; n = 12: 288 cells, a full block and a partial one; 3-D n = 3: 162 cells
@pytest.mark.parametrize("dim,N,deg", [(2, 5, 1), (2, 5, 2), (2, 5, 3), (2, 12, 2), (3, 3, 2)])
def test_constant_table_is_the_constant_form(hip, dim, N, deg):
    """cs2[c] = Cs Cs per cell, and one bin holding Cs Cs behind a cell_bin of zeros, give the nut of Smagorinsky(Cs):
    the same factor enters the same product, so the results are torch.equal."""
    import torch

    import oasisx_amd as ox
    from oasisx_amd import _lib

    S, clock, _ = _problem(dim, N, deg, ox.Smagorinsky(CS), perturb=0.05)
    _assemble_first(S, clock, 0.005, 0.01)
    ref = S._nut.clone()
    nc = int(S._cells.n_cells)
    assert ref.shape == (nc,) and float(ref.max()) > 0.0
    cs2 = torch.full((nc,), CS * CS, dtype=torch.float64, device=ref.device)
    bins = torch.zeros(nc, dtype=torch.int32, device=ref.device)
    for kw in (dict(cs2=_lib.ptr(cs2), cs2_stride=1, n_coef=nc),
               dict(cs2=_lib.ptr(cs2), cs2_stride=1, n_coef=1, cell_bin=_lib.ptr(bins))):
        nut = torch.full_like(ref, -7.0)
        args = _block(S, nut, **kw)
        assert hip.ox_cell_viscosity(C.byref(S._cells), C.byref(args), _lib.current_stream()) == 0, hip.ox_last_error()
        assert torch.equal(nut, ref)
