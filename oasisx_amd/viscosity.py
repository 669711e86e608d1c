"""Eddy-viscosity (LES) models and per-cell viscosities for ``FractionalStep_AB_CN(..., viscosity_model=...)``.

With a model the step's diffusion operator is ``nu K + K_nut``, ``K_nut = sum_c nut_c K_c`` (``K_c``: the stiffness
matrix of cell ``c``): the Laplacian form ``div(nut grad u)`` of a viscosity that is constant per cell.  The transposed
term ``div(nut grad u^T)`` is left out, as in Oasis's default (DESIGN.md sections 4 and 14)::

    A = M/dt + C/2 + (nu K + K_nut)/2          b = (M/dt - C/2 - (nu K + K_nut)/2) u_1 + b0

Per ``assemble_first``: one kernel writes ``nut_c`` from ``grad u_ab`` at the cell centroids (``ox_eddy_viscosity``,
csrc/ox_viscosity.hip; :class:`CellViscosity` has nothing to evaluate), then the fused assembly kernel adds
``nut_c K_c`` to the convection rows it forms anyway (``ox_assemble_first_*_nut``): no second pass over the pattern, no
second matrix.  ``Delta_c = |cell|^(1/gdim)``.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

__all__ = ["Smagorinsky", "Wale", "CellViscosity"]


def _coefficient(what, v):
    v = float(v)
    if not np.isfinite(v) or v < 0.0:
        raise ValueError(f"{what}: the model constant must be finite and >= 0 (got {v})")
    return v


class _KernelModel:
    """A model whose ``nut`` is a function of ``grad u_ab`` at the cell centroid: evaluated by ``ox_eddy_viscosity``."""

    model_id = None

    def check(self, gdim: int):
        pass

    def bind(self, solver):
        pass

    def evaluate(self, solver, nut: torch.Tensor):
        Vi = solver._Vi[0][0]
        import ctypes as C

        _lib.check(solver._lib.ox_eddy_viscosity(self.model_id, Vi.degree, C.byref(solver._cells), _lib.ptr(Vi.cell_dofs),
                                                 solver._UAB.rptr(), self.coefficient, _lib.ptr(nut),
                                                 _lib.current_stream()), "ox_eddy_viscosity")


class Smagorinsky(_KernelModel):
    """``nut_c = (Cs Delta_c)^2 sqrt(2 S:S)``, ``S = sym(grad u_ab)`` at the cell centroid.  2-D and 3-D, P1 / P2 / P3."""

    model_id = 0

    def __init__(self, Cs: float = 0.1677):
        self.coefficient = _coefficient("Smagorinsky", Cs)

    def __repr__(self):
        return f"Smagorinsky(Cs={self.coefficient})"


class Wale(_KernelModel):
    """Wall-adapting local eddy viscosity (Nicoud & Ducros 1999), 3-D only.  With ``g = grad u_ab`` at the centroid,
    ``Sd = sym(g g) - tr(g g)/3 I``::

        nut_c = (Cw Delta_c)^2 (Sd:Sd)^(3/2) / ((S:S)^(5/2) + (Sd:Sd)^(5/4))        (0 where the denominator is 0)
    """

    model_id = 1

    def __init__(self, Cw: float = 0.325):
        self.coefficient = _coefficient("Wale", Cw)

    def check(self, gdim: int):
        if gdim != 3:
            raise ValueError(f"Wale: the model is defined for three-dimensional flow (the mesh has gdim = {gdim})")

    def __repr__(self):
        return f"Wale(Cw={self.coefficient})"


class CellViscosity:
    """A fixed, non-negative additional viscosity per cell (sponge layers in front of outlets; a way to test the
    operator without a turbulence model).

    Args:
        value: a float, a callable ``f(x)`` on the cell centroids (``x: (3, ncells)``, the mesh's cell order) or an array
            of ``ncells`` values in the mesh's cell order.  Evaluated once, when the solver is built.
    """

    model_id = None

    def __init__(self, value):
        if callable(value):
            self.value = value
        elif np.ndim(value) == 0:
            self.value = float(value)
            self._check_values(np.asarray([self.value]))
        else:
            self.value = np.array(torch.as_tensor(value).detach().cpu().numpy(), dtype=np.float64).reshape(-1)
            self._check_values(self.value)
        self._kernel_order = None

    @staticmethod
    def _check_values(v):
        if not np.isfinite(v).all() or (v < 0.0).any():
            raise ValueError("CellViscosity: the values must be finite and >= 0 "
                             f"(min {float(np.min(v))}): a negative viscosity makes the step ill-posed")

    def values(self, mesh) -> np.ndarray:
        """The ``mesh.num_cells`` values in the mesh's cell order."""
        nc = int(mesh.num_cells)
        if callable(self.value):
            gdim = mesh.geometry.dim
            cen = mesh.coords[mesh.cells.to(torch.int64)].mean(dim=1).cpu().numpy()  # (nc, gdim)
            X = np.zeros((3, nc))
            X[:gdim] = cen.T
            v = np.broadcast_to(np.asarray(self.value(X), dtype=np.float64), (nc,)).copy()
        elif isinstance(self.value, float):
            v = np.full(nc, self.value)
        else:
            v = self.value
            if v.shape[0] != nc:
                raise ValueError(f"CellViscosity: {v.shape[0]} values for a mesh of {nc} cells")
        self._check_values(v)
        return v

    def check(self, gdim: int):
        pass

    def bind(self, solver):
        Vi = solver._Vi[0][0]
        v = torch.from_numpy(self.values(solver._mesh)).to(solver._mesh.device)
        self._kernel_order = v[Vi.local_cells.to(torch.int64)].contiguous()

    def evaluate(self, solver, nut: torch.Tensor):
        nut.copy_(self._kernel_order)

    def __repr__(self):
        return f"CellViscosity({self.value!r})"


def check_model(model, mesh, rotational: bool, scalars) -> None:
    """The scope guards of ``viscosity_model=``; run before anything is built (and before the HIP library is loaded)."""
    if not isinstance(model, (_KernelModel, CellViscosity)):
        raise TypeError("viscosity_model: a Smagorinsky, Wale or CellViscosity object is expected "
                        f"(got {type(model).__name__})")
    if rotational:
        raise NotImplementedError("viscosity_model with rotational=True: the xi nu div(u) term of the rotational pressure "
                                  "update is derived for a constant viscosity")
    if scalars:
        raise NotImplementedError("viscosity_model with scalars=: the turbulent diffusivity of a scalar (a turbulent Schmidt "
                                  "number) is a modelling decision that has not been made here")
    comm = getattr(mesh, "comm", None)
    if comm is not None and getattr(comm, "size", 1) > 1:
        raise NotImplementedError("viscosity_model on a mesh partition (comm.size > 1): the per-cell viscosity is built for "
                                  "one GPU")
    model.check(mesh.geometry.dim)
    if isinstance(model, CellViscosity):
        model.values(mesh)  # a callable or an array of the wrong length / sign fails here, not in the first step
