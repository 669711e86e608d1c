"""numpy model of a scalar carried under a per-cell viscosity (oasisx_amd/scalar.py with ``turbulent_schmidt=``,
``ox_scalar_rows_cellvisc`` of csrc/ox_assemble.hip), built on tests/scalar_model.ScalarModel and on
tests/viscosity_model.weighted_stiffness / nut_cells (no GPU):

    A_c = M/dt + C(u_ab)/2 + kappa K/2 + K_w(nut)/(2 Sc_t)          K_w(nut) = sum_c nut_c K_c
    b_c = (2/dt) M c_1 - A_c c_1 + b0_c
    the scalar's own Dirichlet rows -> identity in A_c, boundary value in b_c, as in ``ScalarModel.assemble``.

``Sc_t = inf``: no turbulent part.  ``model``: a tuple of tests/viscosity_model.py, or ``None`` with ``nut`` handed to
``assemble`` / ``step`` (the device's own array, kernel cell order).
"""
import numpy as np

from tests.scalar_model import ScalarModel
from tests.viscosity_model import nut_cells, weighted_stiffness


class _FormsWithTurbulentDiffusion:
    """The oracle's forms with ``convection`` returning C + K_w(nut)/Sc_t: with it ``ScalarModel.assemble`` forms
    M/dt + (C + K_w/Sc_t)/2 + kappa K/2."""

    def __init__(self, forms, kw_over_sct):
        self._F, self._kw = forms, kw_over_sct

    def __getattr__(self, name):
        return getattr(self._F, name)

    def convection(self, uab):
        return self._F.convection(uab) + self._kw


class ScalarLesModel(ScalarModel):
    def __init__(self, forms, x_v, kappa, turbulent_schmidt, model=None, **kw):
        super().__init__(forms, x_v, kappa, **kw)
        self.sct = float(turbulent_schmidt)
        assert self.sct > 0.0
        self.model = model
        self.nut = self.Kw = None

    def assemble(self, uab, dt, nut=None):
        plain = self.F
        self.nut = nut_cells(plain, uab, self.model) if nut is None else np.asarray(nut, dtype=np.float64)
        self.Kw = weighted_stiffness(plain, self.nut)
        self.F = _FormsWithTurbulentDiffusion(plain, (1.0 / self.sct) * self.Kw)
        try:
            return super().assemble(uab, dt)
        finally:
            self.F = plain

    def step(self, uab, dt, nut=None):
        from oracle import ipcs_oracle as O

        self.assemble(uab, dt, nut)
        x0 = self.c1.copy() if self.guess else None
        self.c, self.reason, self.its, _ = O.jacobi_bicgstab(self.A, self.b, x0, self.rtol, self.atol, self.max_it)
        self.c1 = self.c.copy()
        return self.c

    def variance(self):
        """c^T M c of the last completed step."""
        return float(self.c1 @ (self.M @ self.c1))
