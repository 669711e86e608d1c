"""oasisx_amd -- the per-time-step IPCS hot path of oasisx on AMD Instinct MI355X (gfx950).

Same names as reference src/oasisx/__init__.py:12-18; the compute path is the HIP library
``liboasisx_hip.so`` (see include/oasisx_hip.h) and fails loudly when it is missing.
"""
import logging

from . import fem, geometry, io, mesh  # noqa: F401
from .bcs import DirichletBC, LocatorMethod, PressureBC
from .diagnostics import FlowDiagnostics, FlowStatistics, ProfileStatistics, slab_bins
from .drag import DragZone
from .fracstep import FractionalStep_AB_CN
from .function import Projector
from .geometry import Probes, WallDistance  # noqa: F401
from .ksp import KSPSolver  # noqa: F401
from .outlet import FlowRate, Resistance, Windkessel
from .particles import DEPOSITED, InertialParticles
from .reaction import Reaction, ReactionNetwork
from .scalar import SUPG, FluxBC, RobinBC, ScalarFlux, ScalarTransport
from .tracers import Tracers
from .viscosity import (CarreauYasuda, CellViscosity, Cross, DynamicSmagorinsky, PatchFilter, PowerLaw, Smagorinsky, VanDriest,
                        Wale)
from .wall import WallStress

logging.basicConfig()
logger = logging.getLogger("oasisx")
logging.captureWarnings(capture=True)

__all__ = [
    "Projector",
    "FractionalStep_AB_CN",
    "DirichletBC",
    "LocatorMethod",
    "PressureBC",
    "ScalarTransport",
    "SUPG",
    "ScalarFlux",
    "FluxBC",
    "RobinBC",
    "Reaction",
    "ReactionNetwork",
    "Smagorinsky",
    "DynamicSmagorinsky",
    "PatchFilter",
    "Wale",
    "VanDriest",
    "WallDistance",
    "CellViscosity",
    "DragZone",
    "CarreauYasuda",
    "Cross",
    "PowerLaw",
    "WallStress",
    "FlowRate",
    "Resistance",
    "Windkessel",
    "Tracers",
    "InertialParticles",
    "DEPOSITED",
    "FlowDiagnostics",
    "FlowStatistics",
    "ProfileStatistics",
    "slab_bins",
]
