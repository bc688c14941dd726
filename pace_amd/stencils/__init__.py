"""The operators the reference keeps in `pace.stencils`: what a driver runs around the dynamical core's step.

    from pace.stencils import ...  ->  from pace_amd.stencils import ...
"""
from ..fv3core.stencils.c2l_ord import CubedToLatLon  # noqa: F401  (it keeps its place and is re-exported here)
from . import c2l_ord, fv_update_phys, held_suarez, physics_coupling, update_atmos_state, update_dwind_phys  # noqa: F401
from .fv_update_phys import ApplyPhysicsToDycore  # noqa: F401
from .held_suarez import HeldSuarezConfig, HeldSuarezForcing  # noqa: F401
from .physics_coupling import CopyDycoreToPhysics, PhysicsToDycore  # noqa: F401
from .update_atmos_state import DycoreToPhysics, UpdateAtmosphereState  # noqa: F401
from .update_dwind_phys import AGrid2DGridPhysics  # noqa: F401
