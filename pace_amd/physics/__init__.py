"""The reference's `pace.physics`: the GFDL cloud microphysics and the Physics shell around it, on the device.

    from pace.physics import PhysicsConfig, PhysicsState                    ->  from pace_amd.physics import ...
    from pace.physics.stencils.microphysics import Microphysics, MicrophysicsState
    from pace.physics.stencils.physics import Physics

Physics(...)(physics_state, timestep) is atmos_phys_driver_statein, get_prs_fv3, get_phi_fv3 and prepare_microphysics in one
launch, the microphysics in one, update_physics_state_with_tendencies in one.  What carries a dycore state into a PhysicsState
and its result back is in pace_amd.stencils: CopyDycoreToPhysics and PhysicsToDycore.
"""
from ._config import PhysicsConfig  # noqa: F401
from .stencils.microphysics import Microphysics, MicrophysicsState  # noqa: F401
from .physics_state import PhysicsState  # noqa: F401,E402
from .stencils.physics import Physics  # noqa: F401,E402
