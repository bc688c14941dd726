"""The reference's `pace.physics`: the GFDL cloud microphysics on the device.

    from pace.physics import PhysicsConfig                                  ->  from pace_amd.physics import ...
    from pace.physics.stencils.microphysics import Microphysics, MicrophysicsState

The Physics shell around the microphysics (PhysicsState, atmos_phys_driver_statein, get_prs_fv3, get_phi_fv3) and the
dycore_only = False halves of the end-of-step operators are not here yet.
"""
from ._config import PhysicsConfig  # noqa: F401
from .stencils.microphysics import Microphysics, MicrophysicsState  # noqa: F401
