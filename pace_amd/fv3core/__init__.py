from ._config import (  # noqa: F401
    AcousticDynamicsConfig,
    DGridShallowWaterLagrangianDynamicsConfig,
    DynamicalCoreConfig,
    RemappingConfig,
    RiemannConfig,
    SatAdjustConfig,
)
from .initialization.dycore_state import DycoreState  # noqa: F401,E402
from .initialization.geos_wrapper import GeosDycoreWrapper  # noqa: F401,E402
from .stencils.fv_dynamics import DynamicalCore  # noqa: F401,E402
from .stencils.fv_subgridz import DryConvectiveAdjustment  # noqa: F401,E402
from .stencils.rayleigh_super import RayleighSuper  # noqa: F401,E402
