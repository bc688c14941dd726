"""The reference's `pace.driver`: configuration, state and main loop of a model run.

    from pace.driver import Driver, DriverConfig  ->  from pace_amd.driver import Driver, DriverConfig
"""
from .config import (  # noqa: F401
    BaroclinicInit,
    CreatesCommSelector,
    CubeCommConfig,
    DriverConfig,
    FortranRestartConfig,
    FortranRestartInit,
    GeneratedGridConfig,
    GridInitializerSelector,
    InitializerSelector,
    NullCommConfig,
    PerformanceConfig,
    PredefinedStateInit,
    RestartConfig,
    TorchCommConfig,
)
from .diagnostics import (  # noqa: F401
    Diagnostics,
    DiagnosticsConfig,
    LatLonSelect,
    MonitorDiagnostics,
    NpzMonitor,
    NullDiagnostics,
    PSelect,
    WindowPacker,
    ZSelect,
)
from .driver import Driver, run_cube_driver  # noqa: F401
from .forcing import ForcingConfig  # noqa: F401
from .nudging import Nudging, NudgingConfig  # noqa: F401
from .safety_checks import SafetyChecker, VariableBounds  # noqa: F401
from .state import DriverState, TendencyState  # noqa: F401
