from .constants import *  # noqa: F401,F403
from .quantity import Quantity, QuantityFactory, SubtileGridSizer  # noqa: F401
from .comm import DeviceCubeComm, LoopbackComm, NullComm, ThreadComm, TorchDistComm, run_cube, run_tiles  # noqa: F401,E402
from .halo import CubedSphereCommunicator, HaloUpdater, QuantityHaloSpec, WrappedHaloUpdater  # noqa: F401,E402
from .partitioner import CubedSpherePartitioner, RingPartitioner, TilePartitioner  # noqa: F401,E402
from ._timing import KernelTimes, NullTimer, Timer  # noqa: F401,E402
from .checkpointer import (Checkpointer, InsufficientTrialsError, NullCheckpointer, SavepointThresholds, SnapshotCheckpointer,  # noqa: F401,E402
                           Threshold, ThresholdCalibrationCheckpointer, ValidationCheckpointer)
from .restart import LevelOf, open_restart, write_restart  # noqa: F401,E402
from .nudging import apply_nudging, get_nudging_tendencies  # noqa: F401,E402
from .gather import Window, check_cube_items  # noqa: F401,E402
from .latlon import LatLonGrid, build_regrid_table, check_regrid_table  # noqa: F401,E402
from .monitor import NetCDFMonitor  # noqa: F401,E402
from . import testing  # noqa: F401,E402
