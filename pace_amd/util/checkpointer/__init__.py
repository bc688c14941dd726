"""The checkpointer family of pace.util (util/pace/util/checkpointer/): same names, same signatures; calibration and validation
run on the device (pace_amd/csrc/k_ckpt.hip)."""
from .base import Checkpointer  # noqa: F401
from .null import NullCheckpointer  # noqa: F401
from .snapshots import SnapshotCheckpointer  # noqa: F401
from .thresholds import InsufficientTrialsError, SavepointThresholds, Threshold, ThresholdCalibrationCheckpointer  # noqa: F401
from .validation import ValidationCheckpointer  # noqa: F401
