"""The inputs of tests/test_checkpointer.py's calibration cases, regenerated from their seed.  tools/make_golden_checkpointer.py
runs the reference's ThresholdCalibrationCheckpointer on the same arrays and writes tests/golden/checkpointer_thresholds.npz
(the thresholds only).  numpy only: no test and no device code here.

Three trials, two calls of one savepoint per trial.  The shapes are the smallest at which the kernels can go wrong:

    c12     19 x 19 x 8    the storage of C12 x 7: a row is narrower than one wave
    c68     75 x 75 x 6    the storage of C68 x 5: a row is longer than one wave, a workgroup does not cover a level
    plane   19 x 19        a 2-D field
    xzy     19 x 8 x 19    an [x, z_interface, y] view of a 3-D field
    vec     5              a dense numpy vector
    zeros   19 x 19 x 8    all zero (some of them -0.0): relative is 0.0

and they hold, in every call,

    c12[4, 5, 2]    zero in every trial, among non-zero ones (+0.0, -0.0, +0.0): its quotient 0 / 0 is skipped
    plane[7, 11]    a NaN in trial 1 only: absolute is NaN, relative ignores it
    c68[70, 3, 5]   an inf in trial 2 only: its spread is inf (absolute), its quotient inf / inf is skipped
    xzy[2, 7, 18]   -inf in every trial: its spread is a NaN
    vec[3]          -0.0 in trial 0, a small number after
"""
import numpy as np

SEED = 20261018
SAVEPOINT = "Calibration-In"
N_TRIALS, N_CALLS = 3, 2
SHAPES = {"c12": (19, 19, 8), "c68": (75, 75, 6), "plane": (19, 19), "xzy": (19, 8, 19), "vec": (5,), "zeros": (19, 19, 8)}
NAMES = tuple(SHAPES)


def calibration_inputs(dtype=np.float64):
    """inputs[trial][call][name]: float64 arrays; with dtype=np.float32 their values are rounded to float32 first (what the
    float32 libraries' fields hold: the device widens them again before anything else)."""
    rng = np.random.default_rng(SEED)
    base = {(call, name): rng.uniform(-50.0, 50.0, shape) * 10.0 ** rng.integers(-3, 4, shape)
            for call in range(N_CALLS) for name, shape in SHAPES.items()}
    inputs = []
    for trial in range(N_TRIALS):
        calls = []
        for call in range(N_CALLS):
            arrays = {}
            for name, shape in SHAPES.items():
                a = base[call, name] * (1.0 + rng.uniform(-1.0e-6, 1.0e-6, shape))
                if name == "zeros":
                    a = np.zeros(shape)
                    a[::2] = -0.0
                elif name == "c12":
                    a[4, 5, 2] = -0.0 if trial == 1 else 0.0
                elif name == "plane" and trial == 1:
                    a[7, 11] = np.nan
                elif name == "c68" and trial == 2:
                    a[70, 3, 5] = np.inf
                elif name == "xzy":
                    a[2, 7, 18] = -np.inf
                elif name == "vec":
                    a[3] = -0.0 if trial == 0 else 1.0e-9 * trial
                arrays[name] = a.astype(dtype).astype(np.float64)
            calls.append(arrays)
        inputs.append(calls)
    return inputs
