"""Generate tests/golden/checkpointer_thresholds.npz by RUNNING THE REFERENCE's ThresholdCalibrationCheckpointer
(util/pace/util/checkpointer/thresholds.py:59-162) in this container on the inputs of tests/checkpointer_cases.py -- three
trials, two calls of one savepoint per trial, regenerated from their seed -- once as they are and once rounded to float32 (what
the float32 libraries' fields hold).  The file holds the thresholds only: relative_f64 / absolute_f64 / relative_f32 /
absolute_f32, each [call, variable], and the variables' names.  Data only.

    python tools/make_golden_checkpointer.py            write the file
    python tools/make_golden_checkpointer.py --check    compute again and compare with the file, bit for bit

The reference's ValidationCheckpointer needs xarray and cannot run here; its yardstick in the tests is numpy's own
assert_allclose.
"""
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402

PATH = os.path.join(HERE, "..", "tests", "golden", "checkpointer_thresholds.npz")


def compute():
    import refshim

    refshim.install()
    import checkpointer_cases as cases
    from pace.util import ThresholdCalibrationCheckpointer

    out = {"names": np.asarray(cases.NAMES)}
    for tag, dtype in (("f64", np.float64), ("f32", np.float32)):
        calibration = ThresholdCalibrationCheckpointer(factor=1.0)
        for calls in cases.calibration_inputs(dtype):
            with calibration.trial():
                for arrays in calls:
                    with np.errstate(all="ignore"):
                        calibration(cases.SAVEPOINT, **arrays)
        with np.errstate(all="ignore"):
            found = calibration.thresholds.savepoints[cases.SAVEPOINT]
        assert len(found) == cases.N_CALLS
        out[f"relative_{tag}"] = np.array([[call[name].relative for name in cases.NAMES] for call in found])
        out[f"absolute_{tag}"] = np.array([[call[name].absolute for name in cases.NAMES] for call in found])
    return out


def main():
    new = compute()
    if "--check" in sys.argv[1:]:
        old = dict(np.load(PATH, allow_pickle=False))
        assert sorted(old) == sorted(new), (sorted(old), sorted(new))
        for key, value in new.items():
            same = (np.array_equal(old[key], value) if key == "names" else
                    np.array_equal(old[key].view(np.uint64), value.view(np.uint64)))
            assert same, (key, old[key], value)
        print("checkpointer_thresholds.npz: the reference gives the same thresholds again")
        return
    np.savez(PATH, **new)
    for key, value in new.items():
        print(key, value, sep="\n")


if __name__ == "__main__":
    main()
