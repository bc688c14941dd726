"""Generate tests/golden/nudging_reference.npz by RUNNING THE REFERENCE's apply_nudging and get_nudging_tendencies
(util/pace/util/nudging.py) in this container on the inputs of tests/nudging_cases.py, regenerated from their seed.  The file
holds results only: per variable the nudged state's compute domain (state_<name>; the reference writes nothing else), the
tendencies' view (tendency_<name>: apply_nudging's, which get_nudging_tendencies on the un-nudged state is asserted to equal bit
for bit), and the tendencies' dims and units.  Data only.

    python tools/make_golden_nudging.py            write the file
    python tools/make_golden_nudging.py --check    compute again and compare with the file, bit for bit
"""
import os
import sys
import warnings
from datetime import timedelta

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402

PATH = os.path.join(HERE, "..", "tests", "golden", "nudging_reference.npz")


def compute():
    import refshim

    refshim.install()
    import nudging_cases as cases
    from pace.util import Quantity, apply_nudging, get_nudging_tendencies

    def quantities(arrays):
        return {name: Quantity(arrays[name].copy(), dims=cases.VARIABLES[name][0], units=cases.VARIABLES[name][1],
                               origin=cases.ORIGIN, extent=cases.VARIABLES[name][2]) for name in cases.NAMES}

    state_in, reference_in = cases.inputs()
    timescales = {name: timedelta(seconds=cases.VARIABLES[name][3]) for name in cases.NAMES}
    state, reference = quantities(state_in), quantities(reference_in)
    only = get_nudging_tendencies(state, reference, timescales)
    assert all(np.array_equal(state[name].data, state_in[name]) for name in cases.NAMES)
    applied = apply_nudging(state, reference, timescales, timedelta(seconds=cases.TIMESTEP_SECONDS))
    out = {"names": np.asarray(cases.NAMES)}
    for name in cases.NAMES:
        assert np.array_equal(np.asarray(only[name].view[:]), np.asarray(applied[name].view[:]))
        assert tuple(only[name].dims) == tuple(applied[name].dims) and only[name].units == applied[name].units
        after = np.asarray(state[name].data)
        outside = np.ones(after.shape, dtype=bool)
        cases.view(name, outside)[...] = False
        assert np.array_equal(after[outside], state_in[name][outside])  # the reference writes the compute domain only
        assert np.array_equal(np.asarray(reference[name].data), reference_in[name])
        out[f"state_{name}"] = np.ascontiguousarray(cases.view(name, after), dtype=np.float64)
        out[f"tendency_{name}"] = np.ascontiguousarray(np.asarray(applied[name].view[:]), dtype=np.float64)
        out[f"dims_{name}"] = np.asarray(tuple(applied[name].dims))
        out[f"units_{name}"] = np.asarray(applied[name].units)
    return out


def main():
    new = compute()
    if "--check" in sys.argv[1:]:
        old = dict(np.load(PATH, allow_pickle=False))
        assert sorted(old) == sorted(new), (sorted(old), sorted(new))
        for key, value in new.items():
            same = (np.array_equal(old[key].view(np.uint64), value.view(np.uint64)) if value.dtype == np.float64 else
                    np.array_equal(old[key], value))
            assert same, (key, old[key], value)
        print("nudging_reference.npz: the reference gives the same states and tendencies again")
        return
    np.savez(PATH, **new)
    for key, value in new.items():
        print(key, value.shape, value.dtype)
    print(os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
