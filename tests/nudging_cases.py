"""The inputs of tests/test_nudging.py's golden case, regenerated from their seed.  tools/make_golden_nudging.py runs the
reference's apply_nudging and get_nudging_tendencies (util/pace/util/nudging.py) on the same arrays and writes
tests/golden/nudging_reference.npz (results only).  numpy only: no test and no device code here.

Three variables on the storage of C12 x 5, (19, 19, 6) with origin (3, 3, 0) -- one cell-centred, one staggered in y (the D-grid
u), one staggered in x (the D-grid v) -- with different timescales, and one timestep."""
import numpy as np

SEED = 20261020
N, NZ, HALO = 12, 5, 3
SHAPE = (N + 2 * HALO + 1, N + 2 * HALO + 1, NZ + 1)
TIMESTEP_SECONDS = 450.0
# name -> (dims, units, extent of the compute domain, timescale in seconds, typical magnitude)
VARIABLES = {
    "air_temperature": (("x", "y", "z"), "degK", (N, N, NZ), 21600.0, 280.0),
    "x_wind": (("x", "y_interface", "z"), "m/s", (N, N + 1, NZ), 7200.0, 30.0),
    "y_wind": (("x_interface", "y", "z"), "m/s", (N + 1, N, NZ), 10800.0, 30.0),
}
ORIGIN = (HALO, HALO, 0)
NAMES = tuple(VARIABLES)


def inputs(dtype=np.float64):
    """-> (state, reference): name -> float64 array of SHAPE, halo and level nz filled as well; with dtype=np.float32 the values
    are rounded to float32 first (what the float32 library's fields hold)."""
    rng = np.random.default_rng(SEED)
    state, reference = {}, {}
    for name, (_, _, _, _, magnitude) in VARIABLES.items():
        state[name] = (magnitude * rng.uniform(-1.0, 1.0, SHAPE)).astype(dtype).astype(np.float64)
        reference[name] = (state[name] + 0.01 * magnitude * rng.standard_normal(SHAPE)).astype(dtype).astype(np.float64)
    return state, reference


def view(name, array):
    """The compute domain of a storage of variable `name`."""
    extent = VARIABLES[name][2]
    return array[tuple(slice(o, o + e) for o, e in zip(ORIGIN, extent))]
