"""pace_nudge restated in numpy (include/pace_hip.h): the four lines of the contract over a window of whole raw storages.
Everything is computed in double on the stored values and cast on the store; numpy neither contracts nor takes reciprocals."""
import numpy as np


def nudge(field, ref0, ref1, window, timescale, weight, dt, apply, tendency=None):
    """field, ref0, ref1 (or None), tendency (or None): raw storages indexed [i, j, k] ([i, j] for a plane) of one dtype.
    window: (i0, j0, k0, ni, nj, nk).  -> (field after, tendency after): copies; outside the window they are the inputs."""
    i0, j0, k0, ni, nj, nk = window
    box = (slice(i0, i0 + ni), slice(j0, j0 + nj)) + ((slice(k0, k0 + nk),) if field.ndim == 3 else ())
    dtype = field.dtype
    q = field[box].astype(np.float64)
    r0 = ref0[box].astype(np.float64)
    with np.errstate(all="ignore"):
        if ref1 is not None:
            r1 = ref1[box].astype(np.float64)
            r = r0 + (r1 - r0) * np.float64(weight)
        else:
            r = r0
        t = (r - q) / np.float64(timescale)
        out_field = field.copy()
        out_tendency = None if tendency is None else tendency.copy()
        if out_tendency is not None:
            out_tendency[box] = t.astype(dtype)
        if apply:
            out_field[box] = (q + t * np.float64(dt)).astype(dtype)
    return out_field, out_tendency
