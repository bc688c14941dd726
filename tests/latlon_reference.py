"""A numpy restatement of pace_cube_regrid's contract (include/pace_hip.h), as tests/plev_reference.py is for pace_plev_diag:
the same table, the same order of operations, explicit float64.

    dense[offset + p * nk + k] = (dense type)((w0 * f_0(k0 + k) + w1 * f_1(k0 + k)) + w2 * f_2(k0 + k))

with f_m the stored value of source m widened to float64 first, products then adds (numpy never fuses them), a plain cast at the
end.  NaN and inf propagate by ordinary arithmetic: 0 * NaN and 0 * inf are NaN."""
import numpy as np


def regrid(fields6, tile, i, j, w, k0=0, nk=None, dense_dtype=np.float64):
    """fields6: the six tiles' arrays indexed [i, j, k] (3-D) or [i, j] (2-D, a plane) in STORAGE indices; tile, i, j, w: the
    table's [npoints, 3] columns.  Returns [npoints, nk] (3-D) or [npoints] (2-D) in `dense_dtype`."""
    stacked = np.stack([np.asarray(f) for f in fields6])
    plane = stacked.ndim == 3
    if plane:
        stacked = stacked[..., None]
        k0, nk = 0, 1
    elif nk is None:
        nk = stacked.shape[3] - k0
    tile, i, j = (np.asarray(a, dtype=np.int64) for a in (tile, i, j))
    w = np.asarray(w, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        f = [stacked[tile[:, m], i[:, m], j[:, m], k0:k0 + nk].astype(np.float64) for m in range(3)]
        a = [w[:, m, None] * f[m] for m in range(3)]
        out = ((a[0] + a[1]) + a[2]).astype(dense_dtype)
    return out[:, 0] if plane else out
