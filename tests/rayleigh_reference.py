"""The contract of pace_rayleigh_super (include/pace_hip.h) restated sequentially with numpy, in its order, for
tests/test_rayleigh_kernel.py, tests/test_rayleigh_super.py and tests/test_driver_rayleigh_super.py.  Arrays are raw storages
indexed [i, j, k] (planes [i, j]) in the library's storage type; the arithmetic is float64; each stored value is rounded once."""
import math

import numpy as np

RDGAS, CP_AIR = 287.05, 1004.6
RCV = 1.0 / (CP_AIR - RDGAS)
PI = 3.1415926535897931


def factors(pfull, dt, tau, rf_cutoff, ptop):
    """The host side, level by level with the math module: f[k] = 1 / (1 + rf[k]) on the leading run of levels with
    pfull < rf_cutoff, exactly 1.0 elsewhere.  -> (f, rf, kmax) as Python lists / an int."""
    tau0 = tau * 86400.0
    f, rf = [1.0] * len(pfull), [0.0] * len(pfull)
    kmax = 0
    while kmax < len(pfull) and pfull[kmax] < rf_cutoff:
        kmax += 1
    for k in range(kmax):
        rf[k] = dt / tau0 * math.sin(0.5 * PI * math.log(rf_cutoff / pfull[k]) / math.log(rf_cutoff / ptop)) ** 2
        f[k] = 1.0 / (1.0 + rf[k])
    return f, rf, kmax


def kmax_of(factor):
    kmax = 0
    while kmax < len(factor) and factor[kmax] < 1.0:
        kmax += 1
    return kmax


def a_grid_winds(u, v, dx, dy, a11, a12, a21, a22, n, k):
    """u1, v1 -> ua, va of level k on the compute domain (n, n), in float64: pace_c2l_ord order 2's expressions."""
    cs, up = slice(3, 3 + n), slice(4, 4 + n)
    d = np.float64
    with np.errstate(all="ignore"):
        u1 = 2.0 * (u[cs, cs, k].astype(d) * dx[cs, cs].astype(d) + u[cs, up, k].astype(d) * dx[cs, up].astype(d)) \
            / (dx[cs, cs].astype(d) + dx[cs, up].astype(d))
        v1 = 2.0 * (v[cs, cs, k].astype(d) * dy[cs, cs].astype(d) + v[up, cs, k].astype(d) * dy[up, cs].astype(d)) \
            / (dy[cs, cs].astype(d) + dy[up, cs].astype(d))
        ua = a11[cs, cs].astype(d) * u1 + a12[cs, cs].astype(d) * v1
        va = a21[cs, cs].astype(d) * u1 + a22[cs, cs].astype(d) * v1
    return ua, va


def rayleigh_super(u, v, w, pt, dx, dy, a11, a12, a21, a22, factor, n, rcv=RCV, conserve=True):
    """-> (u, v, w, pt) as the call leaves the raw storages it was given (copies).  Level after level; within a level every
    input is read before anything is written."""
    u, v, w, pt = u.copy(), v.copy(), w.copy(), pt.copy()
    cs = slice(3, 3 + n)
    d = np.float64
    for k in range(kmax_of(factor)):
        f = float(factor[k])
        with np.errstate(all="ignore"):
            if conserve:
                ua, va = a_grid_winds(u, v, dx, dy, a11, a12, a21, a22, n, k)
                wk = w[cs, cs, k].astype(d)
                pt[cs, cs, k] = (pt[cs, cs, k].astype(d) + ((0.5 * ((ua * ua + va * va) + wk * wk)) * (1.0 - f * f)) * rcv).astype(pt.dtype)
            w[cs, cs, k] = (f * w[cs, cs, k].astype(d)).astype(w.dtype)
            u[cs, 3:3 + n + 1, k] = (f * u[cs, 3:3 + n + 1, k].astype(d)).astype(u.dtype)
            v[3:3 + n + 1, cs, k] = (f * v[3:3 + n + 1, cs, k].astype(d)).astype(v.dtype)
    return u, v, w, pt
