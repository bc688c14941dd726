"""The contract of pace_held_suarez (include/pace_hip.h) restated with numpy, in its order, for tests/test_held_suarez_kernel.py
and tests/test_held_suarez.py.  Arrays are raw storages indexed [i, j, k] (planes [i, j]) in the library's storage type; the
arithmetic is float64."""
import dataclasses

import numpy as np

RDGAS, CP_AIR = 287.05, 1004.6
CV_AIR = CP_AIR - RDGAS


@dataclasses.dataclass
class Constants:
    dt: float = 225.0
    p0: float = 1.0e5
    kappa: float = RDGAS / CP_AIR
    sigma_b: float = 0.7
    k_f: float = 1.0 / 86400.0
    k_a: float = 1.0 / (40.0 * 86400.0)
    k_s: float = 1.0 / (4.0 * 86400.0)
    delta_t_y: float = 60.0
    delta_theta_z: float = 10.0
    t0: float = 315.0
    t_strat: float = 200.0
    heating_scale: float = 1.0


def terms(c, pe, s2, c2, n, nk, lp=None, pk=None, teq=None):
    """On the compute domain (n, n, nk), in float64: dict of ps, pm, sigma, lp, pk, x, teq, h, kv, kt.  lp and pk come from np.log /
    np.exp unless they are handed in; a teq handed in replaces the clamped x."""
    cs = slice(3, 3 + n)
    pe = pe[cs, cs, :nk + 1].astype(np.float64)
    s2 = s2[cs, cs].astype(np.float64)[:, :, None]
    c2 = c2[cs, cs].astype(np.float64)[:, :, None]
    with np.errstate(all="ignore"):
        ps = pe[:, :, nk:nk + 1]
        pm = 0.5 * (pe[:, :, :nk] + pe[:, :, 1:nk + 1])
        sigma = pm / ps
        if lp is None:
            lp = np.log(pm / c.p0)
        if pk is None:
            pk = np.exp(c.kappa * lp)
        x = ((c.t0 - c.delta_t_y * s2) - (c.delta_theta_z * lp) * c2) * pk
        if teq is None:
            teq = np.where(x < c.t_strat, c.t_strat, x)
        hx = (sigma - c.sigma_b) / (1.0 - c.sigma_b)
        h = np.where(hx < 0.0, 0.0, hx)
        kv = c.k_f * h
        kt = c.k_a + ((c.k_s - c.k_a) * h) * (c2 * c2)
    return dict(ps=ps, pm=pm, sigma=sigma, lp=lp, pk=pk, x=x, teq=teq, hx=hx, h=h, kv=kv, kt=kt, s2=s2, c2=c2)


def held_suarez(c, pe, ua, va, pt, s2, c2, u_dt, v_dt, pt_dt, teq_out, n, nk, accumulate, lp=None, pk=None, teq=None):
    """-> (u_dt, v_dt, pt_dt, teq_out) as the launch leaves the raw storages it was given (copies; teq_out None stays None)."""
    cs = slice(3, 3 + n)
    t = terms(c, pe, s2, c2, n, nk, lp, pk, teq)
    win = (cs, cs, slice(0, nk))
    with np.errstate(all="ignore"):
        du = -((t["kv"] * ua[win].astype(np.float64)) / (1.0 + t["kv"] * c.dt))
        dv = -((t["kv"] * va[win].astype(np.float64)) / (1.0 + t["kv"] * c.dt))
        dpt = -(((t["kt"] * (pt[win].astype(np.float64) - t["teq"])) / (1.0 + t["kt"] * c.dt)) * c.heating_scale)
        out = []
        for old, value in ((u_dt, du), (v_dt, dv), (pt_dt, dpt)):
            new = old.copy()
            new[win] = ((old[win].astype(np.float64) + value) if accumulate else value).astype(old.dtype)
            out.append(new)
        if teq_out is not None:
            new = teq_out.copy()
            new[win] = t["teq"].astype(teq_out.dtype)
            out.append(new)
        else:
            out.append(None)
    return tuple(out)
