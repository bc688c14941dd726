"""numpy / Python restatement of the total-energy fixer (include/pace_hip.h: pace_energy_columns, pace_energy_finalize,
pace_l2e_finish_dtmp): the column pass as a sequential loop over k with numpy over the plane, the accumulator with Python ints,
the decode with exact integer arithmetic and one correctly rounded conversion.  Test infrastructure.

Arrays are indexed [i, j(, k)] on the full storage shape (n + 7, n + 7(, nk + 1)); arithmetic is float64 on the values handed in
(the float32 library's tests hand in what its storages hold, widened)."""
import math
from fractions import Fraction

import numpy as np

from pace_amd.util import constants as c

WATER = ("qvapor", "qliquid", "qrain", "qsnow", "qice", "qgraupel")
LIMB_BITS = 40
LIMB_MASK = (1 << LIMB_BITS) - 1
MAX_ADDENDS = 1 << 23


def column_energy(mode, f, n, nk, zvir=c.ZVIR):
    """(te, zsum) on the compute domain, (n, n) each, float64.  f: dict of float64 arrays by name -- the six species, pt, delp,
    delz, w, u, v, phis, rsin2, cosa_s and (mode 1) pkz."""
    cs = slice(3, 3 + n)
    d = {k: np.asarray(v, dtype=np.float64) for k, v in f.items()}
    rsin2, cosa = d["rsin2"][cs, cs], d["cosa_s"][cs, cs]
    phi_below = d["phis"][cs, cs].copy()
    te = np.zeros((n, n))
    zsum = np.zeros((n, n))
    with np.errstate(all="ignore"):
        for k in range(nk - 1, -1, -1):
            delz, delp, pt, w = (d[name][cs, cs, k] for name in ("delz", "delp", "pt", "w"))
            u0, u1 = d["u"][cs, cs, k], d["u"][cs, 4:4 + n, k]
            v0, v1 = d["v"][cs, cs, k], d["v"][4:4 + n, cs, k]
            qv = d["qvapor"][cs, cs, k]
            ql = d["qliquid"][cs, cs, k] + d["qrain"][cs, cs, k]
            qs = (d["qice"][cs, cs, k] + d["qsnow"][cs, cs, k]) + d["qgraupel"][cs, cs, k]
            phi_above = phi_below - c.GRAV * delz
            ke = (0.5 * rsin2) * ((((u0 * u0 + u1 * u1) + v0 * v0) + v1 * v1) - ((u0 + u1) * (v0 + v1)) * cosa)
            gz = ql + qs
            cvm = (1.0 - (qv + gz)) * c.CV_AIR + qv * c.CV_VAP + ql * c.C_LIQ + qs * c.C_ICE
            e = cvm * pt
            if mode == 1:
                e = e / ((1.0 + zvir * qv) * (1.0 - gz))
            te = te + delp * (e + 0.5 * (((phi_above + phi_below) + w * w) + ke))
            if mode == 1:
                zsum = zsum + d["pkz"][cs, cs, k] * delp
            phi_below = phi_above
    return te, zsum


def encode(v):
    """The five integers one addend contributes."""
    v = float(v)
    if not math.isfinite(v) or abs(v) >= 2.0 ** 120:
        return [0, 0, 0, 0, 1]
    m = int(math.ldexp(abs(v), LIMB_BITS))  # exact scaling, truncated toward zero
    limbs = [(m >> (LIMB_BITS * n)) & LIMB_MASK for n in range(4)]
    return [-x for x in limbs] + [0] if v < 0 else limbs + [0]


def accumulate(values):
    """The five words of the sum of `values` (any iterable of floats), as Python ints."""
    words = [0] * 5
    for v in np.asarray(values, dtype=np.float64).ravel():
        for n, x in enumerate(encode(v)):
            words[n] += x
    return words


def decode(words):
    """The value of five (already summed) words: exact integer, one rounding to nearest-even."""
    if words[4] != 0:
        return float("nan")
    m = sum(int(words[n]) << (LIMB_BITS * n) for n in range(4))
    return float(Fraction(m, 1 << LIMB_BITS))  # (Fraction -> float is correctly rounded)


def mode1(f, te0_2d, area, n, nk, zvir=c.ZVIR):
    """-> (te_2d, zsum1, the ten words) of a mode-1 launch: float64 planes on the compute domain, Python ints."""
    cs = slice(3, 3 + n)
    te, zsum = column_energy(1, f, n, nk, zvir)
    with np.errstate(all="ignore"):
        te_2d = np.asarray(te0_2d, dtype=np.float64)[cs, cs] - te
        a = np.asarray(area, dtype=np.float64)[cs, cs]
        words = accumulate(a * te_2d) + accumulate(a * zsum)
    return te_2d, zsum, words


def finalize(word_sets, consv_te, dt_atmos):
    """(S_te, S_z, dtmp, e_flux) from the ten words of each tile, in Python floats."""
    total = [sum(int(w[m]) for w in word_sets) for m in range(10)]
    s_te, s_z = decode(total[:5]), decode(total[5:])
    return s_te, s_z, dtmp_of(s_te, s_z, consv_te), e_flux_of(s_te, consv_te, dt_atmos)


def dtmp_of(s_te, s_z, consv_te):
    den = c.CV_AIR * s_z
    num = consv_te * s_te
    with np.errstate(all="ignore"):  # (0 / 0 and x / 0 as IEEE has them, not as Python raises them)
        return float(np.float64(num) / np.float64(den))


def e_flux_of(s_te, consv_te, dt_atmos):
    return (consv_te * s_te) / ((((c.GRAV * dt_atmos) * 4.0) * c.PI) * (c.RADIUS * c.RADIUS))


def last_step_pt(pt, pkz, qvapor, gz, dtmp, zvir=c.ZVIR):
    """pace_l2e_finish_dtmp's temperature from float64 arrays."""
    with np.errstate(all="ignore"):
        return (pt + dtmp * pkz) / ((1.0 + zvir * qvapor) * (1.0 - gz))


def flat_gz(tr):
    """pace_l2e_finish's condensate sum, in its order."""
    return (((tr["qliquid"] + tr["qrain"]) + tr["qice"]) + tr["qsnow"]) + tr["qgraupel"]
