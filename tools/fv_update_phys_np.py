"""The end of a dycore-only time step restated in numpy: the three stencil groups of UpdateAtmosphereState /
ApplyPhysicsToDycore (stencils/pace/stencils/update_atmos_state.py:19-37, fv_update_phys.py:30-74,
update_dwind_phys.py:446-653), columns and levels vectorised, the sequential sweeps as loops over levels.

tools/make_golden_fvupdatephys.py asserts that these functions reproduce a run of the reference bit for bit (every field
without a transcendental) before it writes a fixture; tests/test_fv_update_phys.py compares the device against them at sizes
for which no fixture exists.  Arrays are full storages (n + 7, n + 7[, nz + 1]), halo 3, changed IN PLACE.
"""
import numpy as np

# util/pace/util/constants.py (GFS_PHYS), as pace_amd/util/constants.py has them
RDGAS, RVGAS, CP_AIR = 287.05, 461.50, 1004.6
KAPPA = RDGAS / CP_AIR
CV_AIR, CV_VAP = CP_AIR - RDGAS, 3.0 * RVGAS
C_ICE, C_LIQ = 1972.0, 4.1855e3
O = 3  # halo

BRANCHES = ("borrow_from_below", "clamp_to_q_min", "borrow_from_above", "zero_negative")


def fill_gfs_delp(delp, q, q_min, store=np.float64):
    """fill_gfs_delp over origin (0, 0, 0), domain (n + 6, n + 6, nz + 1).  Returns, per branch of BRANCHES, the boolean
    (n + 6, n + 6) map of the columns in which it is taken at some level.
    store: the storage type of the fields.  With np.float32 every statement's fp64 result is rounded to float32 where it is
    assigned and q_min is float32(q_min): arithmetic in fp64 on float32 fields, what the float32-storage library does."""
    def r(a):
        return np.asarray(a, dtype=np.float64) if store == np.float64 else np.asarray(a).astype(store).astype(np.float64)

    q_min = float(r(q_min))
    m = q.shape[0] - 1
    K = q.shape[2]
    W = (slice(0, m), slice(0, m))
    d, x = delp[W], q[W]  # views
    taken = {b: np.zeros((m, m), dtype=bool) for b in BRANCHES}
    for k in range(K - 3, -1, -1):  # BACKWARD, interval(0, -2)
        c = x[:, :, k + 1] < q_min
        with np.errstate(all="ignore"):
            x[:, :, k] = np.where(c, r(x[:, :, k] + (x[:, :, k + 1] - q_min) * d[:, :, k + 1] / d[:, :, k]), x[:, :, k])
        taken["borrow_from_below"] |= c
    c = x[:, :, 1:K - 1] < q_min  # PARALLEL, interval(1, -1)
    x[:, :, 1:K - 1] = np.where(c, q_min, x[:, :, 1:K - 1])
    taken["clamp_to_q_min"] |= c.any(axis=2)
    for k in range(1, K - 1):  # FORWARD, interval(1, -1)
        c = x[:, :, k - 1] < 0.0
        with np.errstate(all="ignore"):
            x[:, :, k] = np.where(c, r(x[:, :, k] + x[:, :, k - 1] * d[:, :, k - 1] / d[:, :, k]), x[:, :, k])
        taken["borrow_from_above"] |= c
    c = x[:, :, 0:K - 1] < 0.0  # FORWARD, interval(0, -1)
    x[:, :, 0:K - 1] = np.where(c, 0.0, x[:, :, 0:K - 1])
    taken["zero_negative"] |= c.any(axis=2)
    return taken


def moist_cv(s, t_dt, dt):
    """moist_cv over origin (3, 3, 0), domain (n, n, nz + 1): s["pt"] and t_dt change."""
    n = s["pt"].shape[0] - 7
    W = (slice(O, O + n), slice(O, O + n))
    ql = s["qliquid"][W] + s["qrain"][W]
    qs = s["qice"][W] + s["qsnow"][W] + s["qgraupel"][W]
    gz = ql + qs
    qv = s["qvapor"][W]
    cvm = (1.0 - (qv + gz)) * CV_AIR + qv * CV_VAP + ql * C_LIQ + qs * C_ICE
    s["pt"][W] = s["pt"][W] + t_dt[W] * dt * CP_AIR / cvm
    t_dt[W] = 0.0


def update_pressure_and_surface_winds(s, u_srf, v_srf):
    """update_pressure_and_surface_winds over origin (3, 3, 0), domain (n, n, nz + 1): pe, peln, pk from level 1 on, ps,
    u_srf, v_srf."""
    n = s["pe"].shape[0] - 7
    K = s["pe"].shape[2]
    W = (slice(O, O + n), slice(O, O + n))
    pe, delp = s["pe"][W], s["delp"][W]
    for k in range(1, K):
        pe[:, :, k] = pe[:, :, k - 1] + delp[:, :, k - 1]
    s["peln"][W][:, :, 1:] = np.log(pe[:, :, 1:])
    s["pk"][W][:, :, 1:] = np.exp(KAPPA * s["peln"][W][:, :, 1:])
    s["ps"][W] = pe[:, :, K - 1]
    u_srf[W] = s["ua"][W][:, :, K - 2]
    v_srf[W] = s["va"][W][:, :, K - 2]


def update_dwinds_phys(u, v, u_dt, v_dt, grid, dt5):
    """AGrid2DGridPhysics.__call__ for one tile per rank.  grid: vlon, vlat, es1, ew2 as (n + 7, n + 7, 3) and the four
    edge_vect_* as (n + 7,) arrays.  The blends read unblended neighbours, as the reference's vt / copy sequence does."""
    n = u.shape[0] - 7
    nz = u.shape[2] - 1
    mid = n // 2 + 2  # _im2 = _jm2
    K = slice(0, nz)
    P = slice(O - 1, O + n + 1)  # the prep stencil's window, 2 .. n + 3
    with np.errstate(all="ignore"):
        v3 = [u_dt[:, :, K] * grid["vlon"][:, :, m, None] + v_dt[:, :, K] * grid["vlat"][:, :, m, None] for m in range(3)]
        ue = [np.full(u_dt[:, :, K].shape, np.nan) for _ in range(3)]
        ve = [np.full(u_dt[:, :, K].shape, np.nan) for _ in range(3)]
        for m in range(3):
            ue[m][P, P] = v3[m][P, O - 2:O + n] + v3[m][P, P]
            ve[m][P, P] = v3[m][O - 2:O + n, P] + v3[m][P, P]
    u_dt[P, P, K] = 0.0
    v_dt[P, P, K] = 0.0
    lo, hi = slice(O, mid + 1), slice(mid + 1, O + n)  # the halves of an edge: neighbour at + 1, at - 1
    lo1, hi1 = slice(O + 1, mid + 2), slice(mid, O + n - 1)
    for m in range(3):
        e0 = ve[m].copy()
        for i, ev in ((O, grid["edge_vect_w"]), (O + n, grid["edge_vect_e"])):
            ve[m][i, lo] = ev[lo, None] * e0[i, lo1] + (1.0 - ev[lo, None]) * e0[i, lo]
            ve[m][i, hi] = ev[hi, None] * e0[i, hi1] + (1.0 - ev[hi, None]) * e0[i, hi]
        e0 = ue[m].copy()
        for j, ev in ((O, grid["edge_vect_s"]), (O + n, grid["edge_vect_n"])):
            ue[m][lo, j] = ev[lo, None] * e0[lo1, j] + (1.0 - ev[lo, None]) * e0[lo, j]
            ue[m][hi, j] = ev[hi, None] * e0[hi1, j] + (1.0 - ev[hi, None]) * e0[hi, j]
    U = (slice(O, O + n), slice(O, O + n + 1))
    V = (slice(O, O + n + 1), slice(O, O + n))
    es1, ew2 = grid["es1"], grid["ew2"]
    u[U + (K,)] = u[U + (K,)] + dt5 * (ue[0][U] * es1[U + (0, None)] + ue[1][U] * es1[U + (1, None)] + ue[2][U] * es1[U + (2, None)])
    v[V + (K,)] = v[V + (K,)] + dt5 * (ve[0][V] * ew2[V + (0, None)] + ve[1][V] * ew2[V + (1, None)] + ve[2][V] * ew2[V + (2, None)])


def apply_before_halo(s, t_dt, dt, u_srf, v_srf):
    """What ApplyPhysicsToDycore does before it waits for the halo updates of u_dt, v_dt."""
    moist_cv(s, t_dt, dt)
    update_pressure_and_surface_winds(s, u_srf, v_srf)


# ---- inputs every machine rebuilds with the same bits: integers of (tile, i, j, k) over powers of two, no transcendental -------
def _h(tile, shape):
    i, j, k = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), np.arange(shape[2]), indexing="ij")
    return 3 * tile + 5 * i + 11 * j + 17 * k


def tendencies(tile, shape):
    """u_dt, v_dt (m/s^2, up to 8e-3) and t_dt (K/s, up to 2e-3) on the whole storage."""
    h = _h(tile, shape)
    u_dt = ((h * 37) % 257 - 128) / 2.0 ** 14
    v_dt = ((h * 53 + 11) % 263 - 131) / 2.0 ** 14
    t_dt = ((h * 17 + 5) % 251 - 125) / 2.0 ** 16
    return u_dt, v_dt, t_dt


def perturb(tile, s):
    """The state UpdateAtmosphereState is run on, from a state `s` (name -> full array) that is left as it is: qvapor scaled
    so that fill_gfs_delp takes each of its branches (negative at one point in seven, below q_min = 1e-9 at another), delp
    and qvapor given values in the halo (fill_gfs_delp covers it; the generated state has 0 and 1e30 there), ua and va set
    (the generated state leaves them unset)."""
    n = s["delp"].shape[0] - 7
    out = {k: np.array(v, dtype=float) for k, v in s.items()}
    shape = out["delp"].shape
    h = _h(tile, shape)
    halo = np.ones(shape, dtype=bool)
    halo[O:O + n, O:O + n, :] = False
    out["delp"] = np.where(halo, 64.0 + (h % 128), out["delp"])
    qv = out["qvapor"]
    qv = np.where(h % 7 == 0, qv * (-(1 + h % 4) / 8.0), qv)
    qv = np.where(h % 7 == 3, qv * 2.0 ** -30, qv)
    out["qvapor"] = np.where(halo, ((h * 41) % 128 - 16) / 2.0 ** 20, qv)
    # winds that vary from column to column but are smooth in the vertical (1/8 m/s per level): no shear-driven mixing
    h0 = _h(tile, shape[:2] + (1,))  # (level 0: h - h0 = 17 k)
    out["ua"] = ((h0 * 19) % 101 - 50) / 4.0 + (h - h0) / 136.0
    out["va"] = ((h0 * 23) % 103 - 51) / 4.0 - (h - h0) / 272.0
    return out


def perturb_for_adjustment(tile, s):
    """What the dry convective adjustment needs on top of perturb(): pkz as the mean of pk at the layer's interfaces, and pt
    moved by -4 ... 4 K from level to level in every third column, so that those columns mix."""
    n = s["delp"].shape[0] - 7
    out = {k: np.array(v, dtype=float) for k, v in s.items()}
    shape = out["delp"].shape
    h = _h(tile, shape)
    i, j, _ = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), np.arange(shape[2]), indexing="ij")
    out["pt"] = np.where((i + 2 * j + tile) % 3 == 0, out["pt"] + 2.0 * (h % 5 - 2), out["pt"])
    pkz = np.ones(shape)
    pkz[:, :, :-1] = 0.5 * (out["pk"][:, :, :-1] + out["pk"][:, :, 1:])
    inside = np.zeros(shape, dtype=bool)
    inside[O:O + n, O:O + n, :-1] = True
    out["pkz"] = np.where(inside, pkz, 1.0)
    return out
