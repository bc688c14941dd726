"""The Physics shell and the physics-to-dycore coupling restated in numpy, statement by statement from the semantics of the
reference's stencils (physics/pace/physics/stencils/physics.py:33-201, get_prs_fv3.py, get_phi_fv3.py;
stencils/pace/stencils/update_atmos_state.py:40-92): fp64, the reference's operand order, its divisions kept.  The yardstick of
tests/test_physics.py and tests/test_physics_coupling.py where no fixture exists; tests/test_physics.py holds it to the
fixtures (tools/make_golden_physics.py, runs of the reference) bit for bit.

Every function works on the compute domain: layer fields are (nx, ny, nk), the interface fields prsi and phii (nx, ny, nk + 1).
Fields are updated in place in the dict `s`."""
import numpy as np

GRAV = 9.80665
RGRAV = 1.0 / GRAV
RDGAS = 287.05
RVGAS = 461.50
ZVIR = RVGAS / RDGAS - 1

MASS_WEIGHTED = ["qvapor", "qliquid", "qrain", "qice", "qsnow", "qgraupel", "qo3mr"]
TENDENCIES = ["qv_dt", "ql_dt", "qr_dt", "qi_dt", "qs_dt", "qg_dt", "qa_dt", "udt", "vdt", "pt_dt"]
UPDATED = [("qvapor", "qv_dt", "physics_updated_specific_humidity"), ("qliquid", "ql_dt", "physics_updated_qliquid"),
           ("qrain", "qr_dt", "physics_updated_qrain"), ("qice", "qi_dt", "physics_updated_qice"),
           ("qsnow", "qs_dt", "physics_updated_qsnow"), ("qgraupel", "qg_dt", "physics_updated_qgraupel"),
           ("qcld", "qa_dt", "physics_updated_cloud_fraction"), ("pt", "pt_dt", "physics_updated_pt"),
           ("ua", "udt", "physics_updated_ua"), ("va", "vdt", "physics_updated_va")]
COPIED = ["qvapor", "qliquid", "qrain", "qsnow", "qice", "qgraupel", "qo3mr", "qsgs_tke", "qcld", "pt", "delp", "delz", "ua", "va",
          "w", "omga"]
SUM_ORDER = ["qvapor", "qliquid", "qrain", "qsnow", "qice", "qgraupel"]


def statein(s, ptop):
    """atmos_phys_driver_statein with nwat = 6, without prsik.  Returns the masks of the two clamps of the mid-layer pressure
    (upper, lower)."""
    nk = s["pt"].shape[2]
    phii = np.zeros(s["pt"].shape[:2] + (nk + 1,))
    for k in range(nk - 1, -1, -1):
        phii[:, :, k] = phii[:, :, k + 1] - s["delz"][:, :, k] * GRAV
    delp = s["delp"]
    for name in MASS_WEIGHTED:
        s[name] = s[name] * delp
    delp = delp - s["qliquid"] - s["qrain"] - s["qice"] - s["qsnow"] - s["qgraupel"]
    prsi = np.empty_like(phii)
    prsi[:, :, 0] = ptop
    for k in range(1, nk + 1):
        prsi[:, :, k] = prsi[:, :, k - 1] + delp[:, :, k - 1]
    for name in MASS_WEIGHTED + ["qsgs_tke"]:
        s[name] = s[name] / delp
    qgrs_rad = np.maximum(1.0e-10, s["qvapor"])
    rtv = RDGAS * s["pt"] * (1.0 + ZVIR * qgrs_rad)
    dm = delp
    delp = dm * rtv / (phii[:, :, :-1] - phii[:, :, 1:])
    upper = prsi[:, :, 1:] - 0.01 * dm
    clamped_hi = delp > upper
    delp = np.minimum(delp, upper)
    lower = prsi[:, :, :-1] + 0.01 * dm
    clamped_lo = delp < lower
    delp = np.maximum(delp, lower)
    s["delp"], s["prsi"], s["phii"] = delp, prsi, phii
    return clamped_hi, clamped_lo


def get_prs_fv3(s):
    """Returns del_gz (the reference's scratch)."""
    s["delprsi"] = s["prsi"][:, :, 1:] - s["prsi"][:, :, :-1]
    return (s["phii"][:, :, :-1] - s["phii"][:, :, 1:]) / (s["pt"] * (1.0 + ZVIR * np.maximum(0.0, s["qvapor"])))


def get_phi_fv3(s, del_gz):
    nk = s["pt"].shape[2]
    del_gz = del_gz * s["pt"] * (1.0 + ZVIR * np.maximum(0.0, s["qvapor"]))
    phii, phil = s["phii"], np.empty_like(s["pt"])
    phii[:, :, nk] = 0.0
    for k in range(nk - 1, -1, -1):
        phil[:, :, k] = 0.5 * (phii[:, :, k + 1] + phii[:, :, k + 1] + del_gz[:, :, k])
        phii[:, :, k] = phii[:, :, k + 1] + del_gz[:, :, k]
    s["phil"] = phil


def prepare_microphysics(s):
    s["dz"] = (s["phii"][:, :, 1:] - s["phii"][:, :, :-1]) * RGRAV
    s["wmp"] = -s["omga"] * (1.0 + ZVIR * s["qvapor"]) * s["pt"] / s["delp"] * (RDGAS * RGRAV)
    for name in TENDENCIES:
        s[name] = np.zeros_like(s["pt"])


def prepare(s, ptop, do_microphysics=True):
    """Everything Physics.__call__ does before the microphysics.  Returns the clamp masks of statein()."""
    clamps = statein(s, ptop)
    get_phi_fv3(s, get_prs_fv3(s))
    if do_microphysics:
        prepare_microphysics(s)
    return clamps


def update_physics_state_with_tendencies(s, dt):
    for x, x_dt, out in UPDATED:
        s[out] = s[x] + s[x_dt] * dt


def copy_dycore_to_physics(dycore, physics, n, nk):
    """On FULL arrays (n + 7, n + 7, nk + 1): origin (3, 3, 0), domain (n + 1, n + 1, nk)."""
    w = (slice(3, 3 + n + 1), slice(3, 3 + n + 1), slice(0, nk))
    for name in COPIED:
        physics[name][w] = dycore[name][w]


def prepare_tendencies_and_update_tracers(tend, phy, dycore, rdt):
    """tend: u_dt, v_dt, pt_dt (accumulated into); phy: the physics state after update_physics_state_with_tendencies, with
    physics_updated_specific_humidity as fill_gfs_delp left it; dycore: delp and the six tracers (replaced)."""
    tend["u_dt"] = tend["u_dt"] + (phy["physics_updated_ua"] - phy["ua"]) * rdt
    tend["v_dt"] = tend["v_dt"] + (phy["physics_updated_va"] - phy["va"]) * rdt
    tend["pt_dt"] = tend["pt_dt"] + (phy["physics_updated_pt"] - phy["pt"]) * rdt
    dp = phy["prsi"][:, :, 1:] - phy["prsi"][:, :, :-1]
    updated = dict(zip(SUM_ORDER, ["physics_updated_specific_humidity", "physics_updated_qliquid", "physics_updated_qrain",
                                   "physics_updated_qsnow", "physics_updated_qice", "physics_updated_qgraupel"]))
    qwat = {name: dp * phy[updated[name]] for name in SUM_ORDER}
    qt = qwat["qvapor"] + qwat["qliquid"] + qwat["qrain"] + qwat["qsnow"] + qwat["qice"] + qwat["qgraupel"]
    q_sum = dycore["qvapor"] + dycore["qliquid"] + dycore["qrain"] + dycore["qsnow"] + dycore["qice"] + dycore["qgraupel"]
    q0 = dycore["delp"] * (1.0 - q_sum) + qt
    dycore["delp"] = q0
    for name in SUM_ORDER:
        dycore[name] = qwat[name] / q0
