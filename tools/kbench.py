"""Per-entry-point timing on the GPU box (HIP events on the launch stream), C192 x 79 by default.

    python tools/kbench.py [--lib path/to/libpace_hip.so] [--n 192] [--reps 20] [--only fvtp2d,riem3,sat_adjust,dry_convective_adjust,apply_physics,microphysics,physics]
    python tools/kbench.py --only safety_check      the driver's state check against a plain torch restatement (host clock
                                                    around whole checks, which end in their own synchronisation; medians)
    python tools/kbench.py --only diag_pack         a diagnostics step (the example file's fourteen variables) against a plain
                                                    torch restatement, the same way
    python tools/kbench.py --only plev_diag         an output step of 16 pressure-level planes (p_select: one pace_plev_diag launch,
                                                    one transfer) against the volumes to the host with numpy there and against
                                                    a torch restatement on the device, the same way, with the launches alone
    python tools/kbench.py --only geos_wrapper      GeosDycoreWrapper's ingest and export (30 windows each way) against a torch
                                                    restatement (one .copy_ per window, .cpu() per output), the same way, with the
                                                    split into host staging, H2D, unpack launch, pack launch and D2H
    python tools/kbench.py --only checkpointer      a calibration call and a validation call with the sixteen fields of D_SW-In
                                                    against a torch restatement and against "to the host and numpy", the same way
    python tools/kbench.py --only restart_pack      write_restart of a state's fifteen 3-D fields and three planes (launch,
                                                    device-to-host copy, file writes) against a torch / numpy restatement, the
                                                    same way, with the split into launch, transfer and write
    python tools/kbench.py --only nudging           apply_nudging of u, v, pt, qvapor between two references with the tendencies
                                                    stored (one pace_nudge launch) against a torch restatement on the device,
                                                    the same way, with the launch alone and its bandwidth
    python tools/kbench.py --only held_suarez       the Held-Suarez forcing of a tile of the baroclinic state, accumulated into the
                                                    tendencies (one pace_held_suarez launch), against a torch restatement on
                                                    the device, the same way, with the launch alone and its bandwidth
    python tools/kbench.py --only rayleigh_super    Rayleigh_Super (rf_fast = false) of a tile of the baroclinic state: the two launches of
                                                    one pace_rayleigh_super against a torch restatement on the device, with the
                                                    sponge's own levels and with every level damped; then --only held_suarez's lines
    python tools/kbench.py --only energy_fixer      the total-energy fixer of one tile (consv_te > 0): pace_energy_columns in both
                                                    modes and pace_energy_finalize against a torch restatement on the device, the
                                                    same way, with each launch alone and its bandwidth
    python tools/kbench.py --only tracer_subcycle   TracerAdvection of seven tracers on one tile of the baroclinic state behind a
                                                    lone-rank LoopbackComm: the reference's three sub-cycles on every level against
                                                    the Courant-number sub-cycling, alternating, medians; pace_tracer_cmax alone
                                                    with its bandwidth, and the finalising launch with its transfer alone
    python tools/kbench.py --only cube_gather       one output step (fourteen variables as float32 on the host) of six C96 and six
                                                    C192 tiles on this device: one pace_cube_gather launch and one transfer
                                                    against six pace_diag_pack passes, one per tile, with a transfer each
    python tools/kbench.py --only cube_regrid       one output step of fourteen 3-D variables of six C96 and six C192 tiles to a
                                                    1 degree lat-lon grid as float32 on the host: one pace_cube_regrid launch and
                                                    one transfer, against one pace_cube_gather launch, the whole cube's transfer
                                                    and the same table applied with numpy, and against a torch restatement on
                                                    the device; alternating, medians, launches and transfers apart
    python tools/kbench.py --only halo_cube         the seven halo-updater groups of an acoustic substep for six tiles on this
                                                    device: the fused path (run_cube: one pace_halo_cube launch per update for
                                                    the whole cube) against the snapshot path (ThreadComm's pack, copies,
                                                    unpack), alternating, medians, with the library calls per update
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--n", type=int, default=192)
    ap.add_argument("--nz", type=int, default=79)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="")
    ap.add_argument("--precision", type=int, default=64, choices=(64, 32), help="storage type of the fields: libpace_hip.so or libpace_hip_f32.so")
    args = ap.parse_args()
    from pace_amd.tile import DSW_ARGS, Env

    from pace_amd import _lib, synthetic
    from pace_amd.fv3core import DGridShallowWaterLagrangianDynamicsConfig, RiemannConfig
    from pace_amd.fv3core.stencils.d_sw import DGridShallowWaterLagrangianDynamics, get_column_namelist
    from pace_amd.fv3core.stencils.delnflux import DelnFlux, DelnFluxNoSG
    from pace_amd.fv3core.stencils.fvtp2d import FiniteVolumeTransport
    from pace_amd.fv3core.stencils.fxadv import FiniteVolumeFluxPrep
    from pace_amd.fv3core.stencils.riem_solver3 import NonhydrostaticVerticalSolver
    from pace_amd.util import constants as c

    lib = _lib.Library(args.lib) if args.lib else _lib.load(args.precision)
    n, nz = args.n, args.nz
    if args.only == "geos_wrapper":  # (its own state: nothing of the set-up below)
        geos_wrapper_bench(lib, n, nz, args.reps)
        return
    if args.only == "restart_pack":  # (its own fields)
        restart_pack_bench(lib, n, nz, args.reps)
        return
    if args.only == "halo_cube":  # (its own fields, six tiles)
        halo_cube_bench(lib, n, nz, args.reps)
        return
    if args.only == "cube_gather":  # (its own fields, six tiles, C96 and C192)
        for size in (96, 192):
            cube_gather_bench(lib, size, nz, args.reps)
        return
    if args.only == "cube_regrid":  # (its own fields, six tiles, C96 and C192)
        for size in (96, 192):
            cube_regrid_bench(lib, size, nz, args.reps)
        return
    if args.only == "plev_diag":  # (its own fields)
        plev_diag_bench(lib, n, nz, max(args.reps, 30))
        return
    if args.only == "checkpointer":  # (its own fields)
        checkpointer_bench(lib, n, nz, args.reps)
        return
    if args.only == "nudging":  # (its own fields)
        nudging_bench(lib, n, nz, args.reps)
        return
    if args.only == "held_suarez":  # (its own fields)
        held_suarez_bench(lib, n, nz, args.reps)
        return
    if args.only == "rayleigh_super":  # (its own fields; then pace_held_suarez in the same job, for its GB/s)
        rayleigh_super_bench(lib, n, nz, args.reps)
        held_suarez_bench(lib, n, nz, args.reps)
        return
    if args.only == "energy_fixer":  # (its own fields)
        energy_fixer_bench(lib, n, nz, args.reps)
        return
    if args.only == "tracer_subcycle":  # (its own fields)
        tracer_subcycle_bench(lib, n, nz, args.reps)
        return
    m = synthetic.tile_metrics(n, nz)
    s = synthetic.acoustic_state(m, n, nz)
    env = Env(lib, "cuda", m, n, nz)
    col = get_column_namelist(DGridShallowWaterLagrangianDynamicsConfig(), env.qf)
    f = {k: env.q3(s[k]) for k in list(DSW_ARGS) + ["cappa", "delz", "pe", "ppe", "pk3", "pk", "peln"]}
    zs, ws = env.q2(s["zs"]), env.q2(s["ws"])
    ut, vt, fx, fy = env.q3(), env.q3(), env.q3(), env.q3()
    prep = FiniteVolumeFluxPrep(env.stencil_factory, env.grid_data)
    prep(f["uc"], f["vc"], f["crx"], f["cry"], f["xfx"], f["yfx"], ut, vt, s["dt"])
    tp = FiniteVolumeTransport(env.stencil_factory, env.qf, env.grid_data, env.damping, 0, 6)
    dn0 = DelnFluxNoSG(env.stencil_factory, env.damping, env.grid_data.rarea, col["nord_w"])
    dn2 = DelnFlux(env.stencil_factory, env.qf, env.damping, env.grid_data.rarea, col["nord_t"], col["damp_t"])
    dsw = DGridShallowWaterLagrangianDynamics(env.stencil_factory, env.qf, env.grid_data, env.damping, col, False, False,
                                              DGridShallowWaterLagrangianDynamicsConfig())
    riem = NonhydrostaticVerticalSolver(env.stencil_factory, env.qf, RiemannConfig())
    cells = n * n * nz
    field_mb = (n + 1) * (n + 1) * nz * (args.precision // 8) / 1e6
    damp_w = torch.as_tensor(np.full(nz, 1.0e9), device="cuda")

    def restore():
        for k in f:
            f[k].set(s[k])

    import ctypes as C

    from pace_amd.fv3core.stencils._common import dptr

    def dsw_phase(mask):
        fields = [f[k] for k in DSW_ARGS]
        dsw.lib.call("pace_d_sw_phases", mask, C.byref(dsw._geom), C.byref(dsw._met), C.byref(dsw._col), C.byref(dsw._cfg),
                     dsw._workspace.data_ptr(), *[dptr(x) for x in fields], float(s["dt"]), dsw.stream())

    from pace_amd.fv3core.stencils.map_single import MapSingle

    rng = np.random.default_rng(1)
    sig = np.linspace(0.0, 1.0, nz + 1) ** 1.6
    ps = 1.0e5 * (1.0 + 0.02 * rng.random((n + 7, n + 7)))
    pe2_h = 300.0 + (ps - 300.0)[:, :, None] * sig[None, None, :]
    s1 = sig[None, None, :] + (1.5 / nz * rng.random((n + 7, n + 7)))[:, :, None] * np.sin(2.0 * np.pi * sig)[None, None, :]
    s1[:, :, 0], s1[:, :, nz] = 0.0, 1.0
    pe1_h = 300.0 + (ps - 300.0)[:, :, None] * s1
    rq, rp1, rp2 = env.q3(s["pt"]), env.q3(pe1_h), env.q3(pe2_h)
    remap = MapSingle(env.stencil_factory, env.qf, 9, 1, ["x", "y", "z"])

    # SatAdjust3d on a moist column state (180 - 310 K, vapour around saturation, condensates), kmp = 2 as on the 79-level grid;
    # the operator works in place, so its inputs are restored before every repetition
    from pace_amd.fv3core import SatAdjustConfig
    from pace_amd.fv3core.stencils.saturation_adjustment import SatAdjust3d

    i3, j3, k3 = np.meshgrid(np.arange(n + 7), np.arange(n + 7), np.arange(nz + 1), indexing="ij")
    t3 = 180.0 + 130.0 * (k3 / nz) + 15.0 * np.sin(0.05 * i3 + 0.07 * j3)
    p3 = 1000.0 + 1.0e5 * (k3 + 0.5) / nz
    sa_h = {"delp": 200.0 + 1500.0 * (k3 / nz)}
    sa_h["delz"] = -c.RDGAS * t3 * sa_h["delp"] / (c.GRAV * p3)
    sa_h["qvapor"] = np.minimum(3.8e-3 * np.exp(17.27 * (t3 - 273.16) / (t3 - 35.86)) * 1.0e5 / p3
                                * (0.7 + 0.6 * (0.5 + 0.5 * np.sin(0.3 * i3 - 0.2 * j3 + 0.5 * k3))), 0.03)
    for q_i, (nm, sc) in enumerate((("qliquid", 4e-4), ("qrain", 2e-4), ("qice", 2e-4), ("qsnow", 1e-4), ("qgraupel", 5e-5))):
        sa_h[nm] = sc * (0.5 + 0.5 * np.cos(0.17 * i3 + 0.23 * j3 + 0.4 * k3 + q_i))
    qc3 = sa_h["qliquid"] + sa_h["qrain"] + sa_h["qice"] + sa_h["qsnow"] + sa_h["qgraupel"]
    sa_h["pt"] = t3 * (1.0 + c.ZVIR * sa_h["qvapor"]) * (1.0 - qc3)
    for nm in ("qcld", "te", "q_con", "pkz", "cappa"):
        sa_h[nm] = np.zeros_like(t3)
    sa = {k: env.q3(v) for k, v in sa_h.items()}
    sa_hs = env.q2(np.zeros((n + 7, n + 7)))
    satadj = SatAdjust3d(env.stencil_factory, SatAdjustConfig(), env.grid_data.area_64, 2)

    def sat_adjust():
        satadj(sa["te"], sa["qvapor"], sa["qliquid"], sa["qice"], sa["qrain"], sa["qsnow"], sa["qgraupel"], sa["qcld"], sa_hs, None,
               sa["delp"], sa["delz"], sa["q_con"], sa["pt"], sa["pkz"], sa["cappa"], c.ZVIR, 225.0, False, True, c.KAPPA, 2)

    def restore_sat_adjust():
        for k in sa:
            sa[k].set(sa_h[k])

    # DryConvectiveAdjustment on a moist state with unstable columns, n_sponge = 48 (in place: inputs restored before every
    # repetition).  Traffic: 17 fields read, 15 written, over the 48 adjusted levels of the nz the table's fields have
    import types

    from pace_amd.fv3core import DryConvectiveAdjustment

    ks = min(48, nz)
    cv_h = synthetic.convective_state(n, nz)
    cv = {k: env.q3(v) for k, v in cv_h.items()}
    cv_state = types.SimpleNamespace(**{k: v for k, v in cv.items() if k not in ("u_dt", "v_dt")})
    dry_adj = DryConvectiveAdjustment(env.stencil_factory, env.qf, 6, 600, ks, False)

    def restore_dry_adj():
        for k in cv:
            cv[k].set(cv_h[k])

    apply_physics = ("fill_gfs_delp", "phys_thermo_pressure", "update_dwinds_phys")
    only = [x for x in args.only.split(",") if x]
    if "safety_check" in only:
        safety_check_bench(lib, env, s, n, nz, max(args.reps, 50))
        only.remove("safety_check")
        if not only:
            return
    if "diag_pack" in only:
        diag_pack_bench(lib, env, s, n, nz, max(args.reps, 50))
        only.remove("diag_pack")
        if not only:
            return
    if "apply_physics" in only:
        only += list(apply_physics)
    ap_cases = {}

    def build_apply_physics():
        # The end-of-step update (k_updphys.hip), each kernel alone on the convective state's fields with pace_amd's own driver grid
        # terms: fill_gfs_delp (delp, q read, q written where it changes), the column kernel (14 field passes) and the wind kernel
        # with its zeroing launch (8).  `--only apply_physics` selects the three.
        from pace_amd.fv3core.stencils.fillz import pointer_table
        from pace_amd.util import gridgen
        from pace_amd.util.grid import DriverGridData, geom_struct

        terms = gridgen.tiles(n, nz)[0]
        info = DriverGridData.new_from_grid_variables(**{k: terms[k] for k in ("vlon", "vlat", "es1", "ew2", "edge_vect_w", "edge_vect_e",
                                                                                "edge_vect_s", "edge_vect_n")}, quantity_factory=env.qf)
        geom = geom_struct(env.qf)
        ap_t_dt, ap_pk, ap_u, ap_v = env.q3(), env.q3(), env.q3(), env.q3()
        ap_2d = [env.q2(), env.q2(), env.q2()]
        ap_vec = [pointer_table([getattr(info, f"{nm}{m}") for m in (1, 2, 3)]) for nm in ("vlon", "vlat", "es1_", "ew2_")]
        ap_edges = [C.c_void_p(e.data_ptr()) for e in (info.edge_vect_w, info.edge_vect_e, info.edge_vect_s, info.edge_vect_n)]
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        water = pointer_table([cv[k] for k in ("qvapor", "qliquid", "qrain", "qsnow", "qice", "qgraupel")])

        def fill_gfs_delp():
            lib.call("pace_fill_gfs_delp", C.byref(geom), dptr(cv["delp"]), dptr(cv["qvapor"]), 1.0e-9, stream)

        def phys_thermo_pressure():
            lib.call("pace_phys_thermo_pressure", C.byref(geom), water, dptr(cv["pt"]), dptr(ap_t_dt), dptr(cv["pe"]), dptr(cv["delp"]),
                     dptr(cv["peln"]), dptr(ap_pk), dptr(cv["ua"]), dptr(cv["va"]), *[dptr(x) for x in ap_2d], 225.0, stream)

        def update_dwinds_phys():
            lib.call("pace_update_dwinds_phys", C.byref(geom), dptr(ap_u), dptr(ap_v), dptr(cv["u_dt"]), dptr(cv["v_dt"]), *ap_vec, *ap_edges,
                     112.5, stream)
        ap_cases.update(fill_gfs_delp=fill_gfs_delp, phys_thermo_pressure=phys_thermo_pressure, update_dwinds_phys=update_dwinds_phys,
                        grid_info=info)  # (the pointer tables hold addresses of grid_info's fields)

    if not only or set(only) & set(apply_physics):  # (the driver grid terms take a grid generation: only when they are timed)
        build_apply_physics()

    # Microphysics (k_microphys.hip) on pace_amd.synthetic's columns and fill, one sub-step (225 s) and two (450 s).  wmp is
    # transported and the tendencies are accumulated: both are restored before every repetition.  Traffic: 12 fields read and 9
    # tendencies read, 15 written (wmp, ten tendencies, the precipitation on every level) -- the algorithm's, not the workspace's.
    mp_cases = {}

    def build_microphysics():
        from pace_amd.physics import Microphysics, MicrophysicsState, PhysicsConfig

        if args.precision != 64:
            raise SystemExit("microphysics needs the float64 library")
        pt_h, delp_h, delz_h = synthetic.microphysics_columns(n, nz)
        mp_h = synthetic.microphysics_state(pt_h, delp_h, delz_h)

        def full(a):
            out = np.zeros((n + 7, n + 7, nz + 1) if a.ndim == 3 else (n + 7, n + 7))
            out[(slice(3, 3 + n), slice(3, 3 + n)) + ((slice(0, nz),) if a.ndim == 3 else ())] = a
            return out

        names = "pt qvapor qliquid qrain qice qsnow qgraupel qcld ua va delp delz omga delprsi wmp dz".split()
        q = {k: env.q3(full(mp_h[k])) for k in names}
        state = MicrophysicsState(*[q[k] for k in names[:13]], q["delprsi"], q["wmp"], q["dz"], env.q3(), env.q2(full(mp_h["land"])))
        op = Microphysics(env.stencil_factory, env.qf, env.grid_data,
                          PhysicsConfig(dt_atmos=225, hydrostatic=False, npx=n + 1, npy=n + 1, npz=nz, nwat=6, do_qa=True))
        wmp0 = full(mp_h["wmp"])

        def restore_microphysics():
            q["wmp"].set(wmp0)
            for k in _lib.MICROPHYSICS_TENDENCIES:
                getattr(state, k).data.zero_()
        mp_cases.update(microphysics=lambda: op(state, 225.0), microphysics_2=lambda: op(state, 450.0), restore=restore_microphysics)

    if not only or "microphysics" in only:
        build_microphysics()
        if "microphysics" in only:
            only.append("microphysics_2")
    # The Physics shell and the coupling (k_physics.hip), each kernel alone on pace_amd.synthetic's columns, fill and extras.  prepare
    # and the coupling change their inputs: the state is restored from device copies before every repetition.  Field passes per
    # cell: the copy 16 + 16; prepare 15 read (nine in the sweep down, six in the sweep up) and 26 written; update 20 + 10; the
    # coupling 23 read and 10 written.  `--only physics` selects the four.
    physics_kernels = ("physics_copy", "physics_prepare", "physics_update", "physics_coupling")
    ph_cases = {}

    def build_physics():
        import types

        from pace_amd.physics import Physics, PhysicsConfig, PhysicsState
        from pace_amd.stencils import CopyDycoreToPhysics, PhysicsToDycore

        if args.precision != 64:
            raise SystemExit("the physics needs the float64 library")
        host = synthetic.microphysics_state(*synthetic.microphysics_columns(n, nz))
        host.update(synthetic.physics_extras(host["pt"].shape))

        def full(a):
            out = np.ones((n + 7, n + 7, nz + 1) if a.ndim == 3 else (n + 7, n + 7))
            out[(slice(3, 3 + n), slice(3, 3 + n)) + ((slice(0, nz),) if a.ndim == 3 else ())] = a
            return out

        nml = PhysicsConfig(dt_atmos=225, hydrostatic=False, npx=n + 1, npy=n + 1, npz=nz, nwat=6, do_qa=True)
        dycore = types.SimpleNamespace(**{k: env.q3(full(host[k])) for k in _lib.PHYSICS_COPY_FIELDS})
        state = PhysicsState.init_zeros(env.qf, ["microphysics"])
        state.land.copy_(env.q2(full(host["land"])).data)
        copy = CopyDycoreToPhysics(env.stencil_factory, env.qf)
        physics = Physics(env.stencil_factory, env.qf, env.grid_data, nml, ["microphysics"])
        couple = PhysicsToDycore(env.stencil_factory, env.qf, nml)
        tend = [env.q3(), env.q3(), env.q3()]
        copy(dycore, state)
        entry = {k: getattr(state, k).clone() for k in _lib.PHYSICS_COPY_FIELDS}  # the physics state before prepare
        physics(state, 225.0)
        dycore_entry = {k: getattr(dycore, k).data.clone() for k in ("delp",) + _lib.PHYSICS_COPY_FIELDS[:6]}
        humidity = state.physics_updated_specific_humidity.clone()

        def restore_physics(name):
            if name == "physics_prepare":
                for k, v in entry.items():
                    getattr(state, k).copy_(v)
            if name == "physics_coupling":
                for k, v in dycore_entry.items():
                    getattr(dycore, k).data.copy_(v)
                state.physics_updated_specific_humidity.copy_(humidity)
        ph_cases.update(physics_copy=lambda: copy(dycore, state), physics_prepare=lambda: physics.prepare(state),
                        physics_update=lambda: physics.update(state, 225.0),
                        physics_coupling=lambda: couple.call(
                            "pace_physics_tendencies_to_dycore", *coupling_args(couple, dycore, state, tend)),
                        restore=restore_physics)

    def coupling_args(couple, dycore, state, tend):
        from pace_amd.stencils.physics_coupling import _SUM_ORDER, _UPDATED, _pointers

        return (_pointers(tend), _pointers([getattr(state, k) for k in _UPDATED]), _pointers([state.ua, state.va, state.pt]),
                _pointers([getattr(dycore, k) for k in _SUM_ORDER]), dptr(state.prsi), dptr(dycore.delp), 1.0 / 225.0, couple.stream())

    if "physics" in only:
        only += list(physics_kernels)
    if not only or set(only) & set(physics_kernels):
        build_physics()
    cases = {
        "physics_copy": (ph_cases.get("physics_copy"), 32),
        "physics_prepare": (ph_cases.get("physics_prepare"), 41),
        "physics_update": (ph_cases.get("physics_update"), 30),
        "physics_coupling": (ph_cases.get("physics_coupling"), 33),
        "fill_gfs_delp": (ap_cases.get("fill_gfs_delp"), 3),
        "phys_thermo_pressure": (ap_cases.get("phys_thermo_pressure"), 14),
        "update_dwinds_phys": (ap_cases.get("update_dwinds_phys"), 8),
        "microphysics": (mp_cases.get("microphysics"), 36),
        "microphysics_2": (mp_cases.get("microphysics_2"), 36),
        "dry_convective_adjust": (lambda: dry_adj(cv_state, cv["u_dt"], cv["v_dt"], 225.0), 32.0 * ks / nz),
        "sat_adjust": (sat_adjust, 19),
        "fxadv": (lambda: prep(f["uc"], f["vc"], f["crx"], f["cry"], f["xfx"], f["yfx"], ut, vt, s["dt"]), 8),
        "fvtp2d": (lambda: tp(f["pt"], f["crx"], f["cry"], f["xfx"], f["yfx"], fx, fy, x_mass_flux=f["mfx"], y_mass_flux=f["mfy"]), 9),
        "delnflux_nosg": (lambda: dn0(f["w"], fx, fy, damp_w, None), 3),
        "delnflux_mass": (lambda: dn2(f["pt"], fx, fy, mass=f["delp"]), 6),
        "riem3": (lambda: riem(False, s["dt"], f["cappa"], m["ptop"], zs, ws, f["delz"], f["q_con"], f["delp"], f["pt"], f["zh"],
                               f["pe"], f["ppe"], f["pk3"], f["pk"], f["peln"], f["w"]), 13),
        "map_single": (lambda: remap(rq, rp1, rp2), 4),
        "dsw_scalars": (lambda: dsw_phase(2), 18),
        "dsw_winds": (lambda: dsw_phase(12), 20),
        "d_sw": (lambda: dsw(*[f[k] for k in DSW_ARGS], s["dt"]), 32),
    }
    print(f"{'case':22s} {'us':>10s} {'alg GB/s':>10s} {'%8TB/s':>8s}")
    for name, (fn, nfields) in cases.items():
        if only and name not in only:
            continue
        restore()
        restore_sat_adjust()
        restore_dry_adj()
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            if name in ("d_sw", "riem3", "dsw_scalars", "dsw_winds"):
                restore()
                torch.cuda.synchronize()
            if name == "sat_adjust":
                restore_sat_adjust()
                torch.cuda.synchronize()
            if name == "dry_convective_adjust" or name in apply_physics:
                restore_dry_adj()
                torch.cuda.synchronize()
            if name.startswith("microphysics"):
                mp_cases["restore"]()
                torch.cuda.synchronize()
            if name in physics_kernels:
                ph_cases["restore"](name)
                torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        us = float(np.median(ts))
        gbs = nfields * field_mb * 1e6 / (us * 1e-6) / 1e9
        print(f"{name:22s} {us:10.1f} {gbs:10.1f} {100*gbs/8000:8.2f}")


def safety_check_bench(lib, env, s, n, nz, reps):
    """SafetyChecker.check_state on the driver's four registered fields (ua, va, delp, pt; compute domain only) against the
    reference's check restated with torch on the same views: amin, amax and isnan().any() per variable, each bound test and the
    NaN test a host synchronisation of its own.  Both are timed with the host clock from an idle device to the decision (each
    ends in its own synchronisation); the two alternate, medians are reported."""
    import time
    import types

    from pace_amd.driver import SafetyChecker
    from pace_amd.driver.driver import _SAFETY_CHECKS

    state = types.SimpleNamespace(ua=env.q3(np.clip(s["ua"], -100.0, 100.0)), va=env.q3(np.clip(s["va"], -100.0, 100.0)), delp=env.q3(np.abs(s["delp"]) * 0 + 100.0),
                                  pt=env.q3(np.abs(s["pt"]) * 0 + 300.0))
    SafetyChecker.clear_all_checks()
    for name, lo, hi in _SAFETY_CHECKS:
        SafetyChecker.register_variable(name, lo, hi, compute_domain_only=True)
    checker = SafetyChecker(lib)

    def torch_check(st):
        for variable, b in SafetyChecker.checks.items():
            var = getattr(st, variable)
            view = var.view[:] if b.compute_domain_only else var.data
            min_value, max_value = view.amin(), view.amax()
            if b.minimum_value and min_value < b.minimum_value:
                raise RuntimeError(f"Variable {variable} is outside of its specified bounds")
            if b.maximum_value and max_value > b.maximum_value:
                raise RuntimeError(f"Variable {variable} is outside of its specified bounds")
            if torch.isnan(var.view[:]).any():
                raise RuntimeError(f"Variable {variable} contains a NaN value")

    paths = {"hip": lambda: checker.check_state(state), "torch": lambda: torch_check(state)}
    times = {k: [] for k in paths}
    for k, fn in paths.items():  # warm-up: code objects, the checker's buffers, torch's reduction kernels
        for _ in range(5):
            fn()
    for _ in range(reps):
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[k].append((time.perf_counter() - t0) * 1e6)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev = []
    for _ in range(reps):  # the launch pair alone, device time
        e0.record()
        checker.extrema([state.ua, state.va, state.delp, state.pt], [True] * 4)
        e1.record()
        torch.cuda.synchronize()
        dev.append(e0.elapsed_time(e1) * 1e3)
    mb = 4 * n * n * nz * lib.real_bytes / 1e6
    hip, ref = float(np.median(times["hip"])), float(np.median(times["torch"]))
    print(f"safety_check C{n} x {nz}, four fields, {mb:.1f} MB read once; medians of {reps} alternating runs")
    print(f"  check_state (pace_state_extrema, one transfer)   {hip:9.1f} us per call   (min {min(times['hip']):.1f}, "
          f"launch pair + transfer in device events {np.median(dev):.1f} us = {mb * 1e6 / (np.median(dev) * 1e-6) / 1e9:.0f} GB/s of the read)")
    print(f"  torch restatement (amin / amax / isnan().any())   {ref:9.1f} us per call   (min {min(times['torch']):.1f})")
    print(f"  ratio torch / hip {ref / hip:.2f}")
    SafetyChecker.clear_all_checks()


def diag_pack_bench(lib, env, s, n, nz, reps):
    """MonitorDiagnostics.pack on what tests/golden/driver_baroclinic_c12.yaml asks for -- its twelve 3-D names, pt at level 65
    and, as a derived variable, column_integrated_qliquid -- against the same step restated with torch: per variable the slice
    of the compute domain, a permute to (x, y, z) C order, contiguous(), .to(float32) and .cpu(), the column integral as
    RGRAV * sum(q * delp).  Both end with the data on the host and are timed with the host clock from an idle device; the two
    alternate, medians are reported, as --only safety_check does."""
    import time
    import types

    from pace_amd.driver import MonitorDiagnostics, ZSelect
    from pace_amd.util import constants as c

    names = ["u", "v", "ua", "va", "pt", "delp", "qvapor", "qliquid", "qice", "qrain", "qsnow", "qgraupel"]
    dims = {"u": ["x", "y_interface", "z"], "v": ["x_interface", "y", "z"]}
    rng = np.random.default_rng(0)
    fields = {}
    for name in names:
        q = env.qf.zeros(dims.get(name, ["x", "y", "z"]), "")
        q.set(s[name] if name in s else rng.uniform(0.0, 1e-3, q.shape))
        fields[name] = q
    state = types.SimpleNamespace(dycore_state=types.SimpleNamespace(**fields), physics_state=types.SimpleNamespace())
    level = min(65, nz - 1)
    diag = MonitorDiagnostics(None, names, ["column_integrated_qliquid"], [ZSelect(level=level, names=["pt"])], lib=lib)

    def hip_step():
        return diag.pack(diag._requests(state))

    def torch_step():
        out = {}
        for name in names:
            out[name] = fields[name].view[:].contiguous().to(torch.float32).cpu()  # (data is already the (x, y, z) view: contiguous() permutes)
        q, delp = fields["qliquid"], fields["delp"]
        out["column_integrated_qliquid"] = (c.RGRAV * torch.sum(q.view[:] * delp.view[:], dim=2)).contiguous().to(torch.float32).cpu()
        out[f"pt_z{level}"] = fields["pt"].view[:][:, :, level].contiguous().to(torch.float32).cpu()
        return out

    got, want = hip_step(), torch_step()
    for name in names + [f"pt_z{level}"]:
        assert torch.equal(got[name].view[:].view(torch.int32), want[name].view(torch.int32)), name  # (bit for bit)
    paths = {"hip": hip_step, "torch": torch_step}
    times = {k: [] for k in paths}
    for k, fn in paths.items():  # warm-up: code objects, the pinned buffer, torch's copy kernels
        for _ in range(5):
            fn()
    for _ in range(reps):
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[k].append((time.perf_counter() - t0) * 1e6)
    requests = diag._requests(state)
    (geom, offsets, packed, host), = diag._plans.values()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev, prep = [], []
    real_to_host = diag._to_host
    diag._to_host = lambda packed, host: None
    burst = 10  # launches queued back to back, so that the device time is the kernel's and not the host's item table
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(burst):
            diag.pack(requests)
        e1.record()
        prep.append((time.perf_counter() - t0) * 1e6 / burst)  # host time to build the table and launch, nothing waited for
        torch.cuda.synchronize()
        dev.append(e0.elapsed_time(e1) * 1e3 / burst)
    diag._to_host = real_to_host
    read_mb = sum(int(np.prod(r.shape)) for r in requests[:12]) * lib.real_bytes / 1e6
    out_mb = packed.numel() * 4 / 1e6
    hip, ref = float(np.median(times["hip"])), float(np.median(times["torch"]))
    print(f"diag_pack C{n} x {nz}, {len(requests)} variables, {read_mb:.1f} MB read, {out_mb:.1f} MB of float32 to the host; "
          f"medians of {reps} alternating runs")
    print(f"  MonitorDiagnostics.pack (pace_diag_pack, one transfer)   {hip:9.1f} us per step   (min {min(times['hip']):.1f}, "
          f"host time to build the item table and launch {np.median(prep):.1f} us; {burst} launches back to back in device events: "
          f"{np.median(dev):.1f} us each = {(read_mb + out_mb) * 1e6 / (np.median(dev) * 1e-6) / 1e9:.0f} GB/s of read + write)")
    print(f"  torch restatement (slice, contiguous, float32, cpu per variable)   {ref:9.1f} us per step   (min {min(times['torch']):.1f})")
    print(f"  ratio torch / hip {ref / hip:.2f}")


def plev_diag_bench(lib, n, nz, reps, device="cuda"):
    """An output step of pressure-level diagnostics: pt, ua, va, w, qvapor at 850, 500 and 200 hPa and the height at 500 hPa
    (16 planes of float32 on the host) of a C<n> x <nz> tile whose surface pressure varies 500 ... 1030 hPa, three ways:

      hip     MonitorDiagnostics with p_select: ONE pace_plev_diag launch, one transfer of the 16 planes, one synchronisation;
      volumes the only route without it: the eight volumes the interpolation needs (the five fields, delz, peln) and phis as
              WINDOW3D / PLANE through pace_diag_pack in float64 to the host, then the numpy restatement
              (tests/plev_reference.py) there;
      torch   the restatement written with torch on the device (gathers along z at the brackets, the heights by a flipped
              cumsum), then .to(float32).cpu() per plane.
    Host clock from an idle device to the data on the host; the three alternate, medians are reported.  Then the launches
    alone: device events around back-to-back pace_plev_diag launches, and around the torch restatement without its copies;
    the launch's GB/s are over its algorithmic bytes: peln once, delz once, two elements per LAYER plane, the outputs."""
    import ctypes as C
    import math
    import time
    import types

    import plev_reference as ref

    from pace_amd.driver import MonitorDiagnostics, PSelect
    from pace_amd.driver.diagnostics import WindowPacker
    from pace_amd.util import QuantityFactory, SubtileGridSizer, constants as c

    X, Y, Z, ZI = "x", "y", "z", "z_interface"
    real = torch.float32 if lib.real_bytes == 4 else torch.float64
    qf = QuantityFactory(SubtileGridSizer(n, n, nz), device, real)
    rng = np.random.default_rng(0)
    side = n + 7
    ps = rng.uniform(50000.0, 103000.0, (side, side))
    peln_h = np.log(300.0 + (ps[..., None] - 300.0) * (np.arange(nz + 1) / nz) ** 1.5)
    layer_names = ["pt", "ua", "va", "w", "qvapor"]
    fields = {}
    for name in layer_names + ["delz"]:
        q = qf.zeros([X, Y, Z], "")
        a = rng.uniform(-50.0, 50.0, q.shape)
        if name == "delz":
            a[..., :nz] = -c.RDGAS * 250.0 / c.GRAV * (peln_h[..., 1:] - peln_h[..., :-1])
        q.set(a)
        fields[name] = q
    fields["peln"] = qf.zeros([X, Y, ZI], "ln(Pa)")
    fields["peln"].set(peln_h)
    fields["phis"] = qf.zeros([X, Y], "")
    fields["phis"].set(rng.uniform(0.0, 3.0e4, (side, side)))
    state = types.SimpleNamespace(dycore_state=types.SimpleNamespace(**fields), physics_state=types.SimpleNamespace())
    pressures = (85000.0, 50000.0, 20000.0)
    p_select = [PSelect(pressures[0], list(layer_names)), PSelect(pressures[1], list(layer_names) + ["height"]),
                PSelect(pressures[2], list(layer_names))]
    diag = MonitorDiagnostics(None, [], [], [], lib=lib, p_select=p_select)
    volumes = WindowPacker(lib)
    volume_requests = [MonitorDiagnostics._whole(name, fields[name]) for name in layer_names + ["delz", "peln", "phis"]]

    def hip_step():
        return {k: v.view[:] for k, v in diag.pack(diag._requests(state)).items()}

    def volumes_step():
        host = {k: v.view[:].numpy() for k, v in volumes.pack(volume_requests, out_is_double=True).items()}
        out = {}
        for sel in p_select:
            lp = math.log(sel.pressure)
            for name in sel.names:
                if name == "height":
                    out[sel.output_name(name)] = ref.height(host["delz"], host["phis"], host["peln"], lp, nz).astype(np.float32)
                else:
                    out[sel.output_name(name)] = ref.layer(host[name], host["peln"], lp, nz).astype(np.float32)
        return out

    def take(a, k):
        return torch.gather(a, 2, k.unsqueeze(2)).squeeze(2)

    def torch_planes():
        peln = fields["peln"].view[:].to(torch.float64)
        pm = 0.5 * (peln[:, :, :-1] + peln[:, :, 1:])
        zi = None
        out = {}
        for sel in p_select:
            lp = math.log(sel.pressure)
            kb = ((pm[:, :, 1:nz - 1] <= lp).sum(dim=2))  # (monotone columns: the count is the largest such k)
            lo, hi = take(pm, kb), take(pm, kb + 1)
            t = (lp - lo) / (hi - lo)
            top, bottom = ~(lp > pm[:, :, 0]), lp >= pm[:, :, nz - 1]
            for name in sel.names:
                if name == "height":
                    if zi is None:
                        delz = fields["delz"].view[:].to(torch.float64)
                        zs = (fields["phis"].view[:].to(torch.float64) * c.RGRAV).unsqueeze(2)
                        zi = torch.cat([(zs - torch.cumsum(delz.flip(2), dim=2)).flip(2), zs], dim=2)  # (summed bottom-up)
                    kh = (peln[:, :, 1:nz] <= lp).sum(dim=2)
                    e_lo, e_hi = take(peln, kh), take(peln, kh + 1)
                    z_lo, z_hi = take(zi, kh), take(zi, kh + 1)
                    out[sel.output_name(name)] = z_lo + (z_hi - z_lo) * ((lp - e_lo) / (e_hi - e_lo))
                else:
                    f = fields[name].view[:].to(torch.float64)
                    v = take(f, kb) + (take(f, kb + 1) - take(f, kb)) * t
                    out[sel.output_name(name)] = torch.where(top, f[:, :, 0], torch.where(bottom, f[:, :, nz - 1], v))
        return out

    def torch_step():
        return {k: v.to(torch.float32).cpu() for k, v in torch_planes().items()}

    got, want, third = hip_step(), volumes_step(), torch_step()
    assert len(got) == 16
    for name in got:  # (the kernel and the restatement bit for bit; torch's cumsum sums in another order: the height to 1e-3 m)
        assert np.array_equal(got[name].numpy().view(np.int32), want[name].view(np.int32)), name
        assert torch.allclose(third[name], got[name], rtol=1e-6, atol=1e-3), name
    paths = {"hip": hip_step, "volumes": volumes_step, "torch": torch_step}
    times = {k: [] for k in paths}
    for fn in paths.values():  # warm-up: code objects, the pinned buffers, torch's kernels
        for _ in range(3):
            fn()
    for _ in range(reps):
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[k].append((time.perf_counter() - t0) * 1e6)
    requests = diag._requests(state)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    real_to_host = diag._to_host
    diag._to_host = lambda packed, host: None
    geom, offsets, packed, _ = diag._plan(requests, False)
    (chunk,) = diag._plev_launches(list(zip(requests, offsets)))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if device == "cuda" else None
    arguments = diag._plev_arguments(geom, chunk, False, packed, stream)  # (built once: the burst below is the kernel's time)
    burst, dev, dev_torch, prep = 10, [], [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        diag.pack(requests)
        prep.append((time.perf_counter() - t0) * 1e6)  # host time to build the item table and launch, nothing waited for
        torch.cuda.synchronize()
        e0.record()
        for _ in range(burst):
            lib.call("pace_plev_diag", *arguments)
        e1.record()
        torch.cuda.synchronize()
        dev.append(e0.elapsed_time(e1) * 1e3 / burst)
        e0.record()
        torch_planes()
        e1.record()
        torch.cuda.synchronize()
        dev_torch.append(e0.elapsed_time(e1) * 1e3)
    diag._to_host = real_to_host
    columns = n * n
    mb = columns * ((nz + 1 + nz + 1) * lib.real_bytes + 15 * 2 * lib.real_bytes + 16 * 4) / 1e6
    volume_mb = sum(int(np.prod(r.shape)) for r in volume_requests) * 8 / 1e6
    hip, vol, ref_t = (float(np.median(times[k])) for k in ("hip", "volumes", "torch"))
    launch, launch_torch = float(np.median(dev)), float(np.median(dev_torch))
    print(f"plev_diag C{n} x {nz}, 16 planes ({16 * columns * 4 / 1e6:.2f} MB of float32 to the host); medians of {reps} alternating runs")
    print(f"  (a) p_select (1 pace_plev_diag, one transfer)              {hip:10.1f} us per step   (min {min(times['hip']):.1f}, host time to build the item table and launch {np.median(prep):.1f} us); "
          f"the launch alone, {burst} back to back in device events: {launch:.1f} us = {mb * 1e6 / (launch * 1e-6) / 1e9:.0f} GB/s "
          f"over {mb:.1f} MB of algorithmic bytes")
    print(f"  (b) volumes to the host ({volume_mb:.0f} MB of float64), numpy there  {vol:10.1f} us per step   (min {min(times['volumes']):.1f})")
    print(f"  (c) torch restatement on the device, .cpu() per plane      {ref_t:10.1f} us per step   (min {min(times['torch']):.1f}); "
          f"its kernels alone in device events: {launch_torch:.1f} us")
    print(f"  ratio (b) / (a) {vol / hip:.1f}   (c) / (a) {ref_t / hip:.2f}   launches alone (c) / (a) {launch_torch / launch:.1f}")


def restart_pack_bench(lib, n, nz, reps):
    """pace_amd.util.write_restart on fifteen 3-D variables and three planes of a C<n> x <nz> tile -- ONE pace_restart_pack
    launch, ONE device-to-host copy, three file.write calls of slices of the pinned buffer (into a directory of /dev/shm where
    there is one: no disk in the figure) -- against the same work restated with torch and numpy: per variable the slice of the
    compute domain, .contiguous() (the storage's own order: the row padding is dropped), .cpu(), then numpy's
    astype('>f8') and the uint64 sum of the bit patterns, written with file.write.  Both end with the files written; the two
    alternate, timed with the host clock from an idle device; medians and minima.  Then the HIP path's parts: the launch alone
    (device events around back-to-back launches), the transfer alone, the writes alone."""
    import datetime
    import shutil
    import tempfile
    import time

    from pace_amd.util import CubedSphereCommunicator, LevelOf, NullComm, QuantityFactory, SubtileGridSizer, restart

    sizer = SubtileGridSizer.from_tile_params(nx_tile=n, ny_tile=n, nz=nz, n_halo=3, extra_dim_lengths={}, layout=(1, 1))
    qf = QuantityFactory(sizer, device="cuda", dtype=torch.float32 if lib.real_bytes == 4 else torch.float64)
    communicator = CubedSphereCommunicator(NullComm(0, 6), device="cuda", lib=lib)
    rng = np.random.default_rng(0)
    names = [name for name, entry in restart.RESTART_PROPERTIES.items() if len(entry["dims"]) == 3 and entry["restart_name"] not in ("ua", "va")]
    assert len(names) == 15
    state = {}
    for name in names:
        q = qf.zeros(restart.RESTART_PROPERTIES[name]["dims"][::-1], "")
        q.set(rng.uniform(-50.0, 50.0, q.shape))
        state[name] = q
    state["surface_geopotential"] = qf.zeros(["x", "y"], "")
    state["surface_geopotential"].set(rng.uniform(0.0, 1e4, state["surface_geopotential"].shape))
    wind = state["vertical_wind"]
    state["eastward_wind_at_surface"], state["northward_wind_at_surface"] = LevelOf(wind, nz - 1), LevelOf(wind, nz - 2)
    base = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    when = datetime.datetime(2016, 8, 1)

    def window(value):
        q, level = (value.quantity, value.level) if isinstance(value, LevelOf) else (value, None)
        t = q._base[tuple(slice(o, o + e) for o, e in zip(q.origin[::-1], q.extent[::-1]))] if level is None else \
            q._base[level, q.origin[1]:q.origin[1] + q.extent[1], q.origin[0]:q.origin[0] + q.extent[0]]
        return t  # [k][j][i]: the file's order

    def hip_step():
        restart.write_restart(os.path.join(base, "hip"), communicator, state, time=when)

    def torch_step():
        os.makedirs(os.path.join(base, "torch"), exist_ok=True)
        sums = {}
        with open(os.path.join(base, "torch", "data.bin"), "wb") as f:
            for name, value in state.items():
                host = window(value).contiguous().cpu().numpy()
                sums[name] = host.astype("=f8").view(np.uint64).sum(dtype=np.uint64)
                f.write(host.astype(">f8").data)
        return sums

    try:
        want = torch_step()
        hip_step()
        # the same bytes and the same sums: every file's variables against the restatement's
        import scipy.io

        for kind in restart.RESTART_NAMES:
            with scipy.io.netcdf_file(os.path.join(base, "hip", f"{kind}.tile1.nc"), "r", mmap=False) as nc:
                for name, value in state.items():
                    variable = nc.variables.get(restart.RESTART_PROPERTIES[name]["restart_name"])
                    if variable is None:
                        continue
                    assert np.array_equal(np.array(variable[0]).view(np.uint64), window(value).cpu().numpy().astype(">f8").view(np.uint64)), name
                    assert variable.tile_checksum.decode() == restart.checksum_text(want[name]), name
        paths = {"hip": hip_step, "torch": torch_step}
        times = {k: [] for k in paths}
        for k, fn in paths.items():  # warm-up: code objects, the pinned buffer, torch's copy kernels
            for _ in range(3):
                fn()
        for _ in range(reps):
            for k, fn in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                times[k].append((time.perf_counter() - t0) * 1e3)
        # the parts of the HIP path: the launch ...
        geom = restart._geometry([v.quantity if isinstance(v, LevelOf) else v for v in state.values()])
        entries = [(v.quantity, v.level) if isinstance(v, LevelOf) else (v, None) for v in state.values()]
        windows = restart._windows_of(entries, lib.real_bytes)
        sizes = [w[5] * w[6] * w[7] * 8 for w in windows]
        offsets = [int(x) for x in np.concatenate(([0], np.cumsum(sizes)[:-1]))]
        total = sum(sizes)
        packed = torch.empty(total // 8 + len(windows), dtype=torch.int64, device="cuda")
        host = torch.empty(total // 8 + len(windows), dtype=torch.int64, pin_memory=True)
        stream = communicator.stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        dev, copy_ms, write_ms, burst = [], [], [], 5
        for _ in range(reps):
            torch.cuda.synchronize()
            e0.record()
            for _ in range(burst):
                keep = restart._pack(lib, geom, windows, offsets, 0, packed.data_ptr(), packed.data_ptr() + total, "cuda", stream)
            e1.record()
            torch.cuda.synchronize()
            del keep
            dev.append(e0.elapsed_time(e1) / burst)
            t0 = time.perf_counter()
            restart._to_host(packed, host)  # ... the transfer ...
            copy_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            data = memoryview(host.numpy()).cast("B")
            with open(os.path.join(base, "hip", "data.bin"), "wb") as f:  # ... and the writes
                f.write(data[:total])
            write_ms.append((time.perf_counter() - t0) * 1e3)
        read_mb = sum(sizes) / 8 * lib.real_bytes / 1e6
        out_mb = total / 1e6
        hip, ref = float(np.median(times["hip"])), float(np.median(times["torch"]))
        launch = float(np.median(dev))
        print(f"restart_pack C{n} x {nz}, {len(windows)} variables (15 3-D, 3 planes), {read_mb:.1f} MB read, {out_mb:.1f} MB of "
              f"big-endian float64 to the host and into files under {base}; medians of {reps} alternating runs")
        print(f"  write_restart (pace_restart_pack, one transfer, file.write of the pinned buffer)   {hip:9.2f} ms per call   "
              f"(min {min(times['hip']):.2f})")
        print(f"    launch  {launch:8.3f} ms (min {min(dev):.3f}; {burst} back to back in device events) = "
              f"{(read_mb + out_mb) / launch:6.0f} GB/s of read + write")
        print(f"    transfer {np.median(copy_ms):7.3f} ms (min {min(copy_ms):.3f}) = {out_mb / np.median(copy_ms):5.1f} GB/s to pinned memory")
        print(f"    write   {np.median(write_ms):8.3f} ms (min {min(write_ms):.3f}) = {out_mb / np.median(write_ms):5.1f} GB/s, one file.write of all of it")
        print(f"  torch / numpy restatement (slice, contiguous, cpu, astype('>f8'), uint64 sum, file.write per variable)   {ref:9.2f} ms "
              f"per call   (min {min(times['torch']):.2f})")
        print(f"  ratio torch / hip {ref / hip:.2f}")
    finally:
        shutil.rmtree(base, ignore_errors=True)


def halo_cube_bench(lib, n, nz, reps, rounds=3):
    """The updater groups of one acoustic substep (dyn_core.py: w, divgd, uc / vc, delp / pt / q_con, zh, pkc, u / v) on six
    tiles of this device, every tile updating all seven one after the other.  Host clock of tile 0 around `reps` such
    sequences, the device drained at both ends, so the time holds the launches AND the copies; the fused and the snapshot
    path alternate `rounds` times and the medians over all sequences are reported, with the library calls and tensor copies
    counted on one sequence."""
    import collections
    import time

    from pace_amd.util import CubedSphereCommunicator, QuantityFactory, SubtileGridSizer, run_cube
    from pace_amd.util import comm as comm_mod

    X, Y, Z, XI, YI, ZI = "x", "y", "z", "x_interface", "y_interface", "z_interface"
    groups = (("w", [[X, Y, Z]], None, 3), ("divgd", [[XI, YI, Z]], None, 3), ("uc__vc", [[XI, Y, Z]], [[X, YI, Z]], 3),
              ("delp__pt__q_con", [[X, Y, Z]] * 3, None, 3), ("zh", [[X, Y, ZI]], None, 3), ("pkc", [[X, Y, ZI]], None, 2),
              ("u__v", [[X, YI, Z]], [[XI, Y, Z]], 3))
    calls = collections.Counter()
    real_call = type(lib).call

    class Counting:
        def __getattr__(self, name):
            return getattr(lib, name)

        def call(self, name, *a):
            calls[name] += 1
            return real_call(lib, name, *a)

    counting = Counting()
    times = {False: [], True: []}
    counted = {}

    def program(snapshot):
        def run(comm):
            sizer = SubtileGridSizer.from_tile_params(nx_tile=n, ny_tile=n, nz=nz, n_halo=3, extra_dim_lengths={}, layout=(1, 1))
            qf = QuantityFactory(sizer, device="cuda", dtype=torch.float32 if lib.real_bytes == 4 else torch.float64)
            cube = CubedSphereCommunicator(comm, device="cuda", lib=counting)
            work = []
            for _, dx, dy, pts in groups:
                xs, ys = [qf.ones(d, "") for d in dx], [qf.ones(d, "") for d in (dy or [])]
                sx = [qf.get_quantity_halo_spec(d, n_halo=pts) for d in dx]
                if dy is None:
                    work.append((cube.get_scalar_halo_updater(sx), xs, None))
                else:
                    work.append((cube.get_vector_halo_updater(sx, [qf.get_quantity_halo_spec(d, n_halo=pts) for d in dy]), xs, ys))

            def sequence():
                for up, xs, ys in work:
                    up.update(xs, ys)

            sequence()  # warm-up: tables built and uploaded
            torch.cuda.synchronize()
            comm.barrier()
            if comm.Get_rank() == 0:
                calls.clear()
            comm.barrier()
            sequence()
            comm.barrier()
            if comm.Get_rank() == 0:
                counted[snapshot] = dict(calls)
            for _ in range(reps):
                torch.cuda.synchronize()
                comm.barrier()
                t0 = time.perf_counter()
                sequence()
                comm.barrier()
                torch.cuda.synchronize()
                if comm.Get_rank() == 0:
                    times[snapshot].append(time.perf_counter() - t0)
        return run

    for _ in range(rounds):
        for snapshot in (False, True):
            run_cube(program(snapshot), snapshot=snapshot)
    nup = len(groups)
    print(f"halo updates of one acoustic substep, six C{n} x {nz} tiles on one device, {nup} updater groups, "
          f"{rounds} x {reps} sequences per path, alternating; host clock, device drained")
    for snapshot, label in ((False, "fused (pace_halo_cube)"), (True, "snapshot (ThreadComm) ")):
        t = np.array(times[snapshot]) * 1e6
        per = {k: v / nup for k, v in counted[snapshot].items()}
        copies = "" if not snapshot else "  + clone / copy_ per message: 24 + 24 per update"
        print(f"  {label}: median {np.median(t) / nup:8.1f} us per update of the whole cube (min {t.min() / nup:8.1f}, max {t.max() / nup:8.1f}); "
              f"library calls per update: {per}{copies}")
    print(f"  ratio snapshot / fused: {np.median(times[True]) / np.median(times[False]):.2f}")


def cube_gather_bench(lib, n, nz, reps, device="cuda"):
    """One output step of the whole cube: fourteen variables (the twelve 3-D fields of the example configuration's diagnostics,
    u and v staggered, a level of pt and a 2-D field) of six tiles on this device, as float32 on the host.

    fused     ONE pace_cube_gather launch for all six tiles and all variables (84 items), one transfer of the dense buffer to
              pinned memory, one synchronisation -- what MonitorDiagnostics does under run_cube_driver;
    per tile  six WindowPacker passes, one per tile: a pace_diag_pack launch, a transfer and a synchronisation each -- what six
              per-tile MonitorDiagnostics do.
    Host clock from an idle device to the end of the last synchronisation; the two alternate, medians are reported.  The
    split: the launches alone (enqueued, then one synchronisation) and the transfers alone (of the buffers they filled)."""
    import time

    from pace_amd.driver.diagnostics import MonitorDiagnostics, WindowPacker, _Request
    from pace_amd.util import CubedSphereCommunicator, NullComm, QuantityFactory, SubtileGridSizer
    from pace_amd.util.gather import Window, _Layout, _meta_of
    from pace_amd import _lib as L

    X, Y, Z, XI, YI = "x", "y", "z", "x_interface", "y_interface"
    real = torch.float32 if lib.real_bytes == 4 else torch.float64
    qf = QuantityFactory(SubtileGridSizer(n, n, nz), device, real)
    names3 = [("u", [X, YI, Z]), ("v", [XI, Y, Z])] + [(k, [X, Y, Z]) for k in ("ua", "va", "pt", "delp", "qvapor", "qliquid", "qice",
                                                                                "qrain", "qsnow", "qgraupel")]
    tiles = []
    for t in range(6):
        fields = {name: qf.ones(dims, "") for name, dims in names3}
        fields["phis"] = qf.ones([X, Y], "")
        requests = [MonitorDiagnostics._whole(name, q) for name, q in fields.items()]
        pt = fields["pt"]
        requests.append(_Request("pt_z65", L.DIAG_PLANE, pt, None, min(65, nz - 1), tuple(pt.origin[:2]) + (0,) + tuple(pt.extent[:2]) + (1,),
                                 (X, Y), ""))
        tiles.append(requests)
    assert len(tiles[0]) == 14
    packers = [WindowPacker(lib) for _ in range(6)]
    cube = CubedSphereCommunicator(NullComm(0, 6), device=device, lib=lib)
    windows = {t: [Window(r.field, r.kind, r.level, r.window, r.dims, r.units) for r in tiles[t]] for t in range(6)}
    layout = _Layout([_meta_of(r.name, w) for r, w in zip(tiles[0], windows[0])], 6)
    dense, host = cube._gs_buffer(layout.total, torch.float32)

    def sync():
        if device == "cuda":
            torch.cuda.synchronize()

    def fused(launch=True, transfer=True):
        if launch:
            cube._gs_launch(False, windows, layout, dense)
        if transfer:
            host.copy_(dense, non_blocking=True)
        sync()

    def per_tile(launch=True, transfer=True):
        if launch and transfer:
            for t in range(6):
                packers[t].pack(tiles[t])
            return
        for t in range(6):
            packer = packers[t]
            geom, offsets, packed, phost = packer._plan(tiles[t], False)
            if launch:
                saved, packer._to_host = packer._to_host, lambda *a: None
                try:
                    packer.pack(tiles[t])
                finally:
                    packer._to_host = saved
            if transfer:
                phost.copy_(packed, non_blocking=True)
        sync()

    fused(), per_tile()  # warm-up: table and plans built, buffers allocated and pinned
    parts = {"step": (True, True), "launches": (True, False), "transfer": (False, True)}
    times = {(path, part): [] for path in ("fused", "per tile") for part in parts}
    for _ in range(reps):
        for part, (launch, transfer) in parts.items():
            for path, fn in (("fused", fused), ("per tile", per_tile)):
                sync()
                t0 = time.perf_counter()
                fn(launch, transfer)
                times[path, part].append(time.perf_counter() - t0)
    mib = layout.total * 4 / 2 ** 20
    print(f"one output step of six C{n} x {nz} tiles, fourteen variables, {mib:.0f} MiB of float32 to the host; {reps} repetitions, "
          "alternating; host clock, idle device to the last synchronisation; medians")
    for path, what in (("fused", "1 pace_cube_gather, 1 transfer "), ("per tile", "6 pace_diag_pack, 6 transfers")):
        med = {part: float(np.median(times[path, part])) * 1e6 for part in parts}
        print(f"  {path:8s} ({what}): step {med['step']:9.1f} us   launches alone {med['launches']:8.1f} us   "
              f"transfers alone {med['transfer']:9.1f} us ({mib / 1024 / (med['transfer'] * 1e-6):5.1f} GiB/s)")
    print(f"  ratio per tile / fused: step {np.median(times['per tile', 'step']) / np.median(times['fused', 'step']):.2f}, "
          f"launches {np.median(times['per tile', 'launches']) / np.median(times['fused', 'launches']):.2f}")


def cube_regrid_bench(lib, n, nz, reps, device="cuda", grid=(360, 180)):
    """One output step of fourteen 3-D cell-centre variables of six tiles on a regular lat-lon grid, as float32 on the host.

    regrid    ONE pace_cube_regrid launch for all variables, one transfer of the lat-lon arrays, one synchronisation -- what
              MonitorDiagnostics does with `latlon` under run_cube_driver;
    gather    the route without the kernel: ONE pace_cube_gather launch for all six tiles and all variables (84 items), the
              whole cube's transfer, then the same table applied on the host with numpy (float64, the contract's order);
    torch     a torch restatement on the device -- per variable the six compute domains stacked, three index_select and the
              weighted sum in float64, narrowed to float32 -- and the transfer of the lat-lon arrays.
    Host clock from an idle device to the end of the last synchronisation (gather: to the end of the numpy step); the three
    alternate, medians are reported.  The split: the launches alone (enqueued, then one synchronisation), the transfers alone
    (of the buffers they filled), and for `gather` the numpy step alone."""
    import time

    from pace_amd import _launch
    from pace_amd import _lib as L
    from pace_amd.util import CubedSphereCommunicator, NullComm, QuantityFactory, SubtileGridSizer, gridgen, latlon
    from pace_amd.util.gather import _Layout, _meta_of

    X, Y, Z, H = "x", "y", "z", 3
    real = torch.float32 if lib.real_bytes == 4 else torch.float64
    qf = QuantityFactory(SubtileGridSizer(n, n, nz), device, real)
    names = ["ua", "va", "w", "pt", "delp", "delz", "qvapor", "qliquid", "qice", "qrain", "qsnow", "qgraupel", "qo3mr", "qcld"]
    rng = np.random.default_rng(n)
    fields = {name: [qf.from_array(rng.random((n + 7, n + 7, nz + 1)), [X, Y, Z], "") for _ in range(6)] for name in names}
    assert len(fields) == 14
    terms = gridgen.tiles(n, nz)
    target = latlon.LatLonGrid(*grid)
    table = latlon.build_regrid_table(np.stack([t["lon_agrid"][H:H + n, H:H + n] for t in terms]),
                                      np.stack([t["lat_agrid"][H:H + n, H:H + n] for t in terms]), *target.targets())
    npoints = table.npoints
    cube = CubedSphereCommunicator(NullComm(0, 6), device=device, lib=lib)
    stream = _launch.stream_of(device)
    # regrid
    some = fields[names[0]][0]
    geom = _launch.geometry([some], lambda q: "", "")
    points = latlon.upload_points(geom, table, torch.device(device))
    items = [latlon.regrid_item([q.ptr for q in fields[name]], L.DIAG_WINDOW3D, 0, nz, f * npoints * nz) for f, name in enumerate(names)]
    ll_dense, ll_host = _launch.staging(len(names) * npoints * nz, torch.float32, device)
    tables = latlon.launch_regrid(lib, geom, points[0], npoints, items, ll_dense, stream)
    # gather
    windows = {t: [fields[name][t] for name in names] for t in range(6)}
    layout = _Layout([_meta_of(name, fields[name][0]) for name in names], 6)
    cube_dense, cube_host = _launch.staging(layout.total, torch.float32, device)
    flat = cube_host.numpy()
    lin = ((table.tile.astype(np.int64) * n + (table.i - H)) * n + (table.j - H))  # into a variable's [6 n n, nz] block
    on_host = np.empty((len(names), npoints, nz), dtype=np.float32)
    # torch
    lin_dev = [torch.as_tensor(lin[:, m].copy(), device=device) for m in range(3)]
    w_dev = [torch.as_tensor(table.w[:, m].copy(), device=device)[:, None] for m in range(3)]
    t_dense, t_host = _launch.staging(len(names) * npoints * nz, torch.float32, device)
    t_view = t_dense.view(len(names), npoints, nz)

    def sync():
        if device == "cuda":
            torch.cuda.synchronize()

    def numpy_step():
        for f in range(len(names)):
            block = layout.array(flat, f).reshape(6 * n * n, nz)
            a = [table.w[:, m, None] * block[lin[:, m]].astype(np.float64) for m in range(3)]
            on_host[f] = (a[0] + a[1]) + a[2]

    def regrid(launch=True, transfer=True, host_step=True):
        if launch:
            latlon.launch_regrid(lib, geom, points[0], npoints, None, ll_dense, stream, tables)
        if transfer:
            ll_host.copy_(ll_dense, non_blocking=True)
        sync()

    def gather(launch=True, transfer=True, host_step=True):
        if launch:
            cube._gs_launch(False, windows, layout, cube_dense)
        if transfer:
            cube_host.copy_(cube_dense, non_blocking=True)
        sync()
        if host_step:
            numpy_step()

    def restated(launch=True, transfer=True, host_step=True):
        if launch:
            for f, name in enumerate(names):
                block = torch.stack([q.data[H:H + n, H:H + n, :nz] for q in fields[name]]).reshape(6 * n * n, nz).to(torch.float64)
                a = [w_dev[m] * block.index_select(0, lin_dev[m]) for m in range(3)]
                t_view[f] = (a[0] + a[1]) + a[2]
        if transfer:
            t_host.copy_(t_dense, non_blocking=True)
        sync()

    paths = (("regrid", regrid), ("gather", gather), ("torch", restated))
    for _, fn in paths:  # warm-up: tables built, buffers allocated and pinned
        fn()
    got = ll_host.numpy().reshape(on_host.shape)
    # (the gather route interpolates what was narrowed to float32 first: the same arrays to rounding, not to the bit)
    assert np.allclose(got, on_host, rtol=1e-6, atol=0) and np.allclose(got, t_host.numpy().reshape(on_host.shape), rtol=1e-6, atol=0), \
        "the three routes differ"
    parts = {"step": (True, True, True), "launches": (True, False, False), "transfer": (False, True, False)}
    times = {(path, part): [] for path, _ in paths for part in parts}
    host_times = []
    for _ in range(reps):
        for part, flags in parts.items():
            for path, fn in paths:
                sync()
                t0 = time.perf_counter()
                fn(*flags)
                times[path, part].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        numpy_step()
        host_times.append(time.perf_counter() - t0)
    ll_mib, cube_mib = ll_dense.numel() * 4 / 2 ** 20, layout.total * 4 / 2 ** 20
    print(f"one output step of six C{n} x {nz} tiles, fourteen 3-D variables, to {grid[0]} x {grid[1]} points as float32 on the host: "
          f"{ll_mib:.1f} MiB of lat-lon arrays ({npoints} points) against {cube_mib:.1f} MiB of the cube ({6 * n * n} cells, ratio "
          f"{ll_mib / cube_mib:.3f}); {reps} repetitions, alternating; host clock, idle device to the end; medians")
    what = {"regrid": "1 pace_cube_regrid, 1 transfer         ", "gather": "1 pace_cube_gather, 1 transfer, numpy  ",
            "torch": "torch index_select + sum, 1 transfer   "}
    for path, _ in paths:
        med = {part: float(np.median(times[path, part])) * 1e6 for part in parts}
        mib = cube_mib if path == "gather" else ll_mib
        extra = f"   numpy alone {float(np.median(host_times)) * 1e6:11.1f} us" if path == "gather" else ""
        print(f"  {path:6s} ({what[path]}): step {med['step']:11.1f} us   launches alone {med['launches']:9.1f} us   "
              f"transfer alone {med['transfer']:9.1f} us ({mib:6.1f} MiB, {mib / 1024 / (med['transfer'] * 1e-6):5.1f} GiB/s){extra}")
    step = {path: float(np.median(times[path, "step"])) for path, _ in paths}
    print(f"  ratio to regrid: gather {step['gather'] / step['regrid']:.2f}, torch {step['torch'] / step['regrid']:.2f}; the cube's "
          f"launch and transfer without the numpy step: {(float(np.median(times['gather', 'launches'])) + float(np.median(times['gather', 'transfer']))) * 1e6:.1f} us")


def checkpointer_bench(lib, n, nz, reps):
    """A calibration call and a validation call with sixteen whole fields (what D_SW-In hands over) of the C<n> x <nz> storage.

    calibration   ThresholdCalibrationCheckpointer.__call__ in a second trial (one pace_ckpt_accumulate launch: 1 pass read
                  and 3 read-modify-write of doubles, 7 element passes) against the reference's fold restated with torch:
                  minimum, maximum, abs and add per field, 64 launches and 11 element passes.  Neither synchronises; both are
                  timed with the host clock from an idle device to the end of a synchronisation added for the measurement.
    validation    ValidationCheckpointer.__call__ against an npz savepoint file with all thresholds 0 (staging, one H2D copy,
                  one launch pair, one transfer of 96 doubles) against "transfer every field to the host and compare in numpy":
                  .cpu().numpy() per field and the reference's two assert_allclose calls on host copies of the same slabs.
    The two of a pair alternate; medians are reported."""
    import tempfile
    import time

    from pace_amd.util import (QuantityFactory, SavepointThresholds, SubtileGridSizer, Threshold, ThresholdCalibrationCheckpointer,
                               ValidationCheckpointer)

    real = torch.float32 if lib.real_bytes == 4 else torch.float64
    sizer = SubtileGridSizer.from_tile_params(nx_tile=n, ny_tile=n, nz=nz, n_halo=3, extra_dim_lengths={}, layout=(1, 1))
    qf = QuantityFactory(sizer, device="cuda", dtype=real)
    rng = np.random.default_rng(0)
    names = [f"f{m}" for m in range(16)]
    host = {name: rng.uniform(1.0, 2.0, (n + 7, n + 7, nz + 1)).astype(np.float32 if lib.real_bytes == 4 else np.float64)
            for name in names}
    fields = {name: qf.from_array(a, ["x", "y", "z_interface"], "u") for name, a in host.items()}
    elements = (n + 7) * (n + 7) * (nz + 1)

    calibration = ThresholdCalibrationCheckpointer(lib=lib)
    with calibration.trial():
        calibration("D_SW-In", **fields)
    state = {name: [torch.full_like(q.data, float("inf")), torch.full_like(q.data, float("-inf")), torch.zeros_like(q.data)]
             for name, q in fields.items()}

    def hip_calibrate():
        calibration._n_calls["D_SW-In"] = 0
        calibration("D_SW-In", **fields)

    def torch_calibrate():
        for name, q in fields.items():
            acc = state[name]
            acc[0] = torch.minimum(acc[0], q.data)
            acc[1] = torch.maximum(acc[1], q.data)
            acc[2] += torch.abs(q.data)

    scratch = tempfile.TemporaryDirectory()  # (406 MB of savepoint data: removed at the end)
    directory = scratch.name
    np.savez(os.path.join(directory, "D_SW-In.npz"), **{name: a[None, None].astype(np.float64) for name, a in host.items()})
    zero = SavepointThresholds({"D_SW-In": [{name: Threshold(0.0, 0.0) for name in names}]})
    validation = ValidationCheckpointer(directory, zero, 0, lib=lib)
    expected = {name: a.astype(np.float64) for name, a in host.items()}

    def hip_validate():
        validation._n_calls["D_SW-In"] = 0
        validation("D_SW-In", **fields)

    def numpy_validate():
        for name, q in fields.items():
            output, want = q.data.cpu().numpy(), expected[name]
            not_zero = want != 0
            np.testing.assert_allclose(output[not_zero], want[not_zero], rtol=0.0, atol=0.0, err_msg=name)
            np.testing.assert_allclose(output, want, rtol=0.0, atol=0.0, err_msg=name)

    print(f"checkpointer C{n} x {nz}, float{8 * lib.real_bytes} fields: sixteen fields of {elements} elements "
          f"({16 * elements * lib.real_bytes / 1e6:.0f} MB); medians of alternating runs, ms")
    for title, paths, count in (("calibration call", {"hip": hip_calibrate, "torch": torch_calibrate}, reps),
                                ("validation call", {"hip": hip_validate, "numpy on the host": numpy_validate}, max(3, reps // 4))):
        times = {k: [] for k in paths}
        for fn in paths.values():
            for _ in range(2):
                fn()
        for _ in range(count):
            for k, fn in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
        med = {k: float(np.median(v)) for k, v in times.items()}
        for k in paths:
            print(f"  {title:18s} {k:18s} {med[k]:10.3f} ms   (min {min(times[k]):.3f}, {count} runs)")
        other = [k for k in paths if k != "hip"][0]
        print(f"  {title:18s} ratio {other} / hip {med[other] / med['hip']:.2f}")
    moved = 16 * elements * (lib.real_bytes + 6 * 8)
    print(f"  the accumulate launch moves {moved / 1e6:.0f} MB: {moved / (np.median(times_hip_calibrate(hip_calibrate)) * 1e-3) / 1e9:.0f} GB/s in device events")
    # the validation's launch pair alone: device events around the entry point (Library.timing)
    from pace_amd.util import KernelTimes

    lib.timing = launches = KernelTimes()
    for _ in range(5):
        hip_validate()
    lib.timing = None
    pair = launches.resolve()["pace_ckpt_validate"]
    pair_ms = pair["total_run_time"] / pair["ncalls"] * 1e3
    read = 16 * elements * (lib.real_bytes + 8)
    print(f"  pace_ckpt_validate alone (launch pair, device events, mean of {pair['ncalls']}): {pair_ms:.3f} ms for {read / 1e6:.0f} MB read "
          f"= {read / (pair_ms * 1e-3) / 1e9:.0f} GB/s (the expected slabs are C-ordered: lanes read them with a stride of {(n + 7) * (nz + 1)} doubles)")
    scratch.cleanup()


def nudging_bench(lib, n, nz, reps):
    """apply_nudging of u, v, pt and qvapor of a C<n> x <nz> tile between two references, tendencies stored (ONE pace_nudge
    launch), against the same four expressions per field restated with torch on the device (views of the compute domains; the
    tendency into its preallocated storage, the state in place).  Neither synchronises; both are timed with the host clock from
    an idle device to the end of a synchronisation added for the measurement, alternating, medians; then the launch alone in
    device events, with its bandwidth over the algorithmic bytes: three reads and two writes per element of the windows."""
    import time
    from datetime import timedelta

    from pace_amd.util import CubedSphereCommunicator, NullComm, QuantityFactory, SubtileGridSizer, apply_nudging

    real = torch.float32 if lib.real_bytes == 4 else torch.float64
    sizer = SubtileGridSizer.from_tile_params(nx_tile=n, ny_tile=n, nz=nz, n_halo=3, extra_dim_lengths={}, layout=(1, 1))
    qf = QuantityFactory(sizer, device="cuda", dtype=real)
    communicator = CubedSphereCommunicator(NullComm(rank=0, total_ranks=6, fill_value=0.0), device="cuda", lib=lib)
    dims = {"u": ["x", "y_interface", "z"], "v": ["x_interface", "y", "z"], "pt": ["x", "y", "z"], "qvapor": ["x", "y", "z"]}
    rng = np.random.default_rng(0)

    def fields(units=""):
        return {name: qf.from_array(rng.uniform(1.0, 2.0, (n + 7, n + 7, nz + 1)), d, units) for name, d in dims.items()}

    state, start, end, tendencies = fields("u"), fields(), fields(), fields()
    timescales = {name: timedelta(seconds=21600) for name in dims}
    step, weight = timedelta(seconds=225), 0.3
    elements = sum(int(np.prod(q.extent)) for q in state.values())

    def hip():
        apply_nudging(state, start, timescales, step, communicator=communicator, end_reference_state=end, weight=weight,
                      tendencies=tendencies)

    def restated():
        for name in dims:
            q, r0, r1, t = state[name].view[:], start[name].view[:], end[name].view[:], tendencies[name].view[:]
            r = r0 + (r1 - r0) * weight
            t.copy_((r - q) / 21600.0)
            q += t * 225.0

    paths = {"hip": hip, "torch": restated}
    times = {k: [] for k in paths}
    for fn in paths.values():
        for _ in range(3):
            fn()
    for _ in range(reps):
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in times.items()}
    moved = elements * 5 * lib.real_bytes
    print(f"nudging C{n} x {nz}, float{8 * lib.real_bytes} fields: u, v, pt, qvapor between two references, tendencies stored; "
          f"{elements} elements, {moved / 1e6:.0f} MB algorithmic (3 reads, 2 writes); medians of {reps} alternating runs, ms")
    for k in paths:
        print(f"  {k:6s} {med[k]:9.3f} ms   (min {min(times[k]):.3f})")
    print(f"  ratio torch / hip {med['torch'] / med['hip']:.2f}")
    events = times_hip_calibrate(hip, reps)
    launch = float(np.median(events))
    print(f"  the pace_nudge launch in device events: median {launch:.3f} ms (min {min(events):.3f}) = "
          f"{moved / (launch * 1e-3) / 1e9:.0f} GB/s over the algorithmic bytes")


def held_suarez_bench(lib, n, nz, reps):
    """HeldSuarezForcing on tile 0 of the C<n> x <nz> baroclinic state with accumulate=True (ONE pace_held_suarez launch),
    against the same expressions restated with torch on the device (views of the compute domains, the tendencies updated in
    place).  Neither synchronises; both are timed with the host clock from an idle device to the end of a synchronisation added
    for the measurement, alternating, medians; then the launch alone in device events, with its bandwidth over the algorithmic
    bytes: pe on nz + 1 levels, ua, va, pt and the two planes read, the three tendencies read and written.  Before the timing
    the two paths' tendencies from zero are compared at this size.  The state's u and v stand in for ua and va."""
    import time
    import types

    from pace_amd.fv3core.initialization.baroclinic import baroclinic_state_six_tiles
    from pace_amd.stencils import HeldSuarezForcing
    from pace_amd.tile import setup_factories
    from pace_amd.util import gridgen

    tiles = gridgen.tiles(n, nz)
    host = baroclinic_state_six_tiles(tiles, n, nz)[0]
    _, qf, _, stencil_factory = setup_factories(lib, "cuda", n, nz)
    forcing = HeldSuarezForcing(stencil_factory, qf, types.SimpleNamespace(lat_agrid=np.asarray(tiles[0]["lat_agrid"])))
    dims = ["x", "y", "z"]
    # (the initial state leaves ua, va undefined -- 1e35 -- until the first c2l_ord: the D-grid winds stand in for them)
    source = {"pe": "pe", "ua": "u", "va": "v", "pt": "pt"}
    state = types.SimpleNamespace(**{name: qf.from_array(host[source[name]], dims, "") for name in source})
    tendencies = [qf.zeros(dims, "") for _ in range(3)]
    restated_tendencies = [qf.zeros(dims, "") for _ in range(3)]
    c, dt, scale = forcing.config, 225.0, forcing.heating_scale
    cs = slice(3, 3 + n)
    pe = state.pe.data[cs, cs]
    ua, va, pt = (getattr(state, name).data[cs, cs, :nz] for name in ("ua", "va", "pt"))
    s2, c2 = forcing.sin2lat.data[cs, cs, None].double(), forcing.cos2lat.data[cs, cs, None].double()
    out = [q.data[cs, cs, :nz] for q in restated_tendencies]

    def hip():
        forcing(state, *tendencies, dt, accumulate=True)

    def restated():
        ps = pe[:, :, nz:nz + 1]
        pm = 0.5 * (pe[:, :, :nz] + pe[:, :, 1:])
        sigma = pm / ps
        lp = torch.log(pm / c.p0)
        pk = torch.exp(c.kappa * lp)
        teq = torch.clamp(((c.t0 - c.delta_t_y * s2) - (c.delta_theta_z * lp) * c2) * pk, min=c.t_strat)
        h = torch.clamp((sigma - c.sigma_b) / (1.0 - c.sigma_b), min=0.0)
        kv = c.k_f * h
        kt = c.k_a + ((c.k_s - c.k_a) * h) * (c2 * c2)
        dv = 1.0 + kv * dt
        out[0].sub_((kv * ua) / dv)
        out[1].sub_((kv * va) / dv)
        out[2].sub_(((kt * (pt - teq)) / (1.0 + kt * dt)) * scale)

    paths = {"hip": hip, "torch": restated}
    hip()
    restated()
    torch.cuda.synchronize()
    for name, mine, theirs in zip(("u_dt", "v_dt", "pt_dt"), tendencies, restated_tendencies):
        a, b = mine.data[cs, cs, :nz].double(), theirs.data[cs, cs, :nz].double()
        print(f"  {name}: max |hip - torch| {float((a - b).abs().max()):.3e} at max |torch| {float(b.abs().max()):.3e}")
    times = {k: [] for k in paths}
    for fn in paths.values():
        for _ in range(3):
            fn()
    for _ in range(reps):
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in times.items()}
    moved = (n * n * nz * 9 + n * n * (nz + 1) + 2 * n * n) * lib.real_bytes
    print(f"held_suarez C{n} x {nz}, float{8 * lib.real_bytes} fields: tile 0 of the baroclinic state, accumulate on; "
          f"{n * n * nz} cells, {moved / 1e6:.0f} MB algorithmic (pe, ua, va, pt, the tendencies read; the tendencies written); "
          f"medians of {reps} alternating runs, ms")
    for k in paths:
        print(f"  {k:6s} {med[k]:9.3f} ms   (min {min(times[k]):.3f})")
    print(f"  ratio torch / hip {med['torch'] / med['hip']:.2f}")
    events = times_hip_calibrate(hip, reps)
    launch = float(np.median(events))
    print(f"  the pace_held_suarez launch in device events: median {launch:.3f} ms (min {min(events):.3f}) = "
          f"{moved / (launch * 1e-3) / 1e9:.0f} GB/s over the algorithmic bytes")


def rayleigh_super_bench(lib, n, nz, reps):
    """RayleighSuper on tile 0 of the C<n> x <nz> baroclinic state (ONE pace_rayleigh_super: the heat launch, then the wind
    launch), against the same expressions restated with torch on the device (views of the windows, updated in place, the
    factors a device vector over the damped levels).  Two rows: the sponge of rf_cutoff = 3000 Pa, and every level damped
    (rf_cutoff above the surface pressure).  Neither side synchronises; both are timed with the host clock from an idle device
    to the end of a synchronisation added for the measurement, alternating, medians; then the call alone in device events, with
    its bandwidth over the algorithmic bytes of the damped levels: u, v, w, pt read and pt, w written by the first launch, u, v
    read and written by the second -- ten fields' worth.  Before the timing the two paths' results from the same state are
    compared at this size.  The winds are damped again in every repetition: they shrink, the work does not."""
    import time

    from pace_amd.fv3core import RayleighSuper
    from pace_amd.fv3core.initialization.baroclinic import baroclinic_state_six_tiles
    from pace_amd.tile import Env
    from pace_amd.util import constants, gridgen

    tiles = gridgen.tiles(n, nz)
    host = baroclinic_state_six_tiles(tiles, n, nz)[0]
    env = Env(lib, "cuda", {k: v for k, v in tiles[0].items() if k not in ("ee1", "ee2", "es1", "ew2")}, n, nz)
    gd, dims, dt = env.grid_data, ["x", "y", "z"], 225.0
    rcv = 1.0 / (constants.CP_AIR - constants.RDGAS)
    cs, up = slice(3, 3 + n), slice(4, 4 + n)
    for label, cutoff in (("the sponge of rf_cutoff 3000 Pa", 3000.0), ("every level damped", 2.0e5)):
        damping = RayleighSuper(env.stencil_factory, env.qf, gd, cutoff, 10.0, gd.ptop)
        table = damping.factors(dt)
        kmax = int((table < 1.0).sum())
        mine = {name: env.qf.from_array(host[name], dims, "") for name in ("u", "v", "w", "pt")}
        theirs = {name: env.qf.from_array(host[name], dims, "") for name in ("u", "v", "w", "pt")}
        f = torch.as_tensor(np.array(table[:kmax]), dtype=torch.float64, device="cuda")
        g = 1.0 - f * f
        dx0, dx1, dy0, dy1 = (a.double()[:, :, None] for a in (gd.dx.data[cs, cs], gd.dx.data[cs, up], gd.dy.data[cs, cs], gd.dy.data[up, cs]))
        a11, a12, a21, a22 = (getattr(gd, name).data[cs, cs, None].double() for name in ("a11", "a12", "a21", "a22"))
        u, v, w, pt = (theirs[name].data for name in ("u", "v", "w", "pt"))
        K = slice(0, kmax)

        def hip():
            damping(mine["u"], mine["v"], mine["w"], mine["pt"], dt)

        def restated():
            u1 = 2.0 * (u[cs, cs, K].double() * dx0 + u[cs, up, K].double() * dx1) / (dx0 + dx1)
            v1 = 2.0 * (v[cs, cs, K].double() * dy0 + v[up, cs, K].double() * dy1) / (dy0 + dy1)
            ua, va = a11 * u1 + a12 * v1, a21 * u1 + a22 * v1
            wk = w[cs, cs, K].double()
            pt[cs, cs, K] += ((0.5 * ((ua * ua + va * va) + wk * wk)) * g) * rcv
            w[cs, cs, K] = f * wk
            u[cs, 3:4 + n, K] = f * u[cs, 3:4 + n, K].double()
            v[3:4 + n, cs, K] = f * v[3:4 + n, cs, K].double()

        paths = {"hip": hip, "torch": restated}
        hip()
        restated()
        torch.cuda.synchronize()
        for name in ("u", "v", "w", "pt"):
            a, b = mine[name].data.double(), theirs[name].data.double()
            print(f"  {name}: max |hip - torch| {float((a - b).abs().max()):.3e} at max |torch| {float(b.abs().max()):.3e}")
        times = {k: [] for k in paths}
        for fn in paths.values():
            for _ in range(3):
                fn()
        for _ in range(reps):
            for k, fn in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
        med = {k: float(np.median(t)) for k, t in times.items()}
        moved = 10 * n * n * kmax * lib.real_bytes
        print(f"rayleigh_super C{n} x {nz}, float{8 * lib.real_bytes} fields, {label}: {kmax} damped levels, {n * n * kmax} cells, "
              f"{moved / 1e6:.1f} MB algorithmic; medians of {reps} alternating runs, ms")
        for k in paths:
            print(f"  {k:6s} {med[k]:9.3f} ms   (min {min(times[k]):.3f})")
        print(f"  ratio torch / hip {med['torch'] / med['hip']:.2f}")
        events = times_hip_calibrate(hip, reps)
        launch = float(np.median(events))
        print(f"  the two launches of pace_rayleigh_super in device events: median {launch:.3f} ms (min {min(events):.3f}) = "
              f"{moved / (launch * 1e-3) / 1e9:.0f} GB/s over the algorithmic bytes")


def energy_fixer_bench(lib, n, nz, reps):
    """EnergyFixer on one tile of C<n> x <nz> (helpers.l2e_synthetic_case on synthetic.tile_metrics): the mode-0 launch, the
    mode-1 launch (the words zeroed first, as in the step) and the finalising launch, each against the same quantities restated
    with torch on the device (views of the compute domain; the geopotential by a cumulative sum, the global sums as float sums --
    neither reproducible nor in the kernel's order).  Neither side synchronises; both are timed with the host clock from an idle
    device to the end of a synchronisation added for the measurement, alternating, medians; then each launch alone in device
    events, with its bandwidth over the algorithmic bytes: the six species, pt, delp, delz, w, u, v (mode 1: and pkz) read once."""
    import time

    from helpers import l2e_synthetic_case
    from pace_amd import synthetic
    from pace_amd.fv3core.stencils.energy_fixer import EnergyFixer
    from pace_amd.tile import Env
    from pace_amd.util import NullComm
    from pace_amd.util import constants as c

    f, tr, _, _, _ = l2e_synthetic_case(n, nz)
    rng = np.random.default_rng(7)
    f["pkz"] = rng.uniform(1.0, 7.0, f["pt"].shape)
    f["phis"] = rng.uniform(0.0, 2.0e4, f["phis"].shape)
    env = Env(lib, "cuda", synthetic.tile_metrics(n, nz), n, nz)
    q = {k: env.q3(f[k]) for k in ("pt", "delp", "delz", "w", "u", "v", "pkz")}
    water = [env.q3(tr[k]) for k in ("qvapor", "qliquid", "qrain", "qsnow", "qice", "qgraupel")]
    phis, te0 = env.q2(f["phis"]), env.q2()
    gd = env.grid_data
    fixer = EnergyFixer(env.stencil_factory, env.qf, NullComm(0, 6))
    cs, cs1 = slice(3, 3 + n), slice(4, 4 + n)
    v3 = {k: x.data[cs, cs, :nz].double() if lib.real_bytes == 4 else x.data[cs, cs, :nz] for k, x in q.items()}
    u1, v1 = q["u"].data[cs, cs1, :nz], q["v"].data[cs1, cs, :nz]
    qv, ql, qr, qs, qi, qg = (x.data[cs, cs, :nz] for x in water)
    rsin2, cosa, area = (x.data[cs, cs, None].double() for x in (gd.rsin2, gd.cosa_s, gd.area_64))
    ph = phis.data[cs, cs, None].double()
    restated = {}

    def columns(mode):
        u0, v0 = v3["u"], v3["v"]
        interfaces = ph + torch.flip(torch.cumsum(torch.flip(-c.GRAV * v3["delz"], [2]), 2), [2])  # phi_above of every level
        below = torch.cat([interfaces[:, :, 1:], ph], 2)
        ke = (0.5 * rsin2) * ((u0 * u0 + u1 * u1 + v0 * v0 + v1 * v1) - ((u0 + u1) * (v0 + v1)) * cosa)
        liquid, solid = ql + qr, qi + qs + qg
        gz = liquid + solid
        cvm = (1.0 - (qv + gz)) * c.CV_AIR + qv * c.CV_VAP + liquid * c.C_LIQ + solid * c.C_ICE
        e = cvm * v3["pt"]
        if mode == 1:
            e = e / ((1.0 + c.ZVIR * qv) * (1.0 - gz))
        te = (v3["delp"] * (e + 0.5 * (interfaces + below + v3["w"] * v3["w"] + ke))).sum(2)
        if mode == 0:
            restated["te0"] = te
        else:
            restated["te_2d"] = restated["te0"] - te
            restated["zsum"] = (v3["pkz"] * v3["delp"]).sum(2)

    def torch_finalize():
        s_te = (area[:, :, 0] * restated["te_2d"]).sum()
        s_z = (area[:, :, 0] * restated["zsum"]).sum()
        restated["out"] = torch.stack([s_te, s_z, s_te / (c.CV_AIR * s_z), s_te / (c.GRAV * 225.0 * 4.0 * c.PI * c.RADIUS ** 2)])

    args = (water, q["pt"], q["delp"], q["delz"], q["w"], q["u"], q["v"])
    pairs = {
        "mode 0": (lambda: fixer.total_energy(0, *args, None, phis, gd.rsin2, gd.cosa_s, None, te0, c.ZVIR), lambda: columns(0)),
        "mode 1": (lambda: fixer.total_energy(1, *args, q["pkz"], phis, gd.rsin2, gd.cosa_s, gd.area_64, te0, c.ZVIR),
                   lambda: columns(1)),
        "finalize": (lambda: fixer.finalize(1.0, 225.0), torch_finalize),
    }
    for hip, restatement in pairs.values():
        hip()
        restatement()
    torch.cuda.synchronize()
    got = fixer.result.cpu().numpy()
    want = restated["out"].cpu().numpy()
    te_err = float((te0.data[cs, cs].double() - restated["te0"]).abs().max() / restated["te0"].abs().max())
    print(f"  te0_2d: max |hip - torch| / max |torch| {te_err:.3e}; S_te hip {got[0]:.12e} torch {want[0]:.12e}; "
          f"S_z hip {got[1]:.12e} torch {want[1]:.12e}; dtmp hip {got[2]:.6e} torch {want[2]:.6e}")
    cells = n * n * nz
    moved = {"mode 0": (12 * cells + 4 * n * n) * lib.real_bytes, "mode 1": (13 * cells + 7 * n * n) * lib.real_bytes, "finalize": 112}
    print(f"energy_fixer C{n} x {nz}, float{8 * lib.real_bytes} fields, one tile: {n * n} columns; medians of {reps} alternating runs, ms")
    for name, (hip, restatement) in pairs.items():
        times = {"hip": [], "torch": []}
        for _ in range(3):
            hip()
            restatement()
        for _ in range(reps):
            for k, fn in (("hip", hip), ("torch", restatement)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
        med = {k: float(np.median(x)) for k, x in times.items()}
        events = times_hip_calibrate(hip, reps)
        launch = float(np.median(events))
        rate = f" = {moved[name] / (launch * 1e-3) / 1e9:.0f} GB/s over {moved[name] / 1e6:.1f} MB" if moved[name] > 1e6 else ""
        print(f"  {name:9s} hip {med['hip']:8.3f} ms (min {min(times['hip']):.3f})   torch {med['torch']:8.3f} ms (min "
              f"{min(times['torch']):.3f})   ratio torch / hip {med['torch'] / med['hip']:.2f}; in device events: median "
              f"{launch * 1e3:.1f} us (min {min(events) * 1e3:.1f}){rate}")


def tracer_subcycle_bench(lib, n, nz, reps, device="cuda"):
    """TracerAdvection of seven tracers on tile 0 of the C<n> x <nz> baroclinic state (the driver's initialisation on the generated
    grid, a lone-rank LoopbackComm; the mass fluxes and Courant numbers are what ONE step_dynamics of that state accumulated):
    the reference's fixed three sub-cycles against courant_subcycling=True.  Every run starts from the same fields (restored
    outside the timed region), both are timed with the host clock from an idle device to the end of a synchronisation,
    alternating, medians.  Then pace_tracer_cmax alone in device events, with its bandwidth over cx + cy read once, and the
    finalising launch with the transfer and its synchronisation alone (host clock)."""
    import ctypes as C
    import time

    import yaml

    from pace_amd.driver import Driver, DriverConfig
    from pace_amd.fv3core.stencils.fillz import tracer_variables
    from pace_amd.fv3core.stencils.tracer_2d_1l import TracerAdvection
    from pace_amd.util import CubedSphereCommunicator, LoopbackComm

    with open(os.path.join(ROOT, "tests", "golden", "driver_baroclinic_c12.yaml")) as f:
        settings = yaml.safe_load(f)
    # (the dynamical core alone: the physics, which the float32 library refuses, never runs here)
    settings.update(nx_tile=n, nz=nz, diagnostics_config={}, stencil_config={}, safety_check_frequency=0, disable_step_physics=True)
    driver = Driver(DriverConfig.from_dict(settings), comm=LoopbackComm(rank=0, total_ranks=6), lib=lib, device=device)
    core, state = driver.dycore, driver.state.dycore_state
    core.step_dynamics(state)
    torch.cuda.synchronize()
    tracers = {name: core.tracers[name] for name in tracer_variables[:7]}
    fields = dict(dp1=core._dp_initial, mfxd=state.mfxd, mfyd=state.mfyd, cxd=state.cxd, cyd=state.cyd, **tracers)
    saved = {name: q._base.clone() for name, q in fields.items()}
    cube = CubedSphereCommunicator(LoopbackComm(rank=0, total_ranks=6), device=device, lib=lib)
    transport = core.tracer_advection.finite_volume_transport
    make = lambda **kw: TracerAdvection(driver.stencil_factory, driver.quantity_factory, transport, driver.state.grid_data, cube,  # noqa: E731
                                        tracers, **kw)
    modes = {"fixed": make(), "courant": make(courant_subcycling=True)}

    def restore():
        for name, q in fields.items():
            q._base.copy_(saved[name])

    def run(mode):
        modes[mode](tracers, fields["dp1"], fields["mfxd"], fields["mfyd"], fields["cxd"], fields["cyd"])

    times = {mode: [] for mode in modes}
    for rep in range(reps + 3):
        for mode in modes:
            restore()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(mode)
            torch.cuda.synchronize()
            if rep >= 3:
                times[mode].append((time.perf_counter() - t0) * 1e3)
    restore()
    adv = modes["courant"]
    counts = adv.subcycles
    cmax = adv._cmax.cpu().numpy()
    med = {mode: float(np.median(x)) for mode, x in times.items()}
    print(f"tracer_subcycle C{n} x {nz}, float{8 * lib.real_bytes} fields, one tile, seven tracers; medians of {reps} alternating runs")
    print(f"  cmax over the tile: {cmax.min():.4f} .. {cmax.max():.4f}; sub-cycles: " +
          ", ".join(f"{int((counts == v).sum())} levels x {int(v)}" for v in np.unique(counts)))
    print(f"  fixed (3 sub-cycles) {med['fixed']:8.3f} ms (min {min(times['fixed']):.3f})   courant {med['courant']:8.3f} ms (min "
          f"{min(times['courant']):.3f})   ratio fixed / courant {med['fixed'] / med['courant']:.2f}")

    def launch():
        adv.call("pace_tracer_cmax", fields["cxd"].ptr, fields["cyd"].ptr, driver.state.grid_data.sin_sg5.ptr,
                 C.c_void_p(adv._cmax.data_ptr()), adv.stream())

    events = times_hip_calibrate(launch, reps)
    alone = float(np.median(events))
    moved = 2 * n * n * nz * lib.real_bytes
    print(f"  pace_tracer_cmax alone, device events: median {alone * 1e3:.1f} us (min {min(events) * 1e3:.1f}) = "
          f"{moved / (alone * 1e-3) / 1e12:.2f} TB/s over {moved / 1e6:.1f} MB (cx + cy)")
    host = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        adv._subcycle_counts()
        host.append((time.perf_counter() - t0) * 1e6)
    print(f"  pace_tracer_subcycles + the transfer of {nz + 2} integers + its synchronisation, host clock: median "
          f"{float(np.median(host)):.1f} us (min {min(host):.1f})")
    driver.cleanup()


def times_hip_calibrate(fn, reps=10):
    """device-event times (ms) of the calibration call"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def geos_wrapper_bench(lib, n, nz, reps):
    """GeosDycoreWrapper's two ends without the step between them: the ingest (_put_fortran_data_in_dycore: np.copyto per
    argument into the pinned staging buffer, one H2D copy, one pace_state_unpack launch) and the export (_prep_outputs_for_geos:
    one pace_diag_pack launch, one D2H copy, one synchronisation) against the same work restated with torch -- per window one
    .copy_ of the argument's slice into the field's window, per output .contiguous().cpu() of the field's window.  Both ends of
    both paths finish with the data where it belongs and are timed with the host clock from an idle device; the paths alternate,
    medians are reported.  The split of the HIP path comes from device events around the two copies and the two launches
    (Library.timing), and the host clock up to the H2D copy."""
    import time

    from pace_amd.fv3core import GeosDycoreWrapper
    from pace_amd.fv3core.initialization.geos_wrapper import ARGUMENTS, TRACERS
    from pace_amd.util import KernelTimes, NullComm

    namelist = {"nx_tile": n, "nz": nz, "dt_atmos": 225, "layout": [1, 1], "dycore_config": {"k_split": 1, "n_split": 1}}
    wrapper = GeosDycoreWrapper(namelist, NullComm(rank=0, total_ranks=6, fill_value=0.0), "hip:gfx950", lib=lib)
    state = wrapper.dycore_state
    rng = np.random.default_rng(0)
    c_args = [rng.uniform(-1.0, 1.0, wrapper._ingest[name][0]) for name in ARGUMENTS]
    f_args = [np.asfortranarray(a) for a in c_args]

    def window(field, w):
        i0, j0, k0, ni, nj, nk = w
        return field.data[i0:i0 + ni, j0:j0 + nj, k0:k0 + nk] if field.data.dim() == 3 else field.data[i0:i0 + ni, j0:j0 + nj]

    def hip_ingest(arguments=c_args):
        wrapper._put_fortran_data_in_dycore(*arguments)
        torch.cuda.current_stream().synchronize()

    def torch_ingest():
        for name, a in zip(ARGUMENTS, c_args):
            _, cut, w = wrapper._ingest[name]
            if name == "q":
                for t, tracer in enumerate(TRACERS):
                    window(getattr(state, tracer), w).copy_(torch.from_numpy(a[cut + (slice(None), t)]))
            else:
                window(getattr(state, name), w).copy_(torch.from_numpy(a[cut]))
        torch.cuda.current_stream().synchronize()

    def hip_export():
        return wrapper._prep_outputs_for_geos()

    def torch_export():
        return {name: window(getattr(state, name), w).contiguous().to(torch.float64).cpu() for name, w in wrapper._export.items()}

    # the two paths do the same thing
    names = list(wrapper._export)
    torch_ingest()
    want_state = {name: getattr(state, name).data.clone() for name in names}
    for name in names:
        getattr(state, name).data.zero_()
    for arguments in (c_args, f_args):
        hip_ingest(arguments)
        for name in names:
            assert torch.equal(getattr(state, name).data, want_state[name]), name
    got, want = hip_export(), torch_export()
    for name in names:
        assert np.array_equal(got[name].view(np.uint64), want[name].numpy().view(np.uint64)), name  # (bit for bit)

    def hip_ingest_one_thread():
        wrapper.staging_threads, threads = 1, wrapper.staging_threads
        hip_ingest()
        wrapper.staging_threads = threads

    paths = {"hip ingest": hip_ingest, "torch ingest": torch_ingest, "hip export": hip_export, "torch export": torch_export,
             "hip ingest, F-ordered arguments": lambda: hip_ingest(f_args), "hip ingest, one staging thread": hip_ingest_one_thread}
    times = {k: [] for k in paths}
    for fn in paths.values():  # warm-up: code objects, the pinned buffers, torch's copy kernels
        for _ in range(2):
            fn()
    for _ in range(reps):
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[k].append((time.perf_counter() - t0) * 1e3)

    # the split: events around the copies, Library.timing around the launches, the host clock up to the H2D copy
    split = {k: [] for k in ("staging C", "staging F", "h2d", "d2h")}
    events = []
    to_device, to_host = wrapper._to_device, wrapper._packer._to_host
    mark = {}

    def timed(kind, fn):
        def run(a, b):
            if kind == "h2d":
                split[mark["staging"]].append((time.perf_counter() - mark["t0"]) * 1e3)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(a, b)
            e1.record()
            events.append((kind, e0, e1))
        return run

    wrapper._to_device, wrapper._packer._to_host = timed("h2d", to_device), timed("d2h", to_host)
    launches = {"C": KernelTimes(), "F": KernelTimes()}
    for _ in range(reps):
        for order, arguments in (("C", c_args), ("F", f_args)):
            lib.timing = launches[order]
            torch.cuda.synchronize()
            mark.update(staging="staging " + order, t0=time.perf_counter())
            hip_ingest(arguments)
        lib.timing = launches["C"]
        hip_export()
        lib.timing = None
        torch.cuda.synchronize()
    wrapper._to_device, wrapper._packer._to_host = to_device, to_host
    for kind, e0, e1 in events:
        split[kind].append(e0.elapsed_time(e1))
    info = {order: kt.resolve() for order, kt in launches.items()}

    def per_call(order, name):
        return info[order][name]["total_run_time"] / info[order][name]["ncalls"] * 1e3

    in_elems, out_elems = wrapper._staging.numel(), sum(int(np.prod(w[3:])) for w in wrapper._export.values())
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(f"geos_wrapper C{n} x {nz}, float{8 * lib.real_bytes} fields: 30 windows in ({in_elems * 8 / 1e6:.0f} MB of float64), 30 out "
          f"({out_elems * 8 / 1e6:.0f} MB of float64); medians of {reps} alternating runs, ms")
    for k in paths:
        print(f"  {k:34s} {med[k]:9.2f}   (min {min(times[k]):.2f})")
    print(f"  ratio torch / hip: ingest {med['torch ingest'] / med['hip ingest']:.2f}, export {med['torch export'] / med['hip export']:.2f}, "
          f"both {(med['torch ingest'] + med['torch export']) / (med['hip ingest'] + med['hip export']):.2f}")
    unpack_c, unpack_f, pack = per_call("C", "pace_state_unpack"), per_call("F", "pace_state_unpack"), per_call("C", "pace_diag_pack")
    h2d, d2h = float(np.median(split["h2d"])), float(np.median(split["d2h"]))
    print(f"  split of the HIP path, {wrapper.staging_threads} staging threads (medians; launches: mean device time between events):")
    print(f"    host staging (np.copyto per argument)  C-ordered {np.median(split['staging C']):8.2f}   F-ordered {np.median(split['staging F']):8.2f}")
    print(f"    H2D copy  {h2d:8.2f} = {in_elems * 8 / (h2d * 1e-3) / 1e9:6.1f} GB/s      D2H copy + synchronisation {d2h:8.2f} = "
          f"{out_elems * 8 / (d2h * 1e-3) / 1e9:6.1f} GB/s")
    gb_in, gb_out = in_elems * (8 + lib.real_bytes) / 1e9, out_elems * (8 + lib.real_bytes) / 1e9
    print(f"    pace_state_unpack  ZFAST items (in_step 7 for q) {unpack_c:7.3f} = {gb_in / (unpack_c * 1e-3):6.0f} GB/s of read + write   "
          f"XFAST items {unpack_f:7.3f} = {gb_in / (unpack_f * 1e-3):6.0f} GB/s")
    print(f"    pace_diag_pack     {pack:7.3f} = {gb_out / (pack * 1e-3):6.0f} GB/s of read + write")


if __name__ == "__main__":
    main()
