"""Shared test plumbing: golden loading, environment construction, the reference's comparison metric."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

import sys

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from pace_amd.tile import (DSW_ARGS, DSW_CFG, DSW_DEAD, RIEM_ARGS, Env, compare, dsw_live_window, dsw_window, run_d_sw, run_riem3,  # noqa: E402,F401
                           window)


def golden(name):
    return dict(np.load(os.path.join(GOLDEN, name), allow_pickle=False))


def column_for_levels(k_sel):
    col = golden("column_namelist_c12.npz")
    return {k: np.ascontiguousarray(v[np.asarray(k_sel)]) for k, v in col.items()}


def oracle_grid(metrics, n, nk):
    from oracle._np import Grid

    return Grid(n, nk, dict(metrics))


def minimal_metrics(n, area=1.0):
    """The metric terms an Env needs at any size, for operators that read none of them but (at most) the cell area.
    (tools/make_golden_physics.py make_env holds the same dictionary plus ptop -- tools/ imports nothing from tests/: keep the
    two alike.)"""
    full = area if isinstance(area, np.ndarray) else np.full((n + 7, n + 7), float(area))
    return {"area": full, "da_min": 1.0, "da_min_c": 1.0,
            **{k: np.zeros((n + 7, n + 7)) for k in ("del6_u", "del6_v", "divg_u", "divg_v")}}


def _make(target):
    """`make <target>` under an exclusive file lock: several test processes (pytest -n) may ask for the same library at once."""
    import fcntl

    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    with open(os.path.join(ROOT, "build", ".make.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            subprocess.run(["make", "-s", "-j4", target], cwd=ROOT, check=True, stdout=subprocess.DEVNULL)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def build_emu():
    """Build tests/emu/libpace_emu.so (the kernel sources compiled for the CPU).  Test infrastructure."""
    _make("emu")
    return os.path.join(ROOT, "tests", "emu", "libpace_emu.so")


def build_emu_f32():
    """tests/emu/libpace_emu_f32.so: the emulation build with float32 storage (Makefile emu-f32).  Every test that wants it asks
    here: a bare `make emu-f32` next to a locked one links the library from objects another process is still writing."""
    _make("emu-f32")
    return os.path.join(ROOT, "tests", "emu", "libpace_emu_f32.so")


def build_emu_canon():
    """8 x 8 transport tiles, runs of 3: the canonical edge path (ppm_run_canon) at C16 / C24 (Makefile emu-canon)."""
    _make("emu-canon")
    return os.path.join(ROOT, "tests", "emu", "libpace_emu_canon.so")


def build_emu_small():
    """tests/emu/libpace_emu_small.so: the emulation build with 4 x 4 LDS tiles (interior code paths at C12)."""
    _make("emu-small")
    return os.path.join(ROOT, "tests", "emu", "libpace_emu_small.so")


def build_wgmap_check():
    """build/wgmap_check and build/wgmap_check_asan: the stand-alone exhaustive check of the workgroup maps (csrc/wgmap.h,
    tests/emu/wgmap_check.cpp; Makefile wgmap-check), plain and under AddressSanitizer + UBSan."""
    _make("wgmap-check")
    return os.path.join(ROOT, "build", "wgmap_check"), os.path.join(ROOT, "build", "wgmap_check_asan")


def riem3_inputs(s, **over):
    """The arguments of riem_solver3 (RIEM_ARGS) from a synthetic acoustic state; `over`: fields taken from elsewhere."""
    inp = {"cappa": s["cappa"], "zs": s["zs"], "ws": s["ws"], "delz": s["delz"], "q_con": s["q_con"], "delp": s["delp"],
           "pt": s["pt"], "zh": s["zh"], "p": s["pe"], "ppe": s["ppe"], "pk3": s["pk3"], "pk": s["pk"],
           "log_p_interface": s["peln"], "w": s["w"]}
    inp.update(over)
    return inp


def oracle_riem3(g, inp, last_call, dt, ptop):
    from oracle import vertical

    b = {k: v.copy() for k, v in inp.items()}
    vertical.riem_solver3(g, last_call, dt, b["cappa"], ptop, b["zs"], b["ws"], b["delz"], b["q_con"], b["delp"], b["pt"],
                          b["zh"], b["p"], b["ppe"], b["pk3"], b["pk"], b["log_p_interface"], b["w"], p_fac=0.05)
    return b


def check_other_level_counts(lib, device, nz, dsw_tol=0.0):
    """d_sw and riem_solver3 (not the last call) at C12 with nz layers against the oracle: d_sw within dsw_tol (0: bit for bit,
    the emulation; 3.2e-10, translate_d_sw.py:19, the device), the column solver to the exp / log rounding (5e-6,
    overrides/standard.yaml:49-61).  Returns {variable: error} of the column solver."""
    from oracle import dgrid_sw
    from pace_amd import synthetic
    from pace_amd.fv3core import DGridShallowWaterLagrangianDynamicsConfig
    from pace_amd.fv3core.stencils.d_sw import get_column_namelist

    n = 12
    metrics = synthetic.tile_metrics(n, nz)
    s = synthetic.acoustic_state(metrics, n, nz)
    env = Env(lib, device, metrics, n, nz)
    colq = get_column_namelist(DGridShallowWaterLagrangianDynamicsConfig(**DSW_CFG), env.qf)
    col = {k: (v.numpy() if hasattr(v, "numpy") else np.asarray(v))[:nz] for k, v in colq.items()}
    out, _ = run_d_sw(env, col, {k: s[k] for k in DSW_ARGS}, s["dt"])
    g = oracle_grid(metrics, n, nz)
    a = {k: s[k].copy() for k in DSW_ARGS}
    dgrid_sw.d_sw(g, col, DSW_CFG, dgrid_sw.DSWState(s["u"].shape), *[a[k] for k in DSW_ARGS], s["dt"])
    for k in DSW_ARGS:
        if k != "zh":
            assert compare(a[k][dsw_window(k, n, nz)], out[k][dsw_window(k, n, nz)]) <= dsw_tol, k
    inp = riem3_inputs(s, q_con=a["q_con"], delp=a["delp"], pt=a["pt"], w=a["w"])
    got = run_riem3(env, inp, False, s["dt"], metrics["ptop"])
    b = oracle_riem3(g, inp, False, s["dt"], metrics["ptop"])
    errs = {}
    for k in ("delz", "zh", "ppe", "pk3", "w"):
        nk = nz if k in ("delz", "w") else nz + 1
        errs[k] = compare(b[k][window(n, 0, 0, nk)], got[k][window(n, 0, 0, nk)], near_zero=1e-9 * float(np.abs(b[k]).max()))
        assert errs[k] < 5e-6, k
    return errs


# the near-zero floors of riem_solver3's check in tests/opchain.py (Chain.cases), as fractions of a field's magnitude: w and the
# perturbation pressure cross zero, the rest have none
RIEM3_OPCHAIN_FLOORS = {"w": 1e-5, "ppe": 1e-5, "delz": 0.0, "zh": 0.0, "pk3": 0.0, "p": 0.0, "pk": 0.0, "log_p_interface": 0.0}


def check_riem_column_windows(lib, device, n, nz=33, last_call=True, solver_c=True, floors=None):
    """riem_solver3 on the compute domain of a C<n> tile with nz layers and (solver_c) riem_solver_c on compute + 1 (other window
    bounds of k_riem3f.hip ColumnWindows), against the oracle: riem_solver3 within 5e-6 (overrides/standard.yaml:49-61),
    riem_solver_c within 5e-14 (translate_riem_solver_c.py:33), and nothing outside the compute domain (compute + 1) is
    written.  floors: the near-zero escape of the comparison per variable, as a fraction of the field's magnitude (default: 1e-9
    for all).  Returns {variable: error} ("c.pef", "c.gz": riem_solver_c)."""
    from oracle import vertical
    from pace_amd import synthetic
    from pace_amd.fv3core.stencils.riem_solver_c import NonhydrostaticVerticalSolverCGrid

    metrics = synthetic.tile_metrics(n, nz)
    s = synthetic.acoustic_state(metrics, n, nz)
    env = Env(lib, device, metrics, n, nz)
    g = oracle_grid(metrics, n, nz)
    inp = riem3_inputs(s)
    got = run_riem3(env, inp, last_call, s["dt"], metrics["ptop"])
    b = oracle_riem3(g, inp, last_call, s["dt"], metrics["ptop"])
    errs = {}
    for k in ("delz", "zh", "ppe", "pk3", "w", "p", "pk", "log_p_interface"):
        nk = nz if k in ("delz", "w") else nz + 1
        floor = 1e-9 if floors is None else floors[k]
        errs[k] = compare(b[k][window(n, 0, 0, nk)], got[k][window(n, 0, 0, nk)], near_zero=floor * float(np.abs(b[k]).max()))
        assert errs[k] < 5e-6, (k, errs[k])
        # nothing outside the compute domain is written
        outside = np.ones(b[k].shape, dtype=bool)
        outside[window(n, 0, 0, nk)] = False
        outside[:, :, nk:] = False
        assert np.array_equal(got[k][outside], inp[k][outside]), k
    if not solver_c:
        return errs
    # riem_solver_c: compute + 1
    solver = NonhydrostaticVerticalSolverCGrid(env.stencil_factory, env.qf, 0.05)
    a = {k: s[k].copy() for k in ("cappa", "pt", "q_con", "delp", "zh", "w")}
    f = {k: env.q3(v) for k, v in a.items()}
    hs = s["zs"] * 9.80665
    ws3 = np.ascontiguousarray(s["ws"])
    pef = env.q3(np.zeros_like(s["zh"]))
    solver(0.5 * s["dt"], f["cappa"], float(metrics["ptop"]), env.q2(hs), env.q2(ws3), f["pt"], f["q_con"], f["delp"], f["zh"], pef, f["w"])
    ref_pef = np.zeros_like(s["zh"])
    vertical.riem_solver_c(g, 0.5 * s["dt"], a["cappa"], float(metrics["ptop"]), hs, ws3, a["pt"], a["q_con"], a["delp"], a["zh"], ref_pef,
                           a["w"], p_fac=0.05)
    W = (slice(2, 4 + n), slice(2, 4 + n), slice(0, nz + 1))
    errs["c.pef"] = compare(ref_pef[W], pef.numpy()[W])
    errs["c.gz"] = compare(a["zh"][W], f["zh"].numpy()[W])
    assert errs["c.pef"] < 5e-14
    assert errs["c.gz"] < 5e-14
    # nothing outside compute + 1 is written (pef started as zeros, gz as the input heights)
    outside = np.ones(s["zh"].shape, dtype=bool)
    outside[W] = False
    assert np.array_equal(pef.numpy()[outside], np.zeros_like(s["zh"])[outside])
    assert np.array_equal(f["zh"].numpy()[outside], s["zh"][outside])
    return errs


def expand_riem_fixture(fix, n=12, nz=79):
    """The fixture stores 4 rows of columns; tile them over the compute domain (columns are independent)."""
    out = {}
    reps = n // 4
    for key, v in fix.items():
        if not key.startswith("in_"):
            continue
        name = key[3:]
        if v.ndim == 3:
            full = np.zeros((n + 7, n + 7, nz + 1))
            full[3 : 3 + n, 3 : 3 + n] = np.tile(v, (1, reps, 1))
        else:
            full = np.zeros((n + 7, n + 7))
            full[3 : 3 + n, 3 : 3 + n] = np.tile(v, (1, reps))
        out[name] = full
    return out


# ------------------------------------------------------------------------------------------------------------------
# whole-AcousticDynamics runs (6 tiles in one process, one thread per tile)
# ------------------------------------------------------------------------------------------------------------------
ACOUSTIC_OUT = "u v w delz delp pt pe pk peln q_con omga ua va uc vc mfxd mfyd cxd cyd diss_estd heat_source".split()


# (u, v: the meridional wind of an equatorial tile of this zonal-flow case is ~0.1 m/s with zero crossings; the full-field
# fixtures contain entries 1e-8 of that, where a relative metric measures the rounding of the last ulp of the 35 m/s zonal wind)
_BANDS = {"mfxd": 1e-6, "mfyd": 1e-6, "cxd": 1e-6, "cyd": 1e-6, "uc": 1e-8, "vc": 1e-8, "diss_estd": 1e-8, "w": 1e-5, "omga": 1e-5,
          "u": 1e-7, "v": 1e-7}


def acoustic_fixture(t):
    """tests/golden/acoustic_c12_tile<t>.npz + what the reference run left in the work fields uc / vc (a later addition kept
    in acoustic_c12_ucvc.npz, tools/make_golden_acoustic.py; TranslateDynCore compares them, translate_dyncore.py:84-85)."""
    fix = golden(f"acoustic_c12_tile{t}.npz")
    extra = golden("acoustic_c12_ucvc.npz")
    for k in ("uc", "vc"):
        fix["out_" + k], fix["col_" + k] = extra[f"out_{k}_tile{t}"], extra[f"col_{k}_tile{t}"]
    # tiles 0 (equatorial) and 2 (polar) also have their FULL output fields: every level of the compute window + the
    # staggered row / column (acoustic_c12_full.npz, a later addition)
    full = golden("acoustic_c12_full.npz")
    if t in full["tiles"]:
        for k in ACOUSTIC_OUT:
            fix["full_" + k] = full[f"out_{k}_tile{t}"]
    return fix


# Bounds of the whole-AcousticDynamics comparisons (GPU and emulation; reference metric, bands above): the reference's own DynCore
# bound, 2e-6 for EVERY variable (translate_dyncore.py:120) is the ceiling; what is measured far below it is held two to three
# orders above the measurement (GPU, profiles/r06_acoustic_c12_gpu_errors.json: masses / temperatures / pressures <= 1.1e-15, the
# A-grid winds 1.4e-11, the accumulators 1e-12, delz 4e-13, heat_source 3e-9, u / v 1.5e-8, omga 8e-8, vc 1.3e-7, w 4e-7).
# The ONE variable not held to 2e-6 is diss_estd (measured 2.2e-6 .. 2.9e-6): w's damping heating of THIS fixture amplifies an ulp of
# the column solver's operands by ~1e10.  That is a property of the loop, not of the kernels: the numpy oracle ITSELF moves by
# diss_estd 1.35e-6 / w 1.7e-7 when only its two column sums of the interface pressures are formed in another order (extended
# precision, rounded once per level: <= 1 ulp away; tests/test_oracle_golden.py::test_loop_conditioning_of_diss_estd), and the
# device forms those sums AND the two tridiagonal sweeps as parallel scans over sixteen lanes (k_riem3f.hip).  With the sequential
# legacy solvers (PACE_LEGACY_COLUMN_SOLVERS=1, bit-identical arithmetic order) the same test measures diss_estd 1.0e-7, w 5.6e-9 --
# exactly what the oracle gives with exp / log evaluated in extended precision.  Round 6 took the solvers' own exp / log from
# ~1 ulp to <= 0.55 ulp (2.9e-6 -> 2.2e-6); the rest is re-association, which no parallel column solver avoids.
ACOUSTIC_TOL = {"w": 2e-6, "omga": 2e-6, "diss_estd": 3e-6, "uc": 2e-6, "vc": 2e-6, "u": 1e-6, "v": 1e-6, "heat_source": 1e-6,
                "ua": 1e-8, "va": 1e-8, "delz": 1e-10, "mfxd": 1e-9, "mfyd": 1e-9, "cxd": 1e-9, "cyd": 1e-9}
ACOUSTIC_TOL_DEFAULT = 1e-12  # delp, pt, pe, pk, peln, q_con


ACOUSTIC_VARIANTS = {"v2": dict(nord=2, d_con=0.0, hord_dp=5, hord_tm=5, hord_vt=5, hord_mt=5)}  # tools/make_golden_acoustic.py


def acoustic_config(n_split, variant=None):
    """The baroclinic_c12 namelist values the fixture was generated with (tools/capture.py dycore_config); `variant`: the
    options changed in acoustic_c12_<variant>.npz."""
    from pace_amd.fv3core import AcousticDynamicsConfig, DGridShallowWaterLagrangianDynamicsConfig, RiemannConfig

    o = dict(nord=3, d_con=1.0, hord_dp=6, hord_tm=6, hord_vt=6, hord_mt=6)
    o.update(ACOUSTIC_VARIANTS.get(variant, {}))
    dsw = DGridShallowWaterLagrangianDynamicsConfig(nord=o["nord"], d_con=o["d_con"], hord_dp=o["hord_dp"], hord_tm=o["hord_tm"],
                                                    hord_vt=o["hord_vt"], hord_mt=o["hord_mt"])
    return AcousticDynamicsConfig(n_split=n_split, k_split=1, nord=o["nord"], d_con=o["d_con"], rf_fast=True, rf_cutoff=3000.0, tau=10.0,
                                  p_fac=0.05, hord_tm=o["hord_tm"], delt_max=0.002, d_grid_shallow_water=dsw,
                                  riemann=RiemannConfig(p_fac=0.05))


def run_acoustic_tile(comm, lib, device, fix, n, nz, variant=None, checkpointer=None):
    """One tile's program: build the environment from the fixture, run one AcousticDynamics call."""
    import torch

    from pace_amd.fv3core.initialization.dycore_state import DycoreState
    from pace_amd.fv3core.stencils.dyn_core import AcousticDynamics
    from pace_amd.util import CubedSphereCommunicator

    metrics = {k[5:]: v for k, v in fix.items() if k.startswith("grid_")}
    env = Env(lib, device, metrics, n, nz)
    cube = CubedSphereCommunicator(comm, device=device, lib=lib)
    state = DycoreState.init_from_numpy_arrays({k[3:]: v for k, v in fix.items() if k.startswith("in_") and k != "in_cappa"}, env.qf)
    n_split = int(fix["n_split"])
    wsd = env.q2()
    dyn = AcousticDynamics(cube, env.stencil_factory, env.qf, env.grid_data, env.damping, 0, False, False,
                           acoustic_config(n_split, variant), state.phis, wsd, state, checkpointer=checkpointer)
    dyn.cappa.set(fix["in_cappa"])
    dyn(state, timestep=float(fix["timestep"]), n_map=1)
    if env.qf.device.type == "cuda":
        torch.cuda.synchronize()
    out = {k: getattr(state, k).numpy() for k in ACOUSTIC_OUT if k != "heat_source"}
    out["heat_source"] = dyn._heat_source.numpy()
    return out


def acoustic_variant_fixture(t, variant):
    """Inputs of the baseline fixture of tile t, outputs of the reference run with the variant's namelist."""
    fix = {k: v for k, v in acoustic_fixture(t).items() if not k.startswith(("out_", "col_", "full_"))}
    var = golden(f"acoustic_c12_{variant}.npz")
    for k in ACOUSTIC_OUT:
        fix["out_" + k], fix["col_" + k] = var[f"out_{k}_tile{t}"], var[f"col_{k}_tile{t}"]
    return fix


def run_acoustic_six_tiles(lib, device, n=12, nz=79, variant=None, checkpointers=None):
    from pace_amd.util import run_tiles

    fixes = [acoustic_variant_fixture(t, variant) if variant else acoustic_fixture(t) for t in range(6)]
    cps = checkpointers or [None] * 6
    return fixes, run_tiles(6, lambda comm: run_acoustic_tile(comm, lib, device, fixes[comm.Get_rank()], n, nz, variant,
                                                              checkpointer=cps[comm.Get_rank()]))


def acoustic_errors(fix, out, n=12):
    """max reference-metric error per variable on the fixture's level subset and full columns (compute domain + the
    staggered interface row/column)."""
    errs = {}
    ks = fix["k_sel"]
    for k in ACOUSTIC_OUT:
        full = out[k]
        di = 1 if k in ("v", "mfxd", "cxd", "uc") else 0
        dj = 1 if k in ("u", "mfyd", "cyd", "vc") else 0
        kk = [x for x in ks if x < (80 if k in ("pe", "pk", "peln") else 79)]
        idx = [list(ks).index(x) for x in kk]
        got = full[3 : 3 + n + di, 3 : 3 + n + dj][:, :, kk]
        ref = fix["out_" + k][: n + di, : n + dj][:, :, idx]
        # values that are zero by symmetry (e.g. the meridional mass flux on the equator row of an equatorial tile) come
        # out as rounding residue 13+ orders below the field's scale; the reference's translate tests skip those through
        # per-variable near_zero overrides (tests/savepoint/translate/overrides/standard.yaml)
        # (mass / Courant fluxes across the tile's symmetry line cancel to ~1e-7 of the field scale and carry the same
        # ABSOLUTE rounding error as every other row, hence the wider band for the four accumulators)
        # (uc / vc after the call are work-field leftovers: the C-grid winds on the sponge levels -- where the meridional one
        # is rounding residue on half of the tiles of this zonal-flow case -- and ~1e-29 elsewhere; the reference ignores them
        # below 1e-13 ABSOLUTE (overrides/baroclinic.yaml:12-20), here: below 1e-8 of the field's magnitude)
        # (diss_estd is a sum of dissipation terms of both signs: entries 1e-10 of the field's magnitude are residue)
        # (w and omga cross zero; the vertical solver's absolute error is ~1e-11 of their magnitude on every implementation
        # -- device or libm exp / log against numpy's, amplified by the tridiagonal solves -- so a RELATIVE bound of 5e-6 only
        # means something above ~1e-5 of the magnitude; tools/riem_check.py prints both measures)
        band = _BANDS.get(k, 1e-12)
        near_zero = band * float(np.abs(ref).max()) + 1e-300
        e = compare(ref, got, near_zero=near_zero)
        nk = 80 if k in ("pe", "pk", "peln") else 79
        cols = np.stack([full[i, j, :nk] for (i, j) in fix["cols"]])
        e = max(e, compare(fix["col_" + k][:, :nk], cols, near_zero=near_zero))
        if "full_" + k in fix:  # the whole field, all levels
            e = max(e, compare(fix["full_" + k][: n + di, : n + dj, :nk], full[3 : 3 + n + di, 3 : 3 + n + dj, :nk], near_zero=near_zero))
        errs[k] = e
    return errs


# ------------------------------------------------------------------------------------------------------------------
# TracerAdvection on six tiles
# ------------------------------------------------------------------------------------------------------------------
def run_tracer_tile(comm, lib, device, fix, metrics, n):
    nk = len(fix["k_sel"])
    return run_tracer_arrays(comm, lib, device, {k: fix["in_" + k] for k in ("qvapor", "q2", "dp1", "mfxd", "mfyd", "cxd", "cyd")}, metrics, n, nk)


def run_tracer_arrays(comm, lib, device, arrays, metrics, n, nk):
    """TracerAdvection of the tracers qvapor and q2 on one rank's tile; arrays: qvapor, q2, dp1, mfxd, mfyd, cxd, cyd.  Returns
    all seven as the call leaves them."""
    import torch

    from pace_amd.fv3core.stencils.fvtp2d import FiniteVolumeTransport
    from pace_amd.fv3core.stencils.tracer_2d_1l import TracerAdvection
    from pace_amd.util import CubedSphereCommunicator

    env = Env(lib, device, metrics, n, nk)
    cube = CubedSphereCommunicator(comm, device=device, lib=lib)
    tracers = {"qvapor": env.q3(arrays["qvapor"]), "q2": env.q3(arrays["q2"])}
    f = {k: env.q3(arrays[k]) for k in ("dp1", "mfxd", "mfyd", "cxd", "cyd")}
    transport = FiniteVolumeTransport(env.stencil_factory, env.qf, env.grid_data, env.damping, 0, 8)
    adv = TracerAdvection(env.stencil_factory, env.qf, transport, env.grid_data, cube, tracers)
    adv(tracers, f["dp1"], f["mfxd"], f["mfyd"], f["cxd"], f["cyd"])
    if env.qf.device.type == "cuda":
        torch.cuda.synchronize()
    out = {k: v.numpy() for k, v in tracers.items()}
    out.update({k: v.numpy() for k, v in f.items()})
    return out


def run_tracer_tiles(lib, device, metrics, arrays, n, nk):
    """TracerAdvection on six tiles of any size joined by the cube communicator; metrics, arrays: one per tile."""
    from pace_amd.util import run_tiles

    return run_tiles(6, lambda comm: run_tracer_arrays(comm, lib, device, arrays[comm.Get_rank()], metrics[comm.Get_rank()], n, nk))


def run_tracer_six_tiles(lib, device, n=12):
    from pace_amd.util import run_tiles

    fixes = [golden(f"tracer_c12_tile{t}.npz") for t in range(6)]
    metrics = [{k[5:]: v for k, v in golden(f"acoustic_c12_tile{t}.npz").items() if k.startswith("grid_")} for t in range(6)]
    outs = run_tiles(6, lambda comm: run_tracer_tile(comm, lib, device, fixes[comm.Get_rank()], metrics[comm.Get_rank()], n))
    return fixes, outs


def check_tracer_outputs(fixes, outs, n=12):
    for t in range(6):
        nk = len(fixes[t]["k_sel"])
        W = (slice(3, 3 + n), slice(3, 3 + n), slice(0, nk))
        for name in ("qvapor", "q2"):
            assert np.array_equal(outs[t][name][W], fixes[t]["out_" + name][W]), (t, name)
        assert np.array_equal(outs[t]["mfxd"][3 : 4 + n, 3 : 3 + n, :nk], fixes[t]["out_mfxd"][3 : 4 + n, 3 : 3 + n, :nk]), t
        assert np.array_equal(outs[t]["cyd"][3 : 3 + n, 3 : 4 + n, :nk], fixes[t]["out_cyd"][3 : 3 + n, 3 : 4 + n, :nk]), t


# ------------------------------------------------------------------------------------------------------------------
# Six-tile GPU runs in a child process (six tiles = six host threads sharing one device; run as coroutines, see
# pace_amd/util/comm.py).  Round 1 retried such a run when the child died from a signal ("seen twice in ~40 runs").  Round 2
# hunted for it: 240 consecutive runs on an MI355X (tools/abort_hunt.py: 140 acoustic, 60 whole-dycore, 40 tracer; fault
# handler on) without a single failure (profiles/r02_abort_hunt.json), so the retry is gone: a child that dies fails the test,
# and its return code + output are kept as an artefact (gpurun_out/child_failure_<what>.txt).
# ------------------------------------------------------------------------------------------------------------------
def _child_main(what, out_path, hard_exit=False):
    import pickle

    from pace_amd import _lib

    lib = _lib.load()
    if what == "acoustic":
        result = run_acoustic_six_tiles(lib, "cuda")
    elif what == "acoustic_v2":
        result = run_acoustic_six_tiles(lib, "cuda", variant="v2")
    elif what == "tracer":
        result = run_tracer_six_tiles(lib, "cuda")
    elif what == "dycore":
        result = run_dycore_six_tiles(lib, "cuda")
    elif what == "dycore_k2":
        result = run_dycore_six_tiles(lib, "cuda", prefix="dycore_k2_c12")
    elif what == "dycore_kord10":
        result = run_dycore_six_tiles(lib, "cuda", prefix="dycore_kord10_c12")
    elif what == "dycore_f32":
        result = run_dycore_six_tiles(_lib.load(32), "cuda")
    elif what == "dycore_c384_f32":
        result = (run_dycore_one_tile_synthetic(_lib.load(32), "cuda", 384, 91), run_dycore_one_tile_synthetic(_lib.load(32), "cuda", 384, 91))
    elif what == "dycore_generated":
        result = (run_dycore_six_tiles(lib, "cuda", generated="metrics"), run_dycore_six_tiles(lib, "cuda", generated="all"))
    else:
        raise ValueError(what)
    with open(out_path, "wb") as f:
        pickle.dump(result, f)
        f.flush()
        os.fsync(f.fileno())
    if hard_exit:
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0)


def run_in_child(what, tmp_path):
    import pickle

    out = os.path.join(str(tmp_path), f"{what}.pkl")
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); "
            f"import helpers; helpers._child_main({what!r}, {out!r})")
    p = subprocess.run([sys.executable, "-X", "faulthandler", "-c", code], capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        report = f"child run {what!r} failed (rc {p.returncode}):\n{p.stdout[-4000:]}\n{p.stderr[:3000]}\n...\n{p.stderr[-8000:]}"
        out_dir = os.path.join(ROOT, "gpurun_out")
        if os.path.isdir(out_dir):
            with open(os.path.join(out_dir, f"child_failure_{what}.txt"), "w") as f:
                f.write(f"child run {what!r} failed (rc {p.returncode}):\n{p.stdout}\n{p.stderr}")
        raise RuntimeError(report)
    with open(out, "rb") as f:
        return pickle.load(f)


def run_dycore_one_tile_synthetic(lib, device, n, nz, n_split=2):
    """One DynamicalCore.step_dynamics of ONE tile at any size behind a lone-rank LoopbackComm (each halo receives what the tile
    itself sent to that neighbour), pace_amd/synthetic.py's balanced state + smooth condensates.  Returns the prognostic fields
    after the step as numpy arrays (compute domain)."""
    import datetime

    import torch

    from pace_amd import synthetic
    from pace_amd.fv3core import DynamicalCoreConfig
    from pace_amd.fv3core.initialization.dycore_state import DycoreState
    from pace_amd.fv3core.stencils.fv_dynamics import DynamicalCore
    from pace_amd.util import CubedSphereCommunicator, LoopbackComm
    from pace_amd.util import constants as c

    metrics = synthetic.tile_metrics(n, nz)
    s = synthetic.acoustic_state(metrics, n, nz)
    dt_atmos = float(s["dt"]) * n_split
    env = Env(lib, device, metrics, n, nz)
    cube = CubedSphereCommunicator(LoopbackComm(rank=0, total_ranks=6), device=device, lib=lib)
    arrays = {k: s[k] for k in "u v w delz delp pt pe uc vc ua va q_con".split()}
    with np.errstate(all="ignore"):
        arrays["peln"] = np.log(s["pe"])
        arrays["pk"] = np.exp(c.KAPPA * arrays["peln"])
    arrays["phis"] = c.GRAV * s["zs"]
    arrays["ps"] = s["pe"][:, :, nz]
    arrays["pt"] = s["pt"] * np.exp(c.KAPPA * np.log(1.0e5))
    arrays["qvapor"] = 0.01 * np.exp(-6.0 * (1.0 - s["pe"] / s["pe"][:, :, nz:])) * (s["delp"] > 0)
    for name, f in dycore_condensates(0, s["delp"].shape).items():
        arrays[name] = np.abs(f)
    state = DycoreState.init_from_numpy_arrays(arrays, env.qf)
    config = DynamicalCoreConfig(npx=n + 1, npy=n + 1, npz=nz, dt_atmos=dt_atmos, k_split=1, n_split=n_split,
                                 acoustic_dynamics=acoustic_config(n_split))
    core = DynamicalCore(cube, env.grid_data, env.stencil_factory, env.qf, env.damping, config, state.phis, state,
                         datetime.timedelta(seconds=dt_atmos))
    core.step_dynamics(state)
    if device != "cpu":
        torch.cuda.synchronize()
    W = (slice(3, 3 + n), slice(3, 3 + n), slice(0, nz))
    return {k: getattr(state, k).numpy()[W].copy() for k in "u v w delz delp pt pe pk peln q_con qvapor qliquid".split() if hasattr(state, k)}


# ---- vertical remapping (tests/golden/remap_c12.npz: a run of the reference's MapSingle, tools/make_golden_remap.py) ----
# name -> (kord, iv, source interfaces, target interfaces, bottom value, qmin)
REMAP_CASES = {
    "pt_k9_iv1": (9, 1, "pn1", "pn2", None, 184.0),
    "qv_k9_iv0": (9, 0, "pe1", "pe2", None, 0.0),
    "w_k9_ivm2": (9, -2, "pe1", "pe2", "wsd", 0.0),
    "delz_k9_iv1": (9, 1, "pe1", "pe2", None, 0.0),
    "u_k9_ivm1": (9, -1, "pe1_u", "pe2_u", None, 0.0),
    "pt_k9_iv1_s": (9, 1, "pn1s", "pn2", None, 184.0),
    "qv_k9_iv0_s": (9, 0, "pe1s", "pe2", None, 0.0),
    "w_k9_ivm2_s": (9, -2, "pe1s", "pe2", "wsd", 0.0),
    "u_k9_ivm1_s": (9, -1, "pe1s_u", "pe2_u", None, 0.0),
    "qv_k10_iv0_s": (10, 0, "pe1s", "pe2", None, 0.0),
    "qv_k10_iv0": (10, 0, "pe1", "pe2", None, 0.0),
    "pt_k10_iv1": (10, 1, "pn1", "pn2", None, 184.0),
}
REMAP_KM = 79


def run_map_single(env, name, d, n=12):
    """One REMAP_CASES entry through the host class MapSingle: the fixture's compute-window arrays are embedded in full
    fields (halo 3; everything outside the window is NaN so that any read from there shows).  Returns the window of
    the remapped field."""
    import torch

    from pace_amd.fv3core.stencils.map_single import MapSingle

    kord, iv, src, dst, qs, qmin = REMAP_CASES[name]
    ustag = name.startswith("u_")
    dims = ["x", "y_interface" if ustag else "y", "z"]
    nj = n + 1 if ustag else n

    def embed(a):
        full = np.full((n + 7, n + 7, REMAP_KM + 1), np.nan)
        full[3:3 + n, 3:3 + nj, :] = a
        return env.q3(full)

    q, p1, p2 = embed(d[name + "_in"]), embed(d[src]), embed(d[dst])
    qsq = None
    if qs is not None:
        full = np.full((n + 7, n + 7), np.nan)
        full[3:3 + n, 3:3 + n] = d[qs]
        qsq = env.q2(full)
    op = MapSingle(env.stencil_factory, env.qf, kord, iv, dims)
    op(q, p1, p2, qs=qsq, qmin=qmin)
    if env.qf.device.type == "cuda":
        torch.cuda.synchronize()
    return q.numpy()[3:3 + n, 3:3 + nj, :REMAP_KM]


def run_mapn_tracer(env, d, kord, nq=7, fill=True, n=12):
    """MapNTracer (+ fillz) through the host classes on tracers made from the fixture's fields (one of them with negative
    values so that fillz acts), and the same through the oracle.  Returns (got, expected): lists of window arrays."""
    import torch

    from oracle import remapping
    from pace_amd.fv3core.stencils.fillz import tracer_variables
    from pace_amd.fv3core.stencils.mapn_tracer import MapNTracer

    km = REMAP_KM

    def embed(a):
        full = np.full((n + 7, n + 7, km + 1), np.nan)
        full[3:3 + n, 3:3 + n, :] = a
        return env.q3(full)

    base = [d["qv_k9_iv0_in"], d["fillz0_in"], d["fillz1_in"], d["pt_k9_iv1_in"] * 1e-3, d["qv_k9_iv0_in"] * 0.5 + 1e-4,
            d["fillz2_in"] * 0.1, d["w_k9_ivm2_in"], d["qv_k9_iv0_in"] * 2.0][:nq]
    names = tracer_variables[:nq]
    tracers = {nm: embed(a) for nm, a in zip(names, base)}
    pe1, pe2 = d["pe1s"], d["pe2"]
    dp2 = np.zeros_like(pe2)
    dp2[:, :, :km] = pe2[:, :, 1:] - pe2[:, :, :-1]
    op = MapNTracer(env.stencil_factory, env.qf, kord, nq, fill, tracers)
    op(embed(pe1), embed(pe2), embed(dp2), tracers)
    if env.qf.device.type == "cuda":
        torch.cuda.synchronize()
    got = [tracers[nm].numpy()[3:3 + n, 3:3 + n, :km] for nm in names]
    exp = []
    for t, a in enumerate(base):
        q = a.copy()
        remapping.map_single(q, pe1, pe2, km, 9 if t == 5 else kord, 0)
        if fill:
            remapping.fillz(q, dp2, km)
        exp.append(q[:, :, :km])
    return got, exp


L2E_OUT3 = ("pt", "delp", "delz", "peln", "u", "v", "w", "q_con", "pkz", "pk", "pe", "cappa")


def l2e_k10_fixture():
    """l2e_c12.npz with the inputs / outputs of the reference's run with every remapping order 10 merged over it
    (tools/make_golden_l2e.py kord10: negatives in four condensates)."""
    d = golden("l2e_c12.npz")
    d.update(golden("l2e_k10_c12.npz"))
    return d


def run_l2e(env, d, last_step, n=12, km=79, kord=9):
    """LagrangianToEulerian through the host class on the reference-run fixture (tests/golden/l2e_c12.npz; its arrays are
    the [2:16, 2:16] window of the 19 x 19 storage).  Returns dict name -> full numpy array."""
    import torch

    from pace_amd.fv3core import RemappingConfig
    from pace_amd.fv3core.stencils.remapping import LagrangianToEulerian
    from pace_amd.util import constants as c

    def embed(a):
        if a.ndim == 3:
            full = np.full((n + 7, n + 7, km + 1), np.nan)
            full[2:16, 2:16, :] = a
            return env.q3(full)
        full = np.full((n + 7, n + 7), np.nan)
        full[2:16, 2:16] = a
        return env.q2(full)

    f = {k[3:]: embed(d[k]) for k in d if k.startswith("in_") and not k.startswith("in_tr_")}
    tracers = {k[6:]: embed(d[k]) for k in d if k.startswith("in_tr_")}
    ak, bk = env.kq(d["ak"]), env.kq(d["bk"])
    op = LagrangianToEulerian(env.stencil_factory, env.qf,
                              RemappingConfig(kord_tm=-kord, kord_tr=kord, kord_wz=kord, kord_mt=kord), None, 8, None, tracers)
    op(tracers, f["pt"], f["delp"], f["delz"], f["peln"], f["u"], f["v"], f["w"], f["cappa"], f["q_con"], f["qcld"], f["pkz"],
       f["pk"], f["pe"], f["phis"], f["ps"], f["wsd"], ak, bk, None, float(d["ptop"]), c.KAPPA, c.ZVIR, last_step, 0.0, 112.5)
    if env.qf.device.type == "cuda":
        torch.cuda.synchronize()
    out = {k: v.numpy() for k, v in f.items()}
    out.update({"tr_" + k: v.numpy() for k, v in tracers.items()})
    return out


def check_l2e(out, d, last_step, tol, n=12, km=79, loose=None):
    """Compare with the fixture on the windows the reference writes; returns the worst metric per variable."""
    cw = (slice(3, 3 + n), slice(3, 3 + n))
    worst = {}

    def ref_full(a):
        full = np.full((n + 7, n + 7) + a.shape[2:], np.nan)
        full[2:16, 2:16] = a
        return full

    if last_step:
        e = compare(ref_full(d["out_last_pt"])[cw][:, :, :km], out["pt"][cw][:, :, :km])
        assert e < tol, ("pt(last)", e)
        return {"pt(last)": e}
    for key in d:
        if not key.startswith("out_") or key == "out_last_pt":
            continue
        name = key[4:]
        ref = ref_full(d[key])
        win = {"u": (slice(3, 3 + n), slice(3, 4 + n)), "v": (slice(3, 4 + n), slice(3, 3 + n))}.get(name, cw)
        if ref.ndim == 2:
            e = compare(ref[cw], out[name][cw])
        else:
            kk = km + 1 if name in ("pe", "peln", "pk") else km
            e = compare(ref[win][:, :, :kk], out[name][win][:, :, :kk], near_zero=1e-18)
        worst[name] = e
        assert e < (loose or {}).get(name, tol), (name, e)
    return worst


# ------------------------------------------------------------------------------------------------------------------
# DynamicalCore.step_dynamics on six tiles (tests/golden/dycore_c12_tile*.npz, tools/make_golden_dycore.py)
# ------------------------------------------------------------------------------------------------------------------
DYCORE_TRACERS = "qvapor qliquid qrain qice qsnow qgraupel qo3mr qsgs_tke qcld".split()
DYCORE_OUT = "u v w delz delp pt pe pk peln pkz q_con omga ua va mfxd mfyd cxd cyd".split() + DYCORE_TRACERS


def dycore_condensates(tile, shape):
    """The deterministic content the fixture generator gives the species the test case leaves at zero (the same function
    as tools/make_golden_dycore.py:condensates -- the generator asserts that its inputs equal it)."""
    i, j, k = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), np.arange(shape[2]), indexing="ij")
    base = 0.5 + 0.5 * np.sin(0.7 * i + 1.3 * j + 0.37 * k + tile)
    out = {}
    for n, (name, scale) in enumerate((("qliquid", 2e-4), ("qrain", 1e-4), ("qice", 5e-5), ("qsnow", 3e-5), ("qgraupel", 2e-5),
                                       ("qo3mr", 1e-6), ("qsgs_tke", 1e-2), ("qcld", 0.3))):
        f = scale * (0.2 + base * (0.5 + 0.5 * np.cos(0.9 * i - 0.4 * j + 0.11 * k + n)))
        neg = ((3 * i + 5 * j + 7 * k + n + tile) % 23) == 0
        if name not in ("qo3mr", "qsgs_tke"):
            f = np.where(neg, -0.3 * f, f)
        out[name] = f
    return out


def generated_inputs(n, nz):
    """Per tile (metrics, state arrays) from pace_amd's OWN grid and initial-state generators -- nothing reference-derived."""
    from pace_amd.fv3core.initialization.baroclinic import baroclinic_state_six_tiles
    from pace_amd.util import gridgen

    tiles = gridgen.tiles(n, nz)
    states = baroclinic_state_six_tiles(tiles, n, nz)
    out = []
    for t in range(6):
        m = {k: v for k, v in tiles[t].items() if k not in ("ee1", "ee2", "es1", "ew2")}
        s = {k: states[t][k] for k in "u v w delz delp pe pk peln phis uc vc ua va pt qvapor ps".split()}
        out.append((m, s))
    return out


def run_dycore_tile(comm, lib, device, fix_ac, fix_dy, n, nz, checkpointer=None, generated=None):
    """One tile's program: state = the acoustic fixture's inputs (identical to the dycore run's, as the generator asserts)
    with the temperature before the preamble, the vapour and the regenerated condensates; one step_dynamics."""
    import datetime

    import torch

    from pace_amd.fv3core import DynamicalCoreConfig
    from pace_amd.fv3core.initialization.dycore_state import DycoreState
    from pace_amd.fv3core.stencils.fv_dynamics import DynamicalCore
    from pace_amd.util import CubedSphereCommunicator

    tile = comm.Get_rank()
    if generated is not None and generated[tile][1] is not None:
        metrics, arrays = generated[tile]
        arrays = {k: v.copy() for k, v in arrays.items()}
        shape = arrays["delp"].shape
    else:
        metrics = {k[5:]: v for k, v in fix_ac.items() if k.startswith("grid_")}
        if generated is not None:
            metrics = generated[tile][0]
        arrays = {k: fix_ac["in_" + k] for k in "u v w delz delp pe pk peln phis uc vc ua va".split()}
        shape = arrays["delp"].shape
        pt = np.zeros(shape)
        pt[3:3 + n, 3:3 + n, :] = fix_dy["in_pt"]
        qv = np.zeros(shape)
        qv[3:3 + n, 3:3 + n, :] = fix_dy["in_qvapor"]
        arrays.update(pt=pt, qvapor=qv, ps=fix_dy["in_ps"])
    env = Env(lib, device, metrics, n, nz)
    cube = CubedSphereCommunicator(comm, device=device, lib=lib)
    for name, f in dycore_condensates(tile, shape).items():
        arrays[name] = f * (arrays["delp"] > 0)
    state = DycoreState.init_from_numpy_arrays(arrays, env.qf)
    n_split = int(fix_dy["n_split"])
    k_split = int(fix_dy["k_split"]) if "k_split" in fix_dy else 1
    ac = acoustic_config(n_split)
    ac.k_split = k_split
    kord = int(fix_dy["kord"]) if "kord" in fix_dy else 9  # (dycore_kord10_c12_*: every remapping order 10)
    config = DynamicalCoreConfig(npx=n + 1, npy=n + 1, npz=nz, dt_atmos=float(fix_dy["timestep"]), k_split=k_split,
                                 n_split=n_split, acoustic_dynamics=ac, kord_tm=-kord, kord_tr=kord, kord_wz=kord, kord_mt=kord)
    core = DynamicalCore(cube, env.grid_data, env.stencil_factory, env.qf, env.damping, config, state.phis, state,
                         datetime.timedelta(seconds=float(fix_dy["timestep"])), checkpointer=checkpointer)
    core.step_dynamics(state)
    if env.qf.device.type == "cuda":
        torch.cuda.synchronize()
    out = {k: getattr(state, k).numpy() for k in DYCORE_OUT}
    out["ps"] = state.ps.numpy()
    return out


def run_dycore_six_tiles(lib, device, n=12, nz=79, checkpointers=None, prefix="dycore_c12", generated=False):
    from pace_amd.util import run_tiles

    fa = [golden(f"acoustic_c12_tile{t}.npz") for t in range(6)]
    fd = [golden(f"{prefix}_tile{t}.npz") for t in range(6)]
    if prefix == "dycore_c12":  # tiles 0 and 2 also have FULL output fields of nine state variables (a later addition)
        full = golden("dycore_c12_full.npz")
        for t in full["tiles"]:
            for k in full:
                if k.endswith(f"_tile{t}"):
                    fd[int(t)]["full_" + k[4:-6]] = full[k]
    cps = checkpointers or [None] * 6
    gen = generated_inputs(n, nz) if generated else None
    if generated == "metrics":  # pace_amd's grid generator, the reference run's initial state
        gen = [(m, None) for m, _ in gen]
    return fd, run_tiles(6, lambda comm: run_dycore_tile(comm, lib, device, fa[comm.Get_rank()], fd[comm.Get_rank()], n, nz,
                                                         cps[comm.Get_rank()], generated=gen))


def dycore_errors(fix, out, n=12):
    """max reference-metric error per variable on the fixture's level subset and full columns."""
    errs = {}
    ks = fix["k_sel"]
    for k in DYCORE_OUT:
        full = out[k]
        di = 1 if k in ("v", "mfxd", "cxd") else 0
        dj = 1 if k in ("u", "mfyd", "cyd") else 0
        nk = 80 if k in ("pe", "pk", "peln") else 79
        kk = [x for x in ks if x < nk]
        idx = [list(ks).index(x) for x in kk]
        got = full[3:3 + n + di, 3:3 + n + dj][:, :, kk]
        ref = fix["out_" + k][:n + di, :n + dj][:, :, idx]
        band = _BANDS.get(k, 1e-12)
        near_zero = band * float(np.abs(ref).max()) + 1e-300
        e = compare(ref, got, near_zero=near_zero)
        cols = np.stack([full[i, j, :nk] for (i, j) in fix["cols"]])
        e = max(e, compare(fix["col_" + k][:, :nk], cols, near_zero=near_zero))
        if "full_" + k in fix:  # the whole field, all levels
            e = max(e, compare(fix["full_" + k][:n + di, :n + dj, :nk], full[3:3 + n + di, 3:3 + n + dj, :nk], near_zero=near_zero))
        errs[k] = e
    errs["ps"] = compare(fix["out_ps"][:n, :n], out["ps"][3:3 + n, 3:3 + n])
    return errs


# (measured on the GPU, profiles/r02_dycore_c12_gpu_errors.json: pressures 1e-15, delp / pt / pkz / tracers <= 1.5e-13, delz 4e-13,
# accumulators 5e-10, u / v / va 1e-8, w 3e-7, omga 8e-7; default bound of check_dycore for everything not listed: 1e-9 -> 1e-11)
DYCORE_TOL = {"w": 2e-6, "omga": 2e-6, "u": 1e-6, "v": 1e-6, "ua": 1e-6, "va": 1e-6, "delz": 1e-10, "mfxd": 1e-7, "mfyd": 1e-7,
              "cxd": 1e-7, "cyd": 1e-7}


def check_dycore(fixes, outs, default=1e-11):
    """Tolerances: the acoustic loop's (2e-6 = the reference's own DynCore bound, translate_dyncore.py:120, see ACOUSTIC_TOL)
    carried through tracer advection, remapping (reference bound 2e-8) and the
    final adjustments; `default` for everything else (masses, temperatures, tracers, pressures): 1e-11 after one remapping step
    (measured <= 1.5e-13), 1e-9 for the k_split = 2 run (two remapping steps: the condensates reach 3e-10)."""
    worst = {}
    for t in range(6):
        for k, e in dycore_errors(fixes[t], outs[t]).items():
            worst[k] = max(worst.get(k, 0.0), e)
    for k, e in worst.items():
        assert e < DYCORE_TOL.get(k, default), (k, e)
    return worst


# Envelope of the fully generated run (tools/wind_noise_sensitivity.py): one step of the REFERENCE ALGORITHM (the oracle)
# moves by u, v 1.8e-4, w 6e-6, ua / va 1.4e-6, delp 6e-9 of the field's magnitude when 1e-13 m/s of noise is added to the
# winds of this zonal-flow state (upwind / limiter branches decided by wind components that are zero by symmetry); the
# generated winds differ from the reference's by up to 3e-13 m/s, so that is the accuracy an end-to-end comparison can have.
GENERATED_TOL = {"u": 1e-3, "v": 1e-3, "va": 1e-3, "ua": 1e-5, "w": 5e-5, "omga": 5e-5, "mfxd": 5e-6, "mfyd": 5e-6,
                 "cxd": 5e-6, "cyd": 5e-6}


# One whole step with every remapping order 10: the kord 10 limiter is discontinuous in its inputs -- the reference algorithm
# (oracle, bit-identical to the reference's LagrangianToEulerian on the same inputs) turns 1e-13 of input noise into 2e-6 (v),
# 1e-5 (w), 6e-7 (pt), 2e-4 (condensates) of each field's magnitude, where kord 9 leaves 1e-13 -- and its inputs here come out
# of the acoustic loop, whose vertical solver carries the device's exp / log.  Hence scaled-error bounds:
KORD10_TOL = {"u": 1e-4, "v": 1e-4, "ua": 1e-4, "va": 1e-4, "w": 1e-4, "omga": 1e-4, "pt": 1e-6, "pkz": 1e-6, "q_con": 1e-3,
              "qliquid": 1e-3, "qrain": 1e-3, "qice": 1e-3, "qsnow": 1e-3, "qsgs_tke": 1e-8}


def check_dycore_kord10(fixes, outs):
    worst = dycore_scaled_errors(fixes, outs)
    for k, e in worst.items():
        assert e < KORD10_TOL.get(k, 1e-10), (k, e)
    return worst


def check_dycore_generated(fixes, outs):
    worst = dycore_scaled_errors(fixes, outs)
    for k, e in worst.items():
        assert e < GENERATED_TOL.get(k, 5e-7), (k, e)
    return worst


def dycore_scaled_errors(fixes, outs, n=12):
    """max |got - ref| / max |ref| per variable over the six tiles (fixture's level subset)."""
    worst = {}
    for fix, out in zip(fixes, outs):
        ks = fix["k_sel"]
        for k in DYCORE_OUT:
            di = 1 if k in ("v", "mfxd", "cxd") else 0
            dj = 1 if k in ("u", "mfyd", "cyd") else 0
            nk = 80 if k in ("pe", "pk", "peln") else 79
            kk = [x for x in ks if x < nk]
            idx = [list(ks).index(x) for x in kk]
            got = out[k][3:3 + n + di, 3:3 + n + dj][:, :, kk]
            ref = fix["out_" + k][:n + di, :n + dj][:, :, idx]
            e = float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-300))
            worst[k] = max(worst.get(k, 0.0), e)
    return worst


def l2e_synthetic_case(n, km, seed=2):
    """Inputs of LagrangianToEulerian at any size: the synthetic balanced state with its Lagrangian surfaces deformed by a
    few per cent of a layer ... two layers (column by column; with fewer than 17 levels: 0.12 of the column), vapour + the
    deterministic condensates.  Returns
    (fields, tracers, ak, bk, ptop) as full numpy arrays."""
    from pace_amd import synthetic

    m = synthetic.tile_metrics(n, km)
    s = synthetic.acoustic_state(m, n, km)
    rng = np.random.default_rng(seed)
    ni = n + 7
    ak, bk = m["ak"], m["bk"]
    ptop = float(ak[0])
    # deform: redistribute the layer thicknesses, keep the column mass
    sig = np.linspace(0.0, 1.0, km + 1)
    # (at most 0.12 of the column: below 17 levels two layers of displacement would fold the column -- negative delp, which
    # the operator is not defined for and which comes out as NaN on both sides of a comparison)
    amp = min(2.0 / km, 0.12) * rng.random((ni, ni))
    pe_e = s["pe"]
    ps = pe_e[:, :, km]
    frac = (pe_e - ptop) / (ps - ptop)[:, :, None]
    frac = frac + amp[:, :, None] * np.sin(2.0 * np.pi * sig)[None, None, :] * frac * (1.0 - frac) * 4.0
    frac[:, :, 0], frac[:, :, km] = 0.0, 1.0
    pe = ptop + (ps - ptop)[:, :, None] * frac
    f = {}
    f["pe"] = pe
    f["peln"] = np.log(pe)
    delp = np.zeros_like(pe)
    delp[:, :, :km] = pe[:, :, 1:] - pe[:, :, :-1]
    f["delp"] = delp
    for k in ("pt", "delz", "u", "v", "w"):
        f[k] = s[k].copy()
    f["pt"][:, :, :km] = s["pt"][:, :, :km] * 300.0  # a temperature-like magnitude (the operator takes logs of it)
    for k in ("cappa", "q_con", "pkz", "pk", "qcld"):
        f[k] = np.zeros_like(pe)
    f["pk"][:, :, km] = np.exp(0.2857 * np.log(pe[:, :, km]))
    f["ps"] = np.zeros((ni, ni))
    f["wsd"] = 0.01 * rng.standard_normal((ni, ni))
    f["phis"] = np.zeros((ni, ni))
    tracers = {"qvapor": 0.01 * np.exp(-4.0 * (1.0 - frac[:, :, :1] * 0 - np.minimum(frac, 1.0))) * (1 + 0.2 * rng.random(pe.shape))}
    tracers.update({k: v for k, v in dycore_condensates(0, pe.shape).items() if k != "qcld"})
    return f, tracers, ak, bk, ptop


DSW_VARIANTS = {  # tools/make_golden_dsw_variants.py: runs of the reference with one namelist option changed
    "h5": dict(hord_dp=5, hord_tm=5, hord_vt=5, hord_mt=5),
    "nord2": dict(nord=2),
    "dcon0": dict(d_con=0.0),
    "skeb": dict(do_skeb=True),
    "dddmp0": dict(dddmp=0.0),
}


def dsw_variant_fixture(variant):
    fix = golden(f"d_sw_{variant}_c12_tile0_call1.npz")
    k_sel = fix["k_sel"]
    cfg = dict(DSW_CFG, **DSW_VARIANTS[variant])
    col = {k[4:]: np.ascontiguousarray(v[np.asarray(k_sel)]) for k, v in fix.items() if k.startswith("col_")}
    return fix, cfg, col, len(k_sel)


def run_d_sw_variant_fixture(env, variant):
    """A run of the reference with one namelist option changed, through the host class; returns {field: error}."""
    fix, cfg, col, nk = dsw_variant_fixture(variant)
    out, _ = run_d_sw(env, col, {k: fix["in_" + k] for k in DSW_ARGS}, float(fix["dt"]), ut0=fix["in_uc_contra"],
                      vt0=fix["in_vc_contra"], cfg=cfg)
    return {k: compare(fix["out_" + k][dsw_window(k, 12, nk)], out[k][dsw_window(k, 12, nk)]) for k in DSW_ARGS if k != "zh"}


def run_d_sw_h5_fixture(env):
    return max(run_d_sw_variant_fixture(env, "h5").values())


# ------------------------------------------------------------------------------------------------------------------
# CubedToLatLon, the preamble kernels and the ord-8 transport at any size (tests/test_emu_kernels.py, tests/test_gpu_parity.py,
# tests/test_vertical_edges.py)
# ------------------------------------------------------------------------------------------------------------------
def check_c2l_and_preamble(lib, device, n, nz, order, storage=None):
    """pace_c2l_ord (order 2 or 4) and, with order 2, pace_fv_setup_pt and pace_omega_from_w on a synthetic C<n> tile with nz
    levels against oracle/dycore_parts.py: the wind transform bit for bit (order 2: compute + 1, order 4: compute), q_con,
    cappa, dp1 and omga bit for bit, pkz and pt within 1e-14 (exp / log).  Returns {"pkz": error, "pt": error} (order 2).

    storage="f32" (a float32-storage library): metrics and inputs are float32 values and the reference is float32(oracle) of them.
    Every kernel here is one pass from its loads to its stores, so ua, va, q_con, cappa, dp1 and omga are in the exact class of
    tests/test_f32_operators.py; pkz and pt (exp, log) in the last-place class: within 1 float32 ulp, at most 1e-4 of the
    window different at all.  Returns {"pkz": number of elements that differ, "pt": the same}."""
    import ctypes as C

    from oracle import dycore_parts
    from pace_amd import synthetic
    from pace_amd.fv3core.stencils._common import dptr
    from pace_amd.fv3core.stencils.fillz import pointer_table
    from pace_amd.util.grid import geom_struct

    assert storage in (None, "f32") and lib.real_bytes == (4 if storage else 8)

    def sync():
        if device != "cpu":
            import torch

            torch.cuda.synchronize()

    def rnd(a):
        """what a `real` field holds of `a`, as float64"""
        from opchain import f32

        return f32(a) if storage else a

    def differ(name, got, ref):
        """None if `got` is the reference as stored, bit for bit; else what differs"""
        ref = ref.astype(np.float32) if storage else ref
        if got.dtype == ref.dtype and np.array_equal(got, ref):
            return None
        worst = f", by up to {np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32)).max()} ulp" if storage else ""
        return f"{name}: {int((got != ref).sum())} of {ref.size} differ{worst}"

    def last_place(name, got, ref):
        if not storage:
            e = compare(ref, got)
            assert e < 1e-14, (name, e)
            return e
        r32 = ref.astype(np.float32)
        for moved in (np.nextafter(ref, np.inf), np.nextafter(ref, -np.inf)):  # (the shape itself stays inside the class's share
            assert (moved.astype(np.float32) != r32).sum() <= 1e-4 * ref.size, name  # under one float64 ulp of numpy's exp / log)
        u = np.abs(got.view(np.int32).astype(np.int64) - r32.view(np.int32).astype(np.int64))  # (positive values: ordered like integers)
        assert (got > 0).all() and (r32 > 0).all() and u.max() <= 1 and (u != 0).sum() <= 1e-4 * u.size, (name, int(u.max()), int((u != 0).sum()), u.size)
        return int((u != 0).sum())

    metrics = synthetic.tile_metrics(n, nz)
    s = synthetic.acoustic_state(metrics, n, nz)
    if storage:
        metrics = {k: (rnd(v) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v) for k, v in metrics.items()}
        s = {k: (rnd(v) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else v) for k, v in s.items()}
    env = Env(lib, device, metrics, n, nz)
    geom = geom_struct(env.qf)
    gd = env.grid_data
    u, v, ua, va = env.q3(s["u"]), env.q3(s["v"]), env.q3(), env.q3()
    lib.call("pace_c2l_ord", C.byref(geom), C.byref(gd.c_struct()), order, dptr(u), dptr(v), dptr(gd.a11), dptr(gd.a12),
             dptr(gd.a21), dptr(gd.a22), dptr(ua), dptr(va), None)
    sync()
    fn = dycore_parts.c2l_ord2 if order == 2 else dycore_parts.c2l_ord4
    rua, rva = fn(s["u"], s["v"], metrics["dx"], metrics["dy"], metrics["a11"], metrics["a12"], metrics["a21"], metrics["a22"], n, nz)
    h = 1 if order == 2 else 0
    w = (slice(3 - h, 3 + n + h), slice(3 - h, 3 + n + h), slice(0, nz))
    wrong = [d for d in (differ("ua", ua.numpy()[w], rua[w]), differ("va", va.numpy()[w], rva[w])) if d]
    assert not wrong, wrong
    if order == 4:
        return {}
    # compute_preamble + omega
    cond = dycore_condensates(0, s["delp"].shape)
    t = {k: rnd(np.abs(cond[k])) for k in ("qliquid", "qrain", "qice", "qsnow", "qgraupel")}
    t["qvapor"] = rnd(0.01 * np.ones_like(s["delp"]))
    qt = {k: env.q3(a) for k, a in t.items()}
    pt0 = rnd(s["pt"] * 300.0)
    f = {k: env.q3(a) for k, a in (("pt", pt0), ("delp", s["delp"]), ("delz", s["delz"]), ("w", s["w"]))}
    q_con, pkz, cappa, dp1, omga = env.q3(), env.q3(), env.q3(), env.q3(), env.q3()
    water = pointer_table([qt[k] for k in ("qvapor", "qliquid", "qrain", "qsnow", "qice", "qgraupel")])
    lib.call("pace_fv_setup_pt", C.byref(geom), water, dptr(q_con), dptr(pkz), dptr(f["pt"]), dptr(cappa), dptr(f["delp"]),
             dptr(f["delz"]), dptr(dp1), None)
    lib.call("pace_omega_from_w", C.byref(geom), dptr(f["delp"]), dptr(f["delz"]), dptr(f["w"]), dptr(omga), None)
    sync()
    cw = (slice(3, 3 + n), slice(3, 3 + n), slice(0, nz))
    tw = {k: a[cw] for k, a in t.items()}
    gz, _, rpkz, rcappa, rdp1 = dycore_parts.fv_setup(tw, pt0[cw], s["delp"][cw], s["delz"][cw])
    wrong = [differ(k, got.numpy()[cw], ref) for k, got, ref in (("q_con", q_con, gz), ("cappa", cappa, rcappa), ("dp1", dp1, rdp1),
                                                                  ("omga", omga, s["delp"][cw] / s["delz"][cw] * s["w"][cw]))]
    assert not any(wrong), [d for d in wrong if d]
    errs = {"pkz": last_place("pkz", pkz.numpy()[cw], rpkz)}
    rpt = pt0[cw] * (1.0 + rdp1) * (1.0 - gz) / rpkz
    errs["pt"] = last_place("pt", f["pt"].numpy()[cw], rpt)
    from oracle import constants as oc

    assert oc.ZVIR > 0
    return errs


def check_ord8_transport(lib, device, n, nz, storage=None):
    """Monotone (ord 8) PPM transport of the synthetic state's pt on a C<n> tile with nz levels, with the oracle's own flux
    preparation, against oracle/ppm_transport.py: both fluxes bit for bit.

    storage="f32" (a float32-storage library): metrics, Courant numbers, area fluxes and pt are float32 values, and both fluxes
    equal float32(oracle) bit for bit -- without mass fluxes k_fvtp2d keeps the inner fluxes and the advected intermediates in
    LDS as double, so nothing lies between the loads and the two stores.  Returns {flux: number of elements compared}."""
    from oracle import dgrid_sw
    from oracle import ppm_transport as tr
    from pace_amd import synthetic
    from pace_amd.fv3core.stencils.fvtp2d import FiniteVolumeTransport

    assert storage in (None, "f32") and lib.real_bytes == (4 if storage else 8)
    metrics = synthetic.tile_metrics(n, nz)
    s = synthetic.acoustic_state(metrics, n, nz)
    if storage:
        from opchain import f32_dict as rnd

        metrics, s = rnd(metrics), rnd(s)
    g = oracle_grid(metrics, n, nz)
    for k in ("crx", "cry", "xfx", "yfx"):
        s[k] = np.zeros_like(s["pt"])
    dgrid_sw.fxadv(g, s["uc"], s["vc"], s["crx"], s["cry"], s["xfx"], s["yfx"], np.zeros_like(s["pt"]), np.zeros_like(s["pt"]), s["dt"])
    if storage:
        s = rnd(s)
    env = Env(lib, device, metrics, n, nz)
    op = FiniteVolumeTransport(env.stencil_factory, env.qf, env.grid_data, env.damping, 0, 8)
    f = {k: env.q3(s[k]) for k in ("pt", "crx", "cry", "xfx", "yfx")}
    fx, fy = env.q3(), env.q3()
    op(f["pt"], f["crx"], f["cry"], f["xfx"], f["yfx"], fx, fy)
    if device != "cpu":
        import torch

        torch.cuda.synchronize()
    ofx, ofy = np.zeros_like(s["pt"]), np.zeros_like(s["pt"])
    tr.fvtp2d(g, s["pt"].copy(), s["crx"], s["cry"], s["xfx"], s["yfx"], ofx, ofy, 8)
    if storage:
        ofx, ofy = ofx.astype(np.float32), ofy.astype(np.float32)
    wx, wy = window(n, 1, 0, nz), window(n, 0, 1, nz)
    gx, gy = fx.numpy(), fy.numpy()
    assert gx.dtype == ofx.dtype
    bad = {k: int((a != b).sum()) for k, a, b in (("fx", ofx[wx], gx[wx]), ("fy", ofy[wy], gy[wy])) if not np.array_equal(a, b)}
    assert not bad, bad
    return {"fx": int(ofx[wx].size), "fy": int(ofy[wy].size)}


def check_l2e_kernels(lib, device, n, km, storage=None):
    """The four kernels of k_l2e.hip one by one through their C entry points (pace_l2e_prepare, pace_l2e_post, pace_l2e_pressures
    in both directions, pace_l2e_finish as the last step and not) on l2e_synthetic_case, against the statements of
    oracle/remapping.lagrangian_to_eulerian that each of them restates, evaluated in float64 on what the fields hold.  Every
    kernel is one pass from its loads to its stores, so with either storage type every output without exp / log equals the
    reference as stored, bit for bit (storage="f32": float32(reference of float32 inputs)); pt, pn2, pk of the prepare kernel and
    pkz of the post kernel (exp, log) are within 1e-14 (float64) or within 1 float32 ulp with at most 1e-4 of the window
    different at all (float32: the last-place class of tests/test_f32_operators.py).  Returns {output: what was measured}."""
    import ctypes as C

    from oracle import constants as oc
    from oracle.remapping import _moist_cvm_gz
    from pace_amd import synthetic
    from pace_amd.fv3core.stencils._common import dptr
    from pace_amd.fv3core.stencils.fillz import pointer_table
    from pace_amd.util.grid import geom_struct

    assert storage in (None, "f32") and lib.real_bytes == (4 if storage else 8)
    real = np.float32 if storage else np.float64

    def rnd(a):
        from opchain import f32

        return f32(a) if storage else a

    def sync():
        if device != "cpu":
            import torch

            torch.cuda.synchronize()

    f, tr, ak, bk, _ = l2e_synthetic_case(n, km)
    f, tr, ak, bk = {k: rnd(v) for k, v in f.items()}, {k: rnd(v) for k, v in tr.items()}, rnd(ak), rnd(bk)
    ptop = float(ak[0])
    env = Env(lib, device, synthetic.tile_metrics(n, km), n, km)
    geom_s = geom_struct(env.qf)
    geom = C.byref(geom_s)
    akq, bkq = env.kq(ak), env.kq(bk)  # (held: a pointer taken from a temporary outlives it)
    report, wrong = {}, []
    K, KK = slice(0, km), slice(0, km + 1)
    cw, cj, ci = (slice(3, 3 + n), slice(3, 3 + n)), (slice(3, 3 + n), slice(3, 4 + n)), (slice(3, 4 + n), slice(3, 3 + n))

    def exact(name, got, ref):
        got, ref = got.numpy(), ref.astype(real)
        assert got.dtype == real and np.isfinite(ref).all(), name
        report[name] = int((got != ref).sum())
        if report[name]:
            wrong.append(f"{name}: {report[name]} of {ref.size} differ")

    def last_place(name, got, ref):
        got = got.numpy()
        assert got.dtype == real and np.isfinite(ref).all(), name
        if not storage:
            report[name] = compare(ref, got)
            if not report[name] < 1e-14:
                wrong.append(f"{name}: {report[name]:.1e}")
            return
        r32 = ref.astype(np.float32)
        u = np.abs(got.view(np.int32).astype(np.int64) - r32.view(np.int32).astype(np.int64))  # (one sign throughout)
        assert (np.sign(got) == np.sign(r32)).all(), name
        report[name] = int((u != 0).sum())
        if u.max() > 1 or report[name] > 1e-4 * u.size:
            wrong.append(f"{name}: {report[name]} of {u.size} differ, by up to {int(u.max())} ulp")

    class View:  # a window of a field, with the numpy() of a Quantity
        def __init__(self, q, w):
            self.q, self.w = q, w

        def numpy(self):
            return self.q.numpy()[self.w]

    def water(qt):
        return pointer_table([qt[k] for k in ("qvapor", "qliquid", "qrain", "qsnow", "qice", "qgraupel")])

    def moist(t, w):
        cvm, gz = _moist_cvm_gz({k: v[w] for k, v in t.items()})
        return gz, oc.RDGAS / (oc.RDGAS + cvm / (1.0 + oc.ZVIR * t["qvapor"][w]))

    # ---- k_l2e_prepare ----
    qt = {k: env.q3(v) for k, v in tr.items()}
    q = {k: env.q3(f[k]) for k in ("pt", "delp", "delz", "pe", "peln", "pk")}
    o = {k: env.q3() for k in ("q_con", "cappa", "pe1", "pe2", "dp2", "pn2")}
    ps = env.q2()
    lib.call("pace_l2e_prepare", geom, water(qt), dptr(o["q_con"]), dptr(q["pt"]), dptr(o["cappa"]), dptr(q["delp"]), dptr(q["delz"]),
             dptr(q["pe"]), dptr(o["pe1"]), dptr(o["pe2"]), dptr(akq), dptr(bkq), dptr(o["dp2"]), dptr(ps), dptr(o["pn2"]),
             dptr(q["peln"]), dptr(q["pk"]), ptop, oc.KAPPA, oc.ZVIR, None)
    sync()
    c3 = cw + (K,)
    gz, cappa = moist(tr, c3)
    psr = f["pe"][cw + (km,)]
    e = np.stack([np.full(psr.shape, ptop) if k == 0 else (psr if k == km else ak[k] + bk[k] * psr) for k in range(km + 1)], axis=2)
    exact("prepare.q_con", View(o["q_con"], c3), gz)
    exact("prepare.cappa", View(o["cappa"], c3), cappa)
    exact("prepare.delz", View(q["delz"], c3), -f["delz"][c3] / f["delp"][c3])
    exact("prepare.pe1", View(o["pe1"], cj + (KK,)), f["pe"][cj + (KK,)])
    exact("prepare.pe2", View(o["pe2"], cw + (KK,)), e)
    exact("prepare.pe2.extra_row", View(o["pe2"], (cj[0], slice(3 + n, 4 + n), slice(km, km + 1))), f["pe"][cj[0], 3 + n:4 + n, km:km + 1])
    exact("prepare.dp2", View(o["dp2"], c3), e[:, :, 1:] - e[:, :, :-1])
    exact("prepare.delp", View(q["delp"], c3), e[:, :, 1:] - e[:, :, :-1])
    exact("prepare.ps", View(ps, cw), psr)
    exact("prepare.pn2.bottom", View(o["pn2"], cw + (slice(km, km + 1),)), f["peln"][cw + (slice(km, km + 1),)])
    p = f["pt"][c3]
    last_place("prepare.pt", View(q["pt"], c3), p * np.exp(cappa / (1.0 - cappa) * np.log(oc.RDG * f["delp"][c3] / f["delz"][c3] * p)))
    last_place("prepare.pn2", View(o["pn2"], c3), np.log(e[:, :, :km]))
    last_place("prepare.pk", View(q["pk"], c3), np.exp(oc.KAPPA * np.log(e[:, :, :km])))
    # ---- k_l2e_post (delz: the adjusted one, -delz / delp) ----
    dz_in = rnd(-f["delz"] / np.where(f["delp"] != 0.0, f["delp"], 1.0))
    pn2_in = rnd(f["peln"] + 1.0e-3)
    q = {k: env.q3(v) for k, v in (("pt", f["pt"]), ("delp", f["delp"]), ("delz", dz_in), ("peln", f["peln"]), ("pn2", pn2_in))}
    o = {k: env.q3() for k in ("q_con", "cappa", "pkz", "pe0")}
    lib.call("pace_l2e_post", geom, water(qt), dptr(o["q_con"]), dptr(o["pkz"]), dptr(q["pt"]), dptr(o["cappa"]), dptr(q["delp"]),
             dptr(q["delz"]), dptr(q["peln"]), dptr(o["pe0"]), dptr(q["pn2"]), oc.ZVIR, None)
    sync()
    dz = -dz_in[c3] * f["delp"][c3]
    exact("post.delz", View(q["delz"], c3), dz)
    exact("post.q_con", View(o["q_con"], c3), gz)
    exact("post.cappa", View(o["cappa"], c3), cappa)
    exact("post.pe0", View(o["pe0"], cw + (KK,)), f["peln"][cw + (KK,)])
    exact("post.peln", View(q["peln"], cw + (KK,)), pn2_in[cw + (KK,)])
    last_place("post.pkz", View(o["pkz"], c3), np.exp(cappa * np.log(oc.RDG * f["delp"][c3] / dz * f["pt"][c3])))
    # ---- k_l2e_pressures ----
    pe = f["pe"]
    pe1_in = rnd(pe * (1.0 + 1.0e-3))  # (distinct from pe: a kernel that read pe where it should read pe1 shows)
    bot = pe[:, :, km]
    for direction, win, nb in ((0, cj, (slice(3, 3 + n), slice(2, 3 + n))), (1, ci, (slice(2, 3 + n), slice(3, 3 + n)))):
        q = {"pe": env.q3(pe), "pe1": env.q3(pe1_in)}
        o = {"pe0": env.q3(), "pe3": env.q3()}
        lib.call("pace_l2e_pressures", geom, direction, dptr(q["pe"]), dptr(q["pe1"]), dptr(akq), dptr(bkq), dptr(o["pe0"]),
                 dptr(o["pe3"]), None)
        sync()
        here = pe1_in if direction == 0 else pe
        pe0 = 0.5 * (pe[nb + (KK,)] + here[win + (KK,)])
        pe0[:, :, 0] = pe[win + (0,)]
        pe3 = np.stack([ak[k] + (0.5 * bk[k]) * (bot[nb] + bot[win]) for k in range(km + 1)], axis=2)
        if direction == 1:
            pe3[:, :, 0] = ak[0]
        exact(f"pressures{direction}.pe0", View(o["pe0"], win + (KK,)), pe0)
        exact(f"pressures{direction}.pe3", View(o["pe3"], win + (KK,)), pe3)
    # ---- k_l2e_finish ----
    pkz_in = rnd(1.0 + 0.1 * np.abs(np.sin(f["pt"])))
    pe2_in = rnd(pe * (1.0 - 1.0e-3))
    for last_step in (True, False):
        q = {"pe": env.q3(pe), "pe2": env.q3(pe2_in), "pt": env.q3(f["pt"]), "pkz": env.q3(pkz_in)}
        lib.call("pace_l2e_finish", geom, water(qt), dptr(q["pe"]), dptr(q["pe2"]), dptr(q["pt"]), dptr(q["pkz"]), oc.ZVIR, int(last_step), None)
        sync()
        want = pe[cw + (KK,)].copy()
        want[:, :, 1:km] = pe2_in[cw + (slice(1, km),)]
        exact(f"finish{int(last_step)}.pe", View(q["pe"], cw + (KK,)), want)
        if last_step:
            g5 = tr["qliquid"][c3] + tr["qrain"][c3] + tr["qice"][c3] + tr["qsnow"][c3] + tr["qgraupel"][c3]
            exact("finish1.pt", View(q["pt"], c3), (f["pt"][c3] + 0.0 * pkz_in[c3]) / ((1.0 + oc.ZVIR * tr["qvapor"][c3]) * (1.0 - g5)))
        else:
            exact("finish0.pt", View(q["pt"], c3), f["pt"][c3] / pkz_in[c3])
    assert not wrong, wrong
    return report
