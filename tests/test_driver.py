"""pace_amd.driver: the configuration, the initial state, the loop against its stages called by hand, the state check inside the
loop, and one step against the reference's own run (tests/golden/driver_c12_tile*_p*.npz, tools/make_golden_driver.py).

The six-tile runs are C12 x 79 on six ThreadComm ranks in one process; on the GPU they run in a child process with a time
limit, as the other six-tile device runs do (helpers.run_in_child), and the child hands back only what the assertions need."""
import copy
import datetime
import math
import os
import pickle
import subprocess
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers  # noqa: E402
from helpers import GOLDEN, ROOT, build_emu, golden  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_microphysics import load_split  # noqa: E402

N, NZ, DT = 12, 79, 225.0
YAML = os.path.join(GOLDEN, "driver_baroclinic_c12.yaml")
TENDENCIES = ("u_dt", "v_dt", "pt_dt")
UPDATED = ("physics_updated_specific_humidity", "physics_updated_qliquid", "physics_updated_qrain", "physics_updated_qice",
           "physics_updated_qsnow", "physics_updated_qgraupel", "physics_updated_cloud_fraction", "physics_updated_pt",
           "physics_updated_ua", "physics_updated_va")
GRID_TERMS = ("vlon", "vlat", "es1", "ew2", "edge_vect_w", "edge_vect_e", "edge_vect_s", "edge_vect_n")
VARIANTS = {"moist": {}, "dycore_only": {"dycore_only": True, "fv_sg_adj": 900}, "no_physics": {"disable_step_physics": True}}
PLANTED = (3, (9, 8, 40), 1000.0)  # tile, a cell of its compute domain, the value its pt gets


@pytest.fixture(scope="module")
def emu_lib():
    from pace_amd import _lib

    return _lib.Library(build_emu())


def settings(**over):
    import yaml

    with open(YAML) as f:
        d = yaml.safe_load(f)
    d.update(over)
    return d


@pytest.fixture
def clean_checks():
    from pace_amd.driver import SafetyChecker

    saved = dict(SafetyChecker.checks)
    SafetyChecker.clear_all_checks()
    yield SafetyChecker
    SafetyChecker.clear_all_checks()
    SafetyChecker.checks.update(saved)


# ---- configuration ------------------------------------------------------------------------------------------------------------
def test_the_reference_file_loads():
    from pace_amd.driver import DriverConfig

    config = DriverConfig.from_yaml(YAML)
    assert config.n_timesteps() == 4
    assert config.timestep == datetime.timedelta(seconds=225) and config.total_time == datetime.timedelta(minutes=15)
    assert config.start_time == datetime.datetime(2000, 1, 1)
    assert (config.nx_tile, config.nz, config.layout, config.dt_atmos) == (12, 79, (1, 1), 225.0)
    assert not config.dycore_only and not config.disable_step_physics and config.safety_check_frequency is None
    assert not config.do_dry_convective_adjustment and config.apply_tendencies
    assert config.initialization.type == "baroclinic" and config.grid_config.type == "generated" and config.comm_config.type == "null"
    # kept, not acted on
    assert config.diagnostics_config.path == "output" and config.diagnostics_config.z_select[0].level == 65
    assert config.performance_config.experiment_name == "c12_baroclinic"
    assert config.stencil_config.requested_backend == "numpy" and config.stencil_config.backend == "hip:gfx950"
    # the derived settings reach both sub-configurations
    for sub in (config.dycore_config, config.physics_config):
        assert (sub.layout, sub.dt_atmos, sub.npx, sub.npy, sub.npz) == ((1, 1), 225.0, 13, 13, 79)
    assert config.physics_config.do_qa and config.physics_config.nwat == 6 and not config.physics_config.hydrostatic


def test_flat_keys_land_in_every_nested_place():
    from pace_amd.driver import DriverConfig
    from pace_amd.fv3core import DynamicalCoreConfig

    flat = dict(settings()["dycore_config"], nord=2, d4_bg=0.12, p_fac=0.07, hord_tr=7, n_sponge=30, do_sat_adj=True, d_con=0.5,
                hord_tm=5, hydrostatic=False, grid_type=0, n_split=3, k_split=2, beta=0.1, d_ext=0.01, use_logp=False)
    for dc in (DriverConfig.from_dict(settings(dycore_config=flat)).dycore_config, DynamicalCoreConfig.from_namelist_dict(flat)):
        ac, dsw, riem = dc.acoustic_dynamics, dc.acoustic_dynamics.d_grid_shallow_water, dc.acoustic_dynamics.riemann
        assert (ac.nord, dsw.nord) == (2, 2)
        assert dsw.d4_bg == 0.12
        assert (ac.p_fac, riem.p_fac) == (0.07, 0.07)
        assert dc.hord_tr == 7
        assert (dc.n_sponge, dsw.n_sponge) == (30, 30)
        assert dc.do_sat_adj is True and dc.remapping.do_sat_adj is True
        assert (ac.d_con, dsw.d_con) == (0.5, 0.5)
        assert (ac.hord_tm, dsw.hord_tm) == (5, 5)
        assert (dc.n_split, ac.n_split, dc.k_split, ac.k_split) == (3, 3, 2, 2)
        assert (ac.beta, riem.beta) == (0.1, 0.1) and (ac.d_ext, dsw.d_ext) == (0.01, 0.01)
        assert (dc.hydrostatic, ac.hydrostatic, dsw.hydrostatic) == (False, False, False)
        assert (riem.a_imp, dsw.vtdm4, dsw.do_vort_damp, dsw.ke_bg, dsw.d2_bg_k1, ac.rf_cutoff, ac.delt_max) == \
            (1.0, 0.06, True, 0.0, 0.2, 3000.0, 0.002)
        assert dc.fv_sg_adj == 0 and not dc.do_dry_convective_adjustment and dc.do_qa and dc.tau_g2v == 1200.0


def test_unknown_and_derived_keys_are_refused():
    from pace_amd.driver import DriverConfig

    for where, bad in (("top", settings(frobnicate=1)),
                       ("dycore", settings(dycore_config=dict(settings()["dycore_config"], frobnicate=1))),
                       ("physics", settings(physics_config={"frobnicate": 1})),
                       ("diagnostics", settings(diagnostics_config={"frobnicate": 1})),
                       ("comm", settings(comm_config={"type": "null", "config": {"frobnicate": 1}})),
                       ("stencil", settings(stencil_config={"compilation_config": {"frobnicate": 1}}))):
        with pytest.raises(ValueError, match="frobnicate"):
            DriverConfig.from_dict(bad)
    for name, value in (("npx", 13), ("npy", 13), ("npz", 79), ("layout", [1, 1]), ("dt_atmos", 225)):
        with pytest.raises(ValueError, match=f"cannot set {name} directly in dycore_config"):
            DriverConfig.from_dict(settings(dycore_config=dict(settings()["dycore_config"], **{name: value})))
    with pytest.raises(ValueError, match="nord"):  # a value of the wrong type names its setting too
        DriverConfig.from_dict(settings(dycore_config=dict(settings()["dycore_config"], nord="three")))


@pytest.mark.parametrize("name,over", [
    ("restart", {"initialization": {"type": "restart", "config": {"path": "."}}}),
    ("mpi", {"comm_config": {"type": "mpi"}}),
    ("write", {"comm_config": {"type": "write", "config": {"ranks": [0]}}}),
    ("read", {"comm_config": {"type": "read", "config": {"rank": 0}}}),
    ("pair_debug", {"pair_debug": True}),
    ("restart_config", {"restart_config": {"save_restart": True}}),
    ("restart_config", {"restart_config": {"intermediate_restart": [2]}}),
    ("layout", {"layout": [2, 2]}),
])
def test_refused_settings_name_themselves(name, over):
    from pace_amd.driver import DriverConfig

    with pytest.raises(NotImplementedError, match=name):
        DriverConfig.from_dict(settings(**over))


def test_accepted_settings():
    from pace_amd.driver import DriverConfig, NullCommConfig, TorchCommConfig

    config = DriverConfig.from_dict(settings(comm_config={"type": "null_comm", "config": {"rank": 2, "total_ranks": 6}},
                                             grid_config={"type": "generated"}, restart_config={"save_restart": False},
                                             safety_check_frequency=2, seconds=10))
    assert isinstance(config.comm_config.config, NullCommConfig) and config.comm_config.get_comm().Get_rank() == 2
    assert config.safety_check_frequency == 2 and config.total_time == datetime.timedelta(minutes=15, seconds=10)
    assert isinstance(DriverConfig.from_dict(settings(comm_config={"type": "torch"})).comm_config.config, TorchCommConfig)


def test_the_diagnostics_warning_is_emitted_once(emu_lib, clean_checks):
    """A Driver on rank 0 says once that the diagnostics (and the foreign backend) of the file are ignored; rank 1 and a file
    without them say nothing."""
    from pace_amd.driver import Driver, DriverConfig
    from pace_amd.util import NullComm

    def count(config, rank):
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            Driver(config, comm=NullComm(rank, 6), lib=emu_lib)
        return [str(w.message) for w in seen if "diagnostics" in str(w.message) or "backend" in str(w.message)]

    first = count(DriverConfig.from_dict(settings(dycore_only=True)), 0)
    assert len(first) == 1 and "no diagnostics are written" in first[0] and "'numpy'" in first[0]
    assert count(DriverConfig.from_dict(settings(dycore_only=True)), 1) == []
    quiet = settings(dycore_only=True, stencil_config={}, diagnostics_config={})
    assert count(DriverConfig.from_dict(quiet), 0) == []
    assert set(clean_checks.checks) == {"ua", "va", "delp", "pt"}  # registered once by three drivers
    b = clean_checks.checks
    assert (b["ua"].minimum_value, b["ua"].maximum_value, b["delp"].minimum_value, b["delp"].maximum_value,
            b["pt"].minimum_value, b["pt"].maximum_value) == (-200, 200, -1.0, 4000, 100, 380)
    assert all(v.compute_domain_only for v in b.values())


def host(x):
    if hasattr(x, "dims"):
        return x.numpy()
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x, dtype=float)


# ---- the initial state --------------------------------------------------------------------------------------------------------
def test_baroclinic_initial_state_is_the_generators(emu_lib, clean_checks):
    """Driver(initialization: baroclinic) on six ThreadComm ranks: grid metrics and dycore state equal, bit for bit, what
    helpers.generated_inputs(12, 79) returns."""
    from pace_amd.driver import Driver, DriverConfig
    from pace_amd.util import run_tiles

    config = DriverConfig.from_dict(settings(diagnostics_config={}, stencil_config={}))
    want = helpers.generated_inputs(N, NZ)

    def program(comm):
        driver = Driver(copy.deepcopy(config), comm=comm, lib=emu_lib)
        metrics, arrays = want[comm.Get_rank()]
        grid, info = driver.state.grid_data, driver.state.driver_grid_data
        assert grid is driver.dycore.grid_data
        for name, value in metrics.items():
            value = np.asarray(value, dtype=float)
            if value.ndim == 3:  # vlon, vlat: the three components are fields of the driver grid data
                for m in range(3):
                    assert np.array_equal(host(getattr(info, f"{name}{m + 1}")), value[:, :, m], equal_nan=True), (name, m)
            elif name.startswith("edge_vect_"):
                assert np.array_equal(host(getattr(info, name)), value, equal_nan=True), name
            else:
                assert np.array_equal(host(getattr(grid, name)), value, equal_nan=True), name
        for name, value in arrays.items():
            assert np.array_equal(getattr(driver.state.dycore_state, name).numpy(), value, equal_nan=True), name
        assert driver.physics is not None and driver.state.physics_state.microphysics is not None
        assert all(float(np.abs(getattr(driver.state.tendency_state, k).numpy()).max()) == 0.0 for k in TENDENCIES)
        assert driver.time == datetime.datetime(2000, 1, 1) and driver.sypd() == -999.0
        return len(metrics) + len(arrays)

    assert min(run_tiles(6, program)) > 40


# ---- six-tile runs from the fixtures' state -----------------------------------------------------------------------------------
def tile_inputs(tile):
    """What helpers.run_dycore_tile starts from, and the reference's driver grid terms (drivergrid_c12.npz)."""
    fix_ac, fix_dy = golden(f"acoustic_c12_tile{tile}.npz"), golden(f"dycore_c12_tile{tile}.npz")
    metrics = {k[5:]: v for k, v in fix_ac.items() if k.startswith("grid_")}
    arrays = {k: fix_ac["in_" + k] for k in "u v w delz delp pe pk peln phis uc vc ua va".split()}
    shape = arrays["delp"].shape
    pt, qv = np.zeros(shape), np.zeros(shape)
    pt[3:3 + N, 3:3 + N, :], qv[3:3 + N, 3:3 + N, :] = fix_dy["in_pt"], fix_dy["in_qvapor"]
    arrays.update(pt=pt, qvapor=qv, ps=fix_dy["in_ps"])
    for name, f in helpers.dycore_condensates(tile, shape).items():
        arrays[name] = f * (arrays["delp"] > 0)
    grid = golden("drivergrid_c12.npz")
    return metrics, arrays, {k: grid[f"{k}_tile{tile}"] for k in GRID_TERMS}


def predefined(lib, device, tile, plant=None):
    """The six objects of a `predefined` initialization for one tile."""
    from pace_amd.driver import TendencyState
    from pace_amd.fv3core import DycoreState
    from pace_amd.physics import PhysicsState
    from pace_amd.tile import setup_factories
    from pace_amd.util.grid import DampingCoefficients, DriverGridData, GridData

    metrics, arrays, terms = tile_inputs(tile)
    if plant is not None and plant[0] == tile:
        arrays["pt"][plant[1]] = plant[2]
    _, qf, _, _ = setup_factories(lib, device, N, NZ)
    grid_data = GridData(qf, metrics)
    return dict(dycore_state=DycoreState.init_from_numpy_arrays(arrays, qf),
                physics_state=PhysicsState.init_zeros(qf, ["microphysics"]), tendency_state=TendencyState.init_zeros(qf),
                grid_data=grid_data, damping_coefficients=DampingCoefficients(grid_data),
                driver_grid_data=DriverGridData.new_from_grid_variables(**terms, quantity_factory=qf))


def driver_config(objects, steps, variant):
    from pace_amd.driver import DriverConfig

    over = dict(VARIANTS[variant])
    d = settings(initialization={"type": "predefined", "config": objects}, minutes=0, seconds=int(steps * DT),
                 safety_check_frequency=1, diagnostics_config={}, stencil_config={})
    if "fv_sg_adj" in over:
        d["dycore_config"] = dict(d["dycore_config"], fv_sg_adj=over.pop("fv_sg_adj"))
    d.update(over)
    return DriverConfig.from_dict(d)


def snapshot(state):
    """Every DycoreState field, the three tendencies and the physics_updated_* fields over the whole storage."""
    import dataclasses

    out = {"dycore." + f.name: np.array(getattr(state.dycore_state, f.name).numpy()) for f in dataclasses.fields(state.dycore_state)}
    out.update({"tendency." + k: np.array(getattr(state.tendency_state, k).numpy()) for k in TENDENCIES})
    for k in UPDATED:
        f = getattr(state.physics_state, k)
        out["physics." + k] = np.array(f.numpy() if hasattr(f, "dims") else f.detach().cpu().numpy())
    return out


def sync(device):
    if device != "cpu":
        import torch

        torch.cuda.synchronize()


def run_driver(lib, device, variant, steps=2, plant=None):
    """Six Drivers on six ThreadComm ranks; per tile (snapshot after the last step, the stored points after the FIRST step, facts
    about the run)."""
    from pace_amd.driver import Driver
    from pace_amd.util import run_tiles

    def program(comm):
        tile = comm.Get_rank()
        config = driver_config(predefined(lib, device, tile, plant), steps, variant)
        assert config.n_timesteps() == steps
        driver = Driver(config, comm=comm, lib=lib, device=device)
        start = driver.time
        after_first = {}
        end_of_step = driver._end_of_step_actions

        def spy(step):
            end_of_step(step)
            if step == 0:
                sync(device)
                after_first.update(stored(driver.state))

        driver._end_of_step_actions = spy
        driver.step_all()
        sync(device)
        timer = driver.performance_collector.timestep_timer
        facts = {"elapsed": (driver.time - start).total_seconds(), "mainloop_hits": timer.hits.get("mainloop"), "sypd": driver.sypd(),
                 "checks": driver.performance_collector.total_timer.hits.get("safety_check"),
                 "physics": driver.physics is not None, "coupled": driver.end_of_step_update is not None}
        driver.cleanup()
        return snapshot(driver.state), after_first, facts

    return run_tiles(6, program)


def run_stages(lib, device, variant, steps=2):
    """The same steps with the stage classes called by hand in the order of the reference's driver.py:618-640, the moist halves
    as the operators of their own (CopyDycoreToPhysics, PhysicsToDycore, ApplyPhysicsToDycore)."""
    import types

    from pace_amd import stencils
    from pace_amd.driver import DriverConfig
    from pace_amd.fv3core import DynamicalCore
    from pace_amd.physics import Physics
    from pace_amd.tile import setup_factories
    from pace_amd.util import CubedSphereCommunicator, run_tiles

    def program(comm):
        tile = comm.Get_rank()
        o = types.SimpleNamespace(**predefined(lib, device, tile))
        config = DriverConfig.from_dict(settings(diagnostics_config={}, stencil_config={}))
        dc, pc = config.dycore_config, config.physics_config
        dc.fv_sg_adj = VARIANTS[variant].get("fv_sg_adj", dc.fv_sg_adj)
        _, qf, _, sf = setup_factories(lib, device, N, NZ)
        cube = CubedSphereCommunicator(comm, device=device, lib=lib)
        state, tend, phy = o.dycore_state, o.tendency_state, o.physics_state
        core = DynamicalCore(cube, o.grid_data, sf, qf, o.damping_coefficients, dc, state.phis, state, datetime.timedelta(seconds=DT))
        if variant == "moist":
            assert not dc.do_dry_convective_adjustment
            to_physics = stencils.CopyDycoreToPhysics(sf, qf)
            physics = Physics(sf, qf, o.grid_data, pc, ["microphysics"])
            gather = stencils.PhysicsToDycore(sf, qf, pc)
            apply = stencils.ApplyPhysicsToDycore(sf, qf, o.grid_data, pc, cube, o.driver_grid_data, state, tend.u_dt, tend.v_dt)
        elif variant == "dycore_only":
            assert dc.do_dry_convective_adjustment
            to_physics = stencils.DycoreToPhysics(sf, qf, dc, True, True)
            update = stencils.UpdateAtmosphereState(sf, o.grid_data, pc, cube, o.driver_grid_data, state, qf, True, True, tend)
        for _ in range(steps):
            core.step_dynamics(state)
            if variant == "moist":
                to_physics(state, phy)
                physics(phy, timestep=DT)
                gather(state, phy, tend.u_dt, tend.v_dt, tend.pt_dt)
                apply(state, tend.u_dt, tend.v_dt, tend.pt_dt, dt=DT)
            elif variant == "dycore_only":
                to_physics(state, None, tend, DT)
                update(state, None, tend.u_dt, tend.v_dt, tend.pt_dt, DT)
        sync(device)
        return snapshot(o)

    return run_tiles(6, program)


def loop_against_stages(lib, device, variant):
    """-> (the fields that differ, per-tile facts)."""
    got, want = run_driver(lib, device, variant), run_stages(lib, device, variant)
    different = [(t, k) for t in range(6) for k in want[t] if not np.array_equal(got[t][0][k], want[t][k], equal_nan=True)]
    moved = [k for k in want[0] if k.startswith("physics.") and np.abs(want[0][k]).max() > 0]
    return different, [g[2] for g in got], len(want[0]), moved


def check_loop(result, variant):
    different, facts, nfields, moved = result
    assert nfields == 32 + 3 + 10
    assert different == [], different[:10]
    for f in facts:
        assert f["elapsed"] == 2 * DT and f["mainloop_hits"] == 2 and f["checks"] == 2
        assert math.isfinite(f["sypd"]) and f["sypd"] > 0
        assert f["physics"] == (variant == "moist") and f["coupled"] == (variant != "no_physics")
    assert (len(moved) == 10) == (variant == "moist"), moved  # the physics ran in the moist variant and only there


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_loop_is_the_stages_emulated(emu_lib, clean_checks, variant):
    check_loop(loop_against_stages(emu_lib, "cpu", variant), variant)


# ---- the state check inside the loop --------------------------------------------------------------------------------------------
def planted_run(lib, device):
    """One pt value in the compute domain of tile 3 is 1000 K before step_all: that tile's driver raises at the end of step 1, and
    ThreadComm unblocks the five others (a failed rank wakes every waiting one), so run_tiles ends and raises for tile 3."""
    try:
        run_driver(lib, device, "moist", steps=2, plant=PLANTED)
    except RuntimeError as e:
        return str(e)
    return None


def check_planted(message):
    assert message is not None, "the run with a 1000 K cell was not stopped"
    assert message.startswith(f"tile {PLANTED[0]} failed: RuntimeError"), message[:300]
    assert "Variable" in message and ("outside of its specified bounds" in message or "contains a NaN value" in message), message[:300]
    assert "in _end_of_step_actions" in message and "check_state" in message  # raised by the check, inside the loop


def test_the_check_acts_inside_the_loop_emulated(emu_lib, clean_checks):
    check_planted(planted_run(emu_lib, "cpu"))


# ---- one step against the reference's run ---------------------------------------------------------------------------------------
STORED = tuple(helpers.DYCORE_OUT) + TENDENCIES + UPDATED


def stored_levels_and_columns():
    """The level subset and the columns of the dycore fixtures, which the driver fixtures share."""
    fix = golden("dycore_c12_tile0.npz")
    return [int(k) for k in fix["k_sel"]], [tuple(int(x) for x in c) for c in fix["cols"]]


def stored(state):
    """The fixture's points of a DriverState: per variable the level subset of the compute window (+ the staggered row / column)
    and the full columns, as tools/make_golden_driver.py stores them."""
    K_SEL, COLS = stored_levels_and_columns()
    out = {}
    for name in STORED:
        owner = state.dycore_state if name in helpers.DYCORE_OUT else (state.tendency_state if name in TENDENCIES else state.physics_state)
        f = getattr(owner, name)
        a = f.numpy() if hasattr(f, "dims") else f.detach().cpu().numpy()
        out["out_" + name] = np.ascontiguousarray(a[3:16, 3:16][:, :, K_SEL])
        out["col_" + name] = np.stack([a[i, j, :] for (i, j) in COLS])
    out["out_ps"] = np.array(state.dycore_state.ps.numpy()[3:16, 3:16])
    return out


def points(d, name):
    K_SEL, _ = stored_levels_and_columns()
    if name == "ps":
        return d["out_ps"][:N, :N].ravel()
    di = 1 if name in ("v", "mfxd", "cxd") else 0
    dj = 1 if name in ("u", "mfyd", "cyd") else 0
    nk = NZ + 1 if name in ("pe", "pk", "peln") else NZ
    idx = [m for m, k in enumerate(K_SEL) if k < nk]
    return np.concatenate([d["out_" + name][:N + di, :N + dj][:, :, idx].ravel(), d["col_" + name][:, :nk].ravel()])


def reference_errors(firsts):
    """helpers.dycore_scaled_errors' metric -- max |got - ref| / max |ref| per variable, the worst of the six tiles -- over EVERY
    stored point (level subset and columns), with the bound max(floor, 10 * sens) per variable."""
    rows = {}
    for tile in range(6):
        fix = load_split(f"driver_c12_tile{tile}")
        for name in STORED + ("ps",):
            ref, got = points(fix, name), points(firsts[tile], name)
            assert ref.shape == got.shape and np.isfinite(ref).all(), name
            e = float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-300))
            floor = helpers.DYCORE_TOL.get(name, 1e-11) if (name in helpers.DYCORE_OUT or name == "ps") else 1e-10
            sens = float(fix["sens_" + name])
            row = rows.setdefault(name, {"floor": floor, "sens": sens, "error": 0.0})
            row["error"] = max(row["error"], e)
            assert row["sens"] == sens
    for row in rows.values():
        row["bound"] = max(row["floor"], 10.0 * row["sens"])
    return rows


def check_reference(rows, where):
    print(f"\n{where}: variable floor sens bound error")
    for name, r in rows.items():
        print(f"  {name:36s} {r['floor']:.0e} {r['sens']:.1e} {r['bound']:.1e} {r['error']:.2e}")
    assert len(rows) == len(STORED) + 1
    bad = {name: (r["error"], r["bound"]) for name, r in rows.items() if not r["error"] <= r["bound"]}
    assert not bad, bad


def test_one_step_against_the_reference_emulated(emu_lib, clean_checks):
    firsts = [r[1] for r in run_driver(emu_lib, "cpu", "moist", steps=1)]
    check_reference(reference_errors(firsts), "emulated")


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------
def _child_main(what, out_path):
    from pace_amd import _lib

    lib = _lib.load()
    if what.startswith("loop_"):
        result = loop_against_stages(lib, "cuda", what[5:])
    elif what == "planted":
        result = planted_run(lib, "cuda")
    elif what == "reference":
        result = [r[1] for r in run_driver(lib, "cuda", "moist", steps=1)]
    else:
        raise ValueError(what)
    with open(out_path, "wb") as f:
        pickle.dump(result, f)


def run_in_child(what, tmp_path, timeout=300):
    """helpers.run_in_child for this module's runs: a fresh process, a time limit, the child's output in the error when it fails."""
    out = os.path.join(str(tmp_path), f"{what}.pkl")
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); "
            f"import test_driver; test_driver._child_main({what!r}, {out!r})")
    p = subprocess.run([sys.executable, "-X", "faulthandler", "-c", code], capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError(f"child run {what!r} failed (rc {p.returncode}):\n{p.stdout[-4000:]}\n{p.stderr[-8000:]}")
    with open(out, "rb") as f:
        return pickle.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_loop_is_the_stages_gpu(tmp_path, variant):
    check_loop(run_in_child("loop_" + variant, tmp_path), variant)


@pytest.mark.gpu
def test_the_check_acts_inside_the_loop_gpu(tmp_path):
    check_planted(run_in_child("planted", tmp_path))


@pytest.mark.gpu
def test_one_step_against_the_reference_gpu(tmp_path):
    check_reference(reference_errors(run_in_child("reference", tmp_path)), "device")
