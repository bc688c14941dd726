"""The driver's forcing_config (pace_amd/driver/forcing.py): tests/golden/driver_held_suarez_c12.yaml -- C12 x 79 from the
baroclinic state, dycore_only, the whole globe on one device -- through run_cube_driver, two steps, six tiles.  (A lone tile on a
NullComm turns NaN in its first step, so the cube it is.)

* the run equals, bit for bit over every DycoreState field and the three tendencies, six Drivers of the same configuration whose
  stages are called by hand in the stated order: dycore.step_dynamics, dycore_to_physics, the forcing with accumulate=True and
  the step's dt, end_of_step_update;
* one pace_held_suarez call per step and tile, each tile's on its own thread;
* the final state is finite and within the SafetyChecker's bounds (checked every step), and the apply left the tendencies zero;
* after the first step pt differs from a run of the same file minus the section, which makes no pace_held_suarez call at all;
* apply_tendencies is true with the section and unchanged (false for this file) without; restart_dict carries the section;
* the refusals: an unknown type, an unknown key, a time scale that is not positive, a value the kernel refuses, dycore_only
  false, disable_step_physics true.

The CPU tier runs the emulation library (about 40 s a six-tile step); the GPU tier a child process with a time limit."""
import copy
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import ROOT, build_emu  # noqa: E402
from test_driver import clean_checks  # noqa: E402,F401

YAML = os.path.join(ROOT, "tests", "golden", "driver_held_suarez_c12.yaml")
TENDENCIES = ("u_dt", "v_dt", "pt_dt")


class SpyLib:
    """A library whose pace_held_suarez calls are recorded with the thread that made them."""

    def __init__(self, lib):
        self._lib, self.forcings, self._lock = lib, [], threading.Lock()

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def call(self, name, *args):
        if name == "pace_held_suarez":
            with self._lock:
                self.forcings.append(threading.get_ident())
        return self._lib.call(name, *args)


def settings(**over):
    import yaml

    with open(YAML) as f:
        d = yaml.safe_load(f)
    d.update(over)
    return d


def snapshot(state):
    import dataclasses

    out = {"dycore." + f.name: np.array(getattr(state.dycore_state, f.name).numpy()) for f in dataclasses.fields(state.dycore_state)}
    out.update({"tendency." + k: np.array(getattr(state.tendency_state, k).numpy()) for k in TENDENCIES})
    return out


def check_run(device):
    from pace_amd import _lib
    from pace_amd.driver import Driver, DriverConfig, run_cube_driver
    from pace_amd.driver.driver import _SAFETY_CHECKS
    from pace_amd.util import run_cube

    lib = SpyLib(_lib.Library(build_emu()) if device == "cpu" else _lib.load())
    config = DriverConfig.from_dict(settings(stencil_config={}, safety_check_frequency=1))
    assert config.comm_config.type == "cube" and config.dycore_only and config.apply_tendencies
    assert (config.nx_tile, config.nz, config.dycore_config.do_sat_adj) == (12, 79, False)
    # ---- the run
    drivers = run_cube_driver(config, steps=2, device=device, lib=lib)
    assert all(d.performance_collector.timestep_timer.hits.get("mainloop") == 2 for d in drivers)
    assert all(d.performance_collector.total_timer.hits.get("safety_check") == 2 for d in drivers)  # (it raises out of bounds)
    got = [snapshot(d.state) for d in drivers]
    calls = {ident: lib.forcings.count(ident) for ident in set(lib.forcings)}
    assert len(lib.forcings) == 12 and sorted(calls.values()) == [2] * 6, calls
    cs = slice(3, 3 + 12)
    for tile in got:
        assert len(tile) > 20 and all(np.isfinite(a).all() for a in tile.values())
        for name, low, high in _SAFETY_CHECKS:
            a = tile["dycore." + name][cs, cs, :79]
            assert low <= a.min() and a.max() <= high, name
        assert all((tile["tendency." + k][cs, cs, :79] == 0.0).all() for k in TENDENCIES)

    # ---- the same stages by hand
    lib.forcings.clear()
    stepped = copy.deepcopy(config)
    dt = float(config.dt_atmos)

    def by_hand(comm):
        driver = Driver(copy.deepcopy(stepped), comm=comm, lib=lib, device=device)
        state, tendency = driver.state.dycore_state, driver.state.tendency_state
        pt_after_first = None
        for step in range(2):
            driver.dycore.step_dynamics(state=state, timer=driver.performance_collector.timestep_timer)
            driver.dycore_to_physics(dycore_state=state, physics_state=driver.state.physics_state, tendency_state=tendency,
                                     timestep=dt)
            driver.forcing(state, tendency.u_dt, tendency.v_dt, tendency.pt_dt, dt, accumulate=True)
            driver.end_of_step_update(dycore_state=state, phy_state=driver.state.physics_state, u_dt=tendency.u_dt,
                                      v_dt=tendency.v_dt, pt_dt=tendency.pt_dt, dt=dt)
            if step == 0:
                pt_after_first = np.array(state.pt.numpy())
        driver.cleanup()
        return snapshot(driver.state), pt_after_first

    want = run_cube(by_hand)
    assert len(lib.forcings) == 12
    for t in range(6):
        assert set(got[t]) == set(want[t][0])
        for k in got[t]:
            assert np.array_equal(got[t][k], want[t][0][k]), (t, k)

    # ---- the same file minus the section, one step
    lib.forcings.clear()
    plain = DriverConfig.from_dict({k: v for k, v in settings(stencil_config={}, safety_check_frequency=1).items()
                                    if k != "forcing_config"})
    assert plain.forcing_config is None and plain.apply_tendencies is False
    unforced = run_cube_driver(plain, steps=1, device=device, lib=lib)
    assert lib.forcings == [] and all(d.forcing is None for d in unforced)
    for t in range(6):
        pt = np.array(unforced[t].state.dycore_state.pt.numpy())
        assert np.isfinite(pt).all() and not np.array_equal(pt[cs, cs, :79], want[t][1][cs, cs, :79]), t


def test_configuration_and_refusals(tmp_path):
    from pace_amd.driver import DriverConfig, ForcingConfig
    from pace_amd.stencils import HeldSuarezConfig

    config = DriverConfig.from_dict(settings())
    assert isinstance(config.forcing_config, ForcingConfig) and config.forcing_config.type == "held_suarez"
    assert config.forcing_config.held_suarez_config() == HeldSuarezConfig()  # (the file spells the defaults out)
    assert config.apply_tendencies is True
    assert config.restart_dict(str(tmp_path))["forcing_config"] == settings()["forcing_config"]
    bare = DriverConfig.from_dict(settings(forcing_config={"type": "held_suarez"}))
    assert bare.forcing_config.held_suarez_config() == HeldSuarezConfig()
    half = DriverConfig.from_dict(settings(forcing_config={"type": "held_suarez", "config": {"k_f_days": 0.5, "sigma_b": 0.8, "t0": 300}}))
    assert half.forcing_config.held_suarez_config() == HeldSuarezConfig(k_f=1.0 / (0.5 * 86400.0), sigma_b=0.8, t0=300.0)
    # absent: no forcing, apply_tendencies as it was
    plain = {k: v for k, v in settings().items() if k != "forcing_config"}
    assert DriverConfig.from_dict(plain).forcing_config is None and DriverConfig.from_dict(plain).apply_tendencies is False
    assert DriverConfig.from_dict(dict(plain, dycore_only=False)).apply_tendencies is True

    def refused(match, top=None, **section):
        d = settings(**(top or {}))
        d["forcing_config"] = dict(d["forcing_config"], **section)
        with pytest.raises(ValueError, match=match):
            DriverConfig.from_dict(d)

    refused("type", type="newtonian")
    refused("frobnicate", frobnicate=1)
    refused("frobnicate", config={"frobnicate": 1.0})
    refused("k_f", config={"k_f": 1.0e-5})  # (the rates are given as time scales in days)
    for key in ("k_f_days", "k_a_days", "k_s_days"):
        for value in (0.0, -1.0, float("inf"), float("nan"), "fast", True):
            refused(key, config={key: value})
    refused("sigma_b", config={"sigma_b": 1.0})
    refused("sigma_b", config={"sigma_b": -0.2})
    refused("p0", config={"p0": 0.0})
    refused("t0", config={"t0": "warm"})
    refused("mapping", config=[1.0])
    refused("dycore_only", top={"dycore_only": False})
    refused("disable_step_physics", top={"disable_step_physics": True})


def test_two_forced_steps_on_the_cube_emulated(clean_checks):  # noqa: F811
    check_run("cpu")


@pytest.mark.gpu
def test_two_forced_steps_on_the_cube_gpu():
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); "
            f"import test_driver_held_suarez; test_driver_held_suarez.check_run('cuda')")
    p = subprocess.run([sys.executable, "-X", "faulthandler", "-c", code], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-6000:])
