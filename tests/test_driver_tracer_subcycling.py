"""dycore_config.tracer_courant_subcycling through the Driver: tests/golden/driver_baroclinic_c12.yaml (the baroclinic state on
the generated C12 x 79 grid, whose metric terms carry sin_sg5) as the whole globe on one device (comm_config.type: cube).

* key true: two steps of Driver.step_all equal, bit for bit, the same two steps with the stages called by hand
  (DynamicalCore.step_dynamics, the dycore-to-physics copy, the physics, the end-of-step update) on a second Driver;
  DynamicalCore.tracer_subcycles() is all ones on every tile -- the accumulated Courant numbers of this case are a few
  hundredths -- ; the state is finite and within the SafetyChecker's bounds (checked after each step); the tracer advection of a
  step makes ONE pace_tracer_subcycles launch for the cube and none of the fixed path's three stencils;
* key false equals a run without the key, bit for bit, and records none of the mode's entry points;
* tracer_subcycles() raises RuntimeError before the first step and with the mode off;
* a misspelt key is refused by name.

The CPU tier runs the emulation library; the GPU tier a child process with a time limit."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import restart_helpers as rh  # noqa: E402
import test_driver  # noqa: E402
from helpers import ROOT, build_emu  # noqa: E402
from test_driver import clean_checks  # noqa: E402,F401

MODE_ENTRY_POINTS = ("pace_tracer_cmax", "pace_tracer_subcycles", "pace_tracer_divide_fluxes_levels", "pace_apply_mass_flux_levels",
                     "pace_apply_tracer_flux_levels", "pace_swap_dp_levels")
FIXED_ENTRY_POINTS = ("pace_tracer_divide_fluxes", "pace_apply_mass_flux", "pace_apply_tracer_flux", "pace_swap_dp")


class Recording:
    def __init__(self, lib):
        self._lib, self.calls = lib, []
        self.cdll, self.path, self.real_bytes = lib.cdll, lib.path, lib.real_bytes

    def call(self, name, *args):
        self.calls.append(name)
        return self._lib.call(name, *args)

    def version(self):
        return self._lib.version()

    timing = None


def configuration(key, steps):
    """key: True / False, or None for a dycore_config without the key."""
    from pace_amd.driver import DriverConfig

    base = test_driver.settings()
    dycore = dict(base["dycore_config"])
    if key is not None:
        dycore["tracer_courant_subcycling"] = key
    config = DriverConfig.from_dict(test_driver.settings(diagnostics_config={}, stencil_config={}, safety_check_frequency=1,
                                                         comm_config={"type": "cube"}, dycore_config=dycore, minutes=0,
                                                         seconds=int(steps * test_driver.DT)))
    assert config.dycore_config.tracer_courant_subcycling == bool(key) and config.n_timesteps() == steps
    return config


def run(key, lib, device, steps, by_hand=False):
    """-> per tile (a snapshot of the whole state, the entry points called, tracer_subcycles() or None, the RuntimeError text of
    tracer_subcycles() before the first step)"""
    from pace_amd.driver import Driver
    from pace_amd.util import run_cube

    config = configuration(key, steps)

    def program(comm):
        recording = Recording(lib)
        driver = Driver(copy.deepcopy(config), comm=comm, lib=recording, device=device)
        assert driver.dycore.config.tracer_courant_subcycling == bool(key)
        with pytest.raises(RuntimeError) as early:
            driver.dycore.tracer_subcycles()
        rh.sync(device)
        del recording.calls[:]
        if by_hand:
            s, dt = driver.state, float(config.timestep.total_seconds())
            for _ in range(steps):
                driver.dycore.step_dynamics(state=s.dycore_state, timer=driver.performance_collector.timestep_timer)
                driver.dycore_to_physics(dycore_state=s.dycore_state, physics_state=s.physics_state, tendency_state=s.tendency_state,
                                         timestep=dt)
                driver.physics(s.physics_state, timestep=dt)
                driver.end_of_step_update(dycore_state=s.dycore_state, phy_state=s.physics_state, u_dt=s.tendency_state.u_dt,
                                          v_dt=s.tendency_state.v_dt, pt_dt=s.tendency_state.pt_dt, dt=dt)
                driver.safety_checker.check_state(s.dycore_state)  # raises outside the bounds
        else:
            driver.step_all()  # (safety_check_frequency 1: the state is checked after each step)
        rh.sync(device)
        calls = list(recording.calls)
        subcycles = driver.dycore.tracer_subcycles() if key else None
        snapshot = rh.snapshot(driver.state)
        driver.cleanup()
        return snapshot, calls, subcycles, str(early.value)

    return run_cube(program)


def same(a, b):
    return [(t, k) for t in range(6) for k in a[t][0] if not np.array_equal(a[t][0][k], b[t][0][k], equal_nan=True)]


def check(device):
    from pace_amd import _lib

    lib = _lib.Library(build_emu()) if device == "cpu" else _lib.load()
    nz = test_driver.NZ
    # ---- the mode: the loop is its stages, the counts are all ones
    loop, hand = run(True, lib, device, 2), run(True, lib, device, 2, by_hand=True)
    assert same(loop, hand) == []
    for tiles in (loop, hand):
        calls = [x for t in tiles for x in t[1]]
        # two steps, k_split 1: two tracer advections a tile; ONE finalising launch a step for the cube
        assert calls.count("pace_tracer_cmax") == 12 and calls.count("pace_tracer_subcycles") == 2
        assert calls.count("pace_apply_mass_flux_levels") == 12  # one sub-cycle
        assert not [x for x in calls if x in FIXED_ENTRY_POINTS + ("pace_tracer_divide_fluxes_levels", "pace_swap_dp_levels")]
        for snapshot, _, subcycles, early in tiles:
            assert subcycles.dtype == np.int32 and subcycles.tolist() == [1] * nz
            assert "no step has run" in early
            assert all(np.isfinite(a).all() for k, a in snapshot.items() if k.startswith("dycore.q") or k in ("dycore.pt", "dycore.delp"))
    # ---- key false is a run without the key, and neither is the mode
    off, absent = run(False, lib, device, 1), run(None, lib, device, 1)
    assert same(off, absent) == []
    for tiles in (off, absent):
        for _, calls, _, early in tiles:
            assert not [x for x in calls if x in MODE_ENTRY_POINTS] and calls.count("pace_apply_mass_flux") == 3
            assert "tracer_courant_subcycling = false" in early


def test_a_misspelt_key_is_refused_by_name():
    from pace_amd.driver import DriverConfig
    from pace_amd.fv3core import DynamicalCoreConfig

    base = test_driver.settings()
    with pytest.raises(ValueError, match="tracer_courant_subcyling"):
        DriverConfig.from_dict(test_driver.settings(dycore_config=dict(base["dycore_config"], tracer_courant_subcyling=True)))
    with pytest.raises(ValueError, match="tracer_courant_subcycling"):  # (a value of the wrong type names the key too)
        DynamicalCoreConfig.from_namelist_dict({"tracer_courant_subcycling": "yes"})
    assert DynamicalCoreConfig.from_namelist_dict({"tracer_courant_subcycling": True}).tracer_courant_subcycling is True
    assert DynamicalCoreConfig().tracer_courant_subcycling is False


def test_tracer_courant_subcycling_through_the_driver_emulated(clean_checks):  # noqa: F811
    check("cpu")


@pytest.mark.gpu
def test_tracer_courant_subcycling_through_the_driver_on_the_gpu():
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); "
            f"import test_driver_tracer_subcycling; test_driver_tracer_subcycling.check('cuda')")
    p = subprocess.run([sys.executable, "-X", "faulthandler", "-c", code], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:])
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-6000:])
