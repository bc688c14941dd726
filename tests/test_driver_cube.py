"""comm_config.type: cube -- a driver configuration as the whole globe on one device (pace_amd.driver.run_cube_driver): the
configuration, the refusal of a lone Driver, and the runs of the two fixture files against the same files on six ThreadComm
ranks, bit for bit per tile.  The CPU tier runs the emulation library; the GPU tier a child process with a time limit."""
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


def _lib(device):
    from pace_amd import _lib

    return _lib.Library(build_emu()) if device == "cpu" else _lib.load()


def _snapshots(drivers, device):
    rh.sync(device)
    return [rh.snapshot(d.state) for d in drivers]


def _threads(settings, steps, lib, device):
    """The same file on six ThreadComm ranks (run_tiles), as tests/test_driver.py and tests/test_fortran_restart.py run it."""
    from pace_amd.driver import Driver, DriverConfig
    from pace_amd.util import run_tiles

    config = DriverConfig.from_dict(dict(settings, comm_config={"type": "null"}, days=0, hours=0, minutes=0,
                                         seconds=int(steps * config_dt(settings))))
    assert config.n_timesteps() == steps

    def program(comm):
        driver = Driver(copy.deepcopy(config), comm=comm, lib=lib, device=device)
        driver.step_all()
        driver.cleanup()
        return driver

    return run_tiles(6, program)


def config_dt(settings):
    return float(settings["dt_atmos"])


def _compare(got, want):
    assert len(got) == len(want) == 6
    for t in range(6):
        assert set(got[t]) == set(want[t]) and len(got[t]) > 40
        for k in want[t]:
            assert np.array_equal(got[t][k], want[t][k], equal_nan=True), (t, k)


def check_baroclinic(device):
    """tests/golden/driver_baroclinic_c12.yaml with comm_config.type: cube, one step."""
    from pace_amd.driver import DriverConfig, run_cube_driver

    lib = _lib(device)
    settings = test_driver.settings(diagnostics_config={}, stencil_config={}, safety_check_frequency=1)
    config = DriverConfig.from_dict(dict(settings, comm_config={"type": "cube"}))
    drivers = run_cube_driver(config, steps=1, device=device, lib=lib)
    assert [d.comm.Get_rank() for d in drivers] == list(range(6))
    assert all(d.performance_collector.timestep_timer.hits.get("mainloop") == 1 for d in drivers)
    assert all(d.performance_collector.total_timer.hits.get("safety_check") == 1 for d in drivers)
    assert all((d.time - d.config.start_time).total_seconds() == config.dt_atmos for d in drivers)
    assert config.n_timesteps() != 1  # (the caller's configuration keeps its run length)
    got = _snapshots(drivers, device)
    assert all(np.isfinite(a).all() for a in got[0].values())
    _compare(got, _snapshots(_threads(settings, 1, lib, device), device))


def check_fortran_restart(device):
    """tests/golden/driver_fortran_restart_c12.yaml, two steps, the state held against the files' checksums over the six ranks
    as it is read."""
    from pace_amd.driver import DriverConfig, run_cube_driver

    lib = _lib(device)
    settings = rh.settings(stencil_config={}, safety_check_frequency=1, comm_config={"type": "cube"})
    settings["initialization"]["config"]["verify_checksums"] = True
    config = DriverConfig.from_dict(settings)
    assert config.initialization.config.verify_checksums is True
    drivers = run_cube_driver(config, steps=2, device=device, lib=lib)
    assert all(d.performance_collector.timestep_timer.hits.get("mainloop") == 2 for d in drivers)
    want = rh.run_driver(lib, device, steps=2)  # six ThreadComm ranks: (snapshot, facts) per tile
    _compare(_snapshots(drivers, device), [w[0] for w in want])


# ---- configuration ------------------------------------------------------------------------------------------------------------
def test_the_cube_type_loads_and_a_lone_driver_is_refused(tmp_path):
    import yaml

    from pace_amd.driver import CubeCommConfig, Driver, DriverConfig
    from pace_amd import _lib

    settings = test_driver.settings(comm_config={"type": "cube"})
    config = DriverConfig.from_dict(settings)
    assert config.comm_config.type == "cube" and isinstance(config.comm_config.config, CubeCommConfig)
    path = tmp_path / "cube.yaml"
    path.write_text(yaml.safe_dump(settings))
    assert isinstance(DriverConfig.from_yaml(str(path)).comm_config.config, CubeCommConfig)
    with pytest.raises(ValueError, match="frobnicate"):
        DriverConfig.from_dict(test_driver.settings(comm_config={"type": "cube", "config": {"frobnicate": 1}}))
    with pytest.raises(ValueError, match="run_cube_driver"):
        Driver(config, lib=_lib.Library(build_emu()))


def test_baroclinic_file_on_the_cube_emulated(clean_checks):  # noqa: F811
    check_baroclinic("cpu")


def test_fortran_restart_file_on_the_cube_emulated(clean_checks):  # noqa: F811
    check_fortran_restart("cpu")


def test_driver_run_tool_runs_the_globe(tmp_path):
    """tools/driver_run.py as a lone process with --cube (emulation): the JSON line of the six-process form."""
    import json

    build_emu()
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "driver_run.py"), rh.YAML, "--steps", "1", "--cpu-emulation", "--cube"],
                       capture_output=True, text=True, timeout=900, env=dict(env, OMP_NUM_THREADS="1"), cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    assert set(out) == {"workload", "n_gpus", "steps", "ms_per_step", "sypd", "safety_checks_in_loop", "safety_check_ms_per_call",
                        "safety_check", "nan_fraction_pt", "transport"}
    assert out["steps"] == 1 and out["ms_per_step"] > 0 and out["nan_fraction_pt"] == 0.0 and "six tiles in one process" in out["workload"]
    assert out["safety_check"] == "within bounds"


# ---- the GPU tier ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("what", ["baroclinic", "fortran_restart"])
def test_on_the_gpu(what):
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); "
            f"import test_driver_cube; test_driver_cube.check_{what}('cuda')")
    p = subprocess.run([sys.executable, "-X", "faulthandler", "-c", code], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-6000:])
