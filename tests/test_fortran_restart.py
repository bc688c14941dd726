"""initialization.type: fortran_restart -- pace_amd.util.open_restart, DycoreState.from_fortran_restart, FortranRestartInit,
grid_config.config.restart_path and a run of the driver from the fixture (tests/golden/c12_restart: the reference's own C12 x 63
test restart; tests/golden/driver_fortran_restart_c12.yaml: the reference's example configuration for it).

The reader is compared bit for bit with the files read here with scipy; the state over the whole raw storage of all 32 fields
with a numpy restatement; the six-tile run (two steps on six ThreadComm ranks) with the same stages called by hand, as
tests/test_driver.py compares its loop.  On the GPU the six-tile runs are in a child process with a time limit.  The kernel
that completes the state, pace_pe_peln_from_delp, has tests/test_fortran_restart_kernel.py.
"""
import datetime
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import restart_helpers as rh  # noqa: E402
from helpers import build_emu, build_emu_f32  # noqa: E402
from restart_helpers import FIELDS, N, NZ, PTOP, RESTART  # noqa: E402

TIME = datetime.datetime(2016, 8, 1, 0, 30)


@pytest.fixture(scope="module")
def emu_lib():
    from pace_amd import _lib

    return _lib.Library(build_emu())


@pytest.fixture(scope="module")
def emu_lib_f32():
    from pace_amd import _lib

    return _lib.Library(build_emu_f32())


@pytest.fixture
def clean_checks():
    from pace_amd.driver import SafetyChecker

    saved = dict(SafetyChecker.checks)
    SafetyChecker.clear_all_checks()
    yield SafetyChecker
    SafetyChecker.clear_all_checks()
    SafetyChecker.checks.update(saved)


# ---- 1. the reader (host only) --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", range(6))
def test_open_restart_is_the_files(tile):
    from pace_amd.util import open_restart

    state = open_restart(RESTART, rh.HostCommunicator(tile))
    assert state["time"] == TIME
    for field, (name, _, _, dims, units) in FIELDS.items():
        got, want = state[name], rh.tile_array(tile, field)
        assert want.dtype == np.dtype(">f8")
        assert got.data.dtype == np.float64 and got.data.dtype.isnative and got.data.flags.c_contiguous, field
        assert got.data.shape == want.shape and np.array_equal(got.data.view(np.uint64), want.astype("=f8").view(np.uint64)), field
        assert tuple(got.dims) == dims and got.units == units, field
    # the surface winds of fv_srf_wnd are variables too; the axes and Time are not
    assert {"eastward_wind_at_surface", "northward_wind_at_surface"} <= set(state)
    assert len(state) == len(FIELDS) + 2 + 1


def test_open_restart_only_names_label_and_errors(tmp_path):
    import shutil

    from pace_amd.util import open_restart

    comm = rh.HostCommunicator(4)
    state = open_restart(RESTART, comm, only_names=["air_temperature", "specific_humidity"])
    assert sorted(state) == ["air_temperature", "specific_humidity"]
    state = open_restart(RESTART, comm, only_names=["time", "x_wind"])
    assert sorted(state) == ["time", "x_wind"] and state["time"] == TIME
    with pytest.raises(ValueError, match="no restart files found at "):
        open_restart(str(tmp_path / "nowhere"), comm)
    with pytest.raises(ValueError, match="no restart files found at "):
        open_restart(RESTART, comm, label="20160801.003000")
    # a labelled copy of one tile's files; fv_srf_wnd is optional
    for kind in ("fv_core.res", "fv_tracer.res"):
        shutil.copy(os.path.join(RESTART, f"{kind}.tile5.nc"), tmp_path / f"later.{kind}.tile5.nc")
    with open(tmp_path / "later.coupler.res", "w") as f:
        f.write("     2        (Calendar)\n  2016     8     1     0     0     0        Model start time\n"
                "  2016     8     3    12     5     9        Current model time\n")
    state = open_restart(str(tmp_path), comm, label="later")
    assert state["time"] == datetime.datetime(2016, 8, 3, 12, 5, 9) and len(state) == len(FIELDS) + 1
    assert np.array_equal(state["vertical_wind"].data, rh.tile_array(4, "w"))


def test_open_restart_reads_a_synthetic_float32_restart(tmp_path):
    """A restart written here with scipy at n = 4, nz = 3, every variable >f4, with a label: it reads back exactly."""
    import scipy.io

    from pace_amd.util import open_restart

    n, nz = 4, 3
    rng = np.random.default_rng(3)
    written = {}
    for kind, variables in (("fv_core.res", ("u", "v", "W", "DZ", "T", "delp", "phis")), ("fv_tracer.res", ("sphum", "cld_amt", "dust"))):
        with scipy.io.netcdf_file(str(tmp_path / f"syn.{kind}.tile2.nc"), "w", version=2) as nc:
            for name, size in (("Time", None), ("xaxis_1", n), ("xaxis_2", n + 1), ("yaxis_1", n + 1), ("yaxis_2", n), ("zaxis_1", nz)):
                nc.createDimension(name, size)
            for name in variables:
                dims = {"u": ("Time", "zaxis_1", "yaxis_1", "xaxis_1"), "v": ("Time", "zaxis_1", "yaxis_2", "xaxis_2"),
                        "phis": ("Time", "yaxis_2", "xaxis_1")}.get(name, ("Time", "zaxis_1", "yaxis_2", "xaxis_1"))
                var = nc.createVariable(name, ">f4", dims)
                shape = tuple({"xaxis_1": n, "xaxis_2": n + 1, "yaxis_1": n + 1, "yaxis_2": n, "zaxis_1": nz}[d] for d in dims[1:])
                written[name] = rng.standard_normal(shape).astype(np.float32)
                var[0] = written[name]
    state = open_restart(str(tmp_path), rh.HostCommunicator(1), label="syn")
    names = {"u": "x_wind", "v": "y_wind", "W": "vertical_wind", "DZ": "vertical_thickness_of_atmospheric_layer", "T": "air_temperature",
             "delp": "pressure_thickness_of_atmospheric_layer", "phis": "surface_geopotential", "sphum": "specific_humidity",
             "cld_amt": "cloud_fraction"}
    assert sorted(state) == sorted(names.values())  # (no coupler.res: no time; dust has no entry in the table: dropped)
    # ... unless tracer_properties gives it one
    extra = {"dust_mixing_ratio": {"restart_name": "dust", "dims": ["z", "y", "x"], "units": "kg/kg"}}
    state = open_restart(str(tmp_path), rh.HostCommunicator(1), label="syn", tracer_properties=extra)
    assert sorted(state) == sorted(list(names.values()) + ["dust_mixing_ratio"])
    assert np.array_equal(state["dust_mixing_ratio"].data, written["dust"].astype(np.float64)) and state["dust_mixing_ratio"].units == "kg/kg"
    for restart_name, name in names.items():
        got = state[name].data
        assert got.dtype == np.float64 and got.dtype.isnative
        assert np.array_equal(got, written[restart_name].astype(np.float64)), restart_name
    assert state["x_wind"].data.shape == (nz, n + 1, n) and state["surface_geopotential"].data.shape == (n, n)


def test_an_hdf5_file_is_named_with_its_format(tmp_path):
    from pace_amd.util import open_restart

    for kind in ("fv_core.res", "fv_tracer.res"):
        with open(tmp_path / f"{kind}.tile1.nc", "wb") as f:
            f.write(b"\x89HDF\r\n\x1a\n" + b"\0" * 64)
    for reader in ("xarray", "netCDF4", "h5py"):
        try:
            __import__(reader)
        except ImportError:
            continue
        return  # (a reader of NetCDF-4 is installed: the refusal below does not apply)
    with pytest.raises(ValueError, match=r"fv_core\.res\.tile1\.nc is a NetCDF-4 / HDF5 file"):
        open_restart(str(tmp_path), rh.HostCommunicator(0))


# ---- 3. the state -----------------------------------------------------------------------------------------------------------------
class CountingLib:
    """A library whose entry-point calls are counted (tests/test_geos_wrapper.py)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def call(self, name, *args):
        self.calls.append(name)
        return self._lib.call(name, *args)


def check_state(lib, device, tile, monkeypatch):
    import dataclasses

    from pace_amd.fv3core import DycoreState
    from pace_amd.util import NullComm, restart

    counting = CountingLib(lib)
    communicator = rh.communicator_of(NullComm(rank=tile, total_ranks=6, fill_value=0.0), counting, device)
    qf = rh.factory(lib, device, N, NZ)
    h2d, to_device = [], restart._to_device

    def counted_to_device(staging, staged):
        h2d.append(staging.numel())
        to_device(staging, staged)

    monkeypatch.setattr(restart, "_to_device", counted_to_device)
    state = DycoreState.from_fortran_restart(quantity_factory=qf, communicator=communicator, path=RESTART)
    rh.sync(device)
    assert counting.calls == ["pace_state_unpack"]
    assert h2d == [sum(rh.tile_array(tile, field).size for field in FIELDS)]
    real = np.float32 if lib.real_bytes == 4 else np.float64
    want = rh.expected_bases(tile, real)
    assert sorted(f.name for f in dataclasses.fields(state)) == sorted(want)
    for name, expected in want.items():
        got = rh.base_of(getattr(state, name))
        assert got.dtype == real and got.shape == expected.shape, name
        assert np.array_equal(got, expected), name
    assert np.abs(want["delp"]).max() > 1000 and np.abs(want["u"]).max() > 10  # (a real atmosphere, not zeros against zeros)


@pytest.mark.parametrize("tile", [0, 3])
def test_from_fortran_restart_emulated(emu_lib, emu_lib_f32, tile, monkeypatch):
    check_state(emu_lib, "cpu", tile, monkeypatch)
    check_state(emu_lib_f32, "cpu", tile, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [0, 3])
def test_from_fortran_restart_gpu(tile, monkeypatch):
    from pace_amd import _lib

    check_state(_lib.load(), "cuda", tile, monkeypatch)
    check_state(_lib.load(32), "cuda", tile, monkeypatch)


# ---- 4. the configuration ---------------------------------------------------------------------------------------------------------
def test_the_configuration_loads():
    from pace_amd.driver import DriverConfig, FortranRestartInit

    config = DriverConfig.from_yaml(rh.YAML)  # (its paths are relative to the repository's root: nothing is read yet)
    assert config.initialization.type == "fortran_restart" and isinstance(config.initialization.config, FortranRestartInit)
    assert config.initialization.config.path == "tests/golden/c12_restart"
    assert config.grid_config.config.restart_path == "tests/golden/c12_restart"
    assert (config.nx_tile, config.nz, config.layout, config.dt_atmos, config.n_timesteps()) == (12, 63, (1, 1), 225.0, 4)
    assert config.diagnostics_config.path is None
    config = DriverConfig.from_dict(rh.settings())
    assert config.start_time == TIME
    assert FortranRestartInit().path == "."


def file_vertical_grid():
    path = os.path.join(RESTART, "fv_core.res.nc")
    return rh.file_array(path, "ak").astype(float), rh.file_array(path, "bk").astype(float)


def check_start(tiles, lib):
    ak, bk = file_vertical_grid()
    assert ak.shape == bk.shape == (64,)
    p_interface = ak + bk * 1e5
    for tile, t in enumerate(tiles):
        assert np.array_equal(t["ak"], ak) and np.array_equal(t["bk"], bk)
        assert t["ptop"] == PTOP and t["p_ref"] == 1e5 and t["time"] == TIME
        assert np.array_equal(t["p"], (p_interface[1:] - p_interface[:-1]) / np.log(p_interface[1:] / p_interface[:-1]))
        assert np.array_equal(t["dp_ref"], ak[1:] - ak[:-1] + (bk[1:] - bk[:-1]) * 1e5)
        assert t["tendencies"] == 0.0 and t["physics"]
        want = rh.expected_bases(tile)
        # the kernel's pe / peln of that delp: by a call of its own on the same storage values
        pe, peln, _ = rh.run_pe_peln(lib, "cpu" if "emulation" in lib.version() else "cuda", N, NZ, want["delp"][:, :, :N + 7], PTOP)
        want["pe"], want["peln"] = pe, peln
        assert np.array_equal(pe[:, :, :N + 7], rh.pe_restatement(want["delp"], PTOP, N, NZ))
        pe[:, :, N + 7:], peln[:, :, N + 7:] = 0.0, 0.0  # (run_pe_peln's sentinel; the driver's fields start as zeros)
        for name, expected in want.items():
            assert np.array_equal(t["bases"][name], expected), (tile, name)


def test_six_drivers_start_from_the_restart_emulated(emu_lib, clean_checks):
    check_start(rh.drivers_at_start(emu_lib, "cpu"), emu_lib)


@pytest.mark.gpu
def test_six_drivers_start_from_the_restart_gpu(tmp_path):
    from pace_amd import _lib

    check_start(rh.run_in_child("start", tmp_path), _lib.load())


def write_vertical_grid(directory, ak, bk):
    import scipy.io

    with scipy.io.netcdf_file(os.path.join(str(directory), "fv_core.res.nc"), "w", version=2) as nc:
        nc.createDimension("Time", None)
        nc.createDimension("xaxis_1", len(ak))
        for name, values in (("ak", ak), ("bk", bk)):
            var = nc.createVariable(name, ">f8", ("Time", "xaxis_1"))
            var[0] = values


def test_a_vertical_grid_that_does_not_fit_is_refused(emu_lib, tmp_path):
    from pace_amd.driver import Driver, DriverConfig
    from pace_amd.util import NullComm

    comm = NullComm(rank=0, total_ranks=6, fill_value=0.0)
    # the restart has 64 interfaces, nz: 79 needs 80
    config = DriverConfig.from_dict(rh.settings(nz=79, stencil_config={}))
    with pytest.raises(ValueError, match=r"64.*80"):
        Driver(config, comm=comm, lib=emu_lib)
    # bk[0] != 0: ptop is not defined
    ak, bk = file_vertical_grid()
    bk = bk.copy()
    bk[0] = 1.0e-3
    write_vertical_grid(tmp_path, ak, bk)
    d = rh.settings(stencil_config={})
    d["grid_config"]["config"]["restart_path"] = str(tmp_path)
    with pytest.raises(ValueError, match="ptop is not well-defined when top-of-atmosphere bk != 0"):
        Driver(DriverConfig.from_dict(d), comm=comm, lib=emu_lib)
    # a directory without fv_core.res.nc
    d["grid_config"]["config"]["restart_path"] = str(tmp_path / "nowhere")
    os.makedirs(tmp_path / "nowhere")
    with pytest.raises(ValueError, match="no fv_core.res.nc"):
        Driver(DriverConfig.from_dict(d), comm=comm, lib=emu_lib)


def test_the_vertical_grid_is_set_before_the_kernels_see_the_grid(emu_lib):
    from pace_amd.driver.config import GeneratedGridConfig
    from pace_amd.util import NullComm

    communicator = rh.communicator_of(NullComm(rank=0, total_ranks=6, fill_value=0.0), emu_lib, "cpu")
    _, _, grid = GeneratedGridConfig(restart_path=RESTART).get_grid(quantity_factory=rh.factory(emu_lib, "cpu", N, NZ),
                                                                    communicator=communicator)
    assert grid._struct is None and grid.ptop == PTOP
    grid.c_struct()
    with pytest.raises(RuntimeError, match="already in use"):
        grid.set_vertical_grid(*file_vertical_grid())


# ---- 5. the run -------------------------------------------------------------------------------------------------------------------
def check_run(result):
    different, not_finite, facts, nfields, moved, winds = result
    assert nfields == 32 + 3 + 10
    assert different == [], different[:10]
    assert not_finite == [], not_finite[:10]
    for f in facts:
        # (two checks of the state by SafetyChecker inside the loop, none of which raised)
        assert f["elapsed"] == 2 * rh.DT and f["start"] == TIME and f["checks"] == 2
    assert len(moved) == 10, moved  # the physics ran
    assert 20.0 < winds < 200.0  # the A-grid winds of the compute domains, zero in the restart's state, were computed by the step


def test_two_steps_from_the_restart_are_the_stages_emulated(emu_lib, clean_checks):
    check_run(rh.loop_against_stages(emu_lib, "cpu"))


@pytest.mark.gpu
def test_two_steps_from_the_restart_are_the_stages_gpu(tmp_path):
    check_run(rh.run_in_child("run", tmp_path))
