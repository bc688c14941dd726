"""The lat-lon diagnostics through the public interface: CubedSphereCommunicator.regrid_state, MonitorDiagnostics with `latlon`,
the monitors' files and a run_cube_driver run.

* regrid_state under run_cube at C12 x 7 equals the numpy restatement (tests/latlon_reference.py) applied to gather_state's
  arrays, bit for bit, in float64 and narrowed to float32; a store is ONE pace_cube_regrid launch and ONE transfer, and over
  three stores the point table and the item table are uploaded once;
* MonitorDiagnostics with `latlon`: names, dims and units of `<name>_ll` and `<name>_z<k>_ll`, lon_ll and lat_ll from store_grid,
  npz and NetCDF files with the dimensions [time, lon, lat(, z)] and no tile axis, read back and compared with the restatement;
* refusals: staggered and interface variables, a per-rank communicator (naming run_cube_driver), an unknown key under `latlon`;
* run_cube_driver on tests/golden/driver_baroclinic_c12.yaml with comm_config.type: cube and a `latlon` block for two steps:
  the lat-lon files exist and are finite, the initial delp (horizontally constant in this initial state: the surface pressure
  is) comes back constant per level, and every other file of the run equals that of a run without `latlon`, byte for byte.

Every check is a function of the device; the CPU tier runs the emulation library, the GPU tier a child process with a time
limit."""
import collections
import datetime
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import latlon_reference  # noqa: E402
import test_driver  # noqa: E402
from helpers import ROOT, build_emu  # noqa: E402
from test_driver import clean_checks  # noqa: E402,F401

N, NZ, H = 12, 7, 3
X, Y, Z, XI, YI, ZI = "x", "y", "z", "x_interface", "y_interface", "z_interface"
GRID = (24, 12)


def _lib(device):
    from pace_amd import _lib

    return _lib.Library(build_emu()) if device == "cpu" else _lib.load()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


class CountingLib:
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def call(self, name, *args):
        self.calls.append(name)
        return self._lib.call(name, *args)


def field_values(rank, which, step=0):
    """The whole storage [i, j, k] of field `which` on `rank` at `step`."""
    return np.random.default_rng(1000 * rank + 10 * which + step).random((N + 7, N + 7, NZ + 1)) + rank


def host_table(grid=GRID, n=N):
    from pace_amd.util import gridgen, latlon

    t = gridgen.tiles(n, NZ)
    lon = np.stack([x["lon_agrid"][H:H + n, H:H + n] for x in t])
    lat = np.stack([x["lat_agrid"][H:H + n, H:H + n] for x in t])
    return latlon.build_regrid_table(lon, lat, *latlon.LatLonGrid(*grid).targets())


def restated(gathered, table, dtype, grid=GRID):
    """The restatement applied to a gathered [6, n, n(, nk)] array (compute domains: the table's indices less the halo)."""
    out = latlon_reference.regrid(list(gathered), table.tile, table.i - H, table.j - H, table.w, dense_dtype=dtype)
    return out.reshape(grid + out.shape[1:])


def make_state(qf, rank, step=0):
    """A driver state's shape: dycore_state, physics_state, no grid_data (the communicator generates the cell centres)."""
    def q(which, dims, units):
        a = field_values(rank, which, step)
        return qf.from_array(a if len(dims) == 3 else a[:, :, 0], dims, units)

    dycore = types.SimpleNamespace(pt=q(0, [X, Y, Z], "degK"), ua=q(1, [X, Y, Z], "m/s"), phis=q(2, [X, Y], "m^2 s^-2"),
                                   u=q(3, [X, YI, Z], "m/s"), pe=q(4, [X, Y, ZI], "Pa"))
    physics = types.SimpleNamespace(prsi=q(5, [X, Y, ZI], "Pa"), physics_updated_pt=q(6, [X, Y, Z], "degK"))
    return types.SimpleNamespace(dycore_state=dycore, physics_state=physics)


# ---- regrid_state ---------------------------------------------------------------------------------------------------------------
def check_regrid_state(device):
    import torch

    from pace_amd import _launch
    from pace_amd.util import (LAT_DIM, LON_DIM, CubedSphereCommunicator, LatLonGrid, QuantityFactory, SubtileGridSizer, Window,
                               gather, run_cube)

    from pace_amd import _lib as binding

    lib = CountingLib(_lib(device))
    uploads, transfers = [], []
    real_upload, real_to_host = _launch.upload_table, gather.GatherScatter._rg_to_host

    def counted_upload(arr, dev):
        uploads.append(len(arr))
        return real_upload(arr, dev)

    def counted_to_host(dense, host):
        transfers.append(dense.numel())
        return real_to_host(dense, host)

    grid = LatLonGrid(*GRID)

    def program(comm):
        qf = QuantityFactory(SubtileGridSizer(N, N, NZ), device, torch.float64)
        cube = CubedSphereCommunicator(comm, device=device, lib=lib)
        s = make_state(qf, cube.rank).dycore_state
        pt = s.pt
        windows = {"time": 7, "pt_ll": pt, "phis_ll": s.phis,
                   "pt_z3_ll": Window(pt, binding.DIAG_PLANE, 3, _launch.window_of(pt, 3)[2:], pt.dims[:2], pt.units),
                   "ua_k2_ll": Window(s.ua, binding.DIAG_WINDOW3D, None, (H, H, 2, N, N, 4), s.ua.dims, s.ua.units)}
        seen = {}
        for step, transfer_type in enumerate((None, np.float32, np.float32)):
            got = cube.regrid_state(windows, grid, transfer_type)
            if cube.rank != 0:
                assert got is None
                continue
            assert list(got) == list(windows) and got["time"] == 7
            assert got["pt_ll"].dims == (LON_DIM, LAT_DIM, Z) and got["pt_ll"].extent == GRID + (NZ,) and got["pt_ll"].units == "degK"
            assert got["phis_ll"].dims == (LON_DIM, LAT_DIM) == got["pt_z3_ll"].dims and got["ua_k2_ll"].extent == GRID + (4,)
            assert all(isinstance(got[k].data, np.ndarray) and got[k].data.dtype == (transfer_type or np.float64) for k in windows if k != "time")
            seen[step] = {k: got[k].data.copy() for k in windows if k != "time"}
        whole = cube.gather_state({"pt": pt, "phis": s.phis, "ua": s.ua})
        with pytest.raises(ValueError, match=r"u_ll has dimensions \('x', 'y_interface', 'z'\)"):
            cube.regrid_state({"u_ll": s.u}, grid)
        with pytest.raises(ValueError, match="pe_ll has dimensions"):
            cube.regrid_state({"pe_ll": s.pe}, grid)
        if cube.rank == 0:
            seen["gathered"] = {k: whole[k].data.copy() for k in ("pt", "phis", "ua")}
        return seen

    _launch.upload_table, gather.GatherScatter._rg_to_host = counted_upload, staticmethod(counted_to_host)
    try:
        seen = run_cube(program)[0]
    finally:
        _launch.upload_table, gather.GatherScatter._rg_to_host = real_upload, staticmethod(real_to_host)
    calls = collections.Counter(lib.calls)
    npoints = GRID[0] * GRID[1]
    # three stores: one launch and one transfer each; the point table and the item table (4 items) uploaded once
    assert calls["pace_cube_regrid"] == 3 and calls["pace_cube_gather"] == 1, calls
    assert transfers == [npoints * (NZ + 1 + 1 + 4)] * 3, transfers
    assert sorted(uploads[:2]) == sorted([64 * npoints, (72 * 4 + 4 * 5 + 7) // 8 * 8]), uploads
    assert uploads[2:] == [(48 * 18 + 4 * 19 + 7) // 8 * 8], uploads  # (gather_state's; the tables do not depend on the dense type)
    table, g = host_table(), seen["gathered"]
    for step, dtype in ((0, np.float64), (1, np.float32), (2, np.float32)):
        want = {"pt_ll": restated(g["pt"], table, dtype), "phis_ll": restated(g["phis"], table, dtype),
                "pt_z3_ll": restated(g["pt"][..., 3], table, dtype), "ua_k2_ll": restated(g["ua"][..., 2:6], table, dtype)}
        for name in want:
            assert np.array_equal(_bits(seen[step][name]), _bits(want[name])), (step, name)


def check_per_rank_refusals(device):
    import torch

    from pace_amd.driver import DiagnosticsConfig, LatLonSelect, MonitorDiagnostics
    from pace_amd.util import CubedSphereCommunicator, LatLonGrid, NullComm, QuantityFactory, SubtileGridSizer, run_tiles

    lib = _lib(device)
    qf = QuantityFactory(SubtileGridSizer(N, N, NZ), device, torch.float64)
    cube = CubedSphereCommunicator(NullComm(0, 6), device=device, lib=lib)
    with pytest.raises(ValueError, match="run_cube"):
        cube.regrid_state({"pt_ll": make_state(qf, 0).dycore_state.pt}, LatLonGrid(*GRID))
    config = DiagnosticsConfig.from_dict({"path": "unused", "output_format": "npz", "latlon": {"nlon": 24, "nlat": 12, "names": ["pt"]}})
    with pytest.raises(ValueError, match=r"comm_config.type: cube.*run_cube_driver"):
        config.diagnostics_factory(cube, lib=lib)
    with pytest.raises(ValueError, match="run_cube_driver"):
        MonitorDiagnostics(object(), [], [], [], lib=lib, latlon=LatLonSelect(24, 12, ["pt"]))

    def program(comm):  # six threads with per-rank communicators: refused as well
        with pytest.raises(ValueError, match="run_cube_driver"):
            config.diagnostics_factory(CubedSphereCommunicator(comm, device=device, lib=lib), lib=lib)

    run_tiles(6, program)


def test_parsing():
    from pace_amd.driver import DiagnosticsConfig, DriverConfig, LatLonSelect

    config = DiagnosticsConfig.from_dict({"path": "out", "output_format": "npz",
                                          "latlon": {"nlon": 360, "nlat": 180, "names": ["pt", "phis"], "levels": [65, 78]}})
    assert config.latlon == LatLonSelect(360, 180, ["pt", "phis"], [65, 78]) and config.latlon.grid().npoints == 64800
    assert DiagnosticsConfig.from_dict({"path": "out"}).latlon is None
    with pytest.raises(ValueError, match="diagnostics_config.latlon has no setting 'nlong'"):
        DiagnosticsConfig.from_dict({"path": "out", "latlon": {"nlong": 360, "nlat": 180, "names": ["pt"]}})
    with pytest.raises(ValueError, match="diagnostics_config.latlon.nlon"):
        DiagnosticsConfig.from_dict({"path": "out", "latlon": {"nlon": "many", "nlat": 180, "names": ["pt"]}})
    with pytest.raises(ValueError, match="at least one point"):
        DiagnosticsConfig.from_dict({"path": "out", "latlon": {"nlon": 0, "nlat": 180, "names": ["pt"]}})
    with pytest.raises(ValueError, match="path must be given"):
        DiagnosticsConfig.from_dict({"latlon": {"nlon": 4, "nlat": 2, "names": ["pt"]}})
    whole = test_driver.settings(comm_config={"type": "cube"})
    whole["diagnostics_config"] = dict(whole["diagnostics_config"], latlon={"nlon": 24, "nlat": 12, "names": ["pt"]})
    assert DriverConfig.from_dict(whole).diagnostics_config.latlon.names == ["pt"]


# ---- MonitorDiagnostics ---------------------------------------------------------------------------------------------------------
class RecordingMonitor:
    def __init__(self):
        self.stored, self.constants = [], []

    def store(self, state):
        self.stored.append({k: (v if k == "time" else (tuple(v.dims), v.units, np.array(v.view[:]))) for k, v in state.items()})

    def store_constant(self, state):
        self.constants.append({k: (tuple(v.dims), v.units, np.array(v.view[:])) for k, v in state.items()})

    def cleanup(self):
        pass


def check_monitor_diagnostics(device, tmp):
    import torch
    from scipy.io import netcdf_file

    from pace_amd.driver import DiagnosticsConfig, LatLonSelect, MonitorDiagnostics, ZSelect
    from pace_amd.util import CubedSphereCommunicator, LatLonGrid, QuantityFactory, SubtileGridSizer, gridgen, run_cube

    lib = _lib(device)
    recorder = RecordingMonitor()
    select = {"nlon": GRID[0], "nlat": GRID[1], "names": ["pt", "phis", "physics_updated_pt"]}
    stamps = [datetime.datetime(2000, 1, 1) + datetime.timedelta(seconds=225 * step) for step in range(3)]

    def program(comm):
        qf = QuantityFactory(SubtileGridSizer(N, N, NZ), device, torch.float64)
        cube = CubedSphereCommunicator(comm, device=device, lib=lib)
        terms = gridgen.tiles(N, NZ)[cube.rank]
        grid_data = types.SimpleNamespace(**{name: terms[name] for name in ("lat", "lon", "lon_agrid", "lat_agrid")})
        diags = [MonitorDiagnostics(recorder, ["pt"], [], [ZSelect(3, ["pt"])], lib=lib, communicator=cube,
                                    latlon=LatLonSelect(GRID[0], GRID[1], ["pt", "phis", "physics_updated_pt"], levels=[0, 5]))]
        for fmt in ("npz", "netcdf"):
            config = DiagnosticsConfig.from_dict({"path": os.path.join(tmp, fmt), "output_format": fmt, "time_chunk_size": 2,
                                                  "names": ["pt"], "latlon": select})
            diags.append(config.diagnostics_factory(cube, lib=lib))
        for bad in ("u", "pe", "prsi"):  # staggered, interface (dycore), interface (physics)
            refused = MonitorDiagnostics(recorder, [], [], [], lib=lib, communicator=cube, latlon=LatLonSelect(4, 2, ["pt", bad]))
            with pytest.raises(ValueError, match=f"{bad} has dimension"):
                refused.store(stamps[0], make_state(qf, cube.rank))
        with pytest.raises(ValueError, match="Invalid state variable nothing"):
            MonitorDiagnostics(recorder, [], [], [], lib=lib, communicator=cube, latlon=LatLonSelect(4, 2, ["nothing"])).store(
                stamps[0], make_state(qf, cube.rank))
        for step, time in enumerate(stamps):
            state = make_state(qf, cube.rank, step)
            state.grid_data = grid_data
            for diag in diags:
                diag.store(time, state)
        for diag in diags:
            diag.store_grid(grid_data)
            diag.cleanup()

    run_cube(program)
    table = host_table()
    grid = LatLonGrid(*GRID)

    def want(which, step, level=None):
        g = np.stack([field_values(r, which, step)[H:H + N, H:H + N, :NZ] for r in range(6)])
        return restated(g[..., 0] if which == 2 else g if level is None else g[..., level], table, np.float32)

    # what the monitor is handed: names, dims, units, values
    assert len(recorder.stored) == 3
    for step, stored in enumerate(recorder.stored):
        assert list(stored) == ["time", "pt", "pt_z3", "pt_z0_ll", "pt_z5_ll", "phis_ll", "physics_updated_pt_z0_ll", "physics_updated_pt_z5_ll"]
        assert stored["pt"][0] == ("tile", X, Y, Z) and stored["pt_z3"][0] == ("tile", X, Y)
        for name, which, level, units in (("pt_z0_ll", 0, 0, "degK"), ("pt_z5_ll", 0, 5, "degK"), ("phis_ll", 2, None, "m^2 s^-2"),
                                          ("physics_updated_pt_z5_ll", 6, 5, "degK")):
            dims, got_units, data = stored[name]
            assert dims == ("lon", "lat") and got_units == units and data.dtype == np.float32 and data.shape == GRID
            assert np.array_equal(_bits(data), _bits(want(which, step, level))), (step, name)
    constants = {k: v for const in recorder.constants for k, v in const.items()}
    assert constants["lon_ll"][0] == ("lon",) and constants["lat_ll"][0] == ("lat",) and constants["lon_ll"][1] == "radians"
    assert np.array_equal(constants["lon_ll"][2], grid.lon) and np.array_equal(constants["lat_ll"][2], grid.lat)
    assert constants["lon_agrid"][0][0] == "tile"
    # the files: [time, lon, lat(, z)], no tile axis, in files of their own
    names = ("pt_ll", "phis_ll", "physics_updated_pt_ll")
    out = os.path.join(tmp, "npz")
    assert sorted(f for f in os.listdir(out) if "ll" in f or "latlon" in f) == ["constants_lat_ll.npz", "constants_lon_ll.npz",
                                                                               "latlon_0000.npz", "latlon_0001.npz"]
    chunks = [np.load(os.path.join(out, f"latlon_{chunk:04d}.npz")) for chunk in range(2)]
    meta = json.loads(str(chunks[0]["__meta__"]))
    assert sorted(chunks[0].files) == sorted(names + ("time", "__meta__"))
    assert meta["pt_ll"] == {"dims": ["time", "lon", "lat", "z"], "units": "degK"} and meta["phis_ll"]["dims"] == ["time", "lon", "lat"]
    assert list(np.concatenate([d["time"] for d in chunks])) == [np.datetime64(s, "us") for s in stamps]
    series = {name: np.concatenate([d[name] for d in chunks]) for name in names}
    d = np.load(os.path.join(out, "constants_lon_ll.npz"))
    assert np.array_equal(d["lon_ll"], grid.lon) and json.loads(str(d["__meta__"]))["lon_ll"] == {"dims": ["lon"], "units": "radians"}
    assert np.array_equal(np.load(os.path.join(out, "constants_lat_ll.npz"))["lat_ll"], grid.lat)
    assert "pt_ll" not in np.load(os.path.join(out, "state_0000_tile0.npz")).files
    out = os.path.join(tmp, "netcdf")
    assert sorted(f for f in os.listdir(out) if "ll" in f or "latlon" in f) == ["constants_lat_ll.nc", "constants_lon_ll.nc",
                                                                               "latlon_0000.nc", "latlon_0001.nc"]
    files = [netcdf_file(os.path.join(out, f"latlon_{chunk:04d}.nc"), "r", mmap=False) for chunk in range(2)]
    assert "tile" not in files[0].dimensions and files[0].dimensions["lon"] == GRID[0] and files[0].dimensions["lat"] == GRID[1]
    assert files[0].variables["pt_ll"].dimensions == ("time", "lon", "lat", "z") and files[0].variables["pt_ll"].units == b"degK"
    assert files[0].variables["phis_ll"].dimensions == ("time", "lon", "lat")
    series_nc = {name: np.concatenate([f.variables[name][:].copy() for f in files]).astype(np.float32) for name in names}
    for f in files:
        f.close()
    with netcdf_file(os.path.join(out, "constants_lat_ll.nc"), "r", mmap=False) as f:
        assert f.variables["lat_ll"].dimensions == ("lat",) and np.array_equal(f.variables["lat_ll"][:], grid.lat)
    for name, which in zip(names, (0, 2, 6)):
        expect = np.stack([want(which, step) for step in range(3)])
        assert series[name].shape == (3,) + GRID + ((NZ,) if which != 2 else ()) and series[name].dtype == np.float32
        assert np.array_equal(_bits(series[name]), _bits(expect)) and np.array_equal(_bits(series_nc[name]), _bits(expect)), name


# ---- the driver -------------------------------------------------------------------------------------------------------------------
def driver_settings(path, latlon):
    base = test_driver.settings()
    diagnostics = dict(base["diagnostics_config"], path=str(path), output_format="npz", time_chunk_size=2)
    if latlon:
        diagnostics["latlon"] = {"nlon": GRID[0], "nlat": GRID[1], "names": ["delp", "pt", "phis"]}
    return test_driver.settings(dycore_only=True, diagnostics_config=diagnostics, output_initial_state=True, stencil_config={},
                                comm_config={"type": "cube"}, days=0, hours=0, minutes=0, seconds=225 * 2)


def check_driver(device, tmp):
    from pace_amd.driver import DriverConfig, run_cube_driver

    lib = _lib(device)
    calls = {}
    for latlon in (False, True):
        counting = CountingLib(lib)
        run_cube_driver(DriverConfig.from_dict(driver_settings(os.path.join(tmp, str(latlon)), latlon)), device=device, lib=counting)
        calls[latlon] = collections.Counter(counting.calls)
    assert calls[True]["pace_cube_regrid"] == 3 and calls[False]["pace_cube_regrid"] == 0  # the initial state and two steps
    assert calls[True] - collections.Counter(pace_cube_regrid=3) == calls[False]  # nothing else changes
    plain, with_ll = os.path.join(tmp, "False"), os.path.join(tmp, "True")
    extra = ["constants_lat_ll.npz", "constants_lon_ll.npz", "latlon_0000.npz", "latlon_0001.npz"]
    assert sorted(os.listdir(with_ll)) == sorted(os.listdir(plain) + extra)
    for name in os.listdir(plain):  # byte for byte
        assert open(os.path.join(plain, name), "rb").read() == open(os.path.join(with_ll, name), "rb").read(), name
    chunks = [np.load(os.path.join(with_ll, f"latlon_{chunk:04d}.npz")) for chunk in range(2)]
    series = {name: np.concatenate([d[name] for d in chunks]) for name in ("delp_ll", "pt_ll", "phis_ll")}
    assert series["delp_ll"].shape == (3,) + GRID + (79,) and series["phis_ll"].shape == (3,) + GRID
    assert all(np.isfinite(a).all() and a.dtype == np.float32 for a in series.values())
    # the initial surface pressure is one number, so the initial delp is constant on every level: the weighted sum of equal
    # float64 values is within 2 ulp of them (the weights sum to 1 within 4e-16), and narrowing to float32 leaves at most two
    # neighbouring values
    first = series["delp_ll"][0].reshape(-1, 79)
    spread = first.max(axis=0) - first.min(axis=0)
    print("initial delp on the lat-lon grid: largest spread per level [float32 ulp]:", (spread / np.spacing(first.max(axis=0))).max())
    assert (spread <= np.spacing(first.max(axis=0))).all() and (first > 0).all()
    assert not np.array_equal(series["pt_ll"][0], series["pt_ll"][-1])


# ---- the tiers ------------------------------------------------------------------------------------------------------------------
def test_regrid_state_emulated():
    check_regrid_state("cpu")


def test_per_rank_refusals_emulated():
    check_per_rank_refusals("cpu")


def test_monitor_diagnostics_emulated(tmp_path):
    check_monitor_diagnostics("cpu", str(tmp_path))


def test_driver_run_emulated(clean_checks, tmp_path):  # noqa: F811
    check_driver("cpu", str(tmp_path))


def _in_child(call, timeout=300):
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); "
            f"import test_latlon_diagnostics; test_latlon_diagnostics.{call}")
    p = subprocess.run([sys.executable, "-X", "faulthandler", "-c", code], capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-6000:])


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["regrid_state", "per_rank_refusals", "monitor_diagnostics", "driver"])
def test_on_the_gpu(what, tmp_path):
    _in_child(f"check_{what}('cuda'" + (f", {str(tmp_path)!r})" if what in ("monitor_diagnostics", "driver") else ")"))
