"""Shared plumbing of tests/test_fortran_restart.py and tests/test_fortran_restart_kernel.py: the fixture restart
(tests/golden/c12_restart: the reference's own C12 x 63 test restart, copied unchanged) read with scipy, the expected state
restated with numpy, the pe / peln kernel's runner and numpy restatements, and the six-tile programs with their child runner."""
import copy
import ctypes as C
import dataclasses
import functools
import os
import pickle
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import GOLDEN, ROOT  # noqa: E402

RESTART = os.path.join(GOLDEN, "c12_restart")
YAML = os.path.join(GOLDEN, "driver_fortran_restart_c12.yaml")
N, NZ, DT = 12, 63, 225.0
PTOP = 64.247
X, Y, Z, XI, YI = "x", "y", "z", "x_interface", "y_interface"
# DycoreState field -> (standard name, file, variable, dims in file order, units): what dycore_state.py:361-427 fills
FIELDS = {
    "pt": ("air_temperature", "fv_core.res", "T", (Z, Y, X), "degK"),
    "delp": ("pressure_thickness_of_atmospheric_layer", "fv_core.res", "delp", (Z, Y, X), "Pa"),
    "phis": ("surface_geopotential", "fv_core.res", "phis", (Y, X), "m^2 s^-2"),
    "w": ("vertical_wind", "fv_core.res", "W", (Z, Y, X), "m/s"),
    "u": ("x_wind", "fv_core.res", "u", (Z, YI, X), "m/s"),
    "v": ("y_wind", "fv_core.res", "v", (Z, Y, XI), "m/s"),
    "qvapor": ("specific_humidity", "fv_tracer.res", "sphum", (Z, Y, X), "kg/kg"),
    "qliquid": ("cloud_liquid_water_mixing_ratio", "fv_tracer.res", "liq_wat", (Z, Y, X), "kg/kg"),
    "qice": ("cloud_ice_mixing_ratio", "fv_tracer.res", "ice_wat", (Z, Y, X), "kg/kg"),
    "qrain": ("rain_mixing_ratio", "fv_tracer.res", "rainwat", (Z, Y, X), "kg/kg"),
    "qsnow": ("snow_mixing_ratio", "fv_tracer.res", "snowwat", (Z, Y, X), "kg/kg"),
    "qgraupel": ("graupel_mixing_ratio", "fv_tracer.res", "graupel", (Z, Y, X), "kg/kg"),
    "qo3mr": ("ozone_mixing_ratio", "fv_tracer.res", "o3mr", (Z, Y, X), "kg/kg"),
    "qcld": ("cloud_fraction", "fv_tracer.res", "cld_amt", (Z, Y, X), ""),
    "delz": ("vertical_thickness_of_atmospheric_layer", "fv_core.res", "DZ", (Z, Y, X), "m"),
}
TENDENCIES = ("u_dt", "v_dt", "pt_dt")
UPDATED = ("physics_updated_specific_humidity", "physics_updated_qliquid", "physics_updated_qrain", "physics_updated_qice",
           "physics_updated_qsnow", "physics_updated_qgraupel", "physics_updated_cloud_fraction", "physics_updated_pt",
           "physics_updated_ua", "physics_updated_va")


# ---- the files, read here with scipy ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def file_array(path, variable):
    """var[0] of a NetCDF-3 file, in the file's own type and byte order."""
    import scipy.io

    with scipy.io.netcdf_file(path, "r", mmap=False) as nc:
        a = np.array(nc.variables[variable][0])
    a.setflags(write=False)
    return a


def tile_array(tile, field):
    _, kind, variable, _, _ = FIELDS[field]
    return file_array(os.path.join(RESTART, f"{kind}.tile{tile + 1}.nc"), variable)


class HostCommunicator:
    """What open_restart needs of a communicator to read into host variables: the rank and the partitioner."""

    def __init__(self, rank):
        from pace_amd.util import CubedSpherePartitioner

        self.rank, self.partitioner = rank, CubedSpherePartitioner()


def expected_bases(tile, real=np.float64, n=N, nz=NZ):
    """The raw storage [k][j][i] (row padding included) of all 32 DycoreState fields after from_fortran_restart: zeros, and the
    file's arrays -- whose (z, y, x) order is the storage's own -- in the compute windows."""
    from pace_amd.fv3core.initialization.dycore_state import _FIELDS
    from pace_amd.util.quantity import row_stride

    sj = row_stride(n + 7, np.dtype(real).itemsize)
    out = {}
    for name, (dims, _) in _FIELDS.items():
        out[name] = np.zeros((nz + 1, n + 7, sj) if len(dims) == 3 else (n + 7, sj), dtype=real)
    for name in FIELDS:
        a = tile_array(tile, name)
        if a.ndim == 3:
            out[name][:a.shape[0], 3:3 + a.shape[1], 3:3 + a.shape[2]] = a
        else:
            out[name][3:3 + a.shape[0], 3:3 + a.shape[1]] = a
    assert len(out) == 32
    return out


def base_of(quantity):
    return np.array(quantity._base.detach().cpu().numpy())


# ---- pace_pe_peln_from_delp ---------------------------------------------------------------------------------------------------
LOG_ULPS = 0.546 + 1.0  # lean_log's documented error (profiles/r06_transcendental_accuracy.txt) plus one ulp for numpy's log
SENTINEL = -12345.0


def factory(lib, device, n, nz):
    import torch

    from pace_amd.util import QuantityFactory, SubtileGridSizer

    sizer = SubtileGridSizer.from_tile_params(nx_tile=n, ny_tile=n, nz=nz, n_halo=3, extra_dim_lengths={}, layout=(1, 1))
    return QuantityFactory(sizer, device=device, dtype=torch.float32 if lib.real_bytes == 4 else torch.float64)


def stream_of(device):
    if str(device) == "cpu":
        return None
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_pe_peln(lib, device, n, nz, delp_zyx, ptop):
    """delp_zyx: (nz + 1, n + 7, n + 7) values of the whole storage, level nz included (it must not be read).  pe and peln
    start as a sentinel everywhere, the row padding included; delp's own padding is NaN.  -> the raw storages
    (pe, peln, delp as stored) as [k][j][sj] arrays."""
    import torch

    from pace_amd.util.grid import geom_struct

    qf = factory(lib, device, n, nz)
    dims = [X, Y, Z]
    delp, pe, peln = qf.zeros(dims, "Pa"), qf.zeros(dims, "Pa"), qf.zeros(dims, "ln(Pa)")
    delp._base[...] = float("nan")
    delp._base[:, :, :n + 7] = torch.as_tensor(np.ascontiguousarray(delp_zyx), dtype=delp._base.dtype, device=delp._base.device)
    pe._base[...] = SENTINEL
    peln._base[...] = SENTINEL
    lib.call("pace_pe_peln_from_delp", C.byref(geom_struct(qf)), delp.ptr, float(ptop), pe.ptr, peln.ptr, stream_of(device))
    if str(device) != "cpu":
        torch.cuda.synchronize()
    return base_of(pe), base_of(peln), base_of(delp)


def pe_restatement(delp_stored, ptop, n, nz):
    """ptop + concatenate(0, cumsum(delp[..., :nz])) in float64 over the (nz + 1, n + 7, n + 7) storage: numpy accumulates along
    the level axis one level after the other, the kernel's order."""
    d = delp_stored[:nz, :, :n + 7].astype(np.float64)
    return ptop + np.concatenate([np.zeros((1,) + d.shape[1:]), np.cumsum(d, axis=0)], axis=0)


def pe_reference_expression(delp_stored, ptop, n, nz):
    """initialization.py:436-437 word for word on an (x, y, z) array: pe[:, :, level] = ptop + np.sum(delp[:, :, :level], 2)."""
    delp = np.ascontiguousarray(delp_stored[:, :, :n + 7].astype(np.float64).transpose(2, 1, 0))
    pe = np.zeros((n + 7, n + 7, nz + 1))
    for level in range(nz + 1):
        pe[:, :, level] = ptop + np.sum(delp[:, :, :level], 2)
    return pe.transpose(2, 1, 0)


def fixture_delp_storage(tile=2, seed=7):
    """The fixture's delp of a tile in the compute window, random positive values planted in the halo, the stagger row and level
    nz (which is not part of the sum)."""
    rng = np.random.default_rng(seed)
    full = rng.uniform(50.0, 4000.0, size=(NZ + 1, N + 7, N + 7))
    full[:NZ, 3:3 + N, 3:3 + N] = tile_array(tile, "delp")
    return full


def synthetic_delp_storage(n, nz, seed):
    return np.random.default_rng(seed).uniform(50.0, 4000.0, size=(nz + 1, n + 7, n + 7))


# ---- six tiles ----------------------------------------------------------------------------------------------------------------
def settings(**over):
    import yaml

    with open(YAML) as f:
        d = yaml.safe_load(f)
    assert d["initialization"]["config"]["path"] == d["grid_config"]["config"]["restart_path"] == "tests/golden/c12_restart"
    d["initialization"]["config"]["path"] = RESTART
    d["grid_config"]["config"]["restart_path"] = RESTART
    d.update(over)
    return d


def sync(device):
    if str(device) != "cpu":
        import torch

        torch.cuda.synchronize()


def communicator_of(comm, lib, device):
    from pace_amd.util import CubedSphereCommunicator

    return CubedSphereCommunicator(comm, device=device, lib=lib)


def restart_state(lib, device, communicator, qf, ptop):
    """The state of item 3 plus the kernel's pe / peln, by hand."""
    from pace_amd.fv3core import DycoreState
    from pace_amd.util.grid import geom_struct

    state = DycoreState.from_fortran_restart(quantity_factory=qf, communicator=communicator, path=RESTART)
    lib.call("pace_pe_peln_from_delp", C.byref(geom_struct(qf)), state.delp.ptr, float(ptop), state.pe.ptr, state.peln.ptr,
             stream_of(device))
    return state


def drivers_at_start(lib, device):
    """Six Drivers on run_tiles; per tile what the configuration test asserts."""
    from pace_amd.driver import Driver, DriverConfig
    from pace_amd.util import run_tiles

    config = DriverConfig.from_dict(settings(stencil_config={}))

    def program(comm):
        driver = Driver(copy.deepcopy(config), comm=comm, lib=lib, device=device)
        sync(device)
        grid, state = driver.state.grid_data, driver.state.dycore_state
        bases = {f.name: base_of(getattr(state, f.name)) for f in dataclasses.fields(state)}
        tendencies = max(float(np.abs(getattr(driver.state.tendency_state, k).numpy()).max()) for k in TENDENCIES)
        return dict(ak=np.array(grid.ak), bk=np.array(grid.bk), ptop=grid.ptop, p=np.array(grid.p), dp_ref=np.array(grid.dp_ref),
                    p_ref=float(grid.p_ref), time=driver.time, bases=bases, tendencies=tendencies,
                    physics=driver.state.physics_state.microphysics is not None)

    return run_tiles(6, program)


def snapshot(state):
    """Every DycoreState field, the three tendencies and the physics_updated_* fields over the whole storage."""
    out = {"dycore." + f.name: np.array(getattr(state.dycore_state, f.name).numpy()) for f in dataclasses.fields(state.dycore_state)}
    out.update({"tendency." + k: np.array(getattr(state.tendency_state, k).numpy()) for k in TENDENCIES})
    for k in UPDATED:
        f = getattr(state.physics_state, k)
        out["physics." + k] = np.array(f.numpy() if hasattr(f, "dims") else f.detach().cpu().numpy())
    return out


def run_driver(lib, device, steps=2, check=True):
    """Six Drivers from the fixture on six ThreadComm ranks, `steps` steps of step_all with the state checked after each."""
    from pace_amd.driver import Driver, DriverConfig
    from pace_amd.util import run_tiles

    config = DriverConfig.from_dict(settings(stencil_config={}, minutes=0, seconds=int(steps * DT),
                                             safety_check_frequency=1 if check else None))
    assert config.n_timesteps() == steps

    def program(comm):
        driver = Driver(copy.deepcopy(config), comm=comm, lib=lib, device=device)
        start = driver.time
        driver.step_all()
        sync(device)
        facts = {"elapsed": (driver.time - start).total_seconds(), "start": start,
                 "checks": driver.performance_collector.total_timer.hits.get("safety_check")}
        driver.cleanup()
        return snapshot(driver.state), facts

    return run_tiles(6, program)


def run_stages(lib, device, steps=2):
    """The same steps with the stage classes called by hand in the order of the reference's driver.py:618-640, on a state built
    by DycoreState.from_fortran_restart and pace_pe_peln_from_delp."""
    import datetime
    import types

    from pace_amd import stencils
    from pace_amd.driver import DriverConfig, TendencyState
    from pace_amd.driver.config import GeneratedGridConfig
    from pace_amd.fv3core import DynamicalCore
    from pace_amd.physics import Physics, PhysicsState
    from pace_amd.tile import setup_factories
    from pace_amd.util import run_tiles

    def program(comm):
        config = DriverConfig.from_dict(settings(stencil_config={}))
        dc, pc = config.dycore_config, config.physics_config
        cube = communicator_of(comm, lib, device)
        _, qf, _, sf = setup_factories(lib, device, N, NZ, communicator=cube)
        damping, driver_grid, grid = GeneratedGridConfig(restart_path=RESTART).get_grid(quantity_factory=qf, communicator=cube)
        state = restart_state(lib, device, cube, qf, grid.ak[0])
        tend, phy = TendencyState.init_zeros(qf), PhysicsState.init_zeros(qf, ["microphysics"])
        core = DynamicalCore(cube, grid, sf, qf, damping, dc, state.phis, state, datetime.timedelta(seconds=DT))
        to_physics = stencils.CopyDycoreToPhysics(sf, qf)
        physics = Physics(sf, qf, grid, pc, ["microphysics"])
        gather = stencils.PhysicsToDycore(sf, qf, pc)
        apply = stencils.ApplyPhysicsToDycore(sf, qf, grid, pc, cube, driver_grid, state, tend.u_dt, tend.v_dt)
        for _ in range(steps):
            core.step_dynamics(state)
            to_physics(state, phy)
            physics(phy, timestep=DT)
            gather(state, phy, tend.u_dt, tend.v_dt, tend.pt_dt)
            apply(state, tend.u_dt, tend.v_dt, tend.pt_dt, dt=DT)
        sync(device)
        return snapshot(types.SimpleNamespace(dycore_state=state, tendency_state=tend, physics_state=phy))

    return run_tiles(6, program)


def loop_against_stages(lib, device):
    """-> what the run test asserts: the fields that differ, the fields that are not finite, per-tile facts, the field count,
    the physics fields that moved, the largest A-grid wind of the compute domains."""
    got, want = run_driver(lib, device), run_stages(lib, device)
    different = [(t, k) for t in range(6) for k in want[t] if not np.array_equal(got[t][0][k], want[t][k], equal_nan=True)]
    not_finite = [(t, k) for t in range(6) for k, a in got[t][0].items() if not np.isfinite(a).all()]
    moved = [k for k in want[0] if k.startswith("physics.") and np.abs(want[0][k]).max() > 0]
    winds = max(float(np.abs(got[t][0]["dycore.ua"][3:3 + N, 3:3 + N, :NZ]).max()) for t in range(6))
    return different, not_finite, [g[1] for g in got], len(want[0]), moved, winds


# ---- the GPU runs' child process ------------------------------------------------------------------------------------------------
def _child_main(what, out_path):
    from pace_amd import _lib

    lib = _lib.load()
    if what == "start":
        result = drivers_at_start(lib, "cuda")
    elif what == "run":
        result = loop_against_stages(lib, "cuda")
    else:
        raise ValueError(what)
    with open(out_path, "wb") as f:
        pickle.dump(result, f)


def run_in_child(what, tmp_path, timeout=300):
    """A fresh process, a time limit, the child's output in the error when it fails."""
    out = os.path.join(str(tmp_path), f"{what}.pkl")
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); "
            f"import restart_helpers; restart_helpers._child_main({what!r}, {out!r})")
    p = subprocess.run([sys.executable, "-X", "faulthandler", "-c", code], capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError(f"child run {what!r} failed (rc {p.returncode}):\n{p.stdout[-4000:]}\n{p.stderr[-8000:]}")
    with open(out, "rb") as f:
        return pickle.load(f)
