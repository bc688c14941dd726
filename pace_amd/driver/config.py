"""DriverConfig and the selectors it is made of (reference: driver/pace/driver/driver.py:46-370, initialization.py, grid.py,
comm.py, performance/config.py; DiagnosticsConfig lives in diagnostics.py).  `DriverConfig.from_dict` takes what `yaml.safe_load` gives for one of
the reference's configuration files; the conversion is strict (an unknown key raises ValueError and names itself), written by
hand where the reference uses dacite.

What is accepted, refused and ignored:

  initialization.type   baroclinic, predefined, fortran_restart (the Fortran model's restart files: FortranRestartInit);
                        restart / serialbox / tropicalcyclone: NotImplementedError
  grid_config.type      generated (the gnomonic grid of pace_amd.util.gridgen, not stretched; config.restart_path: ak / bk and
                        what derives from them come from <restart_path>/fv_core.res.nc); serialbox: NotImplementedError
  layout                (1, 1)
  comm_config.type      null (null_comm), torch, cube (run_cube_driver); mpi, write, read: NotImplementedError.  Absent: null, rank 0 of 6 -- the
                        reference's default is mpi, which does not exist here
  pair_debug            NotImplementedError when true
  restart_config        NotImplementedError when it enables output (save_restart, intermediate_restart): pace's own restart
                        format is not written
  fortran_restart_config  (not in the reference) save_restart, intermediate_restart, path: the state in the FORTRAN model's
                        restart format at the end of the run (<path>) and after the listed steps (<path>_<step>), each with a
                        restart.yaml that resumes from it (Driver.write_fortran_restart)
  initialization.config.verify_checksums  (fortran_restart; not in the reference) hold what was read against the files' checksums
  initialization.config.surface_winds     (fortran_restart; not in the reference) u_srf / v_srf into the lowest level of ua / va
  diagnostics_config    output_format npz with a path: written (driver/diagnostics.py); zarr, netcdf: parsed and kept, nothing is
                        written (the Driver warns once)
  diagnostics_config.latlon  (not in the reference) cell-centre variables on a regular latitude-longitude grid, regridded on the
                        device; with comm_config.type cube only, ValueError with any other
  nudging_config        (not in the reference) timescale_seconds, reference_paths, label, store_tendencies: the state relaxed
                        toward a sequence of Fortran restarts, interpolated in time, one launch per step (driver/nudging.py);
                        delp, delz, phis and anything that is no 3-D field of a Fortran restart: ValueError
  forcing_config        (not in the reference) type held_suarez and its constants: the dry climate benchmark in place of the
                        physics, one launch per step (driver/forcing.py); needs dycore_only true and disable_step_physics false,
                        ValueError otherwise; apply_tendencies is then true
  performance_config    parsed and kept; nothing is written
  stencil_config.compilation_config.backend  kept as `requested_backend`; the backend is always hip:gfx950
"""
import copy
import ctypes as C
import dataclasses
import functools
import os
import warnings
from datetime import datetime, timedelta
from math import floor
from typing import Any, Dict, List, Optional, Tuple, Union

from ..dsl import CompilationConfig, StencilConfig
from ..fv3core import DynamicalCoreConfig
from ..fv3core._config import strict_value
from ..physics import PhysicsConfig, PhysicsState
from .diagnostics import DiagnosticsConfig, ZSelect  # noqa: F401  (ZSelect: named here before diagnostics.py existed)
from .forcing import ForcingConfig
from .nudging import NudgingConfig
from .state import DriverState, TendencyState

_DERIVED = ("dt_atmos", "layout", "npx", "npy", "npz", "ntiles")


def _strict(cls, where: str, values: Dict[str, Any]):
    """cls(**values) with every key checked against the dataclass's fields and every plain value against its type."""
    if not isinstance(values, dict):
        raise ValueError(f"{where}: expected a mapping, got {values!r}")
    fields = {f.name: f for f in dataclasses.fields(cls) if f.init}
    out = {}
    for key, value in values.items():
        if key not in fields:
            raise ValueError(f"{where} has no setting {key!r}")
        out[key] = strict_value(f"{where}.{key}", fields[key].type, value)
    return cls(**out)


def _time(where, value) -> datetime:
    if isinstance(value, datetime):
        return value
    if isinstance(value, str):
        return datetime.fromisoformat(value)
    raise ValueError(f"{where} = {value!r}: expected a date")


# ---- initialization -----------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class BaroclinicInit:
    """Configuration for baroclinic initialization (initialization.py:100-138)."""

    start_time: datetime = datetime(2000, 1, 1)

    def get_driver_state(self, quantity_factory, communicator, damping_coefficients, driver_grid_data, grid_data) -> DriverState:
        from ..fv3core.initialization.baroclinic import init_baroclinic_state

        dycore_state = init_baroclinic_state(grid_data=grid_data, quantity_factory=quantity_factory, adiabatic=False,
                                             hydrostatic=False, moist_phys=True, comm=communicator)
        return DriverState(dycore_state=dycore_state,
                           physics_state=PhysicsState.init_zeros(quantity_factory=quantity_factory, active_packages=["microphysics"]),
                           tendency_state=TendencyState.init_zeros(quantity_factory=quantity_factory), grid_data=grid_data,
                           damping_coefficients=damping_coefficients, driver_grid_data=driver_grid_data)


@dataclasses.dataclass
class PredefinedStateInit:
    """Configuration if the states are already defined (initialization.py:381-416): the objects themselves are part of the
    configuration dictionary, so this is not for yaml files."""

    dycore_state: Any
    physics_state: Any
    tendency_state: Any
    grid_data: Any
    damping_coefficients: Any
    driver_grid_data: Any
    start_time: datetime = datetime(2016, 8, 1)

    def get_driver_state(self, quantity_factory, communicator, damping_coefficients, driver_grid_data, grid_data) -> DriverState:
        return DriverState(dycore_state=self.dycore_state, physics_state=self.physics_state, tendency_state=self.tendency_state,
                           grid_data=self.grid_data, damping_coefficients=self.damping_coefficients,
                           driver_grid_data=self.driver_grid_data)


@dataclasses.dataclass
class FortranRestartInit:
    """Configuration for fortran restart initialization (initialization.py:223-276): the state of `path`'s fv_core, fv_tracer
    and fv_srf_wnd files, the time of its coupler.res."""

    path: str = "."
    verify_checksums: bool = False  # hold the state against the files' tile_checksum / checksum attributes (util/restart.py)
    # u_srf / v_srf into the lowest level of ua / va, where Driver.write_fortran_restart took them from (its restart.yaml says so)
    surface_winds: bool = False

    @property
    def start_time(self) -> datetime:
        """Reads the last line in coupler.res to find the restart time"""
        from ..util.restart import get_current_date_from_coupler_res

        coupler_files = sorted(name for name in os.listdir(self.path) if name.endswith("coupler.res"))
        if not coupler_files:
            raise ValueError(f"no coupler.res found at {self.path}")
        return get_current_date_from_coupler_res(os.path.join(self.path, coupler_files[0]))

    @property
    def model_start_time(self) -> Optional[datetime]:
        """The model start time coupler.res records beside the current time (a restart written from this run carries it on)."""
        from ..util.restart import get_start_date_from_coupler_res

        coupler_files = sorted(name for name in os.listdir(self.path) if name.endswith("coupler.res"))
        return get_start_date_from_coupler_res(os.path.join(self.path, coupler_files[0])) if coupler_files else None

    def get_driver_state(self, quantity_factory, communicator, damping_coefficients, driver_grid_data, grid_data) -> DriverState:
        from ..fv3core.initialization.dycore_state import DycoreState

        dycore_state = DycoreState.from_fortran_restart(quantity_factory=quantity_factory, communicator=communicator, path=self.path,
                                                        verify_checksums=self.verify_checksums, surface_winds=self.surface_winds)
        state = DriverState(dycore_state=dycore_state,
                            physics_state=PhysicsState.init_zeros(quantity_factory=quantity_factory, active_packages=["microphysics"]),
                            tendency_state=TendencyState.init_zeros(quantity_factory=quantity_factory), grid_data=grid_data,
                            damping_coefficients=damping_coefficients, driver_grid_data=driver_grid_data)
        _update_fortran_restart_pe_peln(state, quantity_factory, communicator)
        return state


def _update_fortran_restart_pe_peln(state: DriverState, quantity_factory, communicator) -> None:
    """Fortran restart data don't have information on pressure interface values and their logs (initialization.py:422-442):
    pe = ptop + the sum of delp above, peln = log(pe), over the whole storage, with ptop = ak[0] -- ONE launch of
    pace_pe_peln_from_delp (pace_amd/csrc/k_state.hip)."""
    from ..util.grid import geom_struct

    dycore_state = state.dycore_state
    communicator.lib.call("pace_pe_peln_from_delp", C.byref(geom_struct(quantity_factory)), dycore_state.delp.ptr,
                          float(state.grid_data.ak[0]), dycore_state.pe.ptr, dycore_state.peln.ptr, communicator.stream())


_INITIALIZERS = {"baroclinic": BaroclinicInit, "predefined": PredefinedStateInit, "fortran_restart": FortranRestartInit}
_REFUSED_INITIALIZERS = ("restart", "serialbox", "tropicalcyclone")


@dataclasses.dataclass
class InitializerSelector:
    type: str
    config: Any

    @property
    def start_time(self) -> datetime:
        return self.config.start_time

    def get_driver_state(self, **kwargs) -> DriverState:
        return self.config.get_driver_state(**kwargs)

    @classmethod
    def from_dict(cls, config: dict) -> "InitializerSelector":
        if isinstance(config, cls):
            return config
        kind = _selector_type("initialization", config, ("type", "config"))
        if kind in _REFUSED_INITIALIZERS:
            raise NotImplementedError(f"initialization.type {kind!r}: pace_amd.driver initialises from 'baroclinic', a "
                                      "'fortran_restart' or a 'predefined' state (no reader of pace's own restart or of Serialbox)")
        if kind not in _INITIALIZERS:
            raise ValueError(f"initialization.type {kind!r} is none of {sorted(_INITIALIZERS)}")
        values = dict(config.get("config") or {})
        if "start_time" in values:
            values["start_time"] = _time("initialization.config.start_time", values["start_time"])
        return cls(type=kind, config=_strict(_INITIALIZERS[kind], "initialization.config", values))


def _selector_type(where, config, keys, default=None):
    if not isinstance(config, dict):
        raise ValueError(f"{where}: expected a mapping, got {config!r}")
    for key in config:
        if key not in keys:
            raise ValueError(f"{where} has no setting {key!r}")
    kind = config.get("type", default)
    if not isinstance(kind, str):
        raise ValueError(f"{where}.type = {kind!r}: expected a name")
    return kind


# ---- grid ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class GeneratedGridConfig:
    """grid.py:80-131: the gnomonic cubed sphere, generated; stretching is refused.  restart_path: the directory of a Fortran
    restart whose fv_core.res.nc gives the vertical grid (ak, bk) in place of the generated one."""

    stretch_factor: Optional[float] = 1.0
    lon_target: Optional[float] = 350.0
    lat_target: Optional[float] = -90.0
    restart_path: Optional[str] = None

    def __post_init__(self):
        if self.stretch_factor not in (None, 1.0):
            raise NotImplementedError(f"grid_config.config.stretch_factor {self.stretch_factor}: the stretched grid is not generated")

    def get_grid(self, quantity_factory, communicator):
        from ..util.grid import DampingCoefficients, DriverGridData, GridData, MetricTerms

        metric_terms = MetricTerms(quantity_factory=quantity_factory, communicator=communicator)
        grid_data = GridData.new_from_metric_terms(metric_terms)
        if self.restart_path is not None:
            grid_data.set_vertical_grid(*_vertical_grid_from_restart(self.restart_path))
        damping_coefficients = DampingCoefficients.new_from_metric_terms(metric_terms, grid_data)
        driver_grid_data = DriverGridData.new_from_metric_terms(metric_terms)
        return damping_coefficients, driver_grid_data, grid_data


def _vertical_grid_from_restart(restart_path: str):
    """-> (ak, bk) of <restart_path>/[label.]fv_core.res.nc (grid/helper.py:152-176, VerticalGridData.from_restart)."""
    from ..util.checkpointer.validation import _open_nc

    data_files = sorted(name for name in os.listdir(restart_path) if name.endswith("fv_core.res.nc"))
    if not data_files:
        raise ValueError(f"grid_config.config.restart_path is set, but there is no fv_core.res.nc in {restart_path}")
    file = _open_nc(os.path.join(restart_path, data_files[0]))
    return file.record("ak"), file.record("bk")


@dataclasses.dataclass
class GridInitializerSelector:
    type: str = "generated"
    config: Any = dataclasses.field(default_factory=GeneratedGridConfig)

    def get_grid(self, quantity_factory, communicator):
        return self.config.get_grid(quantity_factory=quantity_factory, communicator=communicator)

    @classmethod
    def from_dict(cls, config: dict) -> "GridInitializerSelector":
        if isinstance(config, cls):
            return config
        kind = _selector_type("grid_config", config, ("type", "config"))
        if kind == "serialbox":
            raise NotImplementedError("grid_config.type 'serialbox': the grid is generated (no Serialbox reader)")
        if kind != "generated":
            raise ValueError(f"grid_config.type {kind!r} is not 'generated'")
        values = dict(config.get("config") or {})
        for key in ("stretch_factor", "lon_target", "lat_target"):
            if isinstance(values.get(key), int) and not isinstance(values.get(key), bool):
                values[key] = float(values[key])
        fields = {f.name for f in dataclasses.fields(GeneratedGridConfig)}
        for key in values:
            if key not in fields:
                raise ValueError(f"grid_config.config has no setting {key!r}")
        return cls(type=kind, config=GeneratedGridConfig(**values))


# ---- communication --------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class NullCommConfig:
    """comm.py:95-121: a rank that runs alone; what it "receives" is fill_value."""

    rank: int = 0
    total_ranks: int = 6
    fill_value: float = 0.0

    def get_comm(self):
        from ..util import NullComm

        return NullComm(rank=self.rank, total_ranks=self.total_ranks, fill_value=self.fill_value)

    def cleanup(self, comm):
        pass


@dataclasses.dataclass
class TorchCommConfig:
    """One process per tile over torch.distributed, which the launcher has initialised (pace_amd.util.TorchDistComm)."""

    def get_comm(self):
        from ..util import TorchDistComm

        return TorchDistComm()

    def cleanup(self, comm):
        pass


@dataclasses.dataclass
class CubeCommConfig:
    """The whole cubed sphere in one process on one device: six Drivers on six tile threads (pace_amd.driver.run_cube_driver,
    pace_amd.util.run_cube).  No rank of such a run can be made alone, so a lone Driver cannot create its communicator."""

    def get_comm(self):
        raise ValueError("comm_config.type 'cube' runs six tiles in one process: run the configuration with "
                         "pace_amd.driver.run_cube_driver(config), which gives every Driver its rank")

    def cleanup(self, comm):
        pass


_COMMS = {"null": NullCommConfig, "null_comm": NullCommConfig, "torch": TorchCommConfig, "cube": CubeCommConfig}


@dataclasses.dataclass
class CreatesCommSelector:
    config: Any = dataclasses.field(default_factory=NullCommConfig)
    type: str = "null"

    def get_comm(self):
        return self.config.get_comm()

    def cleanup(self, comm):
        self.config.cleanup(comm)

    @classmethod
    def from_dict(cls, config: dict) -> "CreatesCommSelector":
        if isinstance(config, cls):
            return config
        kind = _selector_type("comm_config", config, ("type", "config"), default="null")
        if kind in ("mpi", "write", "read"):
            raise NotImplementedError(f"comm_config.type {kind!r}: pace_amd.driver communicates through 'torch' (torch.distributed, "
                                      "one process per tile), 'cube' (six tiles in one process on one device) or runs one rank "
                                      "alone with 'null'")
        if kind not in _COMMS:
            raise ValueError(f"comm_config.type {kind!r} is none of {sorted(_COMMS)}")
        return cls(type=kind, config=_strict(_COMMS[kind], "comm_config.config", dict(config.get("config") or {})))


# ---- kept, not acted on ---------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class PerformanceConfig:
    """performance/config.py:14-29.  Parsed and kept: the Driver times its main loop whatever these say and writes no file."""

    collect_performance: bool = False
    collect_cProfile: bool = False
    collect_communication: bool = False
    experiment_name: str = "test"
    json_all_rank_threshold: int = 1000

    @classmethod
    def from_dict(cls, config) -> "PerformanceConfig":
        return config if isinstance(config, cls) else _strict(cls, "performance_config", dict(config or {}))


@dataclasses.dataclass()
class RestartConfig:
    save_restart: bool = False
    intermediate_restart: List[int] = dataclasses.field(default_factory=list)
    save_intermediate_restart: bool = False

    def __post_init__(self):
        if self.save_restart or self.save_intermediate_restart or len(self.intermediate_restart) > 0:
            raise NotImplementedError("restart_config: writing restart files (save_restart, intermediate_restart) is not implemented")

    @classmethod
    def from_dict(cls, config) -> "RestartConfig":
        return config if isinstance(config, cls) else _strict(cls, "restart_config", dict(config or {}))


@dataclasses.dataclass()
class FortranRestartConfig:
    """Restart files in the Fortran model's format (pace_amd.util.write_restart): the final state to `path`, the state after
    step s of intermediate_restart (1-based, as the reference's RESTART_{step}) to `path`_s."""

    save_restart: bool = False
    intermediate_restart: List[int] = dataclasses.field(default_factory=list)
    path: str = "RESTART"

    @classmethod
    def from_dict(cls, config) -> "FortranRestartConfig":
        return config if isinstance(config, cls) else _strict(cls, "fortran_restart_config", dict(config or {}))


def _plain(value):
    """What yaml.safe_dump takes: tuples as lists, all the way down."""
    if isinstance(value, dict):
        return {key: _plain(v) for key, v in value.items()}
    if isinstance(value, (list, tuple)):
        return [_plain(v) for v in value]
    return value


def _stencil_config(config) -> StencilConfig:
    """The reference's stencil_config section: compilation_config's flags are kept, its backend (a GT4Py one in every reference
    file) is remembered as `requested_backend` and otherwise ignored; dace_config is dropped."""
    if isinstance(config, StencilConfig):
        return config
    if not isinstance(config, dict):
        raise ValueError(f"stencil_config: expected a mapping, got {config!r}")
    for key in config:
        if key not in ("compare_to_numpy", "compilation_config", "dace_config"):
            raise ValueError(f"stencil_config has no setting {key!r}")
    comp = config.get("compilation_config") or {}
    requested = None
    if isinstance(comp, CompilationConfig):
        compilation = comp
    else:
        known = ("backend", "rebuild", "validate_args", "format_source", "device_sync", "run_mode", "use_minimal_caching")
        for key in comp:
            if key not in known:
                raise ValueError(f"stencil_config.compilation_config has no setting {key!r}")
        requested = comp.get("backend")
        compilation = CompilationConfig(**{k: strict_value(f"stencil_config.compilation_config.{k}", bool, comp[k])
                                           for k in ("rebuild", "validate_args", "format_source", "device_sync") if k in comp})
    out = StencilConfig(compare_to_numpy=bool(config.get("compare_to_numpy", False)), compilation_config=compilation)
    out.requested_backend = requested
    return out


# ---- the driver's configuration ---------------------------------------------------------------------------------------------
@dataclasses.dataclass
class DriverConfig:
    """
    Configuration for a run of the model (driver.py:46-158).

    Attributes:
        stencil_config: configuration for stencil compilation (kept; there is one backend)
        initialization: "baroclinic", "fortran_restart" or "predefined", with the chosen type's configuration
        nx_tile: number of gridpoints along the horizontal dimension of a cube
            tile face, same value used for both horizontal dimensions
        nz: number of gridpoints in the vertical dimension
        layout: number of ranks along the x and y dimensions: (1, 1)
        dt_atmos: atmospheric timestep in seconds
        diagnostics_config: configuration for output diagnostics
        performance_config: kept, not acted on
        dycore_config: configuration for dynamical core
        physics_config: configuration for physics
        days, hours, minutes, seconds: add up to the total simulation time
        dycore_only: whether to run just the dycore, or physics too
        disable_step_physics: whether to completely disable the step_physics call,
            including coupling code between the dycore and physics, as well as
            dry static adjustment
        pair_debug: refused when true
        output_initial_state: flag to determine if the first output should be the
            initial state of the model before timestepping
        output_frequency: number of model timesteps between diagnostic timesteps,
            defaults to every timestep
        safety_check_frequency: number of model timesteps between checks of the state, None or 0 for never
        restart_config: the reference's own restart format: refused when it enables output
        fortran_restart_config: restart files in the Fortran model's format (not in the reference)
        nudging_config: relax the state toward a sequence of Fortran restarts (not in the reference); None: no nudging
        forcing_config: a prescribed forcing in place of the physics, the Held-Suarez benchmark (not in the reference); None: none
    """

    stencil_config: StencilConfig
    initialization: InitializerSelector
    nx_tile: int
    nz: int
    layout: Tuple[int, int]
    dt_atmos: float
    grid_config: GridInitializerSelector = dataclasses.field(default_factory=GridInitializerSelector)
    diagnostics_config: DiagnosticsConfig = dataclasses.field(default_factory=DiagnosticsConfig)
    performance_config: PerformanceConfig = dataclasses.field(default_factory=PerformanceConfig)
    comm_config: CreatesCommSelector = dataclasses.field(default_factory=CreatesCommSelector)
    dycore_config: DynamicalCoreConfig = dataclasses.field(default_factory=DynamicalCoreConfig)
    physics_config: PhysicsConfig = dataclasses.field(default_factory=PhysicsConfig)

    days: int = 0
    hours: int = 0
    minutes: int = 0
    seconds: int = 0
    dycore_only: bool = False
    disable_step_physics: bool = False
    restart_config: RestartConfig = dataclasses.field(default_factory=RestartConfig)
    fortran_restart_config: FortranRestartConfig = dataclasses.field(default_factory=FortranRestartConfig)
    pair_debug: bool = False
    output_initial_state: bool = False
    output_frequency: int = 1
    safety_check_frequency: Optional[int] = None
    nudging_config: Optional[NudgingConfig] = None
    forcing_config: Optional[ForcingConfig] = None

    def __post_init__(self):
        if self.pair_debug:
            raise NotImplementedError("pair_debug: running two copies of the model that compare their data is not implemented")
        if self.forcing_config is not None:  # it replaces the physics, and its tendencies are applied by the end-of-step update
            if not self.dycore_only:
                raise ValueError("forcing_config needs dycore_only: true (the forcing replaces the physics)")
            if self.disable_step_physics:
                raise ValueError("forcing_config needs disable_step_physics: false (the end-of-step update applies its tendencies)")

    @functools.cached_property
    def timestep(self) -> timedelta:
        return timedelta(seconds=self.dt_atmos)

    @property
    def start_time(self) -> Union[datetime, timedelta]:
        return self.initialization.start_time

    @functools.cached_property
    def total_time(self) -> timedelta:
        return timedelta(days=self.days, hours=self.hours, minutes=self.minutes, seconds=self.seconds)

    def n_timesteps(self) -> int:
        """Computing how many timestep required to carry the simulation."""
        if self.total_time < self.timestep:
            warnings.warn(f"No simulation possible: you asked for {self.total_time} "
                          f"simulation time but the timestep is {self.timestep}")
        return floor(self.total_time.total_seconds() / self.timestep.total_seconds())

    @functools.cached_property
    def do_dry_convective_adjustment(self) -> bool:
        return self.dycore_config.do_dry_convective_adjustment

    @functools.cached_property
    def apply_tendencies(self) -> bool:
        return self.do_dry_convective_adjustment or not self.dycore_only or self.forcing_config is not None

    def get_grid(self, communicator, quantity_factory):
        return self.grid_config.get_grid(quantity_factory=quantity_factory, communicator=communicator)

    def get_driver_state(self, communicator, damping_coefficients, driver_grid_data, grid_data, quantity_factory) -> DriverState:
        """Load the initial state of the driver."""
        return self.initialization.get_driver_state(quantity_factory=quantity_factory, communicator=communicator,
                                                    damping_coefficients=damping_coefficients, driver_grid_data=driver_grid_data,
                                                    grid_data=grid_data)

    source = None  # the mapping from_dict was given (plain data), from which restart_dict makes a restart.yaml

    def restart_dict(self, directory: str) -> Dict[str, Any]:
        """This run's configuration as a mapping that starts from the Fortran restart in `directory`: initialization and
        grid_config.config.restart_path point there; everything else is what from_dict was given."""
        if self.source is None:
            raise ValueError("a restart.yaml is made of the mapping DriverConfig.from_dict was given; this configuration has none")
        d = _plain(self.source)
        directory = os.path.abspath(directory)
        d["initialization"] = {"type": "fortran_restart", "config": {"path": directory, "surface_winds": True}}
        grid = dict(d.get("grid_config") or {})
        grid.setdefault("type", "generated")
        grid["config"] = {**dict(grid.get("config") or {}), "restart_path": directory}
        d["grid_config"] = grid
        return d

    @classmethod
    def from_dict(cls, kwargs: Dict[str, Any]) -> "DriverConfig":
        kwargs = dict(kwargs)
        source = copy.deepcopy(kwargs)
        fields = {f.name: f for f in dataclasses.fields(cls)}
        for key in kwargs:
            if key not in fields:
                raise ValueError(f"the driver configuration has no setting {key!r}")
        for key in ("stencil_config", "initialization", "nx_tile", "nz", "layout", "dt_atmos"):
            if key not in kwargs:
                raise ValueError(f"the driver configuration needs {key!r}")
        dycore = kwargs.get("dycore_config", {})
        if isinstance(dycore, dict):
            for derived_name in _DERIVED:
                if derived_name in dycore:
                    raise ValueError(f"you cannot set {derived_name} directly in dycore_config, "
                                     "as it is determined based on top-level configuration")
            dycore = DynamicalCoreConfig.from_namelist_dict(dycore)
        physics = kwargs.get("physics_config", {})
        if isinstance(physics, dict):
            physics = _strict(PhysicsConfig, "physics_config", physics)
        for key in ("nx_tile", "nz", "days", "hours", "minutes", "seconds", "output_frequency"):
            if key in kwargs:
                kwargs[key] = strict_value(key, int, kwargs[key])
        for key in ("dycore_only", "disable_step_physics", "pair_debug", "output_initial_state"):
            if key in kwargs:
                kwargs[key] = strict_value(key, bool, kwargs[key])
        if kwargs.get("safety_check_frequency") is not None:
            kwargs["safety_check_frequency"] = strict_value("safety_check_frequency", int, kwargs["safety_check_frequency"])
        kwargs["dt_atmos"] = strict_value("dt_atmos", float, kwargs["dt_atmos"])
        kwargs["layout"] = strict_value("layout", Tuple[int, int], kwargs["layout"])
        if kwargs["layout"] != (1, 1):
            raise NotImplementedError(f"layout {kwargs['layout']}: pace_amd maps one cubed-sphere tile per device, layout must be (1, 1)")
        for config in (dycore, physics):
            config.layout = kwargs["layout"]
            config.dt_atmos = kwargs["dt_atmos"]
            config.npx = kwargs["nx_tile"] + 1
            config.npy = kwargs["nx_tile"] + 1
            config.npz = kwargs["nz"]
        dycore.ntiles = 6
        kwargs["dycore_config"], kwargs["physics_config"] = dycore, physics
        kwargs["comm_config"] = CreatesCommSelector.from_dict(kwargs.get("comm_config", {}))
        kwargs["initialization"] = InitializerSelector.from_dict(kwargs["initialization"])
        if "grid_config" in kwargs:
            kwargs["grid_config"] = GridInitializerSelector.from_dict(kwargs["grid_config"])
        kwargs["stencil_config"] = _stencil_config(kwargs["stencil_config"])
        for key, kind in (("diagnostics_config", DiagnosticsConfig), ("performance_config", PerformanceConfig),
                          ("restart_config", RestartConfig), ("fortran_restart_config", FortranRestartConfig)):
            if key in kwargs:
                kwargs[key] = kind.from_dict(kwargs[key])
        if kwargs.get("nudging_config") is not None:
            kwargs["nudging_config"] = NudgingConfig.from_dict(kwargs["nudging_config"])
        if kwargs.get("forcing_config") is not None:
            kwargs["forcing_config"] = ForcingConfig.from_dict(kwargs["forcing_config"])
        config = cls(**kwargs)
        config.source = source
        return config

    @classmethod
    def from_yaml(cls, path: str) -> "DriverConfig":
        import yaml

        with open(path, "r") as f:
            return cls.from_dict(yaml.safe_load(f))
