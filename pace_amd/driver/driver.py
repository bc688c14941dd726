"""Driver -- the model's main loop (reference: driver/pace/driver/driver.py:372-745).

    driver = Driver(DriverConfig.from_yaml("config.yaml"))
    driver.step_all()
    driver.cleanup()

A step is the reference's (driver.py:618-640): DynamicalCore.step_dynamics, DycoreToPhysics, Physics, UpdateAtmosphereState,
each a class of its own that can also be called by hand; the driver only strings them together, advances the time and, every
safety_check_frequency steps, checks the state (SafetyChecker: one launch pair and one transfer) and, every output_frequency
steps, stores the diagnostics (MonitorDiagnostics: one pack launch and one transfer).  What the reference's constructor does
for DaCe, build modes, its own restart format and the performance collector's files is not here.  With forcing_config the
Held-Suarez forcing adds its tendencies between DycoreToPhysics and UpdateAtmosphereState (driver/forcing.py: one pace_held_suarez
launch a step).  With nudging_config the state is relaxed toward a sequence of
Fortran restarts after the end-of-step update (driver/nudging.py: one pace_nudge launch a step).  Restart files are written in
the FORTRAN model's format (fortran_restart_config, write_fortran_restart: one pack launch and one transfer), which
initialization.type fortran_restart reads back.

One deliberate departure: the reference's constructor registers its four variables with SafetyChecker.register_variable, which
raises on a second registration, so two reference Drivers cannot exist in one process.  Six of these do (one per tile on
threads): the constructor registers each of the four only if it is absent, under a lock.  register_variable itself keeps raising.
"""
import os
import threading
import warnings

from .. import _launch, _lib
from ..fv3core import DynamicalCore
from ..physics import Physics
from ..stencils import update_atmos_state
from ..util import CubedSphereCommunicator, Timer
from .config import DriverConfig
from .nudging import Nudging
from .safety_checks import SafetyChecker

_REGISTRATION_LOCK = threading.Lock()
# driver.py:536-539
_SAFETY_CHECKS = (("ua", -200, 200), ("va", -200, 200), ("delp", -1.0, 4000), ("pt", 100, 380))


class PerformanceCollector:
    """The two timers of the reference's collector (performance/collector.py): `total_timer` for initialization and the whole
    run, `timestep_timer` for the main loop and what the dynamical core clocks inside it.  No file is written."""

    def __init__(self):
        self.total_timer = Timer()
        self.timestep_timer = Timer()


class Driver:
    def __init__(self, config: DriverConfig, comm=None, lib=None, device=None):
        """
        Args:
            config: driver configuration
            comm: communication object behaving like pace_amd.util.TorchDistComm / ThreadComm / NullComm; default: what
                config.comm_config creates
            lib: the kernel library (default: the product library, pace_amd._lib.load())
            device: where the fields live (default: the current device; "cpu" with the emulation test library)
        """
        from ..tile import setup_factories

        self.config: DriverConfig = config
        self.time = self.config.start_time
        self.comm_config = config.comm_config
        self.comm = comm if comm is not None else config.comm_config.get_comm()
        self.lib = lib if lib is not None else _lib.load()
        if device is None:
            device = _launch.default_device(self.lib)
        self.device = device
        self.performance_collector = PerformanceCollector()
        with self.performance_collector.total_timer.clock("initialization"):
            communicator = CubedSphereCommunicator(self.comm, device=device, lib=self.lib)
            self.communicator = communicator
            self._warn_about_what_is_ignored()
            _, self.quantity_factory, _, self.stencil_factory = setup_factories(
                self.lib, device, config.nx_tile, config.nz, layout=config.layout, stencil_config=config.stencil_config,
                communicator=communicator)
            damping_coefficients, driver_grid_data, grid_data = self.config.get_grid(
                quantity_factory=self.quantity_factory, communicator=communicator)
            self.state = self.config.get_driver_state(
                quantity_factory=self.quantity_factory, communicator=communicator, damping_coefficients=damping_coefficients,
                driver_grid_data=driver_grid_data, grid_data=grid_data)
            self._start_time = self.config.initialization.start_time
            self.dycore = DynamicalCore(
                comm=communicator, grid_data=self.state.grid_data, stencil_factory=self.stencil_factory,
                quantity_factory=self.quantity_factory, damping_coefficients=self.state.damping_coefficients,
                config=self.config.dycore_config, timestep=self.config.timestep, phis=self.state.dycore_state.phis,
                state=self.state.dycore_state)
            if not config.dycore_only and not config.disable_step_physics:
                self.physics = Physics(stencil_factory=self.stencil_factory, quantity_factory=self.quantity_factory,
                                       grid_data=self.state.grid_data, namelist=self.config.physics_config,
                                       active_packages=["microphysics"])
            else:
                # Make sure those are set to None to raise any issues
                self.physics = None
            if not config.disable_step_physics:
                couple = not self.config.dycore_only
                self.dycore_to_physics = update_atmos_state.DycoreToPhysics(
                    stencil_factory=self.stencil_factory, quantity_factory=self.quantity_factory,
                    dycore_config=self.config.dycore_config, do_dry_convective_adjust=config.do_dry_convective_adjustment,
                    dycore_only=self.config.dycore_only, couple_physics=couple)
                self.end_of_step_update = update_atmos_state.UpdateAtmosphereState(
                    stencil_factory=self.stencil_factory, grid_data=self.state.grid_data, namelist=self.config.physics_config,
                    comm=communicator, grid_info=self.state.driver_grid_data, state=self.state.dycore_state,
                    quantity_factory=self.quantity_factory, dycore_only=self.config.dycore_only,
                    apply_tendencies=self.config.apply_tendencies, tendency_state=self.state.tendency_state,
                    couple_physics=couple)
            else:
                # Make sure those are set to None to raise any issues
                self.dycore_to_physics = None
                self.end_of_step_update = None
            self.forcing = None
            if config.forcing_config is not None:
                self.forcing = config.forcing_config.forcing_factory(self.stencil_factory, self.quantity_factory,
                                                                     self.state.grid_data)
            self.diagnostics = config.diagnostics_config.diagnostics_factory(communicator=communicator, lib=self.lib)
            self.nudging = None
            if config.nudging_config is not None:
                self.nudging = Nudging(config.nudging_config, quantity_factory=self.quantity_factory, communicator=communicator)
            self.nudging_tendencies = None  # the last step's, with nudging_config.store_tendencies
        if config.output_initial_state:
            self.diagnostics.store(time=self.time, state=self.state)
        self._time_run = self.config.start_time
        self.safety_checker = SafetyChecker(self.lib)
        with _REGISTRATION_LOCK:  # (see the module's docstring)
            for name, minimum, maximum in _SAFETY_CHECKS:
                if name not in SafetyChecker.checks:
                    SafetyChecker.register_variable(name, minimum, maximum, compute_domain_only=True)

    def _warn_about_what_is_ignored(self):
        """One warning per run (rank 0's) for the settings of a reference file that are kept and not acted on."""
        if self.comm.Get_rank() != 0:
            return
        ignored = []
        if self.config.diagnostics_config.path is not None and not self.config.diagnostics_config.writes_files_for(self.communicator):
            ignored.append(f"diagnostics_config (path {self.config.diagnostics_config.path!r}): no diagnostics are written, "
                           "output_initial_state and output_frequency have no effect")
        requested = getattr(self.config.stencil_config, "requested_backend", None)
        if requested is not None and requested != self.config.stencil_config.backend:
            ignored.append(f"stencil_config.compilation_config.backend {requested!r}: the backend is "
                           f"{self.config.stencil_config.backend!r}")
        if ignored:
            warnings.warn("pace_amd.driver ignores " + "; ".join(ignored), UserWarning, stacklevel=3)

    def _end_of_step_actions(self, step: int):
        """
        Gather operations unrelated to computation.
        """
        self.time += self.config.timestep
        if ((step + 1) % self.config.output_frequency) == 0:
            self.diagnostics.store(time=self.time, state=self.state)
        if self.config.safety_check_frequency and ((step + 1) % self.config.safety_check_frequency) == 0:
            with self.performance_collector.total_timer.clock("safety_check"):
                self.safety_checker.check_state(self.state.dycore_state)
        restart = self.config.fortran_restart_config
        if (step + 1) in restart.intermediate_restart:
            self.write_fortran_restart(f"{restart.path}_{step + 1}")

    def write_fortran_restart(self, path: str):
        """The state as restart files of the Fortran model in `path` (DycoreState.to_fortran_restart: one pace_restart_pack
        launch, one device-to-host copy), with the current time in coupler.res; rank 0 adds restart.yaml, this run's
        configuration with initialization and grid_config.config.restart_path pointing at `path`, so that
        DriverConfig.from_yaml(<path>/restart.yaml) resumes."""
        with self.performance_collector.total_timer.clock("restart"):
            # (a run that itself began from a Fortran restart carries that file's model start time on)
            start = getattr(self.config.initialization.config, "model_start_time", None) or self._start_time
            self.state.dycore_state.to_fortran_restart(communicator=self.communicator, path=path, time=self.time,
                                                       start_time=start, grid_data=self.state.grid_data)
            if self.comm.Get_rank() == 0:
                if self.config.source is None:
                    warnings.warn(f"{path}: no restart.yaml is written, the configuration was not made by DriverConfig.from_dict",
                                  UserWarning, stacklevel=2)
                else:
                    import yaml

                    with open(os.path.join(path, "restart.yaml"), "w") as f:
                        yaml.safe_dump(self.config.restart_dict(path), f, sort_keys=False)

    def _critical_path_step_all(self, steps_count: int, timer: Timer, dt: float):
        """Start of code path where performance is critical."""
        for step in range(steps_count):
            with timer.clock("mainloop"):
                self.dycore.step_dynamics(state=self.state.dycore_state, timer=timer)
                if not self.config.disable_step_physics:
                    self.dycore_to_physics(dycore_state=self.state.dycore_state, physics_state=self.state.physics_state,
                                           tendency_state=self.state.tendency_state, timestep=float(dt))
                    if not self.config.dycore_only:
                        self.physics(self.state.physics_state, timestep=float(dt))
                    if self.forcing is not None:  # added to what the dry convective adjustment left in the tendencies
                        self.forcing(self.state.dycore_state, self.state.tendency_state.u_dt, self.state.tendency_state.v_dt,
                                     self.state.tendency_state.pt_dt, float(dt), accumulate=True)
                    self.end_of_step_update(dycore_state=self.state.dycore_state, phy_state=self.state.physics_state,
                                            u_dt=self.state.tendency_state.u_dt, v_dt=self.state.tendency_state.v_dt,
                                            pt_dt=self.state.tendency_state.pt_dt, dt=float(dt))
                if self.nudging is not None:  # toward the reference at the END of the step (self.time is still its beginning)
                    self.nudging_tendencies = self.nudging(self.state.dycore_state, self.time + self.config.timestep,
                                                           self.config.timestep)
            self._end_of_step_actions(step)

    def step_all(self):
        with self.performance_collector.total_timer.clock("total"):
            self._critical_path_step_all(steps_count=self.config.n_timesteps(), timer=self.performance_collector.timestep_timer,
                                         dt=self.config.timestep.total_seconds())
        if self.config.fortran_restart_config.save_restart:
            self.write_fortran_restart(self.config.fortran_restart_config.path)

    def sypd(self) -> float:
        """Simulated years per day of wall time, as the reference reports it (performance/report.py:116-129): dt_atmos over the
        mean time of a main-loop step, over 365; -999.0 before the first step."""
        timer = self.performance_collector.timestep_timer
        hits = timer.hits.get("mainloop", 0)
        if hits == 0:
            return -999.0
        mainloop = timer.times["mainloop"] / hits
        return 1.0 / 365.0 * (self.config.dt_atmos / mainloop)

    def cleanup(self):
        self.diagnostics.store_grid(grid_data=self.state.grid_data)
        self.diagnostics.cleanup()
        self.comm_config.cleanup(self.comm)


def run_cube_driver(config: DriverConfig, steps=None, device=None, lib=None, snapshot=False):
    """Run a configuration as the whole globe on one device (comm_config.type: cube): six Drivers on the six tile threads of
    pace_amd.util.run_cube, whose halo updates are one kernel launch each for the whole cube.  Every Driver gets a copy of the
    configuration, runs step_all (`steps` replaces the file's run length) and cleans up, exactly as one of six processes
    would; diagnostics, the fortran_restart initialisation with verify_checksums and write_fortran_restart work per tile.
    snapshot: the halo updates keep the reference's contract (a field may be rewritten after start()) at ThreadComm's cost.
    Returns the six Drivers in tile order."""
    import copy

    from ..util import run_cube

    if steps is not None:
        config = copy.deepcopy(config)
        config.days = config.hours = config.minutes = 0
        config.seconds = int(round(steps * config.dt_atmos))
        config.__dict__.pop("total_time", None)  # (a cached property of the run length it had)
        if config.n_timesteps() != steps:
            raise ValueError(f"steps={steps} is no whole number of seconds at dt_atmos {config.dt_atmos}")
        if config.source is not None:
            config.source.update(days=0, hours=0, minutes=0, seconds=config.seconds)

    def program(comm):
        driver = Driver(copy.deepcopy(config), comm=comm, lib=lib, device=device)
        driver.step_all()
        driver.cleanup()
        return driver

    return run_cube(program, snapshot=snapshot)
