"""forcing_config -- a prescribed forcing in place of the physics (not in the reference's driver).

    forcing_config:
      type: held_suarez
      config: {sigma_b: 0.7, k_f_days: 1.0, k_a_days: 40.0, k_s_days: 4.0, delta_t_y: 60.0, delta_theta_z: 10.0, t0: 315.0,
               t_strat: 200.0, p0: 100000.0}      # all optional: the values of Held and Suarez (1994)

held_suarez is the dry climate benchmark: Newtonian relaxation of the temperature and Rayleigh friction of the low-level winds
(pace_amd.stencils.HeldSuarezForcing, ONE pace_held_suarez launch a step).  It replaces the physics, so it needs dycore_only: true
and disable_step_physics: false.  In a step it runs after DycoreToPhysics and before UpdateAtmosphereState, and ADDS its
tendencies to the step's tendency state with the step's dt (the dry convective adjustment may already have written wind
tendencies there); ApplyPhysicsToDycore applies them and leaves the three arrays zero.  Under comm_config.type cube each tile
thread launches for its own tile."""
import dataclasses
import math
from typing import Any, Dict

from ..stencils.held_suarez import _SECONDS_PER_DAY, HeldSuarezConfig, HeldSuarezForcing

_TIME_SCALES = {"k_f_days": "k_f", "k_a_days": "k_a", "k_s_days": "k_s"}
_PLAIN = ("sigma_b", "delta_t_y", "delta_theta_z", "t0", "t_strat", "p0")


@dataclasses.dataclass
class ForcingConfig:
    """type: held_suarez; config: its constants, the rates as time scales in days (k_f_days, k_a_days, k_s_days)."""

    type: str = "held_suarez"
    config: Dict[str, Any] = dataclasses.field(default_factory=dict)

    def __post_init__(self):
        if self.type != "held_suarez":
            raise ValueError(f"forcing_config.type = {self.type!r}: the forcings are ('held_suarez',)")
        if not isinstance(self.config, dict):
            raise ValueError(f"forcing_config.config = {self.config!r}: expected a mapping")
        for key, value in self.config.items():
            if key not in _TIME_SCALES and key not in _PLAIN:
                raise ValueError(f"forcing_config.config has no setting {key!r} ({sorted(_TIME_SCALES) + sorted(_PLAIN)})")
            if isinstance(value, bool) or not isinstance(value, (int, float)):
                raise ValueError(f"forcing_config.config.{key} = {value!r}: expected a number")
            if key in _TIME_SCALES and not (math.isfinite(value) and value > 0):
                raise ValueError(f"forcing_config.config.{key} = {value!r}: expected a positive time scale in days")
        self.held_suarez_config()  # (refuses what the kernel's entry point would)

    def held_suarez_config(self) -> HeldSuarezConfig:
        values = {}
        for key, value in self.config.items():
            if key in _TIME_SCALES:
                values[_TIME_SCALES[key]] = 1.0 / (float(value) * _SECONDS_PER_DAY)
            else:
                values[key] = float(value)
        try:
            return HeldSuarezConfig(**values)
        except ValueError as e:
            raise ValueError(f"forcing_config.config: {e}") from None

    def forcing_factory(self, stencil_factory, quantity_factory, grid_data) -> HeldSuarezForcing:
        return HeldSuarezForcing(stencil_factory, quantity_factory, grid_data, self.held_suarez_config(), constant_volume=True)

    @classmethod
    def from_dict(cls, config) -> "ForcingConfig":
        from .config import _strict

        if isinstance(config, cls):
            return config
        return _strict(cls, "forcing_config", dict(config or {}))
