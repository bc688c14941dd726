"""HeldSuarezForcing -- the Held-Suarez (1994) benchmark forcing of a dry dynamical core (the Fortran FV3's Held_Suarez_Tend; the
reference has none): Newtonian relaxation of the temperature toward a prescribed zonally symmetric equilibrium and Rayleigh
friction of the winds below sigma_b, as the tendencies u_dt, v_dt, pt_dt that ApplyPhysicsToDycore applies.

    forcing = HeldSuarezForcing(stencil_factory, quantity_factory, grid_data)
    forcing(dycore_state, u_dt, v_dt, pt_dt, timestep, accumulate=True)

One call is ONE pace_held_suarez launch (include/pace_hip.h has the arithmetic, in its order).  sin(lat)^2 and cos(lat)^2 of the
cell centres are formed with numpy when the operator is built and stay on the device as two planes: nothing is uploaded per
call.  The rates carry the backward-Euler factor 1 / (1 + k dt), so applied over dt they contract for every dt.

heating_scale: the non-hydrostatic apply stage (pace_phys_thermo_pressure) computes pt += t_dt * dt * CP_AIR / cvm -- it takes
t_dt for a heating rate at constant pressure -- while Held-Suarez prescribes the temperature's own rate of change.  With
constant_volume=True pt_dt is scaled by CV_AIR / CP_AIR, so that a dry column (cvm = CV_AIR) relaxes at exactly the prescribed
rate; with condensate present cvm is slightly larger and the relaxation that much slower."""
import ctypes as C
import dataclasses
import math

import numpy as np

from .. import _lib
from ..util import constants
from ..util.constants import X_DIM, Y_DIM
from ._common import Operator, check_layout, dptr, need_3d

_SECONDS_PER_DAY = 86400.0


@dataclasses.dataclass
class HeldSuarezConfig:
    """The constants of Held and Suarez (1994), their values as defaults: rates in 1/s, temperatures in K, p0 in Pa."""

    p0: float = 1.0e5
    kappa: float = constants.RDGAS / constants.CP_AIR
    sigma_b: float = 0.7
    k_f: float = 1.0 / _SECONDS_PER_DAY
    k_a: float = 1.0 / (40.0 * _SECONDS_PER_DAY)
    k_s: float = 1.0 / (4.0 * _SECONDS_PER_DAY)
    delta_t_y: float = 60.0
    delta_theta_z: float = 10.0
    t0: float = 315.0
    t_strat: float = 200.0

    def __post_init__(self):
        for field in dataclasses.fields(self):
            value = getattr(self, field.name)
            if isinstance(value, bool) or not isinstance(value, (int, float)):
                raise ValueError(f"HeldSuarezConfig.{field.name} = {value!r}: expected a number")
        if not (0.0 <= self.sigma_b < 1.0):
            raise ValueError(f"HeldSuarezConfig.sigma_b = {self.sigma_b!r}: expected a value in [0, 1)")
        if not self.p0 > 0.0:
            raise ValueError(f"HeldSuarezConfig.p0 = {self.p0!r}: expected a positive pressure")
        for name in ("k_f", "k_a", "k_s"):
            rate = getattr(self, name)
            if not (math.isfinite(rate) and rate >= 0.0):
                raise ValueError(f"HeldSuarezConfig.{name} = {rate!r}: expected a finite rate >= 0")


class HeldSuarezForcing(Operator):
    def __init__(self, stencil_factory, quantity_factory, grid_data, config=None, *, constant_volume=True):
        """grid_data: gives lat_agrid, the cell centres' latitudes [radians] over the whole storage (host-side there).
        constant_volume: scale pt_dt by CV_AIR / CP_AIR (see the module's docstring)."""
        qf = quantity_factory if quantity_factory is not None else stencil_factory.quantity_factory
        if qf is None:
            raise ValueError("HeldSuarezForcing needs the field layout: a quantity factory")
        super().__init__(stencil_factory, qf)
        if config is None:
            config = HeldSuarezConfig()
        if not isinstance(config, HeldSuarezConfig):
            raise ValueError(f"HeldSuarezForcing: config = {config!r} is no HeldSuarezConfig")
        self.config = config
        lat = getattr(grid_data, "lat_agrid", None)
        if lat is None:
            raise ValueError("HeldSuarezForcing needs grid_data.lat_agrid, the latitudes of the cell centres")
        lat = np.asarray(lat.numpy() if hasattr(lat, "dims") else lat, dtype=np.float64)
        n = self._geom.n
        if lat.shape != (n + 7, n + 7):
            raise ValueError(f"grid_data.lat_agrid has shape {lat.shape}, the {n} x {n} tile's storage is {(n + 7, n + 7)}")
        self.sin2lat = qf.zeros([X_DIM, Y_DIM], units="")
        self.cos2lat = qf.zeros([X_DIM, Y_DIM], units="")
        self.sin2lat.set(np.sin(lat) ** 2)
        self.cos2lat.set(np.cos(lat) ** 2)
        self.heating_scale = constants.CV_AIR / constants.CP_AIR if constant_volume else 1.0
        c = _lib.HeldSuarezConfig()
        c.struct_bytes = C.sizeof(_lib.HeldSuarezConfig)
        for field in dataclasses.fields(config):
            setattr(c, field.name, float(getattr(config, field.name)))
        c.heating_scale = self.heating_scale
        self._cfg = c

    def __call__(self, state, u_dt, v_dt, pt_dt, timestep, *, accumulate=False, teq=None):
        """state: a DycoreState or any namespace with pe, ua, va, pt -- Quantity objects or tensors of the library's layout; only
        read.  u_dt, v_dt, pt_dt (out, or inout with accumulate): the forcing's tendencies on the compute domain.  timestep:
        seconds (or a timedelta), >= 0; 0 gives the plain Held-Suarez rates.  teq (out, optional): the equilibrium temperature."""
        dt = float(timestep.total_seconds() if hasattr(timestep, "total_seconds") else timestep)
        if not (math.isfinite(dt) and dt >= 0.0):
            raise ValueError(f"HeldSuarezForcing: timestep = {timestep!r}: expected a finite number of seconds >= 0")
        fields = [state.pe, state.ua, state.va, state.pt, u_dt, v_dt, pt_dt]
        need_3d("HeldSuarezForcing", *fields)
        if teq is not None:
            need_3d("HeldSuarezForcing", teq)
        check_layout(self._geom, *fields, teq)
        self._cfg.accumulate = int(bool(accumulate))
        self._cfg.dt = dt
        self.call("pace_held_suarez", C.byref(self._cfg), *[dptr(f) for f in fields[:4]], self.sin2lat.ptr, self.cos2lat.ptr,
                  dptr(u_dt), dptr(v_dt), dptr(pt_dt), dptr(teq), self.stream())
