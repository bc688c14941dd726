"""DycoreState: the fields the acoustic dynamics read and write, with the reference's names and dims
(fv3core/pace/fv3core/initialization/dycore_state.py:11-340), and the tracer species that the tracer advection, the
remapping and neg_adj3 work on."""
import dataclasses

from ...util.constants import X_DIM, X_INTERFACE_DIM, Y_DIM, Y_INTERFACE_DIM, Z_DIM, Z_INTERFACE_DIM

_C = [X_DIM, Y_DIM, Z_DIM]
_FIELDS = {
    "u": ([X_DIM, Y_INTERFACE_DIM, Z_DIM], "m/s"), "v": ([X_INTERFACE_DIM, Y_DIM, Z_DIM], "m/s"), "w": (_C, "m/s"),
    "ua": (_C, "m/s"), "va": (_C, "m/s"), "uc": ([X_INTERFACE_DIM, Y_DIM, Z_DIM], "m/s"),
    "vc": ([X_DIM, Y_INTERFACE_DIM, Z_DIM], "m/s"), "delp": (_C, "Pa"), "delz": (_C, "m"), "ps": ([X_DIM, Y_DIM], "Pa"),
    "pe": ([X_DIM, Y_DIM, Z_INTERFACE_DIM], "Pa"), "pt": (_C, "degK"), "peln": ([X_DIM, Y_DIM, Z_INTERFACE_DIM], "ln(Pa)"),
    "pk": ([X_DIM, Y_DIM, Z_INTERFACE_DIM], "unknown"), "pkz": (_C, "unknown"), "q_con": (_C, "kg/kg"), "omga": (_C, "Pa/s"),
    "mfxd": ([X_INTERFACE_DIM, Y_DIM, Z_DIM], "unknown"), "mfyd": ([X_DIM, Y_INTERFACE_DIM, Z_DIM], "unknown"),
    "cxd": ([X_INTERFACE_DIM, Y_DIM, Z_DIM], ""), "cyd": ([X_DIM, Y_INTERFACE_DIM, Z_DIM], ""), "diss_estd": (_C, "unknown"),
    "phis": ([X_DIM, Y_DIM], "m^2 s^-2"),
    "qvapor": (_C, "kg/kg"), "qliquid": (_C, "kg/kg"), "qrain": (_C, "kg/kg"), "qice": (_C, "kg/kg"), "qsnow": (_C, "kg/kg"),
    "qgraupel": (_C, "kg/kg"), "qo3mr": (_C, "kg/kg"), "qsgs_tke": (_C, "m**2/s**2"), "qcld": (_C, ""),
}

# the fields DycoreState.from_fortran_restart fills -> their standard names (pace_amd.util.restart.RESTART_PROPERTIES)
FORTRAN_RESTART_FIELDS = {
    "pt": "air_temperature", "delp": "pressure_thickness_of_atmospheric_layer", "phis": "surface_geopotential",
    "w": "vertical_wind", "u": "x_wind", "v": "y_wind", "qvapor": "specific_humidity",
    "qliquid": "cloud_liquid_water_mixing_ratio", "qice": "cloud_ice_mixing_ratio", "qrain": "rain_mixing_ratio",
    "qsnow": "snow_mixing_ratio", "qgraupel": "graupel_mixing_ratio", "qo3mr": "ozone_mixing_ratio", "qcld": "cloud_fraction",
    "delz": "vertical_thickness_of_atmospheric_layer",
}


@dataclasses.dataclass
class DycoreState:
    u: object = None
    v: object = None
    w: object = None
    ua: object = None
    va: object = None
    uc: object = None
    vc: object = None
    delp: object = None
    delz: object = None
    ps: object = None
    pe: object = None
    pt: object = None
    peln: object = None
    pk: object = None
    pkz: object = None
    q_con: object = None
    omga: object = None
    mfxd: object = None
    mfyd: object = None
    cxd: object = None
    cyd: object = None
    diss_estd: object = None
    phis: object = None
    qvapor: object = None
    qliquid: object = None
    qrain: object = None
    qice: object = None
    qsnow: object = None
    qgraupel: object = None
    qo3mr: object = None
    qsgs_tke: object = None
    qcld: object = None

    @classmethod
    def init_zeros(cls, quantity_factory):
        return cls(**{name: quantity_factory.zeros(dims, units, dtype=float) for name, (dims, units) in _FIELDS.items()})

    @classmethod
    def init_from_numpy_arrays(cls, dict_of_numpy_arrays, quantity_factory):
        for name in dict_of_numpy_arrays:
            if name not in _FIELDS:
                raise KeyError(name + " is provided, but not part of the dycore state")
        state = cls.init_zeros(quantity_factory)
        for name, a in dict_of_numpy_arrays.items():
            getattr(state, name).set(a)
        return state

    @classmethod
    def from_fortran_restart(cls, *, quantity_factory, communicator, path: str, verify_checksums: bool = False,
                             surface_winds: bool = False):
        """dycore_state.py:361-427: zeros, then the compute domains of the fifteen fields a Fortran restart holds, through
        pace_amd.util.open_restart -- one staging buffer, one host-to-device copy, one pace_state_unpack launch.  Halos and every
        other field (ua, va, pe, peln, pk, pkz, ps, q_con, ...) stay zero, as in the reference.  Two additions for restarts
        written by to_fortran_restart: sgs_tke goes to qsgs_tke where the files have it (the Fortran model's need not), and with
        surface_winds u_srf / v_srf go back where to_fortran_restart took them from, the lowest level of ua / va."""
        from ...util.restart import LevelOf, open_restart

        new = cls.init_zeros(quantity_factory=quantity_factory)
        to_state = {name: getattr(new, field) for field, name in FORTRAN_RESTART_FIELDS.items()}
        to_state["turbulent_kinetic_energy"] = new.qsgs_tke
        if surface_winds:
            lowest = new.ua.extent[2] - 1
            to_state["eastward_wind_at_surface"] = LevelOf(new.ua, lowest)
            to_state["northward_wind_at_surface"] = LevelOf(new.va, lowest)
        open_restart(dirname=path, communicator=communicator, only_names=list(to_state), to_state=to_state,
                     verify_checksums=verify_checksums, missing_ok=["turbulent_kinetic_energy"])
        return new

    def to_fortran_restart(self, *, communicator, path: str, time, start_time=None, grid_data=None, label: str = "",
                           file_dtype=None):
        """The inverse of from_fortran_restart, in the Fortran model's format (the reference's DriverState.save_state leaves
        this as a commented-out starter, driver/pace/driver/state.py:118-145): the fifteen fields of FORTRAN_RESTART_FIELDS, qsgs_tke
        as sgs_tke, and the lowest level of ua / va as u_srf / v_srf, through pace_amd.util.write_restart -- one
        pace_restart_pack launch, one device-to-host copy.  grid_data: its ak / bk go to fv_core.res.nc (rank 0)."""
        import numpy as np

        from ...util.restart import LevelOf, write_restart

        from_state = {name: getattr(self, field) for field, name in FORTRAN_RESTART_FIELDS.items()}
        from_state["turbulent_kinetic_energy"] = self.qsgs_tke
        lowest = self.ua.extent[2] - 1
        from_state["eastward_wind_at_surface"] = LevelOf(self.ua, lowest)
        from_state["northward_wind_at_surface"] = LevelOf(self.va, lowest)
        ak, bk = (None, None) if grid_data is None else (np.asarray(grid_data.ak), np.asarray(grid_data.bk))
        write_restart(path, communicator, from_state, time=time, start_time=start_time, label=label, ak=ak, bk=bk,
                      file_dtype=np.float64 if file_dtype is None else file_dtype)
