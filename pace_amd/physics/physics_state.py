"""PhysicsState (reference: physics/pace/physics/physics_state.py): the fields the Physics shell works on, under the
reference's names, with its metadata (name, dims, units), its `quantity_factory` / `active_packages` init vars and
`.microphysics`, a MicrophysicsState that SHARES the fields (or None without the package).  `xr_dataset` is left out."""
from dataclasses import InitVar, dataclass, field, fields
from typing import Any, Dict, List, Mapping, Optional

from ..util import Quantity, QuantityFactory, constants
from .stencils.microphysics import MicrophysicsState

_XYZ = [constants.X_DIM, constants.Y_DIM, constants.Z_DIM]
_XYZI = [constants.X_DIM, constants.Y_DIM, constants.Z_INTERFACE_DIM]


def _meta(name, units, dims=None, intent="inout"):
    metadata = {"name": name, "dims": list(_XYZ if dims is None else dims), "units": units}
    if intent is not None:
        metadata["intent"] = intent
    return field(metadata=metadata)


@dataclass()
class PhysicsState:
    qvapor: Quantity = _meta("specific_humidity", "kg/kg", intent=None)
    qliquid: Quantity = _meta("cloud_water_mixing_ratio", "kg/kg")
    qice: Quantity = _meta("cloud_ice_mixing_ratio", "kg/kg")
    qrain: Quantity = _meta("rain_mixing_ratio", "kg/kg")
    qsnow: Quantity = _meta("snow_mixing_ratio", "kg/kg")
    qgraupel: Quantity = _meta("graupel_mixing_ratio", "kg/kg")
    qo3mr: Quantity = _meta("ozone_mixing_ratio", "kg/kg")
    qsgs_tke: Quantity = _meta("turbulent_kinetic_energy", "m**2/s**2")
    qcld: Quantity = _meta("cloud_fraction", "")
    pt: Quantity = _meta("air_temperature", "degK")
    delp: Quantity = _meta("pressure_thickness_of_atmospheric_layer", "Pa")
    delz: Quantity = _meta("vertical_thickness_of_atmospheric_layer", "m")
    ua: Quantity = _meta("eastward_wind", "m/s")
    va: Quantity = _meta("northward_wind", "m/s", intent=None)
    w: Quantity = _meta("vertical_wind", "m/s")
    omga: Quantity = _meta("vertical_pressure_velocity", "Pa/s")
    physics_updated_specific_humidity: Quantity = _meta("physics_updated_specific_humidity", "kg/kg", intent=None)
    physics_updated_qliquid: Quantity = _meta("physics_updated_liquid_water_mixing_ratio", "kg/kg")
    physics_updated_qice: Quantity = _meta("physics_updated_ice_water_mixing_ratio", "kg/kg")
    physics_updated_qrain: Quantity = _meta("physics_updated_rain_water_mixing_ratio", "kg/kg")
    physics_updated_qsnow: Quantity = _meta("physics_updated_snow_mixing_ratio", "kg/kg")
    physics_updated_qgraupel: Quantity = _meta("physics_updated_graupel_mixing_ratio", "kg/kg")
    physics_updated_cloud_fraction: Quantity = _meta("physics_cloud_fraction", "")
    physics_updated_pt: Quantity = _meta("physics_air_temperature", "degK")
    physics_updated_ua: Quantity = _meta("physics_eastward_wind", "m/s")
    physics_updated_va: Quantity = _meta("physics_northward_wind", "m/s")
    delprsi: Quantity = _meta("model_level_pressure_thickness_in_physics", "Pa")
    phii: Quantity = _meta("interface_geopotential_height", "m", _XYZI)
    phil: Quantity = _meta("layer_geopotential_height", "m")
    dz: Quantity = _meta("geopotential_height_thickness", "m")
    wmp: Quantity = _meta("layer_mean_vertical_velocity_microph", "m/s")
    prsi: Quantity = _meta("interface_pressure", "Pa", _XYZI)
    prsik: Quantity = _meta("log_interface_pressure", "Pa", _XYZI)
    land: Quantity = _meta("land_mask", "-", [constants.X_DIM, constants.Y_DIM], intent="in")
    quantity_factory: InitVar[QuantityFactory]
    active_packages: InitVar[List[str]]

    def __post_init__(self, quantity_factory: QuantityFactory, active_packages: List[str]):
        # storage for tendency variables not in PhysicsState
        if "microphysics" in active_packages:
            tendency = quantity_factory.zeros(_XYZ, "unknown", dtype=float)
            self.microphysics: Optional[MicrophysicsState] = MicrophysicsState(
                pt=self.pt, qvapor=self.qvapor, qliquid=self.qliquid, qrain=self.qrain, qice=self.qice, qsnow=self.qsnow,
                qgraupel=self.qgraupel, qcld=self.qcld, ua=self.ua, va=self.va, delp=self.delp, delz=self.delz, omga=self.omga,
                delprsi=self.delprsi, wmp=self.wmp, dz=self.dz, tendency=tendency, land=self.land)
        else:
            self.microphysics = None

    @classmethod
    def init_zeros(cls, quantity_factory, active_packages: List[str]) -> "PhysicsState":
        """As the reference's, whose fields are then the bare storages (`.data`): here tensors of the library's layout."""
        initial_arrays = {}
        for _field in fields(cls):
            if "dims" in _field.metadata.keys():
                initial_arrays[_field.name] = quantity_factory.zeros(_field.metadata["dims"], _field.metadata["units"],
                                                                     dtype=float).data
        return cls(**initial_arrays, quantity_factory=quantity_factory, active_packages=active_packages)

    @classmethod
    def init_from_storages(cls, storages: Mapping[str, Any], sizer, quantity_factory: QuantityFactory,
                           active_packages: List[str]) -> "PhysicsState":
        """storages: name -> tensor of the library's layout (QuantityFactory's `.data`)."""
        inputs: Dict[str, Quantity] = {}
        for _field in fields(cls):
            if "dims" in _field.metadata.keys():
                dims = _field.metadata["dims"]
                inputs[_field.name] = Quantity(storages[_field.name], dims, _field.metadata["units"], origin=sizer.get_origin(dims),
                                               extent=sizer.get_extent(dims))
        return cls(**inputs, quantity_factory=quantity_factory, active_packages=active_packages)
