"""TendencyState and DriverState (reference: driver/pace/driver/state.py:13-64)."""
import dataclasses

from ..fv3core.initialization.dycore_state import DycoreState
from ..physics import PhysicsState
from ..util import constants as c
from ..util.grid import DampingCoefficients, DriverGridData, GridData
from ..util.quantity import Quantity, QuantityFactory

_XYZ = [c.X_DIM, c.Y_DIM, c.Z_DIM]


@dataclasses.dataclass()
class TendencyState:
    """
    Accumulated tendencies from physical parameterizations to be applied
    to the dynamical core model state.
    """

    u_dt: Quantity = dataclasses.field(
        metadata={"name": "eastward_wind_tendency_due_to_physics", "dims": _XYZ, "units": "m/s**2", "intent": "inout"})
    v_dt: Quantity = dataclasses.field(
        metadata={"name": "northward_wind_tendency_due_to_physics", "dims": _XYZ, "units": "m/s**2", "intent": "inout"})
    pt_dt: Quantity = dataclasses.field(
        metadata={"name": "temperature_tendency_due_to_physics", "dims": _XYZ, "units": "K/s", "intent": "inout"})

    @classmethod
    def init_zeros(cls, quantity_factory: QuantityFactory) -> "TendencyState":
        initial_quantities = {}
        for _field in dataclasses.fields(cls):
            initial_quantities[_field.name] = quantity_factory.zeros(_field.metadata["dims"], _field.metadata["units"], dtype=float)
        return cls(**initial_quantities)


@dataclasses.dataclass
class DriverState:
    dycore_state: DycoreState
    physics_state: PhysicsState
    tendency_state: TendencyState
    grid_data: GridData
    damping_coefficients: DampingCoefficients
    driver_grid_data: DriverGridData
