"""DryConvectiveAdjustment -- the Fortran fv_subgrid_z (reference: fv3core/pace/fv3core/stencils/fv_subgridz.py:740-964),
non-hydrostatic: the dry convective adjustment a driver with fv_sg_adj > 0 applies to the dycore state once per physics step.

Each call is ONE launch of pace_dry_convective_adjust over origin (isc, jsc, 0), domain (nx, ny, k_sponge), without a host
synchronisation: the kernel itself reads pe[isc, jsc, 0], which the reference reads on the host to choose t_min.

One departure from the reference: with n_sponge < 3 its constructor returns early and its __call__ then raises AttributeError;
here such an object's call does nothing, which is the Fortran's early return."""
import collections

from ._common import Operator, check_layout, dptr
from .fillz import pointer_table, tracer_variables

ArgSpec = collections.namedtuple("ArgSpec", ["arg_name", "standard_name", "units", "intent"])


class DryConvectiveAdjustment(Operator):
    """Corresponds to fv_subgrid_z in Fortran's fv_sg module."""

    arg_specs = (
        ArgSpec("delp", "pressure_thickness_of_atmospheric_layer", "Pa", intent="in"),
        ArgSpec("delz", "vertical_thickness_of_atmospheric_layer", "m", intent="in"),
        ArgSpec("pe", "interface_pressure", "Pa", intent="in"),
        ArgSpec("pkz", "layer_mean_pressure_raised_to_power_of_kappa", "unknown", intent="in"),
        ArgSpec("peln", "logarithm_of_interface_pressure", "ln(Pa)", intent="in"),
        ArgSpec("pt", "air_temperature", "degK", intent="inout"),
        ArgSpec("ua", "eastward_wind", "m/s", intent="inout"),
        ArgSpec("va", "northward_wind", "m/s", intent="inout"),
        ArgSpec("w", "vertical_wind", "m/s", intent="inout"),
        ArgSpec("qvapor", "specific_humidity", "kg/kg", intent="inout"),
        ArgSpec("qliquid", "cloud_water_mixing_ratio", "kg/kg", intent="inout"),
        ArgSpec("qrain", "rain_mixing_ratio", "kg/kg", intent="inout"),
        ArgSpec("qsnow", "snow_mixing_ratio", "kg/kg", intent="inout"),
        ArgSpec("qice", "cloud_ice_mixing_ratio", "kg/kg", intent="inout"),
        ArgSpec("qgraupel", "graupel_mixing_ratio", "kg/kg", intent="inout"),
        ArgSpec("qo3mr", "ozone_mixing_ratio", "kg/kg", intent="inout"),
        ArgSpec("qsgs_tke", "turbulent_kinetic_energy", "m**2/s**2", intent="inout"),
        ArgSpec("qcld", "cloud_fraction", "", intent="inout"),
        ArgSpec("u_dt", "eastward_wind_tendency_due_to_physics", "m/s**2", intent="inout"),
        ArgSpec("v_dt", "northward_wind_tendency_due_to_physics", "m/s**2", intent="inout"),
    )

    def __init__(self, stencil_factory, quantity_factory, nwat: int, fv_sg_adj: float, n_sponge: int, hydrostatic: bool):
        """The reference's arguments (:777-785).  n_sponge = None: every level."""
        if hydrostatic:
            raise NotImplementedError("Hydrostatic not implemented for fv_subgridz")
        qf = quantity_factory if quantity_factory is not None else stencil_factory.quantity_factory
        if qf is None:
            raise ValueError("DryConvectiveAdjustment needs the field layout: a quantity factory")
        super().__init__(stencil_factory, qf)
        nk = self._geom.nk
        self._k_sponge = nk if n_sponge is None else int(n_sponge)
        if self._k_sponge > nk:
            raise ValueError(f"n_sponge = {n_sponge} exceeds the {nk} levels")
        self._nwat = int(nwat)
        self._fv_sg_adj = float(fv_sg_adj)
        if self._k_sponge >= 3 and not self._fv_sg_adj > 0:
            raise ValueError(f"fv_sg_adj = {fv_sg_adj}: the adjustment's time scale must be positive")

    def __call__(self, state, u_dt, v_dt, timestep: float):
        """Performs dry convective adjustment mixing on the subgrid vertical scale.

        state: see arg_specs -- a DycoreState or any namespace with these fields, Quantity objects or tensors of the library's
        layout; pt, ua, va, w and the nine tracers are adjusted in place.  u_dt, v_dt: the wind tendencies of the adjustment
        (overwritten).  timestep: seconds."""
        if self._k_sponge < 3:
            return
        tracers = [getattr(state, name) for name in tracer_variables]
        fields = [state.pt, state.ua, state.va, state.w, u_dt, v_dt, state.delp, state.delz, state.pkz, state.peln, state.pe]
        for f in tracers + fields:
            if f is None:
                raise ValueError("DryConvectiveAdjustment needs every field of arg_specs")
            t = f.data if hasattr(f, "dims") else f
            if t.dim() != 3:
                raise ValueError(f"field of shape {tuple(t.shape)}: DryConvectiveAdjustment takes 3-D fields")
        check_layout(self._geom, *tracers, *fields)
        self.call("pace_dry_convective_adjust", pointer_table(tracers), *[dptr(f) for f in fields], self._k_sponge, self._nwat,
                  self._fv_sg_adj, float(timestep), self.stream())
