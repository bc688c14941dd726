"""DycoreToPhysics and UpdateAtmosphereState -- the two stages with which the reference's driver closes a time step
(reference: stencils/pace/stencils/update_atmos_state.py:148-349, the Fortran atmosphere_state_update).  Dycore-only:

    DycoreToPhysics(...)(dycore_state, None, tendency_state, timestep)       the dry convective adjustment
    UpdateAtmosphereState(...)(dycore_state, None, u_dt, v_dt, pt_dt, dt)    fill_gfs_delp, then ApplyPhysicsToDycore

With dycore_only=False the two compose the operators of physics_coupling.py in the reference's order (:184-232, :301-349):

    DycoreToPhysics          the dry convective adjustment if it is on, then CopyDycoreToPhysics
    UpdateAtmosphereState    PhysicsToDycore (fill_gfs_delp on physics_updated_specific_humidity, then the tendency and tracer
                             update), then ApplyPhysicsToDycore if apply_tendencies

That composition is asked for with the keyword couple_physics=True next to dycore_only=False, which is what pace_amd.driver.Driver
passes.  dycore_only=False WITHOUT it keeps raising NotImplementedError, as it did before the driver existed: the bare
reference-signature call was refused, callers (and tests/test_fv_update_phys.py::test_refusals) rely on that, and a constructor
that silently began to build the physics coupling for them would change their behaviour.  The float32 library is refused on the
physics side by the composed operators themselves."""
from typing import Optional

from ..fv3core.stencils.fv_subgridz import DryConvectiveAdjustment
from ._common import Operator, check_layout, dptr, need_3d, refuse_other_layouts
from .fv_update_phys import ApplyPhysicsToDycore
from .physics_coupling import CopyDycoreToPhysics, PhysicsToDycore


class DycoreToPhysics:
    def __init__(self, stencil_factory, quantity_factory, dycore_config, do_dry_convective_adjust: bool, dycore_only: bool,
                 *, couple_physics: bool = False):
        if not dycore_only and not couple_physics:
            raise NotImplementedError("DycoreToPhysics: dycore_only=False needs couple_physics=True (the copy to a physics state, "
                                      "pace_amd.stencils.CopyDycoreToPhysics, is then run after the adjustment)")
        refuse_other_layouts(dycore_config)
        self._copy_dycore_to_physics = None if dycore_only else CopyDycoreToPhysics(stencil_factory, quantity_factory)
        self._do_dry_convective_adjustment = do_dry_convective_adjust
        self._dycore_only = dycore_only
        if self._do_dry_convective_adjustment:
            self._fv_subgridz = DryConvectiveAdjustment(stencil_factory=stencil_factory, quantity_factory=quantity_factory,
                                                        nwat=dycore_config.nwat, fv_sg_adj=dycore_config.fv_sg_adj,
                                                        n_sponge=dycore_config.n_sponge, hydrostatic=dycore_config.hydrostatic)

    def __call__(self, dycore_state, physics_state, tendency_state=None, timestep: Optional[float] = None):
        if self._do_dry_convective_adjustment:
            self._fv_subgridz(state=dycore_state, u_dt=tendency_state.u_dt, v_dt=tendency_state.v_dt, timestep=timestep)
        if not self._dycore_only:
            self._copy_dycore_to_physics(dycore_state, physics_state)


class UpdateAtmosphereState(Operator):
    """Fortran name is atmosphere_state_update
    This is an API to apply tendencies and compute a consistent prognostic state.
    """

    def __init__(self, stencil_factory, grid_data, namelist, comm, grid_info, state, quantity_factory, dycore_only: bool,
                 apply_tendencies: bool, tendency_state, *, couple_physics: bool = False):
        if not dycore_only and not couple_physics:
            raise NotImplementedError("UpdateAtmosphereState: dycore_only=False needs couple_physics=True (the physics tendencies "
                                      "are then gathered by pace_amd.stencils.PhysicsToDycore before they are applied)")
        refuse_other_layouts(namelist)
        qf = quantity_factory if quantity_factory is not None else stencil_factory.quantity_factory
        if qf is None:
            raise ValueError("UpdateAtmosphereState needs the field layout: a quantity factory")
        super().__init__(stencil_factory, qf)
        self.namelist = namelist
        self._apply_physics_to_dycore = ApplyPhysicsToDycore(stencil_factory, qf, grid_data, namelist, comm, grid_info, state,
                                                             tendency_state.u_dt, tendency_state.v_dt)
        self._physics_to_dycore = None if dycore_only else PhysicsToDycore(stencil_factory, qf, namelist)
        self._dycore_only = dycore_only
        # apply_tendencies when the physics or fv_subgridz has run; without them fill_GFS_delp still runs
        self._apply_tendencies = apply_tendencies

    def fill_gfs_delp(self, delp, q, q_min: float):
        """fill_gfs_delp (:19-37) over the full domain, halo included."""
        need_3d("fill_gfs_delp", delp, q)
        check_layout(self._geom, delp, q)
        self.call("pace_fill_gfs_delp", dptr(delp), dptr(q), float(q_min), self.stream())

    def __call__(self, dycore_state, phy_state, u_dt, v_dt, pt_dt, dt: float):
        if self._dycore_only:
            self.fill_gfs_delp(dycore_state.delp, dycore_state.qvapor, 1.0e-9)
        else:
            self._physics_to_dycore(dycore_state, phy_state, u_dt, v_dt, pt_dt)
        if self._apply_tendencies:
            self._apply_physics_to_dycore(dycore_state, u_dt, v_dt, pt_dt, dt=dt)
