"""DycoreToPhysics and UpdateAtmosphereState -- the two stages with which the reference's driver closes a time step
(reference: stencils/pace/stencils/update_atmos_state.py:148-349, the Fortran atmosphere_state_update), dycore-only:

    DycoreToPhysics(...)(dycore_state, None, tendency_state, timestep)       the dry convective adjustment
    UpdateAtmosphereState(...)(dycore_state, None, u_dt, v_dt, pt_dt, dt)    fill_gfs_delp, then ApplyPhysicsToDycore

dycore_only=False raises NotImplementedError in both constructors: what the reference does there are operators of their own,
pace_amd.stencils.CopyDycoreToPhysics and PhysicsToDycore (physics_coupling.py), run around pace_amd.physics.Physics."""
from typing import Optional

from ..fv3core.stencils.fv_subgridz import DryConvectiveAdjustment
from ._common import Operator, check_layout, dptr, need_3d, refuse_other_layouts
from .fv_update_phys import ApplyPhysicsToDycore


class DycoreToPhysics:
    def __init__(self, stencil_factory, quantity_factory, dycore_config, do_dry_convective_adjust: bool, dycore_only: bool):
        if not dycore_only:
            raise NotImplementedError("DycoreToPhysics: only dycore_only=True -- the copy to a physics state is pace_amd.stencils.CopyDycoreToPhysics")
        refuse_other_layouts(dycore_config)
        self._do_dry_convective_adjustment = do_dry_convective_adjust
        self._dycore_only = dycore_only
        if self._do_dry_convective_adjustment:
            self._fv_subgridz = DryConvectiveAdjustment(stencil_factory=stencil_factory, quantity_factory=quantity_factory,
                                                        nwat=dycore_config.nwat, fv_sg_adj=dycore_config.fv_sg_adj,
                                                        n_sponge=dycore_config.n_sponge, hydrostatic=dycore_config.hydrostatic)

    def __call__(self, dycore_state, physics_state, tendency_state=None, timestep: Optional[float] = None):
        if self._do_dry_convective_adjustment:
            self._fv_subgridz(state=dycore_state, u_dt=tendency_state.u_dt, v_dt=tendency_state.v_dt, timestep=timestep)


class UpdateAtmosphereState(Operator):
    """Fortran name is atmosphere_state_update
    This is an API to apply tendencies and compute a consistent prognostic state.
    """

    def __init__(self, stencil_factory, grid_data, namelist, comm, grid_info, state, quantity_factory, dycore_only: bool,
                 apply_tendencies: bool, tendency_state):
        if not dycore_only:
            raise NotImplementedError("UpdateAtmosphereState: only dycore_only=True -- physics tendencies are gathered by "
                                      "pace_amd.stencils.PhysicsToDycore")
        refuse_other_layouts(namelist)
        qf = quantity_factory if quantity_factory is not None else stencil_factory.quantity_factory
        if qf is None:
            raise ValueError("UpdateAtmosphereState needs the field layout: a quantity factory")
        super().__init__(stencil_factory, qf)
        self.namelist = namelist
        self._apply_physics_to_dycore = ApplyPhysicsToDycore(stencil_factory, qf, grid_data, namelist, comm, grid_info, state,
                                                             tendency_state.u_dt, tendency_state.v_dt)
        self._dycore_only = dycore_only
        # apply_tendencies when fv_subgridz has run; without it fill_GFS_delp still runs
        self._apply_tendencies = apply_tendencies

    def fill_gfs_delp(self, delp, q, q_min: float):
        """fill_gfs_delp (:19-37) over the full domain, halo included."""
        need_3d("fill_gfs_delp", delp, q)
        check_layout(self._geom, delp, q)
        self.call("pace_fill_gfs_delp", dptr(delp), dptr(q), float(q_min), self.stream())

    def __call__(self, dycore_state, phy_state, u_dt, v_dt, pt_dt, dt: float):
        self.fill_gfs_delp(dycore_state.delp, dycore_state.qvapor, 1.0e-9)
        if self._apply_tendencies:
            self._apply_physics_to_dycore(dycore_state, u_dt, v_dt, pt_dt, dt=dt)
