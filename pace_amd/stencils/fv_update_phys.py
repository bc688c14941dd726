"""ApplyPhysicsToDycore -- the Fortran fv_update_phys (reference: stencils/pace/stencils/fv_update_phys.py:77-192): apply the
tendencies u_dt, v_dt, t_dt consistently with the FV3 discretisation and make the pressures consistent with delp.

The reference's order is kept: the two one-point halo updates of u_dt, v_dt are started, the column kernel
(pace_phys_thermo_pressure: moist_cv and update_pressure_and_surface_winds in one launch) runs while they are in flight, then
the wait, the wind update and CubedToLatLon."""
from ..fv3core.stencils.c2l_ord import CubedToLatLon
from ..fv3core.stencils.fillz import pointer_table
from ..util.constants import X_DIM, Y_DIM, Z_DIM
from ._common import AddressedState, Operator, addressed, check_layout, dptr, need_3d, refuse_other_layouts
from .update_dwind_phys import AGrid2DGridPhysics

WATER = ("qvapor", "qliquid", "qrain", "qsnow", "qice", "qgraupel")


class ApplyPhysicsToDycore(Operator):
    """
    Fortran name is fv_update_phys
    Apply the physics tendencies (u_dt, v_dt, t_dt, q_dt) consistent with
    the FV3 discretization and definition of the prognostic variables
    """

    def __init__(self, stencil_factory, quantity_factory, grid_data, namelist, comm, grid_info, state, u_dt, v_dt):
        """The reference's arguments (:84-95).  state, u_dt, v_dt: what the halo updaters are built for; the fields of a call
        may be others of the same layout."""
        refuse_other_layouts(namelist)
        qf = quantity_factory if quantity_factory is not None else stencil_factory.quantity_factory
        if qf is None:
            raise ValueError("ApplyPhysicsToDycore needs the field layout: a quantity factory")
        super().__init__(stencil_factory, qf, grid_data)
        self.comm = comm
        self._AGrid2DGridPhysics = AGrid2DGridPhysics(stencil_factory, qf, comm.partitioner.tile, comm.rank, namelist, grid_info)
        self._c2l_state = AddressedState(state)
        self._do_cubed_to_latlon = CubedToLatLon(self._c2l_state, stencil_factory, quantity_factory=qf, grid_data=grid_data,
                                                 order=namelist.c2l_ord, comm=comm)
        spec = qf.get_quantity_halo_spec(dims=[X_DIM, Y_DIM, Z_DIM], n_halo=1)
        self._udt_halo_updater = comm.get_scalar_halo_updater([spec])
        self._vdt_halo_updater = comm.get_scalar_halo_updater([spec])
        # (the reference's own TODO: "check if we actually need surface winds")
        self._u_srf = qf.zeros(dims=[X_DIM, Y_DIM], units="m/s")
        self._v_srf = qf.zeros(dims=[X_DIM, Y_DIM], units="m/s")

    def __call__(self, state, u_dt, v_dt, t_dt, dt: float):
        """state: a DycoreState or any namespace with qvapor ... qgraupel, pt, pe, delp, peln, pk, ps, u, v, ua, va -- Quantity
        objects or tensors of the library's layout.  u_dt, v_dt, t_dt: the tendencies (zero afterwards, u_dt and v_dt on the
        compute domain plus one point).  dt: seconds."""
        water = [getattr(state, name) for name in WATER]
        fields = [state.pt, t_dt, state.pe, state.delp, state.peln, state.pk, state.ua, state.va]
        need_3d("ApplyPhysicsToDycore", *water, *fields, u_dt, v_dt, state.u, state.v)
        check_layout(self._geom, *water, *fields, u_dt, v_dt, state.u, state.v, state.ps)
        self._c2l_state._state = state  # (CubedToLatLon's halo updater looks u, v up by name at call time)
        self._udt_halo_updater.start([addressed(u_dt)])
        self._vdt_halo_updater.start([addressed(v_dt)])
        self.call("pace_phys_thermo_pressure", pointer_table(water), *[dptr(f) for f in fields], dptr(state.ps),
                  dptr(self._u_srf), dptr(self._v_srf), float(dt), self.stream())
        self._udt_halo_updater.wait()
        self._vdt_halo_updater.wait()
        self._AGrid2DGridPhysics(state.u, state.v, u_dt, v_dt)
        self._do_cubed_to_latlon(state.u, state.v, state.ua, state.va)
