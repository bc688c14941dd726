"""CopyDycoreToPhysics and PhysicsToDycore -- the dycore_only = False halves of the reference's DycoreToPhysics and
UpdateAtmosphereState (stencils/pace/stencils/update_atmos_state.py:95-145, 198-232 and 40-92, 312-341), as operators of their
own; those two classes compose them when they are built with dycore_only=False and couple_physics=True (update_atmos_state.py),
as pace_amd.driver.Driver builds them.  By hand, a moist step is

    DycoreToPhysics(..., dycore_only=True)(dycore_state, None, tendency_state, timestep)     the dry convective adjustment
    CopyDycoreToPhysics(...)(dycore_state, physics_state)
    Physics(...)(physics_state, timestep)
    PhysicsToDycore(...)(dycore_state, physics_state, u_dt, v_dt, pt_dt)
    ApplyPhysicsToDycore(...)(dycore_state, u_dt, v_dt, pt_dt, dt=timestep)

One launch each (pace_amd/csrc/k_physics.hip), PhysicsToDycore after the existing pace_fill_gfs_delp."""
import ctypes as C

from .. import _lib
from ._common import Operator, check_layout, dptr, need_3d, refuse_other_layouts

# prepare_tendencies_and_update_tracers sums the species in this order
_SUM_ORDER = ("qvapor", "qliquid", "qrain", "qsnow", "qice", "qgraupel")
_UPDATED = ("physics_updated_ua", "physics_updated_va", "physics_updated_pt", "physics_updated_specific_humidity",
            "physics_updated_qliquid", "physics_updated_qrain", "physics_updated_qsnow", "physics_updated_qice",
            "physics_updated_qgraupel")


def _pointers(fields):
    return (C.c_void_p * len(fields))(*[dptr(f) for f in fields])


def _float64_only(owner, stencil_factory):
    if stencil_factory.lib.real_bytes != 8:
        raise NotImplementedError(f"{owner} needs the float64 library, as the physics does")


class CopyDycoreToPhysics(Operator):
    """copy_dycore_to_physics: sixteen fields over origin (3, 3, 0), domain (n + 1, n + 1, nk) -- the reference launches it on
    interface dims with interval(0, -1)."""

    def __init__(self, stencil_factory, quantity_factory):
        qf = quantity_factory if quantity_factory is not None else stencil_factory.quantity_factory
        if qf is None:
            raise ValueError("CopyDycoreToPhysics needs the field layout: a quantity factory")
        _float64_only("CopyDycoreToPhysics", stencil_factory)
        super().__init__(stencil_factory, qf)

    def __call__(self, dycore_state, physics_state):
        src = [getattr(dycore_state, name) for name in _lib.PHYSICS_COPY_FIELDS]
        dst = [getattr(physics_state, name) for name in _lib.PHYSICS_COPY_FIELDS]
        need_3d("CopyDycoreToPhysics", *src, *dst)
        check_layout(self._geom, *src, *dst)
        self.call("pace_copy_dycore_to_physics", _pointers(src), _pointers(dst), self.stream())


class PhysicsToDycore(Operator):
    """The `else` branch of UpdateAtmosphereState.__call__: fill_gfs_delp(dycore delp, physics_updated_specific_humidity, 1e-9)
    over the full domain, then prepare_tendencies_and_update_tracers over the compute domain with rdt = 1 / namelist.dt_atmos:
    u_dt, v_dt and pt_dt are ACCUMULATED into, the dycore's delp and six tracers go back from the physics' air mass (dry air
    and vapour) to the dycore's (condensates included)."""

    def __init__(self, stencil_factory, quantity_factory, namelist):
        refuse_other_layouts(namelist)
        qf = quantity_factory if quantity_factory is not None else stencil_factory.quantity_factory
        if qf is None:
            raise ValueError("PhysicsToDycore needs the field layout: a quantity factory")
        _float64_only("PhysicsToDycore", stencil_factory)
        super().__init__(stencil_factory, qf)
        self.namelist = namelist
        self._rdt = 1.0 / float(namelist.dt_atmos)

    def __call__(self, dycore_state, phy_state, u_dt, v_dt, pt_dt):
        tendencies = [u_dt, v_dt, pt_dt]
        updated = [getattr(phy_state, name) for name in _UPDATED]
        before = [phy_state.ua, phy_state.va, phy_state.pt]
        tracers = [getattr(dycore_state, name) for name in _SUM_ORDER]
        fields = tendencies + updated + before + tracers + [phy_state.prsi, dycore_state.delp]
        need_3d("PhysicsToDycore", *fields)
        check_layout(self._geom, *fields)
        self.call("pace_fill_gfs_delp", dptr(dycore_state.delp), dptr(phy_state.physics_updated_specific_humidity), 1.0e-9,
                  self.stream())
        self.call("pace_physics_tendencies_to_dycore", _pointers(tendencies), _pointers(updated), _pointers(before),
                  _pointers(tracers), dptr(phy_state.prsi), dptr(dycore_state.delp), self._rdt, self.stream())
