"""Physics -- the shell that feeds the microphysics from a physics state and turns its tendencies into an updated state
(reference: physics/pace/physics/stencils/physics.py:204-369).

    Physics(stencil_factory, quantity_factory, grid_data, namelist, active_packages)(physics_state, timestep)

is three launches (pace_amd/csrc/k_physics.hip, k_microphys.hip), none with a host synchronisation or an allocation:

    prepare(physics_state)           pace_physics_prepare: atmos_phys_driver_statein, get_prs_fv3, get_phi_fv3, prepare_microphysics
    Microphysics                     pace_microphysics
    update(physics_state, timestep)  pace_physics_update_state: update_physics_state_with_tendencies

With active_packages = [] only the first runs, without prepare_microphysics (dz, wmp and the tendencies are not touched).

Two departures from the reference, both about values nothing reads: nothing outside the compute domain is written (the
reference runs get_prs_fv3 / get_phi_fv3 over the halo, where a zero-initialised state gives 0 / 0 and leaves NaN in the halo
of phii and phil), and level nk of the layer fields is neither read nor written (the reference multiplies its zero padding by
zero).  The reference's scratch fields _prsik, _dm3d and _del_gz do not exist: prsik is never read after the call and is not
computed (PhysicsState.prsik is not touched, as in the reference, which passes its own scratch), the other two live in
registers."""
from typing import List

from ... import _lib
from ...fv3core.stencils._common import Operator, check_layout, dptr
from ...stencils._common import need_3d
from .._config import PhysicsConfig
from ..physics_state import PhysicsState
from .microphysics import Microphysics, _pointers

PHYSICS_PACKAGES = ("microphysics",)


class Physics(Operator):
    def __init__(self, stencil_factory, quantity_factory, grid_data, namelist: PhysicsConfig, active_packages: List[str]):
        qf = quantity_factory if quantity_factory is not None else stencil_factory.quantity_factory
        if qf is None:
            raise ValueError("Physics needs the field layout: a quantity factory")
        self._setup_statein()
        if namelist.nwat != self._nwat:
            raise NotImplementedError(f"Physics: nwat = {namelist.nwat!r} is not implemented, only {self._nwat} (_setup_statein)")
        if namelist.hydrostatic:
            raise NotImplementedError("Physics: hydrostatic = True is not implemented")
        if tuple(namelist.layout) != (1, 1):
            raise NotImplementedError(f"layout {tuple(namelist.layout)}: pace_amd maps one cubed-sphere tile per device, layout "
                                      "must be (1, 1)")
        if stencil_factory.lib.real_bytes != 8:
            raise NotImplementedError("Physics needs the float64 library, as Microphysics does")
        unknown = [p for p in active_packages if p not in PHYSICS_PACKAGES]
        if unknown:
            raise NotImplementedError(f"Physics: packages {unknown} are not implemented, only {list(PHYSICS_PACKAGES)}")
        super().__init__(stencil_factory, qf)
        self.namelist = namelist
        self._ptop = float(grid_data.ptop)
        if "microphysics" in active_packages:
            self._do_microphysics = True
            self._microphysics = Microphysics(stencil_factory, qf, grid_data, namelist=namelist)
        else:
            self._do_microphysics = False

    def _setup_statein(self):
        self._NQ = 8  # state.nq_tot - spec.namelist.dnats
        self._dnats = 1  # spec.namelist.dnats
        self._nwat = 6  # spec.namelist.nwat
        self._p00 = 1.0e5

    def prepare(self, physics_state: PhysicsState):
        """Everything before the microphysics, in one launch."""
        s = physics_state
        tracers = [getattr(s, name) for name in _lib.PHYSICS_PREPARE_TRACERS]
        always = tracers + [s.pt, s.delz, s.delp, s.prsi, s.phii, s.phil, s.delprsi]
        optional, tendencies = [None, None, None], None
        if self._do_microphysics:
            if s.microphysics is None:
                raise ValueError("Physics with the microphysics needs a PhysicsState built with active_packages=['microphysics']")
            optional = [s.omga, s.dz, s.wmp]
            tendencies = [getattr(s.microphysics, name) for name in _lib.MICROPHYSICS_TENDENCIES]
            need_3d("Physics", *always, *optional, *tendencies)
            check_layout(self._geom, *always, *optional, *tendencies)
        else:
            need_3d("Physics", *always)
            check_layout(self._geom, *always)
        self.call("pace_physics_prepare", _pointers(tracers), dptr(s.pt), dptr(s.delz), dptr(s.delp), dptr(optional[0]),
                  dptr(s.prsi), dptr(s.phii), dptr(s.phil), dptr(s.delprsi), dptr(optional[1]), dptr(optional[2]),
                  _pointers(tendencies) if tendencies else None, self._ptop, int(self._do_microphysics), self.stream())

    def update(self, physics_state: PhysicsState, timestep: float):
        """physics_updated_<x> = x + x_dt * timestep for the ten fields the microphysics has a tendency of."""
        if not self._do_microphysics:
            return
        s = physics_state
        x = [getattr(s, name) for name, _, _ in _lib.PHYSICS_UPDATED]
        x_dt = [getattr(s.microphysics, name) for _, name, _ in _lib.PHYSICS_UPDATED]
        out = [getattr(s, name) for _, _, name in _lib.PHYSICS_UPDATED]
        need_3d("Physics", *x, *x_dt, *out)
        check_layout(self._geom, *x, *x_dt, *out)
        self.call("pace_physics_update_state", _pointers(x), _pointers(x_dt), _pointers(out), float(timestep), self.stream())

    def __call__(self, physics_state: PhysicsState, timestep: float):
        self.prepare(physics_state)
        if self._do_microphysics:
            self._microphysics(physics_state.microphysics, timestep=timestep)
            # Fortran uses IPD interface, here we use physics_updated_<var> to denote the updated field
            self.update(physics_state, timestep)
