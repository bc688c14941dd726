"""LagrangianToEulerian -- Fortran Lagrangian_to_Eulerian (reference: fv3core/pace/fv3core/stencils/remapping.py:286-695).

With ``do_sat_adj = True`` the saturation adjustment (SatAdjust3d) runs between the remap of v and the last stencil, as in
the reference (:627-672)."""
from typing import Dict

from ...util.constants import X_DIM, X_INTERFACE_DIM, Y_DIM, Y_INTERFACE_DIM, Z_DIM, Z_INTERFACE_DIM
from .._config import RemappingConfig
from ._common import Operator, check_layout, dptr
from .fillz import pointer_table
from .map_single import MapSingle
from .mapn_tracer import MapNTracer
from .saturation_adjustment import SatAdjust3d

# TODO(reference): "Should this be set here or in global_constants?" (remapping.py:38-39)
CONSV_MIN = 0.001
_WATER = ("qvapor", "qliquid", "qrain", "qsnow", "qice", "qgraupel")


class LagrangianToEulerian(Operator):
    """Remap the deformed Lagrangian surfaces onto the reference, or "Eulerian", coordinate levels."""

    def __init__(self, stencil_factory, quantity_factory, config: RemappingConfig, area_64, nq, pfull, tracers: Dict[str, object],
                 checkpointer=None):
        super().__init__(stencil_factory, quantity_factory)
        if config.kord_tm >= 0:
            raise NotImplementedError("map ppm, untested mode where kord_tm >= 0")
        if config.hydrostatic:
            raise NotImplementedError("Hydrostatic is not implemented")
        self._t_min = 184.0
        self._nq = nq
        qf = quantity_factory
        self._pe1 = qf.zeros([X_DIM, Y_DIM, Z_INTERFACE_DIM], units="Pa")
        self._pe2 = qf.zeros([X_DIM, Y_DIM, Z_INTERFACE_DIM], units="Pa")
        self._pe3 = qf.zeros([X_DIM, Y_DIM, Z_INTERFACE_DIM], units="Pa")
        self._dp2 = qf.zeros([X_DIM, Y_DIM, Z_DIM], units="Pa")
        self._pn2 = qf.zeros([X_DIM, Y_DIM, Z_DIM], units="Pa")
        self._pe0 = qf.zeros([X_DIM, Y_DIM, Z_INTERFACE_DIM], units="Pa")
        self._kord_tm = abs(config.kord_tm)
        self._kord_wz = config.kord_wz
        self._kord_mt = config.kord_mt
        self._do_sat_adjust = config.do_sat_adj
        sf = stencil_factory
        self._map_single_pt = MapSingle(sf, qf, self._kord_tm, 1, dims=[X_DIM, Y_DIM, Z_DIM])
        self._mapn_tracer = MapNTracer(sf, qf, abs(config.kord_tr), nq, fill=config.fill, tracers=tracers)
        self._map_single_w = MapSingle(sf, qf, self._kord_wz, -2, dims=[X_DIM, Y_DIM, Z_DIM])
        self._map_single_delz = MapSingle(sf, qf, self._kord_wz, 1, dims=[X_DIM, Y_DIM, Z_DIM])
        self._map_single_u = MapSingle(sf, qf, self._kord_mt, -1, dims=[X_DIM, Y_INTERFACE_DIM, Z_DIM])
        self._map_single_v = MapSingle(sf, qf, self._kord_mt, -1, dims=[X_INTERFACE_DIM, Y_DIM, Z_DIM])
        if self._do_sat_adjust:
            # the first level below 10 hPa (:344-348)
            nk = self._geom.nk
            pf = pfull.view[:] if hasattr(pfull, "dims") else pfull
            pf = pf.detach().cpu().numpy() if hasattr(pf, "detach") else pf
            self.kmp = nk - 1
            for k in range(min(len(pf), nk)):
                if float(pf[k]) > 10.0e2:
                    self.kmp = k
                    break
            self._saturation_adjustment = SatAdjust3d(sf, config.sat_adjust, area_64, self.kmp, quantity_factory=qf)

    def __call__(self, tracers, pt, delp, delz, peln, u, v, w, cappa, q_con, q_cld, pkz, pk, pe, hs, ps, wsd, ak, bk, dp1,
                 ptop: float, akap: float, zvir: float, last_step: bool, consv_te: float, mdt: float, *, te0_2d=None,
                 rsin2=None, cosa_s=None, area_64=None, energy_fixer=None, dt_atmos=None):
        """Same arguments as the reference (remapping.py:485-563): tracers, pt, delp, delz, peln, u, v, w, cappa (inout);
        q_con, pk, ps (out); pkz, pe (inout); wsd, ak, bk (in); q_cld, hs, dp1, mdt are only used by the saturation
        adjustment.

        Keyword-only, for consv_te > CONSV_MIN on the last step (the total-energy fixer, energy_fixer.py): te0_2d, the column
        energies at the top of the step (EnergyFixer.total_energy(0, ...)); the metric planes rsin2, cosa_s and area_64; the
        EnergyFixer that owns the buffers and the communicator of the global sum; dt_atmos, the seconds e_flux refers to
        (mdt where it is not given).  Without them such a call raises as the reference does."""
        check_layout(self._geom, pt, delp, delz, peln, u, v, w, cappa, q_con, pkz, pk, pe)
        fix_energy = False
        if last_step:
            if consv_te > CONSV_MIN:
                if any(x is None for x in (te0_2d, rsin2, cosa_s, area_64, energy_fixer)):
                    raise NotImplementedError("We do not support consv_te > 0.001 because that would trigger an allReduce")
                fix_energy = True
            elif consv_te < -CONSV_MIN:
                raise NotImplementedError("Unimplemented/untested case consv(" + str(consv_te) + ")  < -CONSV_MIN("
                                          + str(-CONSV_MIN) + ")")
        water = pointer_table([tracers[name] for name in _WATER])
        st = self.stream
        self.call("pace_l2e_prepare", water, dptr(q_con), dptr(pt), dptr(cappa), dptr(delp), dptr(delz), dptr(pe),
                  dptr(self._pe1), dptr(self._pe2), dptr(ak), dptr(bk), dptr(self._dp2), dptr(ps), dptr(self._pn2), dptr(peln),
                  dptr(pk), float(ptop), float(akap), float(zvir), st())
        # now that we have the pressure profiles, we can start remapping
        self._map_single_pt(pt, peln, self._pn2, qmin=self._t_min)
        self._mapn_tracer(self._pe1, self._pe2, self._dp2, tracers)
        self._map_single_w(w, self._pe1, self._pe2, qs=wsd)
        self._map_single_delz(delz, self._pe1, self._pe2)
        self.call("pace_l2e_post", water, dptr(q_con), dptr(pkz), dptr(pt), dptr(cappa), dptr(delp), dptr(delz), dptr(peln),
                  dptr(self._pe0), dptr(self._pn2), float(zvir), st())
        self.call("pace_l2e_pressures", 0, dptr(pe), dptr(self._pe1), dptr(ak), dptr(bk), dptr(self._pe0), dptr(self._pe3), st())
        self._map_single_u(u, self._pe0, self._pe3)
        self.call("pace_l2e_pressures", 1, dptr(pe), dptr(self._pe1), dptr(ak), dptr(bk), dptr(self._pe0), dptr(self._pe3), st())
        self._map_single_v(v, self._pe0, self._pe3)
        if fix_energy:
            # the energy of the remapped state against te0_2d, then the global sum: dtmp stays on the device
            energy_fixer.total_energy(1, [tracers[name] for name in _WATER], pt, delp, delz, w, u, v, pkz, hs, rsin2, cosa_s,
                                      area_64, te0_2d, zvir)
            result = energy_fixer.finalize(consv_te, mdt if dt_atmos is None else dt_atmos)
        if self._do_sat_adjust:
            fast_mp_consv = consv_te > CONSV_MIN
            self._saturation_adjustment(dp1, tracers["qvapor"], tracers["qliquid"], tracers["qice"], tracers["qrain"],
                                        tracers["qsnow"], tracers["qgraupel"], q_cld, hs, peln, delp, delz, q_con, pt, pkz, cappa,
                                        zvir, mdt, fast_mp_consv, last_step, akap, self.kmp)
        # on the last step, we need the regular temperature to send to the physics, but if we're staying in dynamics we
        # need to keep it as the virtual potential temperature
        if fix_energy:
            self.call("pace_l2e_finish_dtmp", water, dptr(pe), dptr(self._pe2), dptr(pt), dptr(pkz), float(zvir), result.data_ptr(),
                      st())
        else:
            self.call("pace_l2e_finish", water, dptr(pe), dptr(self._pe2), dptr(pt), dptr(pkz), float(zvir), int(bool(last_step)),
                      st())
