"""Microphysics -- the GFDL cloud microphysics (reference: physics/pace/physics/stencils/microphysics.py:1830-2533), the one
package of the reference's Physics.

Each call is ONE launch of pace_microphysics (pace_amd/csrc/k_microphys.hip) over the compute domain, all levels, without a
host synchronisation or an allocation.  setupm and _set_timestep run on the host in numpy exactly as the reference computes
them; their results reach the device by value.  The tendencies are ACCUMULATED into the state's fields (a caller zeroes them
first, as the reference's prepare_microphysics does); qa_dt is set to zero (do_qa).

Every switch of the namelist has to have its NamelistDefaults value; anything else raises NotImplementedError."""
import copy
import ctypes as C

import numpy as np
import torch

from ... import _lib
from ...fv3core.stencils._common import Operator, check_layout, dptr
from ...util import constants
from .._config import PhysicsConfig

# microphysics_funcs.py:35-38
SFCRHO = 1.2
RHOS = 1.0e2
RHOG = 4.0e2
RHOR = 1.0e3

# the switches and the one value of each that the kernel implements (NamelistDefaults)
REQUIRED_SWITCHES = dict(use_ppm=False, const_vg=False, const_vi=False, const_vr=False, const_vs=False, prog_ccn=False,
                         do_sedi_heat=False, de_ice=False, irain_f=0, do_sedi_w=True, sedi_transport=True, fix_negative=True,
                         do_qa=True, fast_sat_adj=True, z_slope_liq=True, z_slope_ice=True, rad_snow=True, rad_rain=True)


class MicrophysicsState:
    """
    pt, qvapor, qrain, qice, qsnow, qgraupel, qcld,
    ua, va, delp, delz, omga: same as physics state
    qv_dt ... qg_dt: tendencies of the six species; qa_dt: cloud fraction tendency
    udt, vdt: wind tendencies; pt_dt: air temperature tendency
    land: land mask

    Fields are Quantity objects or tensors of the library's layout.  The ten tendencies are independent copies of `tendency`.
    """

    def __init__(self, pt, qvapor, qliquid, qrain, qice, qsnow, qgraupel, qcld, ua, va, delp, delz, omga, delprsi, wmp, dz,
                 tendency, land):
        self.pt = pt
        self.qvapor = qvapor
        self.qliquid = qliquid
        self.qrain = qrain
        self.qice = qice
        self.qsnow = qsnow
        self.qgraupel = qgraupel
        self.qcld = qcld
        self.ua = ua
        self.va = va
        self.delp = delp
        self.delz = delz
        self.omga = omga
        self.qv_dt = copy.deepcopy(tendency)
        self.ql_dt = copy.deepcopy(tendency)
        self.qr_dt = copy.deepcopy(tendency)
        self.qi_dt = copy.deepcopy(tendency)
        self.qs_dt = copy.deepcopy(tendency)
        self.qg_dt = copy.deepcopy(tendency)
        self.qa_dt = copy.deepcopy(tendency)
        self.udt = copy.deepcopy(tendency)
        self.vdt = copy.deepcopy(tendency)
        self.pt_dt = copy.deepcopy(tendency)
        self.delprsi = delprsi
        self.wmp = wmp
        self.dz = dz
        self.land = land


def _pointers(fields):
    return (C.c_void_p * len(fields))(*[dptr(f) for f in fields])


class Microphysics(Operator):
    def __init__(self, stencil_factory, quantity_factory, grid_data, namelist: PhysicsConfig):
        qf = quantity_factory if quantity_factory is not None else stencil_factory.quantity_factory
        if qf is None:
            raise ValueError("Microphysics needs the field layout: a quantity factory")
        self.namelist = namelist
        if namelist.hydrostatic:
            raise NotImplementedError("Microphysics: hydrostatic = True is not implemented")
        if tuple(namelist.layout) != (1, 1):
            raise NotImplementedError(f"layout {tuple(namelist.layout)}: pace_amd maps one cubed-sphere tile per device, layout "
                                      "must be (1, 1)")
        for name, value in REQUIRED_SWITCHES.items():
            if getattr(namelist, name) != value:
                raise NotImplementedError(f"Microphysics: {name} = {getattr(namelist, name)!r} is not implemented, only {value!r}")
        if stencil_factory.lib.real_bytes != 8:
            raise NotImplementedError("Microphysics needs the float64 library: QCMIN = 1e-12 and QVMIN = 1e-20 are no float32 "
                                      "quantities")
        super().__init__(stencil_factory, qf)
        self._hydrostatic = namelist.hydrostatic
        # heat capacity of dry air and water vapor (microphysics.py:1922-1932)
        self._c_air = constants.CP_AIR
        self._c_vap = constants.CP_VAP
        self._d0_vap = self._c_vap - constants.C_LIQ
        self._lv00 = constants.HLV - self._d0_vap * constants.TICE
        self._cpaut = namelist.c_paut * 0.104 * constants.GRAV / 1.717e-5
        self._area = grid_data.area

        def make_quantity():
            return qf.zeros(dims=[constants.X_DIM, constants.Y_DIM, constants.Z_DIM], units="unknown")

        # surface precipitation, mm/day (the column's value on every level, as the reference keeps it)
        self._rain = make_quantity()
        self._graupel = make_quantity()
        self._ice = make_quantity()
        self._snow = make_quantity()
        nbytes = self.lib.cdll.pace_microphysics_workspace_bytes(C.byref(self._geom))
        self._workspace = torch.zeros(nbytes // 8 + 1, dtype=torch.float64, device=qf.device)
        self._precip = _pointers([self._rain, self._snow, self._ice, self._graupel])
        self._cfg = _lib.MicrophysicsConfig()
        self._cfg.struct_bytes = C.sizeof(_lib.MicrophysicsConfig)

        self.gfdl_cloud_microphys_init(namelist.dt_atmos)
        self._so3 = 7.0 / 3.0
        self._zs = 0.0
        self._fill_config()

    def gfdl_cloud_microphys_init(self, dt_atmos: float):
        self.setupm(dt_atmos)
        self._log_10 = np.log(10.0)
        self._tice0 = self.namelist.tice - 0.01
        # supercooled water can exist down to -48 C, which is the "absolute"
        self._t_wfr = self.namelist.tice - 40.0

    def setupm(self, dt_atmos: float):
        """microphysics.py:2087-2228, operand for operand."""
        gam263 = 1.456943
        gam275 = 1.608355
        gam290 = 1.827363
        gam325 = 2.54925
        gam350 = 3.323363
        gam380 = 4.694155
        # intercept parameters
        rnzs = 3.0e6
        rnzr = 8.0e6
        rnzg = 4.0e6
        # density parameters
        acc = np.array([5.0, 2.0, 0.5])
        pie = 4.0 * np.arctan(1.0)
        # S. Klein's formula (eq 16) from am2
        fac_rc = (4.0 / 3.0) * pie * RHOR * self.namelist.rthresh ** 3
        vdifu = 2.11e-5
        tcond = 2.36e-2
        visk = 1.259e-5
        hlts = 2.8336e6
        hltc = 2.5e6
        hltf = 3.336e5
        ch2o = 4.1855e3
        pisq = pie * pie
        scm3 = (visk / vdifu) ** (1.0 / 3.0)

        cracs = pisq * rnzr * rnzs * RHOS
        csacr = pisq * rnzr * rnzs * RHOR
        cgacr = pisq * rnzr * rnzg * RHOR
        cgacs = pisq * rnzg * rnzs * RHOS
        cgacs = cgacs * self.namelist.c_pgacs

        act = np.empty(8)
        act[0] = pie * rnzs * RHOS
        act[1] = pie * rnzr * RHOR
        act[5] = pie * rnzg * RHOG
        act[2] = act[1]
        act[3] = act[0]
        act[4] = act[1]
        act[6] = act[0]
        act[7] = act[5]

        acco = np.empty((3, 4))
        for i in range(3):
            for k in range(4):
                acco[i, k] = acc[i] / (act[2 * k] ** ((6 - i) * 0.25) * act[2 * k + 1] ** ((i + 1) * 0.25))

        gcon = 40.74 * np.sqrt(SFCRHO)
        # decreasing csacw to reduce cloud water --> snow
        csacw = pie * rnzs * self.namelist.clin * gam325 / (4.0 * act[0] ** 0.8125)
        craci = pie * rnzr * self.namelist.alin * gam380 / (4.0 * act[1] ** 0.95)
        csaci = csacw * self.namelist.c_psaci
        cgacw = pie * rnzg * gam350 * gcon / (4.0 * act[5] ** 0.875)
        cgaci = cgacw * 0.05
        cracw = craci
        cracw = self.namelist.c_cracw * cracw

        # subl and revap: five constants for three separate processes
        self._cssub_0 = 2.0 * pie * vdifu * tcond * constants.RVGAS * rnzs
        self._cssub_1 = 0.78 / np.sqrt(act[0])
        self._cssub_2 = 0.31 * scm3 * gam263 * np.sqrt(self.namelist.clin / visk) / act[0] ** 0.65625
        self._cssub_3 = tcond * constants.RVGAS
        self._cssub_4 = (hlts ** 2) * vdifu

        self._cgsub_0 = 2.0 * pie * vdifu * tcond * constants.RVGAS * rnzg
        self._cgsub_1 = 0.78 / np.sqrt(act[5])
        self._cgsub_2 = 0.31 * scm3 * gam275 * np.sqrt(gcon / visk) / act[5] ** 0.6875
        self._cgsub_3 = self._cssub_3
        self._cgsub_4 = self._cssub_4

        self._crevp_0 = 2.0 * pie * vdifu * tcond * constants.RVGAS * rnzr
        self._crevp_1 = 0.78 / np.sqrt(act[1])
        self._crevp_2 = 0.31 * scm3 * gam290 * np.sqrt(self.namelist.alin / visk) / act[1] ** 0.725
        self._crevp_3 = self._cssub_3
        self._crevp_4 = hltc ** 2 * vdifu

        self._cgfr_0 = 20.0e2 * pisq * rnzr * RHOR / act[1] ** 1.75
        self._cgfr_1 = 0.66

        # smlt: five constants (lin et al. 1983)
        self._csmlt_0 = 2.0 * pie * tcond * rnzs / hltf
        self._csmlt_1 = 2.0 * pie * vdifu * rnzs * hltc / hltf
        self._csmlt_2 = self._cssub_1
        self._csmlt_3 = self._cssub_2
        self._csmlt_4 = ch2o / hltf

        # gmlt: five constants
        self._cgmlt_0 = 2.0 * pie * tcond * rnzg / hltf
        self._cgmlt_1 = 2.0 * pie * vdifu * rnzg * hltc / hltf
        self._cgmlt_2 = self._cgsub_1
        self._cgmlt_3 = self._cgsub_2
        self._cgmlt_4 = ch2o / hltf

        es0 = 6.107799961e2  # ~6.1 mb
        self._fac_rc = fac_rc
        self._cracs = cracs
        self._csacr = csacr
        self._cgacr = cgacr
        self._cgacs = cgacs
        self._acco = acco
        for i in range(3):
            for k in range(4):
                setattr(self, f"_acco{i}{k}", acco[i, k])
        self._csacw = csacw
        self._csaci = csaci
        self._cgacw = cgacw
        self._cgaci = cgaci
        self._cracw = cracw
        self._ces0 = constants.EPS * es0
        self._set_timestep(dt_atmos)

    def _update_timestep_if_needed(self, timestep: float):
        if timestep != self._timestep:
            self._set_timestep(timestep=timestep)
            self._fill_timestep()

    def _set_timestep(self, timestep: float):
        # cloud microphysics sub time step
        self._mpdt: float = min(timestep, self.namelist.mp_time)
        self._rdt: float = 1.0 / timestep
        self._ntimes: int = int(round(timestep / self._mpdt))
        # small time step
        self._dts = timestep / self._ntimes
        self._dt_rain = self._dts * 0.5
        self._rdts = 1.0 / self._dts
        self._dt_evap = 0.5 * self._dts if self.namelist.fast_sat_adj else self._dts
        self._fac_i2s = 1.0 - np.exp(-self._dts / self.namelist.tau_i2s)
        self._fac_g2v = 1.0 - np.exp(-self._dts / self.namelist.tau_g2v)
        self._fac_v2g = 1.0 - np.exp(-self._dts / self.namelist.tau_v2g)
        self._fac_imlt = 1.0 - np.exp(-0.5 * self._dts / self.namelist.tau_imlt)
        self._fac_l2v = 1.0 - np.exp(-self._dt_evap / self.namelist.tau_l2v)
        self._timestep = timestep

    def _fill_timestep(self):
        c = self._cfg
        c.ntimes = self._ntimes
        c.timestep, c.rdt, c.dts, c.rdts, c.dt_rain = self._timestep, self._rdt, self._dts, self._rdts, self._dt_rain
        c.fac_i2s, c.fac_g2v, c.fac_v2g, c.fac_imlt, c.fac_l2v = (self._fac_i2s, self._fac_g2v, self._fac_v2g, self._fac_imlt,
                                                                  self._fac_l2v)

    def _fill_config(self):
        c, nl = self._cfg, self.namelist
        for name in ("c_air", "c_vap", "d0_vap", "lv00", "cpaut", "fac_rc", "so3", "zs", "log_10", "tice0", "t_wfr", "cracs",
                     "csacr", "cgacr", "cgacs", "csacw", "csaci", "cgacw", "cgaci", "cracw", "ces0"):
            setattr(c, name, float(getattr(self, "_" + name)))
        for name in ("tice", "t_sub", "ccn_l", "ccn_o", "dw_land", "dw_ocean", "rh_inc", "rh_inr", "vr_fac", "vr_max", "vi_fac",
                     "vi_max", "vs_fac", "vs_max", "vg_fac", "vg_max", "ql_mlt", "qs_mlt", "qi0_crt", "qs0_crt", "qi_gen",
                     "qi_lim"):
            setattr(c, name, float(getattr(nl, name)))
        for i in range(3):
            for k in range(4):
                c.acco[i][k] = float(self._acco[i, k])
        for name, count in (("cssub", 5), ("crevp", 5), ("cgfr", 2), ("csmlt", 5), ("cgmlt", 5)):
            for m in range(count):
                getattr(c, name)[m] = float(getattr(self, f"_{name}_{m}"))
        self._fill_timestep()

    def __call__(self, state: MicrophysicsState, timestep: float):
        self._update_timestep_if_needed(timestep)
        inputs = [state.pt, state.qvapor, state.qliquid, state.qrain, state.qice, state.qsnow, state.qgraupel, state.ua, state.va,
                  state.delprsi, state.delz, state.land, self._area]
        tendencies = [getattr(state, name) for name in _lib.MICROPHYSICS_TENDENCIES]
        for f in inputs + tendencies + [state.wmp]:
            if f is None:
                raise ValueError("Microphysics needs every field of MicrophysicsState")
        for f in inputs[:11] + tendencies + [state.wmp]:
            t = f.data if hasattr(f, "dims") else f
            if t.dim() != 3:
                raise ValueError(f"field of shape {tuple(t.shape)}: Microphysics takes 3-D fields (land: 2-D)")
        land = state.land.data if hasattr(state.land, "dims") else state.land
        if land.dim() != 2 or tuple(land.stride()) != (1, self._geom.sj):
            raise ValueError(f"land of shape {tuple(land.shape)}, strides {tuple(land.stride())}: a 2-D field of the library's "
                             "layout is needed")
        check_layout(self._geom, *inputs, *tendencies, state.wmp)
        self.call("pace_microphysics", self._workspace.data_ptr(), C.byref(self._cfg), _pointers(inputs), dptr(state.wmp),
                  _pointers(tendencies), self._precip, self.stream())
