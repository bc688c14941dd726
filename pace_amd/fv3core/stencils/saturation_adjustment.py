"""SatAdjust3d -- the fast saturation adjustment of the GFDL microphysics (reference:
fv3core/pace/fv3core/stencils/saturation_adjustment.py:947-1108), non-hydrostatic.

The saturation tables the stencil interpolates from (table2, des2, tablew, desw) are built once per object into a device
buffer of this object (pace_sat_adjust_tables); each call is one launch of pace_sat_adjust over the reference's window,
origin (isc, jsc, kmp), domain (nx, ny, nz - kmp)."""
import ctypes as C
import math

import torch

from ... import _lib
from ...util import constants
from .._config import SatAdjustConfig
from ._common import Operator, check_layout, dptr
from .fillz import pointer_table


def _check_2d(geom, *fields):
    """The kernel reads hs and area as 2-D fields of the library's storage type with the row stride of the 3-D fields."""
    for f in fields:
        t = f.data if hasattr(f, "dims") else f
        if t.dim() != 2 or tuple(t.stride()) != (1, geom.sj):
            raise ValueError(f"2-D field of shape {tuple(t.shape)} and layout {tuple(t.stride())} does not match (1, {geom.sj}); "
                             "allocate it with pace_amd.util.QuantityFactory")


class SatAdjust3d(Operator):
    def __init__(self, stencil_factory, config: SatAdjustConfig, area_64, kmp, quantity_factory=None):
        """As the reference's (stencil_factory, config, area_64, kmp); the field layout is the stencil factory's quantity
        factory unless one is given."""
        if config.hydrostatic:
            raise NotImplementedError("Hydrostatic is not implemented")
        if area_64 is None:
            raise ValueError("SatAdjust3d needs the cell area (grid_data.area_64)")
        qf = quantity_factory if quantity_factory is not None else stencil_factory.quantity_factory
        if qf is None:
            raise ValueError("SatAdjust3d needs the field layout: a StencilFactory with a quantity_factory")
        super().__init__(stencil_factory, qf)
        self._config = config
        self._area_64 = area_64
        self._kmp = int(kmp)
        nk = self._geom.nk
        if not 0 <= self._kmp < nk:
            raise ValueError(f"kmp = {kmp} is outside the {nk} levels")
        self._tables = torch.empty(_lib.SAT_ADJUST_TABLE_DOUBLES, dtype=torch.float64, device=qf.device)
        self.lib.call("pace_sat_adjust_tables", dptr(self._tables), self.stream())
        p = _lib.SatAdjustParams()
        for name in ("hydrostatic", "rad_snow", "rad_rain", "rad_graupel", "tintqs", "icloud_f"):
            setattr(p, name, int(getattr(config, name)))
        for name in ("sat_adj0", "ql_gen", "qs_mlt", "ql0_max", "t_sub", "qi_gen", "qi_lim", "qi0_max", "dw_ocean", "dw_land",
                     "cld_min"):
            setattr(p, name, float(getattr(config, name)))
        self._params = p

    def __call__(self, te, qvapor, qliquid, qice, qrain, qsnow, qgraupel, qcld, hs, peln, delp, delz, q_con, pt, pkz, cappa,
                 r_vir: float, mdt: float, fast_mp_consv: bool, last_step: bool, akap: float, kmp: int):
        """Same arguments as the reference (:982-1003): te (out, only if fast_mp_consv); qvapor .. qgraupel, pt (inout); qcld
        (out, on the last step); hs, delp, delz (in); q_con, pkz, cappa (out); peln, akap, kmp (unused)."""
        check_layout(self._geom, te, qvapor, qliquid, qice, qrain, qsnow, qgraupel, qcld, delp, delz, q_con, pt, pkz, cappa, hs,
                     self._area_64)
        _check_2d(self._geom, hs, self._area_64)
        cfg = self._config
        mdt = float(mdt)
        sdt = 0.5 * mdt  # half remapping time step
        # conversion factors (:1038-1069)
        p = self._params
        p.sdt = sdt
        p.zvir = float(r_vir)
        p.mdt = mdt
        p.fac_i2s = 1.0 - math.exp(-mdt / cfg.tau_i2s)
        p.fac_v2l = 1.0 - math.exp(-sdt / cfg.tau_v2l)
        p.fac_r2g = 1.0 - math.exp(-mdt / cfg.tau_r2g)
        p.fac_l2r = 1.0 - math.exp(-mdt / cfg.tau_l2r)
        p.fac_l2v = min(cfg.sat_adj0, 1.0 - math.exp(-sdt / cfg.tau_l2v))
        p.fac_imlt = 1.0 - math.exp(-sdt / cfg.tau_imlt)
        p.fac_smlt = 1.0 - math.exp(-mdt / cfg.tau_smlt)
        p.c_air = constants.CV_AIR
        p.c_vap = constants.CV_VAP
        p.d0_vap = p.c_vap - constants.C_LIQ
        p.lv00 = constants.HLV - p.d0_vap * constants.TICE
        p.do_qa = 1  # (:1071)
        water = pointer_table([qvapor, qliquid, qrain, qsnow, qice, qgraupel])
        consv = bool(fast_mp_consv)
        self.call("pace_sat_adjust", water, dptr(qcld), dptr(te) if consv else None, dptr(pt), dptr(q_con), dptr(pkz),
                  dptr(cappa), dptr(delp), dptr(delz), dptr(self._area_64), dptr(hs), dptr(self._tables), C.byref(p),
                  self._kmp, int(bool(last_step)), int(consv), self.stream())
