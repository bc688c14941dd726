"""RayleighSuper -- the Fortran fv_dynamics.F90's Rayleigh_Super (rf_fast = .false., tau > 0; the reference raises
NotImplementedError there): once per dycore step the sponge levels' u, v and w are damped and the kinetic energy lost is added to
the temperature."""
import ctypes as C
import math

import numpy as np

from ...util import constants
from ._common import Operator, check_layout, dptr, host_column

SECONDS_PER_DAY = 86400.0


class RayleighSuper(Operator):
    """Non-hydrostatic, on a cubed-sphere grid.  The host forms the per-level factor f = 1 / (1 + rf) from grid_data.p once per
    dt and keeps it; a call is one pace_rayleigh_super (two ordered launches with conserve, one without, none where no level lies
    above rf_cutoff) and touches the device nowhere else."""

    def __init__(self, stencil_factory, quantity_factory, grid_data, rf_cutoff, tau, ptop, conserve=True, hydrostatic=False):
        if hydrostatic:
            raise NotImplementedError("RayleighSuper: hydrostatic is not implemented")
        rf_cutoff, tau, ptop = float(rf_cutoff), float(tau), float(ptop)
        if not (math.isfinite(tau) and tau > 0.0):
            raise ValueError(f"RayleighSuper: tau = {tau} days; the damping needs tau > 0")
        if not (math.isfinite(ptop) and ptop > 0.0 and math.isfinite(rf_cutoff) and rf_cutoff > ptop):
            raise ValueError(f"RayleighSuper: rf_cutoff = {rf_cutoff} Pa must lie below the model top, ptop = {ptop} Pa")
        super().__init__(stencil_factory, quantity_factory, grid_data)
        self._a = [grid_data.a11, grid_data.a12, grid_data.a21, grid_data.a22]
        self._rf_cutoff, self._tau, self._ptop, self._conserve = rf_cutoff, tau, ptop, bool(conserve)
        self._pfull = host_column(grid_data.p, self.grid_indexing.domain[2])
        self._rcv = 1.0 / (constants.CP_AIR - constants.RDGAS)
        self._tables = {}  # dt -> the factor table: formed once, then reused

    def rates(self, dt) -> np.ndarray:
        """rf[k] for a dycore step of dt seconds (numpy float64, one per level): dt / (tau * 86400) * sin(0.5 * pi *
        log(rf_cutoff / pfull[k]) / log(rf_cutoff / ptop)) ** 2 on the leading levels with pfull < rf_cutoff, 0.0 elsewhere."""
        dt = float(dt)
        if not (math.isfinite(dt) and dt >= 0.0):
            raise ValueError(f"RayleighSuper: timestep {dt} is not a finite number of seconds >= 0")
        rf = np.zeros(len(self._pfull), dtype=np.float64)
        kmax = 0
        while kmax < len(rf) and self._pfull[kmax] < self._rf_cutoff:
            kmax += 1
        p = self._pfull[:kmax]
        rf[:kmax] = dt / (self._tau * SECONDS_PER_DAY) * np.sin(0.5 * constants.PI * np.log(self._rf_cutoff / p)
                                                                / np.log(self._rf_cutoff / self._ptop)) ** 2
        return rf

    def factors(self, dt) -> np.ndarray:
        """f[k] = 1 / (1 + rf[k]) of rates(dt) (numpy float64, one per level, read-only): exactly 1.0 from the first level with
        pfull >= rf_cutoff on.  Formed once per dt, then reused."""
        dt = float(dt)
        table = self._tables.get(dt)
        if table is None:
            table = 1.0 / (1.0 + self.rates(dt))
            table.setflags(write=False)
            self._tables[dt] = table
        return table

    def __call__(self, u, v, w, pt, dt):
        """u, v: D-grid winds; w: vertical wind; pt: temperature (all in/out); dt: the whole dycore step in seconds."""
        check_layout(self._geom, u, v, w, pt)
        table = self.factors(dt)
        self.call("pace_rayleigh_super", C.byref(self._met), *[dptr(a) for a in self._a], dptr(u), dptr(v), dptr(w), dptr(pt),
                  table.ctypes.data_as(C.POINTER(C.c_double)), self._rcv, int(self._conserve), self.stream())
