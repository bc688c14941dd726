"""TracerAdvection -- Fortran tracer_2d_1l (reference: fv3core/pace/fv3core/stencils/tracer_2d_1l.py:171-392).

Two modes.  The default is the reference's: cmax fixed at 2.0, so every level takes n_split = 3 sub-cycles.  With
``courant_subcycling=True`` the operator does what the Fortran model does (tracer_2d_1L: mp_reduce_max(cmax, npz), level k
sub-cycled int(1. + cmax(k)) times; the reference keeps the two cmax stencils, :103-112, and their call site, :312-339, commented
out behind "TODO mpi allreduce"): one pace_tracer_cmax launch, the maximum over the globe through
``comm.allreduce_level_max`` (pace_amd/util/comm.py), whose finalising launch turns it into sub-cycle counts, and ONE transfer of
those nk + 2 integers -- the mode's one synchronisation with the host per call, as the Fortran's reduction is.  The sub-cycles
then run the `_levels` forms of the stencils, and the unchanged transport once per maximal run of consecutive levels that still
have a sub-cycle to take.  include/pace_hip.h has the arithmetic."""
import ctypes as C
import math
from typing import Dict

import numpy as np
import torch

from ... import _lib
from ...util.constants import X_DIM, X_INTERFACE_DIM, Y_DIM, Y_INTERFACE_DIM, Z_DIM
from ...util.halo import WrappedHaloUpdater
from ._common import Operator, check_layout, dptr
from .fvtp2d import FiniteVolumeTransport


def level_runs(ksplt, it):
    """[(k0, nlev)]: the maximal runs of consecutive levels with ksplt[k] > it, in order."""
    runs, k0 = [], None
    for k, s in enumerate(ksplt):
        if s > it:
            if k0 is None:
                k0 = k
        elif k0 is not None:
            runs.append((k0, k - k0))
            k0 = None
    if k0 is not None:
        runs.append((k0, len(ksplt) - k0))
    return runs


class SubcycleCounts(np.ndarray):
    """The nk + 2 integers of pace_tracer_subcycles on the host, with the device buffer they were copied from."""

    device = None


class TracerAdvection(Operator):
    """Performs horizontal advection on tracers: sub-cycled monotone-PPM transport of every tracer with the mass fluxes and
    Courant numbers accumulated over the acoustic substeps.  n_split = 3 on every level (the reference hard-codes cmax = 2.0), or,
    with courant_subcycling, int(1 + cmax(k)) on level k with cmax(k) the level's largest Courant number over the globe; a level
    that would need more than max_subcycles, or whose Courant number is not finite, raises FloatingPointError before anything of
    the caller's is modified.  `subcycles`: the counts of the last call (numpy int32, one per level)."""

    def __init__(self, stencil_factory, quantity_factory, transport: FiniteVolumeTransport, grid_data, comm,
                 tracers: Dict[str, object], courant_subcycling: bool = False, max_subcycles: int = 16):
        super().__init__(stencil_factory, quantity_factory, grid_data)
        self._tracer_count = len(tracers)
        self.grid_data = grid_data
        self._x_area_flux = quantity_factory.zeros([X_INTERFACE_DIM, Y_DIM, Z_DIM], units="unknown")
        self._y_area_flux = quantity_factory.zeros([X_DIM, Y_INTERFACE_DIM, Z_DIM], units="unknown")
        self._x_flux = quantity_factory.zeros([X_INTERFACE_DIM, Y_INTERFACE_DIM, Z_DIM], units="unknown")
        self._y_flux = quantity_factory.zeros([X_INTERFACE_DIM, Y_INTERFACE_DIM, Z_DIM], units="unknown")
        self._tmp_dp = quantity_factory.zeros([X_DIM, Y_DIM, Z_DIM], units="Pa")
        self.finite_volume_transport = transport
        spec = quantity_factory.get_quantity_halo_spec([X_DIM, Y_DIM, Z_DIM], n_halo=3)
        self._tracers_halo_updater = WrappedHaloUpdater(comm.get_scalar_halo_updater([spec] * self._tracer_count), tracers,
                                                        [t for t in tracers.keys()])
        self._courant_subcycling = bool(courant_subcycling)
        self.subcycles = None
        if self._courant_subcycling:
            self._max_subcycles = int(max_subcycles)
            if not 1 <= self._max_subcycles <= _lib.TRACER_MAX_SUBCYCLES:
                raise ValueError(f"TracerAdvection: max_subcycles = {max_subcycles} outside 1 .. {_lib.TRACER_MAX_SUBCYCLES}")
            if getattr(grid_data, "sin_sg5", None) is None:
                raise ValueError("TracerAdvection(courant_subcycling=True): the grid data have no sin_sg5 (the cell-centre sine "
                                 "of the Courant number's widened form); pace_amd.util.gridgen.MetricTerms generates it")
            transport_comm = comm.comm if hasattr(comm, "comm") and not hasattr(comm, "allreduce_level_max") else comm
            if not hasattr(transport_comm, "allreduce_level_max"):
                raise ValueError(f"TracerAdvection(courant_subcycling=True): {transport_comm!r} has no allreduce_level_max")
            self._reduce_comm = transport_comm
            nk = self._geom.nk
            if nk > _lib.TRACER_MAX_LEVELS:
                raise ValueError(f"TracerAdvection(courant_subcycling=True): {nk} levels, at most {_lib.TRACER_MAX_LEVELS}")
            self._cmax = torch.zeros(nk, dtype=torch.float64, device=self._device)
            self._counts = torch.zeros(nk + 2, dtype=torch.int32, device=self._device)  # [largest, refused, ksplt[0 .. nk - 1]]
            self._counts_host = torch.zeros(nk + 2, dtype=torch.int32, pin_memory=not self._emu)

    def __call__(self, tracers, dp1, x_mass_flux, y_mass_flux, x_courant, y_courant):
        check_layout(self._geom, dp1, x_mass_flux, y_mass_flux, x_courant, y_courant, *tracers.values())
        if self._courant_subcycling:
            return self._call_courant(tracers, dp1, x_mass_flux, y_mass_flux, x_courant, y_courant)
        met, st = C.byref(self._met), self.stream
        self.call("pace_tracer_flux_compute", met, dptr(x_courant), dptr(y_courant), dptr(self._x_area_flux),
                  dptr(self._y_area_flux), st())
        cmax_max_all_ranks = 2.0  # tracer_2d_1l.py:336-339
        n_split = math.floor(1.0 + cmax_max_all_ranks)
        if n_split > 1.0:
            self.call("pace_tracer_divide_fluxes", dptr(x_courant), dptr(self._x_area_flux), dptr(x_mass_flux), dptr(y_courant),
                      dptr(self._y_area_flux), dptr(y_mass_flux), int(n_split), st())
        self._tracers_halo_updater.update()
        dp2 = self._tmp_dp
        for it in range(n_split):
            last_call = it == n_split - 1
            self.call("pace_apply_mass_flux", met, dptr(dp1), dptr(x_mass_flux), dptr(y_mass_flux), dptr(dp2), st())
            for q in tracers.values():
                self.finite_volume_transport(q, x_courant, y_courant, self._x_area_flux, self._y_area_flux, self._x_flux,
                                             self._y_flux, x_mass_flux=x_mass_flux, y_mass_flux=y_mass_flux)
                self.call("pace_apply_tracer_flux", met, dptr(q), dptr(dp1), dptr(self._x_flux), dptr(self._y_flux), dptr(dp2), st())
            if not last_call:
                self._tracers_halo_updater.update()
                self.call("pace_swap_dp", dptr(dp1), dptr(dp2), st())

    # ---- Courant-number sub-cycling per level ----
    def _transfer_counts(self):
        """The one transfer of a call, device to host through the pinned buffer, and its one synchronisation.  -> numpy int32"""
        if self._emu:
            self._counts_host.copy_(self._counts)
        else:
            self._counts_host.copy_(self._counts, non_blocking=True)
            torch.cuda.current_stream(self._device).synchronize()
        return self._counts_host.numpy().copy()

    def _subcycle_counts(self):
        """cmax over the globe -> the host array [largest, refused, ksplt[0 .. nk - 1]] (numpy int32; a SubcycleCounts, whose
        `device` is the device buffer that holds the same integers: this rank's, or, where one launch served the whole cube
        (DeviceCubeComm), the launching rank's -- every rank's `_levels` launches read that one buffer, on the one stream)."""
        stream = self.stream()

        def finalize(buffers):
            table = (C.c_void_p * len(buffers))(*[b.data_ptr() for b in buffers])
            self.lib.call("pace_tracer_subcycles", table, len(buffers), self._geom.nk, self._max_subcycles,
                          C.c_void_p(self._counts.data_ptr()), stream)
            counts = self._transfer_counts().view(SubcycleCounts)
            counts.device = self._counts
            return counts

        return self._reduce_comm.allreduce_level_max(self._cmax, finalize, stream=stream)

    def _call_courant(self, tracers, dp1, x_mass_flux, y_mass_flux, x_courant, y_courant):
        met, st = C.byref(self._met), self.stream
        self.call("pace_tracer_flux_compute", met, dptr(x_courant), dptr(y_courant), dptr(self._x_area_flux),
                  dptr(self._y_area_flux), st())
        self._cmax.zero_()
        self.call("pace_tracer_cmax", dptr(x_courant), dptr(y_courant), dptr(self.grid_data.sin_sg5),
                  C.c_void_p(self._cmax.data_ptr()), st())
        counts = self._subcycle_counts()
        ksplt = np.asarray(counts)[2:]
        if counts[1] != 0:
            levels = [int(k) for k in np.flatnonzero(ksplt == 0)]
            raise FloatingPointError(f"TracerAdvection: the Courant number of level(s) {levels} is not finite or asks for more "
                                     f"than max_subcycles = {self._max_subcycles} sub-cycles; the tracers are untouched")
        self.subcycles = np.array(ksplt, dtype=np.int32)
        kdev = C.c_void_p(counts.device.data_ptr() + 2 * 4)
        n_split = int(counts[0])
        if n_split > 1:
            self.call("pace_tracer_divide_fluxes_levels", dptr(x_courant), dptr(self._x_area_flux), dptr(x_mass_flux),
                      dptr(y_courant), dptr(self._y_area_flux), dptr(y_mass_flux), kdev, st())
        self._tracers_halo_updater.update()
        dp2 = self._tmp_dp
        for it in range(n_split):
            last_call = it == n_split - 1
            runs = level_runs(ksplt, it)
            self.call("pace_apply_mass_flux_levels", met, dptr(dp1), dptr(x_mass_flux), dptr(y_mass_flux), dptr(dp2), kdev,
                      it + 1, st())
            for q in tracers.values():
                for run in runs:
                    self.finite_volume_transport(q, x_courant, y_courant, self._x_area_flux, self._y_area_flux, self._x_flux,
                                                 self._y_flux, x_mass_flux=x_mass_flux, y_mass_flux=y_mass_flux, levels=run)
                self.call("pace_apply_tracer_flux_levels", met, dptr(q), dptr(dp1), dptr(self._x_flux), dptr(self._y_flux),
                          dptr(dp2), kdev, it + 1, st())
            if not last_call:
                self._tracers_halo_updater.update()
                self.call("pace_swap_dp_levels", dptr(dp1), dptr(dp2), kdev, it + 2, st())
