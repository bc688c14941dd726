"""EnergyFixer -- the total-energy fixer of consv_te > 0 (the Fortran FV3's compute_total_energy and the consv > consv_min block of
Lagrangian_to_Eulerian; the reference carries te_2d / te0_2d / dtmp and stops at the global sum, remapping.py:618-622).

The object owns the buffers of one rank -- the ten fixed-point words, the planes te_2d and zsum1 and the four result doubles -- and
the communicator the global sum goes through.  include/pace_hip.h has the arithmetic of the three entry points:

    fixer.total_energy(0, ...)             DynamicalCore.compute_preamble: te0_2d from the state at the top of the step
    fixer.total_energy(1, ...)             LagrangianToEulerian, last remapping step, after the remap of v: te_2d, zsum1, the words
    result = fixer.finalize(consv_te, dt)  the global sum: comm.allreduce_fixed_point (pace_amd/util/comm.py), whose finalising
                                           launch writes S_te, S_z, dtmp, e_flux to four doubles ON THE DEVICE
    pace_l2e_finish_dtmp reads dtmp from `result`; the host never needs it.  fixer.diagnostics() copies the four doubles on demand.

The sum is a fixed-point sum in integers: bitwise the same for every summation order, tile partition and communicator."""
import ctypes as C

import torch

from ... import _lib
from ...util.constants import X_DIM, Y_DIM
from ._common import Operator, check_layout, dptr
from .fillz import pointer_table

MAX_ADDENDS = 1 << 23  # 40-bit limbs in 64-bit words (minus the sign): the headroom of the accumulator


def _raw_comm(comm):
    """The transport of a CubedSphereCommunicator, or the transport itself."""
    return comm.comm if hasattr(comm, "comm") and not hasattr(comm, "allreduce_fixed_point") else comm


class EnergyFixer(Operator):
    def __init__(self, stencil_factory, quantity_factory, comm, total_tiles: int = 6):
        super().__init__(stencil_factory, quantity_factory)
        self._comm = _raw_comm(comm)
        if not hasattr(self._comm, "allreduce_fixed_point"):
            raise ValueError(f"EnergyFixer: {self._comm!r} has no allreduce_fixed_point: the global sum needs a communicator")
        n = self._geom.n
        if total_tiles * n * n >= MAX_ADDENDS:
            raise ValueError(f"EnergyFixer: {total_tiles} x {n} x {n} columns: the fixed-point sum holds fewer than 2^23 addends")
        qf = quantity_factory
        self.te_2d = qf.zeros([X_DIM, Y_DIM], units="J/m^2")
        self.zsum1 = qf.zeros([X_DIM, Y_DIM], units="Pa")
        self.words = torch.zeros(_lib.ENERGY_WORDS, dtype=torch.int64, device=self._device)
        self._own_result = torch.zeros(4, dtype=torch.float64, device=self._device)
        self.result = self._own_result  # after finalize(): the buffer the finalising launch wrote (one for the whole cube)
        self.finalized = False

    def total_energy(self, mode, water, pt, delp, delz, w, u, v, pkz, phis, rsin2, cosa_s, area, te0_2d, zvir):
        """One pace_energy_columns launch.  mode 0 writes te0_2d (pkz, area may be None); mode 1 reads it, writes this object's
        te_2d and zsum1 and fills its (zeroed) words."""
        check_layout(self._geom, pt, delp, delz, w, u, v, pkz, phis, rsin2, cosa_s, area, te0_2d)
        if mode == 1:
            self.words.zero_()
        self.call("pace_energy_columns", int(mode), pointer_table(water), dptr(pt), dptr(delp), dptr(delz), dptr(w), dptr(u),
                  dptr(v), dptr(pkz), dptr(phis), dptr(rsin2), dptr(cosa_s), dptr(area), dptr(te0_2d),
                  dptr(self.te_2d) if mode == 1 else None, dptr(self.zsum1) if mode == 1 else None,
                  C.c_void_p(self.words.data_ptr()) if mode == 1 else None, float(zvir), self.stream())

    def finalize(self, consv_te: float, dt_atmos: float):
        """The global sum and the four doubles.  -> the device buffer that holds them (DeviceCubeComm: one for the six ranks)."""
        stream = self.stream()

        def launch(buffers):
            table = (C.c_void_p * len(buffers))(*[b.data_ptr() for b in buffers])
            self.lib.call("pace_energy_finalize", table, len(buffers), float(consv_te), float(dt_atmos),
                          self._own_result.data_ptr(), stream)
            return self._own_result

        self.result = self._comm.allreduce_fixed_point(self.words, launch, stream=stream)
        self.finalized = True
        return self.result

    def diagnostics(self):
        """{"dtmp", "e_flux", "te_deficit", "zsum"} of the last finalize() as Python floats: one small transfer, on demand."""
        if not self.finalized:
            raise RuntimeError("EnergyFixer.diagnostics: no step with consv_te > 0 has run yet")
        s_te, s_z, dtmp, e_flux = (float(x) for x in self.result.detach().cpu().tolist())
        return {"dtmp": dtmp, "e_flux": e_flux, "te_deficit": s_te, "zsum": s_z}
