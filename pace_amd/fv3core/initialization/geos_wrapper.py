"""GeosDycoreWrapper -- the dycore under a host model (reference: fv3core/pace/fv3core/initialization/geos_wrapper.py).

    wrapper = GeosDycoreWrapper(namelist, comm, backend)
    out = wrapper(u, v, w, delz, pt, delp, q, ps, pe, pk, peln, pkz, phis, q_con, omga, ua, va, uc, vc, mfxd, mfyd, cxd, cyd,
                  diss_estd)                               # numpy arrays in, a dict of numpy arrays out, once per physics step

The reference assigns 30 windows into its state and 30 out of it, array by array.  Here a call is

    move_to_pace     every argument's window is copied (np.copyto) into its slot of ONE pinned float64 staging buffer -- C-ordered,
                     or F-ordered where the argument is F-contiguous, so that the host copy runs along the argument's own memory --
                     then ONE host-to-device copy and ONE pace_state_unpack launch (pace_amd/csrc/k_state.hip) with 30 items, which
                     transposes the C-ordered slots, picks the seven species out of q and narrows for the float32 library;
    dycore           DynamicalCore.step_dynamics;
    move_to_fortran  ONE pace_diag_pack launch with 30 float64 items, ONE transfer and ONE synchronisation
                     (pace_amd.driver.WindowPacker).

What the windows do not cover -- the halos, level nz of the centred fields, qo3mr and qsgs_tke -- keeps its value from the
previous call, as in the reference.  The returned arrays are views of the pinned host buffer and are overwritten by the next call,
as the reference reuses its output arrays.
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor
from datetime import timedelta
from typing import Dict

import numpy as np
import torch

from ... import _launch, _lib
from ...util import CubedSphereCommunicator, Timer
from ...util.constants import N_HALO_DEFAULT
from .._config import DynamicalCoreConfig
from .dycore_state import DycoreState

ARGUMENTS = ("u", "v", "w", "delz", "pt", "delp", "q", "ps", "pe", "pk", "peln", "pkz", "phis", "q_con", "omga", "ua", "va", "uc",
             "vc", "mfxd", "mfyd", "cxd", "cyd", "diss_estd")
# the species of q's last axis (geos_wrapper.py:252-270)
TRACERS = ("qvapor", "qliquid", "qice", "qrain", "qsnow", "qgraupel", "qcld")
# the order of the reference's output dictionary (geos_wrapper.py:382-440)
OUTPUTS = ("u", "v", "w", "ua", "va", "uc", "vc", "delz", "pt", "delp", "mfxd", "mfyd", "cxd", "cyd", "ps", "pe", "pk", "peln",
           "pkz", "phis", "q_con", "omga", "diss_estd") + TRACERS
_CENTRED = ("w", "ua", "va", "delz", "pt", "delp", "q_con", "omga", "diss_estd")


def windows(n: int, nz: int):
    """-> (ingest, export) for a C<n> x <nz> tile, by the reference's slices (geos_wrapper.py:207-270 and 282-378).
    ingest: argument -> (the argument's shape, the slices of it that are taken, the destination window (i0, j0, k0, ni, nj, nk) in
    the storage); export: output -> the window of the storage.  2-D fields have nk = 1."""
    h = N_HALO_DEFAULT
    full = n + 2 * h
    c, c1, whole = slice(h, h + n), slice(h, h + n + 1), slice(None)
    ingest = {"u": ((full, full + 1, nz), (c, c1), (h, h, 0, n, n + 1, nz)),
              "v": ((full + 1, full, nz), (c1, c), (h, h, 0, n + 1, n, nz)),
              "mfxd": ((n + 1, n, nz), (whole, whole), (h, h, 0, n + 1, n, nz)),
              "mfyd": ((n, n + 1, nz), (whole, whole), (h, h, 0, n, n + 1, nz)),
              "cxd": ((n + 1, full, nz), (whole, c), (h, h, 0, n + 1, n, nz)),
              "cyd": ((full, n + 1, nz), (c, whole), (h, h, 0, n, n + 1, nz)),
              "pe": ((n + 2, n + 2, nz + 1), (whole, whole), (h - 1, h - 1, 0, n + 2, n + 2, nz + 1)),
              "pk": ((n, n, nz + 1), (whole, whole), (h, h, 0, n, n, nz + 1)),
              "peln": ((n, n, nz + 1), (whole, whole), (h, h, 0, n, n, nz + 1)),
              "pkz": ((n, n, nz), (whole, whole), (h, h, 0, n, n, nz)),
              "ps": ((full, full), (c, c), (h, h, 0, n, n, 1)),
              "phis": ((full, full), (c, c), (h, h, 0, n, n, 1)),
              "q": ((full, full, nz, len(TRACERS)), (c, c), (h, h, 0, n, n, nz))}
    ingest["uc"], ingest["vc"] = ingest["v"], ingest["u"]
    for name in _CENTRED:
        ingest[name] = ((full, full, nz), (c, c), (h, h, 0, n, n, nz))
    export = {"u": (0, 0, 0, full, full + 1, nz), "v": (0, 0, 0, full + 1, full, nz),
              "mfxd": (h, h, 0, n + 1, n, nz), "mfyd": (h, h, 0, n, n + 1, nz),
              "cxd": (h, 0, 0, n + 1, full, nz), "cyd": (0, h, 0, full, n + 1, nz),
              "ps": (0, 0, 0, full, full, 1), "phis": (0, 0, 0, full, full, 1),
              "pe": ingest["pe"][2], "pk": ingest["pk"][2], "peln": ingest["peln"][2], "pkz": ingest["pkz"][2]}
    export["uc"], export["vc"] = export["v"], export["u"]
    for name in _CENTRED + TRACERS:
        export[name] = (0, 0, 0, full, full, nz)
    return {name: ingest[name] for name in ARGUMENTS}, {name: export[name] for name in OUTPUTS}


class PerformanceCollector:
    """The wrapper's timer (the reference makes a pace.driver PerformanceCollector("GEOS wrapper", comm) and writes a report
    for rank 0 after every call; no file is written here): `timestep_timer` clocks move_to_pace, dycore and move_to_fortran,
    and what the dynamical core clocks inside its step."""

    def __init__(self, experiment_name: str, comm):
        self.experiment_name = experiment_name
        self.comm = comm
        self.timestep_timer = Timer()
        self.total_timer = Timer()


class GeosDycoreWrapper:
    """
    Provides an interface for the Geos model to access the Pace dycore.
    Takes numpy arrays as inputs, returns a dictionary of numpy arrays as outputs
    """

    staging_threads = 4  # host threads that copy the arguments' windows into the staging buffer (1: the calling thread alone)

    def __init__(self, namelist, comm, backend: str, lib=None, device=None):
        """
        Args:
            namelist: any mapping (an f90nml.Namelist is one) in one of the two forms of DynamicalCoreConfig.from_f90nml
            comm: communication object behaving like pace_amd.util.TorchDistComm / ThreadComm / NullComm
            backend: kept; the backend is always hip:gfx950
            lib: the kernel library (default: the product library, pace_amd._lib.load())
            device: where the fields live (default: the current device; "cpu" with the emulation test library)
        """
        from ...driver.diagnostics import WindowPacker  # (pace_amd.driver imports pace_amd.fv3core)
        from ...tile import setup_factories
        from ...util.grid import DampingCoefficients, GridData, MetricTerms, geom_struct
        from ..stencils.fv_dynamics import DynamicalCore

        self.perf_collector = PerformanceCollector("GEOS wrapper", comm)
        self.backend = backend
        self.namelist = namelist
        self.dycore_config = DynamicalCoreConfig.from_f90nml(namelist)
        self.layout = self.dycore_config.layout
        if tuple(self.layout) != (1, 1):
            raise NotImplementedError(f"layout {tuple(self.layout)}: pace_amd maps one cubed-sphere tile per device, layout must be (1, 1)")
        self._lib = lib if lib is not None else _lib.load()
        self.device = device = torch.device(device) if device is not None else _launch.default_device(self._lib)
        self.communicator = CubedSphereCommunicator(comm, device=device, lib=self._lib)
        self._n, self._nz = self.dycore_config.npx - 1, self.dycore_config.npz
        _, quantity_factory, self._grid_indexing, stencil_factory = setup_factories(
            self._lib, device, self._n, self._nz, layout=self.layout, communicator=self.communicator)
        self._geom = geom_struct(quantity_factory)

        # set up the metric terms and grid data
        metric_terms = MetricTerms(quantity_factory=quantity_factory, communicator=self.communicator)
        grid_data = GridData.new_from_metric_terms(metric_terms)
        damping_coefficients = DampingCoefficients.new_from_metric_terms(metric_terms, grid_data)

        self.dycore_state = DycoreState.init_zeros(quantity_factory=quantity_factory)
        # geos_wrapper.py:72-82
        if "fv_core_nml" in namelist.keys():
            group = namelist["fv_core_nml"]
        elif "dycore_config" in namelist.keys():
            group = namelist["dycore_config"]
        else:
            group = {}
        if "k_split" not in group:
            raise KeyError("Cannot find k_split in namelist")
        self.dycore_state.bdt = self.dycore_config.dt_atmos / group["k_split"]

        self.dynamical_core = DynamicalCore(
            comm=self.communicator, grid_data=grid_data, stencil_factory=stencil_factory, quantity_factory=quantity_factory,
            damping_coefficients=damping_coefficients, config=self.dycore_config,
            timestep=timedelta(seconds=self.dycore_config.dt_atmos), phis=self.dycore_state.phis, state=self.dycore_state)

        self._ingest, self._export = windows(self._n, self._nz)
        self._slots, total = {}, 0
        for name, (_, _, window) in self._ingest.items():
            self._slots[name] = total
            total += int(np.prod(window[3:])) * (len(TRACERS) if name == "q" else 1)
        self._staged, self._staging = _launch.staging(total, torch.float64, self.device)
        self._staging_array = self._staging.numpy()
        self._packer = WindowPacker(self._lib)
        self._pool = None
        self.output_dict: Dict[str, np.ndarray] = {}

    # ---- in --------------------------------------------------------------------------------------------------------------------
    def _slot(self, name, shape, f_order):
        """The argument's slot of the staging buffer as an array of `shape`, C- or F-ordered."""
        flat = self._staging_array[self._slots[name]:self._slots[name] + int(np.prod(shape))]
        return flat.reshape(shape[::-1]).T if f_order else flat.reshape(shape)

    # the call's one host-to-device copy (the call goes through this name: the one-transfer test counts it here)
    _to_device = staticmethod(_launch.to_device)

    def _stage(self, copies):
        """The host copies of a call, (slot, window of the argument) each: one np.copyto per argument, spread over
        staging_threads threads (numpy copies without the interpreter lock), the largest first."""
        if self.staging_threads <= 1:
            for slot, source in copies:
                np.copyto(slot, source)
            return
        if self._pool is None:
            self._pool = ThreadPoolExecutor(max_workers=self.staging_threads)
        copies = sorted(copies, key=lambda copy: -copy[0].size)
        for done in [self._pool.submit(np.copyto, slot, source) for slot, source in copies]:
            done.result()

    def _put_fortran_data_in_dycore(self, *arguments) -> DycoreState:
        state = self.dycore_state
        items = (_lib.UnpackItem * (len(ARGUMENTS) - 1 + len(TRACERS)))()
        m, copies = 0, []
        for name, a in zip(ARGUMENTS, arguments):
            shape, cut, window = self._ingest[name]
            f_order = a.flags.f_contiguous and not a.flags.c_contiguous
            extent = window[3:] if len(shape) > 2 else window[3:5]
            offset = self._slots[name]
            if name == "q":
                copies.append((self._slot(name, extent + (len(TRACERS),), f_order), a[cut]))
                fields = [(getattr(state, tracer), offset + t * int(np.prod(extent)) if f_order else offset + t,
                           1 if f_order else len(TRACERS)) for t, tracer in enumerate(TRACERS)]
            else:
                copies.append((self._slot(name, extent, f_order), a[cut]))
                fields = [(getattr(state, name), offset, 1)]
            for field, in_offset, in_step in fields:
                item = items[m]
                _launch.set_window(item, _launch.window_of(field, window=window))  # (THIS call's storage: the step swaps storages)
                item.order = _lib.ORDER_XFAST if f_order else _lib.ORDER_ZFAST
                item.in_step, item.in_offset = in_step, in_offset
                m += 1
        self._stage(copies)
        self._to_device(self._staging, self._staged)
        self._lib.call("pace_state_unpack", C.byref(self._geom), items, m, C.c_void_p(self._staged.data_ptr()),
                       _launch.stream_of(self.device))
        return state

    # ---- out -------------------------------------------------------------------------------------------------------------------
    def _prep_outputs_for_geos(self) -> Dict[str, np.ndarray]:
        from ...driver.diagnostics import _Request

        requests = []
        for name, window in self._export.items():
            field = getattr(self.dycore_state, name)
            kind = _lib.DIAG_WINDOW3D if len(field.dims) == 3 else _lib.DIAG_PLANE
            requests.append(_Request(name, kind, field, None, 0, window, tuple(field.dims), field.units))
        packed = self._packer.pack(requests, out_is_double=True)
        return {name: quantity.data.numpy() for name, quantity in packed.items()}

    def __call__(self, u, v, w, delz, pt, delp, q, ps, pe, pk, peln, pkz, phis, q_con, omga, ua, va, uc, vc, mfxd, mfyd, cxd, cyd,
                 diss_estd) -> Dict[str, np.ndarray]:
        arguments = [np.asarray(a) for a in (u, v, w, delz, pt, delp, q, ps, pe, pk, peln, pkz, phis, q_con, omga, ua, va, uc, vc, mfxd,
                                             mfyd, cxd, cyd, diss_estd)]
        for name, a in zip(ARGUMENTS, arguments):  # (before anything is staged or clocked)
            if a.shape != self._ingest[name][0]:
                raise ValueError(f"{name}: expected an array of shape {self._ingest[name][0]}, got {a.shape}")
        timer = self.perf_collector.timestep_timer
        with timer.clock("move_to_pace"):
            self.dycore_state = self._put_fortran_data_in_dycore(*arguments)
        with timer.clock("dycore"):
            self.dynamical_core.step_dynamics(state=self.dycore_state, timer=timer)
        with timer.clock("move_to_fortran"):
            self.output_dict = self._prep_outputs_for_geos()
        return self.output_dict
