"""open_restart -- the restart files of the Fortran model into a state (reference: util/pace/util/_legacy_restart.py).

    state = open_restart(dirname, communicator)                         # host variables, as the files hold them
    open_restart(dirname, communicator, to_state={name: quantity})      # into device Quantities

The rank's tile decides the files: [label.]fv_core.res.tile<t + 1>.nc, fv_tracer.res..., fv_srf_wnd.res... where present, and
[label.]coupler.res for `time`.  FMS writes NetCDF-3 (64-bit offset); the files are opened by the checkpointer's opener
(checkpointer/validation.py), which reads NetCDF-4 where a reader for it is installed.  A variable is known by RESTART_PROPERTIES
(standard name -> restart name, dims, units; `tracer_properties` extends it); one without an entry is dropped.

Without `to_state` the result maps standard names to RestartVariable: the file's array of the one Time level in file order
(z, y, x), native-endian float64, with dims and units.  A stated departure: the reference returns (z, y, x) Quantities, and a
pace_amd Quantity is always (x, y, z) on the device.

With `to_state` the compute domains of the given device Quantities are filled: every variable is copied (np.copyto: byte order
made native, float32 widened) into its slot of ONE pinned float64 staging buffer, then ONE host-to-device copy and ONE
pace_state_unpack launch (pace_amd/csrc/k_state.hip; more only above 32 variables).  The items are PACE_ORDER_XFAST -- the file's
(z, y, x) C order is the storage's own order, nothing is transposed -- and PACE_DIAG_PLANE for a 2-D variable; the float32
library narrows on the device.  Halos and the levels below the file's keep what they held.
"""
import ctypes as C
import dataclasses
import os
from datetime import datetime
from typing import Iterable, Optional, Tuple

import numpy as np
import torch

from .. import _lib
from .checkpointer.validation import _open_nc
from .constants import X_DIM, X_INTERFACE_DIM, Y_DIM, Y_INTERFACE_DIM, Z_DIM

__all__ = ["open_restart", "RestartVariable", "RESTART_PROPERTIES"]

RESTART_NAMES = ("fv_core.res", "fv_srf_wnd.res", "fv_tracer.res")
COUPLER_RES_NAME = "coupler.res"

_ZYX = (Z_DIM, Y_DIM, X_DIM)
_YX = (Y_DIM, X_DIM)


def _entry(restart_name, dims, units):
    return {"restart_name": restart_name, "dims": list(dims), "units": units}


# standard name -> the variable's name in the restart files, its dims there (after Time) and its units
RESTART_PROPERTIES = {
    # fv_core.res
    "x_wind": _entry("u", (Z_DIM, Y_INTERFACE_DIM, X_DIM), "m/s"),
    "y_wind": _entry("v", (Z_DIM, Y_DIM, X_INTERFACE_DIM), "m/s"),
    "vertical_wind": _entry("W", _ZYX, "m/s"),
    "vertical_thickness_of_atmospheric_layer": _entry("DZ", _ZYX, "m"),
    "air_temperature": _entry("T", _ZYX, "degK"),
    "pressure_thickness_of_atmospheric_layer": _entry("delp", _ZYX, "Pa"),
    "surface_geopotential": _entry("phis", _YX, "m^2 s^-2"),
    "eastward_wind": _entry("ua", _ZYX, "m/s"),
    "northward_wind": _entry("va", _ZYX, "m/s"),
    # fv_srf_wnd.res
    "eastward_wind_at_surface": _entry("u_srf", _YX, "m/s"),
    "northward_wind_at_surface": _entry("v_srf", _YX, "m/s"),
    # fv_tracer.res
    "specific_humidity": _entry("sphum", _ZYX, "kg/kg"),
    "cloud_liquid_water_mixing_ratio": _entry("liq_wat", _ZYX, "kg/kg"),
    "rain_mixing_ratio": _entry("rainwat", _ZYX, "kg/kg"),
    "cloud_ice_mixing_ratio": _entry("ice_wat", _ZYX, "kg/kg"),
    "snow_mixing_ratio": _entry("snowwat", _ZYX, "kg/kg"),
    "graupel_mixing_ratio": _entry("graupel", _ZYX, "kg/kg"),
    "ozone_mixing_ratio": _entry("o3mr", _ZYX, "kg/kg"),
    "turbulent_kinetic_energy": _entry("sgs_tke", _ZYX, "m**2/s**2"),
    "cloud_fraction": _entry("cld_amt", _ZYX, ""),
}


@dataclasses.dataclass
class RestartVariable:
    """A variable as a restart file holds it: `data` in file order (dims), native-endian float64."""

    data: np.ndarray
    dims: Tuple[str, ...]
    units: str


def prepend_label(filename, label=None):
    return f"{label}.{filename}" if label is not None and len(label) > 0 else filename


def restart_filenames(dirname, tile_index, label):
    """The tile's restart files that exist, in the order they are read."""
    names = [os.path.join(dirname, prepend_label(name, label) + f".tile{tile_index + 1}.nc") for name in RESTART_NAMES]
    return [name for name in names if os.path.isfile(name)]


def get_coupler_res_filename(dirname, label):
    return os.path.join(dirname, prepend_label(COUPLER_RES_NAME, label))


def get_current_date_from_coupler_res(path) -> datetime:
    """The last line of coupler.res: the current model time as year, month, day, hour, minute, second."""
    with open(path, "r") as f:
        lines = [line for line in f.read().splitlines() if line.strip()]
    if not lines:
        raise ValueError(f"{path} is empty")
    try:
        return datetime(*[int(token) for token in lines[-1].split()[:6]])
    except (TypeError, ValueError) as e:
        raise ValueError(f"{path}: the last line does not begin with a date: {lines[-1]!r}") from e


def _to_device(staging, staged):
    """The call's one host-to-device copy (on the current stream: the unpack launch follows it there)."""
    staged.copy_(staging, non_blocking=True)


def _geometry(quantities):
    """The storage layout the Quantities share, as the C ABI takes it."""
    sj = nk = sk = None
    for q in quantities:
        stride, shape = q.data.stride(), q.data.shape
        if len(shape) not in (2, 3) or stride[0] != 1:
            raise ValueError(f"to_state: cannot fill a quantity of dims {q.dims}")
        layout = (shape[0] - 7, stride[1])
        if sj is not None and layout != sj:
            raise ValueError("to_state: the quantities do not share one storage layout")
        sj = layout
        if len(shape) == 3:
            if nk is not None and (shape[2] - 1, stride[2]) != (nk, sk):
                raise ValueError("to_state: the quantities do not share one storage layout")
            nk, sk = shape[2] - 1, stride[2]
    n, row = sj
    if nk is None:
        nk, sk = 1, row * (n + 7)
    return _lib.Geom(n, nk, row, 0, sk)


def _fill(found, to_state, communicator):
    """found: standard name -> (file, restart name, dims).  One staging buffer, one copy, one launch per 32 variables."""
    lib, device = communicator.lib, torch.device(communicator.device)
    entries, total = [], 0
    for name, quantity in to_state.items():
        if name == "time":
            continue
        if name not in found:
            raise KeyError(f"{name}: no such variable in the restart files")
        file, restart_name, dims = found[name]
        array = file.record(restart_name)
        want = tuple(dims[::-1])
        if tuple(quantity.dims) != want:
            raise ValueError(f"{name}: a quantity of dims {tuple(quantity.dims)} cannot take a variable of dims {want[::-1]}")
        if array.shape != tuple(quantity.extent)[::-1]:
            raise ValueError(f"{name} ({restart_name} of {file.path}): shape {array.shape}, but the quantity's compute domain "
                             f"is {tuple(quantity.extent)[::-1]}")
        entries.append((quantity, array, total))
        total += array.size
    if not entries:
        return
    geom = _geometry([quantity for quantity, _, _ in entries])
    staging = torch.empty(total, dtype=torch.float64, pin_memory=device.type != "cpu")
    flat = staging.numpy()
    for _, array, offset in entries:
        np.copyto(flat[offset:offset + array.size].reshape(array.shape), array, casting="same_kind")
    staged = torch.empty(total, dtype=torch.float64, device=device)
    _to_device(staging, staged)
    stream = communicator.stream()
    for start in range(0, len(entries), _lib.UNPACK_MAX_ITEMS):
        chunk = entries[start:start + _lib.UNPACK_MAX_ITEMS]
        items = (_lib.UnpackItem * len(chunk))()
        for item, (quantity, array, offset) in zip(items, chunk):
            item.field = quantity.ptr
            item.kind = _lib.DIAG_WINDOW3D if array.ndim == 3 else _lib.DIAG_PLANE
            item.order = _lib.ORDER_XFAST
            item.i0, item.j0 = quantity.origin[0], quantity.origin[1]
            item.ni, item.nj = quantity.extent[0], quantity.extent[1]
            item.k0, item.nk = (quantity.origin[2], quantity.extent[2]) if array.ndim == 3 else (0, 1)
            item.in_step, item.in_offset = 1, offset
        lib.call("pace_state_unpack", C.byref(geom), items, len(chunk), C.c_void_p(staged.data_ptr()), stream)


def open_restart(dirname: str, communicator, label: str = "", only_names: Optional[Iterable[str]] = None,
                 to_state: Optional[dict] = None, tracer_properties: Optional[dict] = None):
    """Load restart files output by the Fortran model into a state dictionary.

    Args:
        dirname: location of restart files
        communicator: object for communication over the cubed sphere (its rank's tile decides the files)
        label: prepended string on the restart files to load
        only_names (optional): list of standard names to load
        to_state (optional): if given, assign loaded data into pre-allocated quantities
            in this state dictionary
        tracer_properties (optional): entries added to RESTART_PROPERTIES

    Returns:
        state: model state dictionary
    """
    properties = RESTART_PROPERTIES if tracer_properties is None else {**tracer_properties, **RESTART_PROPERTIES}
    standard_names = {entry["restart_name"]: name for name, entry in properties.items()}
    tile_index = communicator.partitioner.tile_index(communicator.rank)
    filenames = restart_filenames(dirname, tile_index, label)
    if len(filenames) == 0:
        raise ValueError("no restart files found at {}".format(dirname))
    only = None if only_names is None else set(only_names)
    found = {}
    for filename in filenames:
        file = _open_nc(filename)
        for restart_name in file.names():
            name = standard_names.get(restart_name)
            if name is not None and (only is None or name in only):
                found[name] = (file, restart_name, tuple(properties[name]["dims"]))
    time = None
    coupler_res = get_coupler_res_filename(dirname, label)
    if os.path.isfile(coupler_res) and (only is None or "time" in only):
        time = get_current_date_from_coupler_res(coupler_res)
    if to_state is None:
        state = {}
        for name, (file, restart_name, dims) in found.items():
            array = file.record(restart_name)
            if array.ndim != len(dims):
                raise ValueError(f"{name} ({restart_name} of {file.path}): {array.ndim} dimensions after Time, expected {dims}")
            state[name] = RestartVariable(np.ascontiguousarray(array, dtype=np.float64), dims, properties[name]["units"])
    else:
        _fill(found, to_state, communicator)
        state = to_state
    if time is not None:
        state["time"] = time
    return state
