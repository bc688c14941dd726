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
library narrows on the device.  Halos and the levels below the file's keep what they held.  With `verify_checksums` one
sums-only pace_restart_pack launch over the same windows follows, and the sums are held against the files' attributes.

    write_restart(dirname, communicator, {name: quantity}, time=...)    # the inverse: device Quantities into restart files

ONE pace_restart_pack launch (pace_amd/csrc/k_restart.hip; more only above 32 variables) gathers every variable's compute domain
into ONE device byte buffer laid out as the files' data sections -- dense, big-endian -- with every variable's checksum behind
them; ONE non-blocking copy brings it to ONE pinned buffer, and each file is its header (pace_amd/util/_nc3.py) followed by
`file.write` of a slice of that buffer.  The host never converts, swaps or copies the values.

The attribute FMS stamps every variable with, `checksum`, was established on the fixture (tests/golden/c12_restart) to be the
wrapping (mod 2^64) sum over the SIX tiles of the wrapping sum of the 64-bit patterns of the tile's values, as 16 upper-case hex
digits, right-justified and blank-padded; it is the same in all six tiles' files.  write_restart adds `tile_checksum`, the
tile's own sum in the same form, which a rank can verify alone.
"""
import ctypes as C
import dataclasses
import os
import warnings
from datetime import datetime
from typing import Iterable, Optional, Tuple

import numpy as np
import torch

from .. import _launch, _lib
from . import _nc3
from .checkpointer.validation import _open_nc
from .constants import X_DIM, X_INTERFACE_DIM, Y_DIM, Y_INTERFACE_DIM, Z_DIM

__all__ = ["open_restart", "write_restart", "LevelOf", "RestartVariable", "RESTART_PROPERTIES"]

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


# the file of a restart variable; a variable that is in neither list is a tracer (fv_tracer.res)
_CORE_VARIABLES = ("u", "v", "W", "DZ", "T", "delp", "phis", "ua", "va")
_SRF_WND_VARIABLES = ("u_srf", "v_srf")


def _file_of(restart_name):
    if restart_name in _CORE_VARIABLES:
        return "fv_core.res"
    return "fv_srf_wnd.res" if restart_name in _SRF_WND_VARIABLES else "fv_tracer.res"


def checksum_text(value) -> str:
    """FMS's form of a checksum attribute: 16 upper-case hex digits, right-justified and blank-padded."""
    return "%16X" % int(value)


def get_start_date_from_coupler_res(path) -> Optional[datetime]:
    """The line before the last of coupler.res: the model's start time, or None where the file has no such line."""
    with open(path, "r") as f:
        lines = [line for line in f.read().splitlines() if line.strip()]
    try:
        return datetime(*[int(token) for token in lines[-2].split()[:6]])
    except (IndexError, TypeError, ValueError):
        return None


# the call's one host-to-device copy, and its one device-to-host copy with the one wait for it (the calls go through these names:
# the one-transfer tests count them here)
_to_device, _to_host = _launch.to_device, _launch.to_host


def _geometry(quantities):
    """The storage layout the Quantities share, as the C ABI takes it."""
    return _launch.geometry(quantities, lambda q: f"to_state: cannot fill a quantity of dims {q.dims}",
                            "to_state: the quantities do not share one storage layout")


def _attribute(file, restart_name, attribute):
    """A text attribute of a variable of an opened file, or None."""
    variable = file._variables[restart_name]
    attrs = getattr(variable, "attrs", None)
    if attrs is not None:
        value = attrs.get(attribute)
    elif hasattr(variable, "ncattrs"):
        value = variable.getncattr(attribute) if attribute in variable.ncattrs() else None
    else:
        value = getattr(variable, "_attributes", {}).get(attribute)
    if value is None:
        return None
    return value.decode("ascii", "replace") if isinstance(value, bytes) else str(value)


def _windows_of(entries, real_bytes):
    """(quantity, level or None) pairs -> the windows pace_restart_pack takes: (pointer, kind, i0, j0, k0, ni, nj, nk)."""
    return [_launch.window_of(quantity, level) for quantity, level in entries]


def _pack(lib, geom, windows, offsets, out_type, out, sums, device, stream):
    """pace_restart_pack over the windows, one launch per 32: the bytes to out + offsets[m] (device address, or None) and the
    sums to sums + 8 * m (device address, or None).  -> the workspace, which the launches read until the stream has run them."""
    tables, need = [], 0
    for first, chunk in _launch.chunks(windows, _lib.RESTART_MAX_ITEMS):
        items = (_lib.RestartItem * len(chunk))()
        for m, (item, window) in enumerate(zip(items, chunk), first):
            _launch.set_window(item, window)
            item.out_offset = offsets[m] if out is not None else 0
        tables.append((first, items))
        if sums is not None:
            need = max(need, int(lib.cdll.pace_restart_pack_workspace_bytes(C.byref(geom), items, len(items))))
    workspace = torch.empty(max(need, 8) // 8, dtype=torch.int64, device=device)
    for first, items in tables:
        lib.call("pace_restart_pack", C.byref(geom), items, len(items), out_type, None if out is None else C.c_void_p(out),
                 None if sums is None else C.c_void_p(sums + 8 * first), C.c_void_p(workspace.data_ptr()), stream)
    return workspace


def _verify(entries, geom, communicator):
    """entries: (quantity, level or None, file, restart name).  One sums-only launch over the windows just filled; the tile's sums against
    `tile_checksum` where the files have it, else the sum over the ranks against FMS's `checksum`."""
    lib, device = communicator.lib, torch.device(communicator.device)
    windows = _windows_of([(quantity, level) for quantity, level, _, _ in entries], lib.real_bytes)
    sums = torch.empty(len(windows), dtype=torch.int64, device=device)
    workspace = _pack(lib, geom, windows, None, _lib.RESTART_BE_F64, None, sums.data_ptr(), device, communicator.stream())
    mine = sums.cpu().numpy().view(np.uint64)
    del workspace
    tile = [_attribute(file, restart_name, "tile_checksum") for _, _, file, restart_name in entries]
    globe = None
    if any(t is None for t in tile):
        globe = communicator.comm.allreduce_sum_u64(mine)
    unverified = []
    for m, (_, _, file, restart_name) in enumerate(entries):
        if tile[m] is not None:
            want, got, what = tile[m], checksum_text(mine[m]), "tile_checksum"
        else:
            want, what = _attribute(file, restart_name, "checksum"), "checksum"
            if want is None or globe is None:
                unverified.append(restart_name)
                continue
            got = checksum_text(globe[m])
        if want.strip().upper() != got.strip():
            raise ValueError(f"{restart_name} of {file.path}: the values read sum to {got.strip()}, but the file's {what} is "
                             f"{want.strip()}")
    if unverified:
        warnings.warn(f"verify_checksums: {', '.join(unverified)} could not be verified: the files have no tile_checksum, and "
                      "a checksum over the globe needs the sums of all six ranks", stacklevel=3)


def _fill(found, to_state, communicator, verify_checksums=False, missing_ok=()):
    """found: standard name -> (file, restart name, dims).  One staging buffer, one copy, one launch per 32 variables."""
    lib, device = communicator.lib, torch.device(communicator.device)
    if verify_checksums and lib.real_bytes != 8:
        raise ValueError("verify_checksums: the float32 library narrows the values as it reads them, so the sums of what it "
                         "holds are not the files'; verify with the float64 library")
    entries, sources, total = [], [], 0
    for name, quantity in to_state.items():
        if name == "time":
            continue
        if name not in found:
            if name in missing_ok:
                continue
            raise KeyError(f"{name}: no such variable in the restart files")
        file, restart_name, dims = found[name]
        array = file.record(restart_name)
        want = tuple(dims[::-1])
        quantity, level = (quantity.quantity, quantity.level) if isinstance(quantity, LevelOf) else (quantity, None)
        if (tuple(quantity.dims) if level is None else tuple(quantity.dims[:2])) != want:
            raise ValueError(f"{name}: a quantity of dims {tuple(quantity.dims)} cannot take a variable of dims {want[::-1]}")
        if array.shape != tuple(quantity.extent[:len(want)])[::-1]:
            raise ValueError(f"{name} ({restart_name} of {file.path}): shape {array.shape}, but the quantity's compute domain "
                             f"is {tuple(quantity.extent[:len(want)])[::-1]}")
        entries.append((quantity, array, total, level))
        sources.append((quantity, level, file, restart_name))
        total += array.size
    if not entries:
        return
    geom = _geometry([quantity for quantity, _, _, _ in entries])
    staged, staging = _launch.staging(total, torch.float64, device)
    flat = staging.numpy()
    for _, array, offset, _ in entries:
        np.copyto(flat[offset:offset + array.size].reshape(array.shape), array, casting="same_kind")
    _to_device(staging, staged)
    stream = communicator.stream()
    for _, chunk in _launch.chunks(entries, _lib.UNPACK_MAX_ITEMS):
        items = (_lib.UnpackItem * len(chunk))()
        for item, (quantity, _, offset, level) in zip(items, chunk):
            _launch.set_window(item, _launch.window_of(quantity, level))
            item.order, item.in_step, item.in_offset = _lib.ORDER_XFAST, 1, offset
        lib.call("pace_state_unpack", C.byref(geom), items, len(chunk), C.c_void_p(staged.data_ptr()), stream)
    if verify_checksums:
        _verify(sources, geom, communicator)


def open_restart(dirname: str, communicator, label: str = "", only_names: Optional[Iterable[str]] = None,
                 to_state: Optional[dict] = None, tracer_properties: Optional[dict] = None, verify_checksums: bool = False,
                 missing_ok: Iterable[str] = ()):
    """Load restart files output by the Fortran model into a state dictionary.

    Args:
        dirname: location of restart files
        communicator: object for communication over the cubed sphere (its rank's tile decides the files)
        label: prepended string on the restart files to load
        only_names (optional): list of standard names to load
        to_state (optional): if given, assign loaded data into pre-allocated quantities
            in this state dictionary; LevelOf(quantity, level) takes a 2-D variable into one level of a 3-D quantity
        missing_ok (optional, with to_state): names of to_state that the files need not have (they keep what they held)
        tracer_properties (optional): entries added to RESTART_PROPERTIES
        verify_checksums (optional, with to_state): after the state is filled, one sums-only pace_restart_pack launch over
            the same windows; the sums are compared with the files' `tile_checksum` where they have it, otherwise the ranks'
            sums are added (communicator.comm.allreduce_sum_u64: every rank must call) and compared with FMS's `checksum`.
            A mismatch raises ValueError naming the variable and the file; where neither comparison is possible one warning
            is given.  Refused by the float32 library, which narrows on ingest.

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
        _fill(found, to_state, communicator, verify_checksums, tuple(missing_ok))
        state = to_state
    if time is not None:
        state["time"] = time
    return state


class LevelOf:
    """One level of a 3-D quantity as a 2-D restart variable (write_restart: the surface winds are the lowest level of the
    A-grid winds)."""

    def __init__(self, quantity, level):
        if len(quantity.dims) != 3 or not 0 <= level < quantity.data.shape[2]:
            raise ValueError(f"LevelOf: level {level} of a quantity of dims {quantity.dims} and shape {quantity.shape}")
        self.quantity, self.level = quantity, int(level)


_COUPLER_RES = ("{:6d}        (Calendar: no_calendar=0, thirty_day_months=1, julian=2, gregorian=3, noleap=4)\n"
                "{:6d}{:6d}{:6d}{:6d}{:6d}{:6d}        Model start time:   year, month, day, hour, minute, second\n"
                "{:6d}{:6d}{:6d}{:6d}{:6d}{:6d}        Current model time: year, month, day, hour, minute, second\n")


def _axes(variables):
    """variables: (restart name, file-order shape).  FMS numbers a file's axes per direction in the order their lengths first
    appear: -> ({dimension: size} in the files' order x, y, z, Time; per variable its dimension names)."""
    found = {"x": [], "y": [], "z": []}
    named = []
    for _, shape in variables:
        letters = ("z", "y", "x")[3 - len(shape):]
        dims = []
        for letter, size in zip(letters, shape):
            if size not in found[letter]:
                found[letter].append(size)
            dims.append(f"{letter}axis_{found[letter].index(size) + 1}")
        named.append(("Time",) + tuple(dims))
    dimensions = {f"{letter}axis_{k + 1}": size for letter in ("x", "y", "z") for k, size in enumerate(found[letter])}
    dimensions["Time"] = None
    return dimensions, named


def _file_layout(filename, variables, dtype, attributes):
    """variables: (restart name, file-order shape); attributes: per variable {name: text}.  The file as FMS shapes it:
    -> (header + axis data + the Time record's bytes, the file offset of the first variable's data)."""
    dimensions, named = _axes(variables)
    axis_attrs = {"x": "X", "y": "Y", "z": "Z"}
    listed = [_nc3.Variable(name, (name,), ">f8", {"long_name": name, "units": "none", "cartesian_axis": axis_attrs[name[0]]})
              for name in dimensions if name != "Time"]
    listed.append(_nc3.Variable("Time", ("Time",), ">f8", {"long_name": "Time", "units": "time level", "cartesian_axis": "T"}))
    for (name, _), dims, attrs in zip(variables, named, attributes):
        listed.append(_nc3.Variable(name, dims, dtype, {"long_name": name, "units": "none", **attrs}))
    axis_values = {name: np.arange(1, size + 1, dtype=np.float64) for name, size in dimensions.items() if name != "Time"}
    header, fixed, records, _ = _nc3.layout(dimensions, "Time", {"filename": "RESTART/" + filename}, listed, axis_values)
    first = records[variables[0][0]]
    assert records["Time"] + 8 == first
    return header + fixed + np.array([1.0], dtype=">f8").tobytes(), first


def _checksum_attributes(tile_sum, globe_sum):
    attrs = {}
    if globe_sum is not None:
        attrs["checksum"] = checksum_text(globe_sum)
    attrs["tile_checksum"] = checksum_text(tile_sum)
    return attrs


def write_restart(dirname: str, communicator, from_state: dict, *, time: datetime, start_time: Optional[datetime] = None,
                  label: str = "", ak=None, bk=None, file_dtype=np.float64, tracer_properties: Optional[dict] = None):
    """Write the state as restart files of the Fortran model: the inverse of open_restart(..., to_state=...).

    Args:
        dirname: the directory (made if it is missing)
        communicator: object for communication over the cubed sphere (its rank's tile decides the files' names)
        from_state: standard name (RESTART_PROPERTIES, tracer_properties) -> Quantity whose compute domain is the variable,
            or LevelOf(quantity, level) for a 2-D variable that is one level of a 3-D quantity
        time, start_time: the current model time and the model's start time (default: time) for coupler.res
        label: prepended string on the files
        ak, bk (optional): the vertical grid; rank 0 writes them to fv_core.res.nc
        file_dtype: np.float64, or np.float32 for `>f4` variables
        tracer_properties (optional): entries added to RESTART_PROPERTIES

    Per tile [label.]fv_core.res.tile<t + 1>.nc, fv_tracer.res..., fv_srf_wnd.res... -- each only if one of its variables is
    given -- in NetCDF-3 64-bit offset as FMS writes it (axes xaxis_1 ..., an unlimited Time with one record, long_name, units
    "none", the global attribute filename); rank 0 also writes [label.]fv_core.res.nc and [label.]coupler.res.

    Every variable carries `tile_checksum`, this tile's wrapping sum of its values' bit patterns, and -- where the ranks can
    form it (communicator.comm.allreduce_sum_u64: every rank must call write_restart; a lone NullComm cannot) -- FMS's
    `checksum`, the sum over the six tiles.  With file_dtype=np.float32 only `tile_checksum` (of the 32-bit patterns,
    zero-extended) is written: FMS's convention for 4-byte data could not be checked against a file of the Fortran model.

    ONE pace_restart_pack launch per 32 variables, ONE device-to-host copy, one `file.write` of a slice of the pinned buffer per
    file: the host does not convert, swap or copy the values.
    """
    lib, device = communicator.lib, torch.device(communicator.device)
    properties = RESTART_PROPERTIES if tracer_properties is None else {**RESTART_PROPERTIES, **tracer_properties}
    dtype = np.dtype(file_dtype).newbyteorder(">")
    if dtype not in (np.dtype(">f8"), np.dtype(">f4")):
        raise ValueError(f"file_dtype is float64 or float32, not {file_dtype}")
    out_type = _lib.RESTART_BE_F64 if dtype.itemsize == 8 else _lib.RESTART_BE_F32
    unknown = [name for name in from_state if name != "time" and name not in properties]
    if unknown:
        raise KeyError(f"{unknown}: no restart variable of that standard name (RESTART_PROPERTIES, tracer_properties)")
    # the variables in the table's order, which is the files'
    files = {}  # file kind -> [(restart name, file-order shape, quantity, level)]
    for name, entry in properties.items():
        if name not in from_state:
            continue
        value = from_state[name]
        quantity, level = (value.quantity, value.level) if isinstance(value, LevelOf) else (value, None)
        want = tuple(entry["dims"][::-1])
        have = tuple(quantity.dims) if level is None else tuple(quantity.dims[:2])
        if have != want:
            raise ValueError(f"{name}: a quantity of dims {tuple(quantity.dims)} cannot give a variable of dims {want[::-1]}")
        shape = tuple(quantity.extent[:len(want)])[::-1]
        files.setdefault(_file_of(entry["restart_name"]), []).append((entry["restart_name"], shape, quantity, level))
    tile_index = communicator.partitioner.tile_index(communicator.rank)
    os.makedirs(dirname, exist_ok=True)
    kinds = [kind for kind in RESTART_NAMES if kind in files]
    entries = [entry for kind in kinds for entry in files[kind]]
    if entries:
        # the device buffer: the files' data sections one after the other, then the variables' sums
        offsets, total = [], 0
        for _, shape, _, _ in entries:
            offsets.append(total)
            total += int(np.prod(shape)) * dtype.itemsize
        sums_at = (total + 7) // 8 * 8
        words = sums_at // 8 + len(entries)
        geom = _geometry([quantity for _, _, quantity, _ in entries])
        packed, host = _launch.staging(words, torch.int64, device)
        windows = _windows_of([(quantity, level) for _, _, quantity, level in entries], lib.real_bytes)
        workspace = _pack(lib, geom, windows, offsets, out_type, packed.data_ptr(), packed.data_ptr() + sums_at, device,
                          communicator.stream())
        _to_host(packed, host)
        del workspace
        data = memoryview(host.numpy()).cast("B")
        tile_sums = host.numpy()[sums_at // 8:].view(np.uint64)
        globe_sums = communicator.comm.allreduce_sum_u64(tile_sums) if out_type == _lib.RESTART_BE_F64 else None
        m = 0
        for kind in kinds:
            variables = [(restart_name, shape) for restart_name, shape, _, _ in files[kind]]
            attributes = [_checksum_attributes(tile_sums[m + v], None if globe_sums is None else globe_sums[m + v])
                          for v in range(len(variables))]
            filename = prepend_label(kind, label) + f".tile{tile_index + 1}.nc"
            head, first = _file_layout(filename, variables, dtype, attributes)
            assert len(head) == first
            begin = offsets[m]
            end = begin + sum(int(np.prod(shape)) * dtype.itemsize for _, shape in variables)
            with open(os.path.join(dirname, filename), "wb") as f:
                f.write(head)
                f.write(data[begin:end])
            m += len(variables)
    if communicator.rank == 0:
        if ak is not None and bk is not None:
            _write_vertical_grid(dirname, prepend_label("fv_core.res", label) + ".nc", ak, bk)
        start = time if start_time is None else start_time
        with open(get_coupler_res_filename(dirname, label), "w") as f:
            f.write(_COUPLER_RES.format(2, start.year, start.month, start.day, start.hour, start.minute, start.second,
                                        time.year, time.month, time.day, time.hour, time.minute, time.second))


def _write_vertical_grid(dirname, filename, ak, bk):
    """fv_core.res.nc: ak and bk (host arrays of nz + 1 doubles), each with FMS's checksum of its one array."""
    arrays = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (ak, bk)]
    if arrays[0].shape != arrays[1].shape:
        raise ValueError("ak and bk differ in length")
    attributes = [{"checksum": checksum_text(a.view(np.uint64).sum(dtype=np.uint64))} for a in arrays]
    head, first = _file_layout(filename, [("ak", arrays[0].shape), ("bk", arrays[1].shape)], np.dtype(">f8"), attributes)
    assert len(head) == first
    with open(os.path.join(dirname, filename), "wb") as f:
        f.write(head)
        for a in arrays:
            f.write(a.astype(">f8").tobytes())
