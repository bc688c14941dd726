"""NetCDFMonitor: the reference's sympl-style monitor (util/pace/util/monitor/netcdf_monitor.py) with its constructor and its
``store``, ``store_constant`` and ``cleanup``, writing NetCDF-3 (64-bit offset) through pace_amd/util/_nc3.py -- neither xarray
nor netCDF4 is needed.

``store(state)`` gathers the state over the communicator (``gather_state`` with ``transfer_type=numpy.float32``: under
``run_cube`` one launch and one transfer for all six tiles and every variable) and the root appends it to the current time
chunk; a full chunk, or ``cleanup()``, writes ``state_{chunk:04d}_tile{t}.nc``.  Variables have the dimensions
``[time, tile, *dims]`` and their ``units`` as an attribute; ``time`` is a double with CF ``units`` ("seconds since 1970-01-01
00:00:00" and ``calendar`` "proleptic_gregorian" for datetimes, "seconds" for timedeltas).  ``store_constant`` writes
``constants_{name}.nc`` with the dimensions ``[tile, *dims]``.

Where the chunks differ from the reference: it gathers a state over the TILE communicator, so every tile's root writes its
own chunks with a tile axis of length 1, and only the constants are gathered over the globe.  With layout (1, 1) a tile is one
rank and that gather moves nothing; here the state is gathered over the globe as the constants are, the tile axis has its true
length of 6, and the one file per chunk carries the root's tile in its name (``_tile0``).  A state whose quantities already
lead with TILE_DIM (what MonitorDiagnostics hands over after its own gather) is appended as it is, and so is one that leads
with LON_DIM or LAT_DIM (a regridded array: ``[time, lon, lat(, z)]``, no tile axis).
"""
import os
from datetime import datetime, timedelta
from typing import Dict, Optional

import numpy as np

from . import _nc3
from . import constants as c

_EPOCH = datetime(1970, 1, 1)


def _host(quantity) -> np.ndarray:
    view = quantity.view[:]
    return np.asarray(view) if isinstance(view, np.ndarray) else view.detach().cpu().numpy()


def _ascii(text) -> str:
    return str(text).encode("ascii", "replace").decode("ascii")


def write_nc3(path, dimensions, variables):
    """One NetCDF-3 file of fixed-size variables.  dimensions: {name: size}; variables: [(name, dims, array, attrs)] with
    float32 or float64 arrays."""
    defs = [_nc3.Variable(name, dims, ">f8" if np.asarray(a).dtype == np.float64 else ">f4", attrs) for name, dims, a, attrs in variables]
    header, fixed, _, _ = _nc3.layout(dimensions, None, {}, defs, {name: a for name, _, a, _ in variables})
    if os.path.exists(path):
        os.remove(path)
    with open(path, "wb") as f:
        f.write(header)
        f.write(fixed)


def time_variable(times):
    """('time', dims, float64 array, CF attributes) of a list of datetimes or timedeltas (None: 0)."""
    if times and isinstance(times[0], (timedelta, np.timedelta64)):
        seconds = [(t / np.timedelta64(1, "us")) / 1e6 if isinstance(t, np.timedelta64) else t.total_seconds() for t in times]
        attrs = {"units": "seconds"}
    else:
        seconds = [0.0 if t is None else (t - _EPOCH).total_seconds() if isinstance(t, datetime) else float(t) for t in times]
        attrs = {"units": "seconds since 1970-01-01 00:00:00", "calendar": "proleptic_gregorian"}
    return "time", ("time",), np.asarray(seconds, dtype=np.float64), attrs


class _Chunk:
    """The variables of one time chunk: (time_chunk_size, tiles, *extent) each."""

    def __init__(self, state, time_chunk_size):
        self.size, self.count = time_chunk_size, 0
        self.dims = {name: tuple(q.dims) for name, q in state.items()}
        self.units = {name: q.units for name, q in state.items()}
        self.data = {name: np.zeros((time_chunk_size,) + tuple(_host(q).shape), dtype=_host(q).dtype) for name, q in state.items()}

    def append(self, state):
        for name, q in state.items():
            if tuple(q.dims) != self.dims[name]:
                q = q.transpose(self.dims[name])
            self.data[name][self.count] = _host(q)
        self.count += 1


class NetCDFMonitor:
    """sympl.Monitor-style object for storing model state dictionaries in netCDF files."""

    FILENAME_FORMAT = "state_{chunk:04d}_tile{tile}.nc"
    CONSTANT_FILENAME_FORMAT = "constants_{name}.nc"

    def __init__(self, path: str, communicator, time_chunk_size: int = 1):
        """
        Args:
            path: directory in which to store data
            communicator: provides global communication to gather state
            time_chunk_size: number of times per file
        """
        self._tile_index = communicator.partitioner.tile_index(communicator.rank)
        self._path = path
        self._communicator = communicator
        self._time_chunk_size = time_chunk_size
        self._i_time = 0
        self._chunk: Optional[_Chunk] = None
        self._times = []
        self._expected_vars = None

    def _gathered(self, state):
        """The state over the globe: on the root {name: Quantity leading with TILE_DIM} (and "time"), None elsewhere."""
        fields = [q for name, q in state.items() if name != "time"]
        if fields and all(tuple(q.dims[:1]) in ((c.TILE_DIM,), (c.LON_DIM,), (c.LAT_DIM,)) for q in fields):  # (global already)
            return dict(state)
        return self._communicator.gather_state(state, transfer_type=np.float32)

    def store(self, state: dict) -> None:
        """Append the model state dictionary.  Writes to disk only when a full time chunk has been accumulated, or when
        .cleanup() is called.  The keys must be those of the first call; dimension order may change between calls."""
        if self._expected_vars is None:
            self._expected_vars = set(state.keys())
        elif self._expected_vars != set(state.keys()):
            raise ValueError("state keys must be the same each time store is called, "
                             f"got {set(state.keys())} but previously got {self._expected_vars}")
        state = self._gathered(state)
        if state is None:  # (not the root)
            return
        time = state.pop("time", None)
        if self._chunk is None:
            self._chunk = _Chunk(state, self._time_chunk_size)
        self._chunk.append(state)
        self._times.append(time)
        if (self._i_time + 1) % self._time_chunk_size == 0:
            self.flush()
        self._i_time += 1

    def flush(self):
        chunk = self._chunk
        if chunk is not None:
            dimensions = {"time": chunk.count}
            variables = [time_variable(self._times)]
            for name, data in chunk.data.items():
                dims = ("time",) + chunk.dims[name]
                for d, size in zip(dims[1:], data.shape[1:]):
                    if dimensions.setdefault(d, size) != size:
                        raise ValueError(f"{name}: dimension {d} has {size} points, another variable's has {dimensions[d]}")
                variables.append((name, dims, data[:chunk.count], {"units": _ascii(chunk.units[name])}))
            index = self._i_time // self._time_chunk_size
            write_nc3(os.path.join(self._path, self.FILENAME_FORMAT.format(chunk=index, tile=self._tile_index)), dimensions, variables)
        self._chunk = None
        self._times.clear()

    def store_constant(self, state: Dict[str, object]) -> None:
        state = self._gathered(state)
        if state is None:
            return
        for name, quantity in state.items():
            data = _host(quantity)
            write_nc3(os.path.join(self._path, self.CONSTANT_FILENAME_FORMAT.format(name=name)),
                      dict(zip(quantity.dims, data.shape)), [(name, tuple(quantity.dims), data, {"units": _ascii(quantity.units)})])

    def cleanup(self):
        self.flush()
