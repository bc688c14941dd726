"""Diagnostics -- what a run leaves behind (reference: driver/pace/driver/diagnostics.py:25-253, util/pace/util/monitor/
netcdf_monitor.py).

The reference hands its monitor the state's own Quantities, and the monitor slices, transposes, narrows and copies each of
them.  Here a diagnostics step is ONE launch of pace_diag_pack (pace_amd/csrc/k_diag.hip) per PACE_DIAG_MAX_ITEMS variables --
it gathers the compute windows, the selected levels and the column integrals, transposes them to the files' (x, y, z) C order
and narrows them to float32 in one packed device buffer -- ONE copy of that buffer to pinned host memory and ONE
synchronisation of the stream.  The monitor gets host-resident Quantities that are views of the host buffer: it copies them
(NpzMonitor: a memcpy into its time-chunk arrays), and they are overwritten by the next store.

Files are written by NpzMonitor, the reference's NetCDFMonitor without its file format (neither xarray, zarr nor netCDF4 is
required): `output_format: npz` is this project's extension.

Where one communicator holds the whole cubed sphere (`comm_config.type: cube`, run_cube_driver: DeviceCubeComm ranks) the globe
is written as a whole: a store is ONE pace_cube_gather launch for all six tiles and every requested variable
(CubedSphereCommunicator.gather_state) and one transfer, the column integrals still go through each rank's pace_diag_pack and
are joined on the host, and rank 0 alone writes -- one file per time chunk with a tile axis of 6, as npz (NpzMonitor) or as
NetCDF-3 (`output_format: netcdf`, pace_amd.util.NetCDFMonitor).  Per-rank communicators (one process per tile, a lone tile)
keep their per-tile npz files with a tile axis of 1, and `netcdf` writes nothing there; `zarr` writes nothing anywhere.

Fields on pressure surfaces (`p_select`: pt_p850, height_p500, ...; this project's extension, the reference stops at z_select)
are interpolated on the device by pace_plev_diag (pace_amd/csrc/k_plev.hip), one launch per PACE_PLEV_MAX_LEVELS pressures and
PACE_PLEV_MAX_ITEMS planes, into the same packed buffer: a step is still one transfer and one synchronisation, and a plane is
1 / nz of the volume a host-side interpolation would need.

Fields on a regular latitude-longitude grid (`latlon`: pt_ll, phis_ll, pt_z65_ll, ...; this project's extension, the horizontal
counterpart of p_select) are regridded on the device by pace_cube_regrid (pace_amd/csrc/k_regrid.hip) where one communicator
holds the whole cube: a store adds ONE launch for every requested variable and ONE transfer of the lat-lon arrays alone
(CubedSphereCommunicator.regrid_state) -- 64 800 points of a 1 degree grid against the 221 184 cells of C192.  The monitors write
them with the dimensions [time, lon, lat(, z)], without a tile axis.
"""
import abc
import ctypes as C
import dataclasses
import json
import math
import os
import warnings
from datetime import datetime, timedelta
from typing import Dict, List, Optional, Union

import numpy as np
import torch

from .. import _launch, _lib
from ..util import constants as c
from ..util.quantity import Quantity

_OUTPUT_FORMATS = ("zarr", "netcdf", "npz")


class Diagnostics(abc.ABC):
    @abc.abstractmethod
    def store(self, time: Union[datetime, timedelta], state):
        ...

    @abc.abstractmethod
    def store_grid(self, grid_data):
        ...

    @abc.abstractmethod
    def cleanup(self):
        ...


@dataclasses.dataclass
class ZSelect:
    level: int
    names: List[str]

    def variable(self, state, name: str) -> Quantity:
        """The state's variable `name` if a level of it can be selected, by the reference's rules (diagnostics.py:44-56) -- its
        quirk included: `Z_DIM or Z_INTERFACE_DIM` evaluates to Z_DIM, so interface fields are refused."""
        if name not in state.__dict__.keys():
            raise ValueError(f"Invalid state variable {name} for level select")
        quantity = getattr(state, name)
        assert len(quantity.dims) > 2
        if quantity.dims[2] != c.Z_DIM:
            raise ValueError(f"z_select only works for state variables with dimension (x, y, z). \n {name} has dimension "
                             f"{quantity.dims}")
        return quantity

    def select_data(self, state) -> Dict[str, Quantity]:
        """diagnostics.py:44-65: `<name>_z<level>` -> the level as a 2-D Quantity over the state's own storage."""
        output = {}
        for name in self.names:
            quantity = self.variable(state, name)
            output[f"{name}_z{self.level}"] = Quantity(quantity.data[:, :, self.level], dims=quantity.dims[0:2],
                                                       units=quantity.units, origin=quantity.origin[0:2],
                                                       extent=quantity.extent[0:2])
        return output


HEIGHT = "height"  # p_select's pseudo-name: the geometric height of the pressure surface, from phis and delz


@dataclasses.dataclass
class PSelect:
    """Variables on one pressure surface [Pa], interpolated linearly in log p from the state's own peln (include/pace_hip.h,
    pace_plev_diag): `<name>_p<pressure / 100:g>`, e.g. pt_p850, height_p500."""

    pressure: float
    names: List[str]

    def __post_init__(self):
        if not self.pressure > 0:
            raise ValueError(f"p_select of {', '.join(self.names)}: the pressure must be positive, got {self.pressure!r} Pa")

    def output_name(self, name: str) -> str:
        return f"{name}_p{self.pressure / 100:g}"

    def variable(self, state, name: str) -> Quantity:
        """The state's cell-centre variable `name` (`height`: delz, which the height is summed from)."""
        field = "delz" if name == HEIGHT else name
        quantity = getattr(state, field, None) if field in getattr(state, "__dict__", {}) else None
        if quantity is None:
            raise ValueError(f"Invalid state variable {name} for pressure level select")
        if tuple(quantity.dims) != (c.X_DIM, c.Y_DIM, c.Z_DIM):
            raise ValueError(f"p_select only works for state variables with dimension (x, y, z) and for `{HEIGHT}`. \n {name} has "
                             f"dimension {quantity.dims}")
        return quantity


@dataclasses.dataclass
class LatLonSelect:
    """Cell-centre variables on a regular nlon x nlat latitude-longitude grid (pace_amd/util/latlon.py; piecewise-linear on the
    spherical Delaunay triangulation of the cell centres): `<name>_ll` with dims (lon, lat, z) or (lon, lat); with `levels`,
    every 3-D variable as the planes `<name>_z<k>_ll` of those levels instead.  The names are looked up in the dycore state,
    then the physics state: pt, delp, ua, va (the zonal and meridional A-grid winds: scalars on the sphere), w, qvapor, phis,
    ..."""

    nlon: int
    nlat: int
    names: List[str]
    levels: Optional[List[int]] = None

    def __post_init__(self):
        if self.nlon < 1 or self.nlat < 1:
            raise ValueError(f"latlon: the grid has at least one point each way, not {self.nlon} x {self.nlat}")

    def grid(self):
        from ..util.latlon import LatLonGrid

        return LatLonGrid(self.nlon, self.nlat)

    def variable(self, state, name: str) -> Quantity:
        """The state's cell-centre variable `name`."""
        quantity = None
        for part in (getattr(state, "dycore_state", None), getattr(state, "physics_state", None)):
            if name in getattr(part, "__dict__", {}):
                quantity = getattr(part, name)
                break
        if quantity is None:
            raise ValueError(f"Invalid state variable {name} for latlon")
        if tuple(quantity.dims) not in ((c.X_DIM, c.Y_DIM), (c.X_DIM, c.Y_DIM, c.Z_DIM)):
            raise ValueError(f"latlon only works for cell-centre state variables with dimension (x, y) or (x, y, z). \n {name} has "
                             f"dimension {quantity.dims}")
        return quantity

    def windows(self, state):
        """{output name: Quantity or gather Window} of a store, in the names' order."""
        from ..util.gather import Window

        out = {}
        for name in self.names:
            quantity = self.variable(state, name)
            if len(quantity.dims) == 2 or self.levels is None:
                out[f"{name}_ll"] = quantity
                continue
            for level in self.levels:
                if not 0 <= level < quantity.data.shape[2]:
                    raise IndexError(f"latlon level {level} of {name}: the storage has {quantity.data.shape[2]} levels")
                window = _launch.window_of(quantity, level)[2:]
                out[f"{name}_z{level}_ll"] = Window(quantity, _lib.DIAG_PLANE, level, window, quantity.dims[:2], quantity.units)
        return out


@dataclasses.dataclass
class DiagnosticsConfig:
    """
    Attributes:
        path: directory to save diagnostics if given, otherwise no diagnostics
            will be stored
        output_format: one of "zarr", "netcdf" or "npz".  Only "npz" (this project's extension: numpy archives with the
            reference's NetCDFMonitor layout, one file per tile and time chunk) writes anything
        time_chunk_size: number of timesteps stored in each file
        names: state variables to save as diagnostics
        derived_names: derived diagnostics to save
        z_select: save a vertical slice of a 3D state
        p_select: save state variables, or `height`, on pressure surfaces (this project's extension)
        latlon: save cell-centre state variables on a regular latitude-longitude grid (this project's extension; needs a
            communicator that holds the whole cube: comm_config.type: cube)
    """

    path: Optional[str] = None
    output_format: str = "zarr"
    time_chunk_size: int = 1
    names: List[str] = dataclasses.field(default_factory=list)
    derived_names: List[str] = dataclasses.field(default_factory=list)
    z_select: List[ZSelect] = dataclasses.field(default_factory=list)
    p_select: List[PSelect] = dataclasses.field(default_factory=list)
    latlon: Optional[LatLonSelect] = None

    def __post_init__(self):
        if (len(self.names) > 0 or len(self.derived_names) > 0 or len(self.p_select) > 0 or self.latlon is not None) and self.path is None:
            raise ValueError("DiagnosticsConfig.path must be given to enable diagnostics")
        if self.output_format not in _OUTPUT_FORMATS:
            raise ValueError(f"output_format must be one of 'zarr', 'netcdf' or 'npz', got {self.output_format}")

    @property
    def writes_files(self) -> bool:
        return self.path is not None and self.output_format == "npz"

    def writes_files_for(self, communicator) -> bool:
        """... with this communicator: `netcdf` is written where the communicator holds the whole cube."""
        return self.writes_files or (self.path is not None and self.output_format == "netcdf" and whole_cube(communicator))

    def diagnostics_factory(self, communicator, lib=None) -> Diagnostics:
        """
        Create a diagnostics object.

        Args:
            communicator: tells which tile this rank holds (layout (1, 1): every rank is its tile's root and writes its own
                files; nothing is gathered)
            lib: the kernel library the state's fields belong to (default: the product library)
        """
        if self.latlon is not None and not whole_cube(communicator):
            raise ValueError("diagnostics_config.latlon regrids the whole cube on one device: run the configuration with "
                             "comm_config.type: cube (pace_amd.driver.run_cube_driver); a per-rank communicator holds one tile")
        if not self.writes_files_for(communicator):
            return NullDiagnostics()
        os.makedirs(self.path, exist_ok=True)
        if self.output_format == "netcdf":
            from ..util.monitor import NetCDFMonitor

            monitor = NetCDFMonitor(self.path, communicator, time_chunk_size=self.time_chunk_size)
        else:
            monitor = NpzMonitor(self.path, tile=communicator.partitioner.tile_index(communicator.rank),
                                 time_chunk_size=self.time_chunk_size)
        latlon_monitor = None
        if self.latlon is not None:  # files of their own: the per-tile and whole-cube files are what they are without `latlon`
            if self.output_format == "netcdf":
                latlon_monitor = NetCDFMonitor(self.path, communicator, time_chunk_size=self.time_chunk_size)
                latlon_monitor.FILENAME_FORMAT = "latlon_{chunk:04d}.nc"
            else:
                latlon_monitor = NpzMonitor(self.path, tile=0, time_chunk_size=self.time_chunk_size)
                latlon_monitor.FILENAME_FORMAT, latlon_monitor.CONSTANT_FILENAME_FORMAT = "latlon_{chunk:04d}.npz", "constants_{name}.npz"
        return MonitorDiagnostics(monitor=monitor, names=self.names, derived_names=self.derived_names, z_select=self.z_select,
                                  lib=lib, communicator=communicator if whole_cube(communicator) else None, p_select=self.p_select,
                                  latlon=self.latlon, latlon_monitor=latlon_monitor)

    @classmethod
    def from_dict(cls, config) -> "DiagnosticsConfig":
        from .config import _strict

        if isinstance(config, cls):
            return config
        config = dict(config or {})
        # (parsed before the constructor sees them: a pressure that is no number is named as the setting it is)
        config["p_select"] = [p if isinstance(p, PSelect) else _strict(PSelect, "diagnostics_config.p_select", p)
                              for p in config.get("p_select") or []]
        if config.get("latlon") is not None and not isinstance(config["latlon"], LatLonSelect):
            config["latlon"] = _strict(LatLonSelect, "diagnostics_config.latlon", config["latlon"])
        out = _strict(cls, "diagnostics_config", config)
        out.z_select = [z if isinstance(z, ZSelect) else _strict(ZSelect, "diagnostics_config.z_select", z) for z in out.z_select]
        return out


def whole_cube(communicator) -> bool:
    """Does this communicator's transport hold all six tiles on one device (DeviceCubeComm: run_cube, run_cube_driver)?"""
    return hasattr(getattr(communicator, "comm", None), "halo_post")


class NullDiagnostics(Diagnostics):
    """Diagnostics that do nothing."""

    def store(self, time: Union[datetime, timedelta], state):
        pass

    def store_grid(self, grid_data):
        pass

    def cleanup(self):
        pass


@dataclasses.dataclass
class _Request:
    """One variable of a diagnostics step: what pace_diag_pack is asked for and what the monitor is told about it."""

    name: str
    kind: int
    field: Quantity
    weight: Optional[Quantity]
    level: int  # PLANE of a 3-D field: the level; otherwise 0
    window: tuple  # (i0, j0, k0, ni, nj, nk)
    dims: tuple
    units: str

    @property
    def shape(self):
        ni, nj, nk = self.window[3:]
        return (ni, nj, nk) if self.kind == _lib.DIAG_WINDOW3D else (ni, nj)

    @property
    def tensors(self):
        return [self.field.data] + ([self.weight.data] if self.weight is not None else [])

    @property
    def packed_by_rank(self):
        """Under a whole-cube communicator: does every rank pack this itself (the windows and planes are gathered)?"""
        return self.kind == _lib.DIAG_COLUMN_INTEGRAL


@dataclasses.dataclass
class _PlevRequest:
    """One plane on a pressure surface: what pace_plev_diag is asked for and what the monitor is told about it."""

    name: str
    kind: int  # _lib.PLEV_LAYER | _lib.PLEV_HEIGHT
    field: Quantity  # LAYER: the field; HEIGHT: delz
    surface: Optional[Quantity]  # HEIGHT: phis
    peln: Quantity
    log_p: float
    window: tuple  # (i0, j0, ni, nj)
    dims: tuple
    units: str
    packed_by_rank = True

    @property
    def shape(self):
        return tuple(self.window[2:])

    @property
    def tensors(self):
        return [self.field.data, self.peln.data] + ([self.surface.data] if self.surface is not None else [])


class WindowPacker:
    """Windows of fields to the host: ONE pace_diag_pack launch per PACE_DIAG_MAX_ITEMS requests, ONE pace_plev_diag launch per
    PACE_PLEV_MAX_LEVELS pressures and PACE_PLEV_MAX_ITEMS planes on them, all into one packed buffer, ONE transfer of that
    buffer to pinned host memory and ONE synchronisation.  What MonitorDiagnostics stores with, and what
    pace_amd.fv3core.GeosDycoreWrapper hands a host model its arrays with."""

    def __init__(self, lib=None):
        """lib: the library the fields belong to (default: the product library, loaded at the first pack)"""
        self._lib = lib
        self._plans = {}  # what is asked for, where and as which type -> (geometry, offsets, device buffer, host buffer)

    def _plan(self, requests, out_is_double):
        tensors = [t for r in requests for t in r.tensors]
        differ = "diagnostics take fields of one layout and type on one device"
        geom = _launch.geometry(
            tensors, lambda t: f"field of shape {tuple(t.shape)}, strides {tuple(t.stride())}: diagnostics take 2-D and 3-D fields "
                               "allocated with pace_amd.util.QuantityFactory", differ)
        if len({(t.device, t.dtype) for t in tensors}) > 1:
            raise ValueError(differ)
        device = tensors[0].device
        key = (device, geom.n, geom.nk, geom.sj, geom.sk, bool(out_is_double), tuple((r.name, type(r), r.kind, r.window, getattr(r, "log_p", None)) for r in requests))
        if key not in self._plans:
            offsets, total = [], 0
            for r in requests:
                offsets.append(total)
                total += int(np.prod(r.shape))
            packed, host = _launch.staging(total, torch.float64 if out_is_double else torch.float32, device)
            self._plans[key] = (geom, offsets, packed, host)
        return self._plans[key]

    @staticmethod
    def _plev_launches(placed):
        """The pressure-level requests cut into launches, in their order: one log interface pressure and one window, at most
        PACE_PLEV_MAX_LEVELS different pressures and PACE_PLEV_MAX_ITEMS planes each."""
        launches, key, levels = [], None, set()
        for r, offset in placed:
            this = (r.peln.ptr, r.window)
            if (this != key or len(launches[-1]) == _lib.PLEV_MAX_ITEMS
                    or (r.log_p not in levels and len(levels) == _lib.PLEV_MAX_LEVELS)):
                launches.append([])
                key, levels = this, set()
            levels.add(r.log_p)
            launches[-1].append((r, offset))
        return launches

    @staticmethod
    def _plev_arguments(geom, chunk, out_is_double, packed, stream):
        """pace_plev_diag's arguments for one launch's requests and their places in the packed buffer."""
        log_p = sorted({r.log_p for r, _ in chunk})
        items = (_lib.PlevItem * len(chunk))()
        for item, (r, offset) in zip(items, chunk):
            item.field = r.field.ptr  # (the pointers of THIS call's storages)
            item.surface = r.surface.ptr if r.surface is not None else None
            item.kind, item.level, item.out_offset = r.kind, log_p.index(r.log_p), offset
        peln, window = chunk[0][0].peln, chunk[0][0].window
        return (C.byref(geom), peln.ptr, (C.c_double * len(log_p))(*log_p), len(log_p), items, len(chunk), *window,
                int(bool(out_is_double)), C.c_void_p(packed.data_ptr()), stream)

    # the step's one transfer and one synchronisation (pack calls it through this name: the one-transfer tests count it here)
    _to_host = staticmethod(_launch.to_host)

    def pack(self, requests: List[_Request], out_is_double: bool = False) -> Dict[str, Quantity]:
        """name -> host-resident Quantity, C-contiguous over the request's window; views of a buffer that the next call with the
        same requests overwrites."""
        if not requests:
            return {}
        if self._lib is None:
            self._lib = _lib.load()
        geom, offsets, packed, host = self._plan(requests, out_is_double)
        tensor = requests[0].field.data
        _launch.check_library(self._lib, tensor.device, tensor.dtype)
        stream = _launch.stream_of(tensor.device)
        placed = list(zip(requests, offsets))
        windows = [(r, offset) for r, offset in placed if not isinstance(r, _PlevRequest)]
        for _, chunk in _launch.chunks(windows, _lib.DIAG_MAX_ITEMS):
            items = (_lib.DiagItem * len(chunk))()
            for item, (r, offset) in zip(items, chunk):
                _launch.set_window(item, _launch.window_of(r.field, r.level or None, r.window))  # (THIS call's storages)
                item.weight = r.weight.ptr if r.weight is not None else None
                item.kind, item.out_offset = r.kind, offset  # (the kind as asked for: a column integral is no window_of's)
            self._lib.call("pace_diag_pack", C.byref(geom), items, len(chunk), int(bool(out_is_double)),
                           C.c_void_p(packed.data_ptr()), stream)
        for chunk in self._plev_launches([(r, offset) for r, offset in placed if isinstance(r, _PlevRequest)]):
            self._lib.call("pace_plev_diag", *self._plev_arguments(geom, chunk, out_is_double, packed, stream))
        self._to_host(packed, host)
        out = {}
        for r, offset in zip(requests, offsets):
            data = host[offset:offset + int(np.prod(r.shape))].view(r.shape)
            out[r.name] = Quantity(data, dims=r.dims, units=r.units, origin=(0,) * len(r.shape), extent=r.shape)
        return out


class MonitorDiagnostics(Diagnostics, WindowPacker):
    """Diagnostics that save to a sympl-style Monitor."""

    def __init__(self, monitor, names: List[str], derived_names: List[str], z_select: List[ZSelect], lib=None, communicator=None,
                 p_select=(), latlon=None, latlon_monitor=None):
        """
        Args:
            monitor: a sympl-style Monitor object
            names: list of names of diagnostics to save
            derived_names: list of names of derived diagnostics to save
            z_select: the levels to save of variables of the dycore state
            lib: the library the state's fields belong to (default: the product library, loaded at the first store)
            communicator: a communicator that holds the whole cube (run_cube): every store is gathered over it and only its
                root hands the monitor anything -- quantities that lead with TILE_DIM.  None: this rank's tile alone
            p_select: the pressure surfaces to save variables of the dycore state (or `height`) on
            latlon: a LatLonSelect: the variables to save on a regular latitude-longitude grid (needs `communicator`)
            latlon_monitor: the monitor the lat-lon variables go to with the step's time (default: `monitor`, in one state with
                the others)
        """
        if latlon is not None and communicator is None:
            raise ValueError("latlon regrids the whole cube on one device: MonitorDiagnostics needs the whole-cube communicator of "
                             "pace_amd.util.run_cube (the driver: comm_config.type: cube, run_cube_driver)")
        self.latlon = latlon
        self.latlon_monitor = latlon_monitor if latlon_monitor is not None else monitor
        self.communicator = communicator
        self.names = names
        self.derived_names = derived_names
        self.z_select = z_select
        self.p_select = list(p_select)
        self.monitor = monitor
        WindowPacker.__init__(self, lib)

    # ---- what a step asks for ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _whole(name, quantity) -> _Request:
        if len(quantity.dims) not in (2, 3):
            raise ValueError(f"{name} has dimensions {quantity.dims}: diagnostics take 2-D and 3-D variables")
        _, kind, *window = _launch.window_of(quantity)
        return _Request(name, kind, quantity, None, 0, tuple(window), tuple(quantity.dims), quantity.units)

    def _requests(self, state) -> List[_Request]:
        """The reference's order (diagnostics.py:166-178): names, derived names, level selections; then the pressure levels.  The
        Quantities are looked up at every call: Quantity.swap_storage replaces storages during a step."""
        requests = []
        for name in self.names:
            try:
                quantity = getattr(state.dycore_state, name)
            except AttributeError:
                quantity = getattr(state.physics_state, name)
            requests.append(self._whole(name, quantity))
        for name in self.derived_names:
            if name.startswith("column_integrated_"):
                q_in = getattr(state.dycore_state, name[len("column_integrated_"):])
                assert len(q_in.dims) > 2
                if q_in.dims[2] != c.Z_DIM:
                    raise NotImplementedError("this function assumes the z-dimension is the third dimension")
                requests.append(_Request(name, _lib.DIAG_COLUMN_INTEGRAL, q_in, state.dycore_state.delp,
                                         0, tuple(q_in.origin) + tuple(q_in.extent), tuple(q_in.dims[:2]), "kg/m**2"))
            else:
                warnings.warn(f"{name} is not a supported diagnostic variable.")
        for zselect in self.z_select:
            for name in zselect.names:
                quantity = zselect.variable(state.dycore_state, name)
                if not 0 <= zselect.level < quantity.data.shape[2]:
                    raise IndexError(f"z_select level {zselect.level} of {name}: the storage has {quantity.data.shape[2]} levels")
                window = _launch.window_of(quantity, zselect.level)[2:]
                requests.append(_Request(f"{name}_z{zselect.level}", _lib.DIAG_PLANE, quantity, None, zselect.level, window,
                                         tuple(quantity.dims[:2]), quantity.units))
        for pselect in self.p_select:
            for name in pselect.names:
                dycore = state.dycore_state
                quantity = pselect.variable(dycore, name)
                height = name == HEIGHT
                window = tuple(quantity.origin[:2]) + tuple(quantity.extent[:2])
                requests.append(_PlevRequest(pselect.output_name(name), _lib.PLEV_HEIGHT if height else _lib.PLEV_LAYER, quantity,
                                             dycore.phis if height else None, dycore.peln, math.log(pselect.pressure), window,
                                             tuple(quantity.dims[:2]), "m" if height else quantity.units))
        return requests

    # ---- the reference's interface ------------------------------------------------------------------------------------------------
    def _gather(self, requests, packed, transfer_type):
        """The whole cube's arrays of a step, in the requests' order: the windows and planes by ONE pace_cube_gather launch and
        one transfer for all six tiles (gather_state), the column integrals -- which every rank has packed itself: `packed` --
        and the planes on pressure surfaces
        likewise -- stacked on the host.  {name: Quantity leading with TILE_DIM} on the root, None elsewhere."""
        from ..util.gather import Window

        cube = self.communicator
        windows = {r.name: Window(r.field, r.kind, r.level, r.window, r.dims, r.units) for r in requests
                   if not r.packed_by_rank}
        gathered = cube.gather_state(windows, transfer_type=transfer_type) if windows else ({} if cube.rank == c.ROOT_RANK else None)
        mine = {name: q.data.numpy().copy() for name, q in packed.items()}
        if mine:
            stacked = cube.comm.rendezvous(("diagnostics", "columns"), mine,
                                           lambda posts: {name: np.stack([posts[r][name] for r in sorted(posts)]) for name in mine})
        if gathered is None:
            return None
        out = {}
        for r in requests:
            if r.name in gathered:
                out[r.name] = gathered[r.name]
            else:
                out[r.name] = Quantity(stacked[r.name], dims=(c.TILE_DIM,) + r.dims, units=r.units)
        return out

    def store(self, time: Union[datetime, timedelta], state):
        monitor_state = {"time": time}
        requests = self._requests(state)
        if self.communicator is None:
            monitor_state.update(self.pack(requests))
        else:
            columns = self.pack([r for r in requests if r.packed_by_rank])
            gathered = self._gather(requests, columns, np.float32)
            regridded = self._regrid(state) if self.latlon is not None else {}
            if gathered is None:
                return
            monitor_state.update(gathered)
            if self.latlon is not None and self.latlon_monitor is not self.monitor:
                self.latlon_monitor.store({"time": time, **regridded})
            else:
                monitor_state.update(regridded)
        self.monitor.store(monitor_state)

    def _regrid(self, state):
        """The lat-lon arrays of a step: ONE pace_cube_regrid launch for all six tiles and ONE transfer (regrid_state).
        {name: Quantity leading with LON_DIM} on the root, None elsewhere.  They are views of a buffer of their own, apart from
        the gathered arrays'."""
        grid_data = getattr(state, "grid_data", None)
        centres = (grid_data.lon_agrid, grid_data.lat_agrid) if grid_data is not None else None
        return self.communicator.regrid_state(self.latlon.windows(state), self.latlon.grid(), np.float32, centres=centres)

    def store_grid(self, grid_data):
        """lat, lon, lon_agrid, lat_agrid over their compute domains in float64.  GridData keeps these four on the host (numpy,
        the whole storage): those are cut there; a device Quantity goes through the pack as a PLANE."""
        dims = {"lat": (c.X_INTERFACE_DIM, c.Y_INTERFACE_DIM), "lon": (c.X_INTERFACE_DIM, c.Y_INTERFACE_DIM),
                "lon_agrid": (c.X_DIM, c.Y_DIM), "lat_agrid": (c.X_DIM, c.Y_DIM)}
        names = ("lat", "lon", "lon_agrid", "lat_agrid")
        values = {name: getattr(grid_data, name) for name in names}
        if self.communicator is not None:
            self._store_grid_of_the_cube(names, values, dims)
            return
        packed = self.pack([self._whole(name, v) for name, v in values.items() if hasattr(v, "dims")], out_is_double=True)
        for name in names:
            if name in packed:
                self.monitor.store_constant({name: packed[name]})
                continue
            a = np.asarray(values[name], dtype=np.float64)
            n, extra = a.shape[0] - 2 * c.N_HALO_DEFAULT - 1, int(dims[name][0] == c.X_INTERFACE_DIM)
            cut = slice(c.N_HALO_DEFAULT, c.N_HALO_DEFAULT + n + extra)
            data = torch.from_numpy(np.ascontiguousarray(a[cut, cut]))
            self.monitor.store_constant({name: Quantity(data, dims=dims[name], units="radians")})

    def _store_grid_of_the_cube(self, names, values, dims):
        """The same four constants of all six tiles, gathered to the root as the reference's NetCDFMonitor gathers them: device
        Quantities by one pace_cube_gather launch, what GridData keeps on the host by stacking the ranks' cuts."""
        cube = self.communicator
        on_device = [self._whole(name, v) for name, v in values.items() if hasattr(v, "dims")]
        gathered = self._gather(on_device, {}, np.float64) if on_device else None
        cuts = {}
        for name in names:
            if not hasattr(values[name], "dims"):
                a = np.asarray(values[name], dtype=np.float64)
                n, extra = a.shape[0] - 2 * c.N_HALO_DEFAULT - 1, int(dims[name][0] == c.X_INTERFACE_DIM)
                cut = slice(c.N_HALO_DEFAULT, c.N_HALO_DEFAULT + n + extra)
                cuts[name] = a[cut, cut]
        if cuts:
            stacked = cube.comm.rendezvous(("diagnostics", "grid"), cuts,
                                           lambda posts: {name: np.stack([posts[r][name] for r in sorted(posts)]) for name in cuts})
        if cube.rank != c.ROOT_RANK:
            return
        for name in names:
            if name in cuts:
                self.monitor.store_constant({name: Quantity(stacked[name], dims=(c.TILE_DIM,) + dims[name], units="radians")})
            else:
                self.monitor.store_constant({name: gathered[name]})
        if self.latlon is not None:  # the targets' coordinates: lon_ll (nlon values) and lat_ll (nlat values)
            grid = self.latlon.grid()
            self.latlon_monitor.store_constant({"lon_ll": Quantity(grid.lon.copy(), dims=(c.LON_DIM,), units="radians")})
            self.latlon_monitor.store_constant({"lat_ll": Quantity(grid.lat.copy(), dims=(c.LAT_DIM,), units="radians")})

    def cleanup(self):
        if self.communicator is None or self.communicator.rank == c.ROOT_RANK:
            self.monitor.cleanup()
            if self.latlon_monitor is not self.monitor:
                self.latlon_monitor.cleanup()


# ---- the monitor ------------------------------------------------------------------------------------------------------------------
def _host_array(quantity, dims=None) -> np.ndarray:
    if dims is not None and tuple(quantity.dims) != tuple(dims):
        quantity = quantity.transpose(dims)
    view = quantity.view[:]
    return view.detach().cpu().numpy() if torch.is_tensor(view) else np.asarray(view)


GLOBAL_GRID_DIMS = ((c.LON_DIM,), (c.LAT_DIM,))  # what a global array on a regular grid leads with: it has no tile axis


class _TimeChunkedVariable:
    """netcdf_monitor.py:20-40 with the tile axis already in place: (time_chunk_size, 1, *extent)."""

    def __init__(self, initial, time_chunk_size: int):
        first = _host_array(initial)
        self._global = tuple(initial.dims[:1]) == (c.TILE_DIM,)  # (the whole cube: the tile axis comes with the data)
        self.latlon = tuple(initial.dims[:1]) in GLOBAL_GRID_DIMS  # (a lat-lon array: global, and no tile axis at all)
        self._data = np.zeros((time_chunk_size,) + (() if self._global or self.latlon else (1,)) + first.shape, dtype=first.dtype)
        self._data[0].reshape(first.shape)[...] = first
        self.dims = tuple(initial.dims[1:]) if self._global else tuple(initial.dims)
        self.units = initial.units
        self._i_time = 1

    def append(self, quantity):
        a = _host_array(quantity) if self._global or self.latlon else _host_array(quantity, self.dims)
        self._data[self._i_time].reshape(a.shape)[...] = a
        self._i_time += 1

    @property
    def data(self) -> np.ndarray:
        return self._data[:self._i_time]


class NpzMonitor:
    """sympl.Monitor-style object storing model state dictionaries in numpy archives: the reference's NetCDFMonitor
    (netcdf_monitor.py:43-202) without its file format.

    `state_{chunk:04d}_tile{tile}.npz` holds `time` (datetime64[us] or timedelta64[us], dimension [time]), every variable with
    the dimensions [time, tile] followed by its own, and `__meta__`, a JSON string with the dims and units of every variable.
    `constants_<name>_tile{tile}.npz` holds one constant with the leading dimension [tile].  Nothing is pickled.  There is one
    file per tile and no gather: with layout (1, 1) every rank is its tile's root.
    """

    FILENAME_FORMAT = "state_{chunk:04d}_tile{tile}.npz"
    CONSTANT_FILENAME_FORMAT = "constants_{name}_tile{tile}.npz"

    def __init__(self, path: str, tile: int, time_chunk_size: int = 1):
        """
        Args:
            path: directory in which to store data
            tile: the tile this rank holds
            time_chunk_size: number of times per file
        """
        self._path = path
        self._tile = int(tile)
        self._time_chunk_size = time_chunk_size
        self._i_time = 0
        self._chunked: Optional[Dict[str, _TimeChunkedVariable]] = None
        self._times = []
        self._expected_vars = None

    def store(self, state: dict) -> None:
        """Append the model state dictionary.  Writes to disk only when a full time chunk has been accumulated, or when
        .cleanup() is called.  The keys must be those of the first call."""
        if self._expected_vars is None:
            self._expected_vars = set(state.keys())
        elif self._expected_vars != set(state.keys()):
            raise ValueError("state keys must be the same each time store is called, "
                             f"got {set(state.keys())} but previously got {self._expected_vars}")
        state = {**state}  # copy so we don't mutate the input
        time = state.pop("time", None)
        if self._chunked is None:
            self._chunked = {name: _TimeChunkedVariable(quantity, self._time_chunk_size) for name, quantity in state.items()}
        else:
            for name, quantity in state.items():
                self._chunked[name].append(quantity)
        self._times.append(time)
        if (self._i_time + 1) % self._time_chunk_size == 0:
            self.flush()
        self._i_time += 1

    @staticmethod
    def _time_array(times) -> np.ndarray:
        kind = "timedelta64[us]" if times and isinstance(times[0], (timedelta, np.timedelta64)) else "datetime64[us]"
        return np.array(times, dtype=kind)

    def _write(self, filename, arrays, meta):
        path = os.path.join(self._path, filename)
        if os.path.exists(path):
            os.remove(path)
        np.savez(path, __meta__=np.array(json.dumps(meta)), **arrays)

    def flush(self):
        if self._chunked is not None:
            arrays = {"time": self._time_array(self._times)}
            meta = {"time": {"dims": ["time"], "units": ""}}
            for name, chunked in self._chunked.items():
                arrays[name] = chunked.data
                meta[name] = {"dims": ["time"] + ([] if chunked.latlon else ["tile"]) + list(chunked.dims), "units": chunked.units}
            chunk_index = self._i_time // self._time_chunk_size
            self._write(self.FILENAME_FORMAT.format(chunk=chunk_index, tile=self._tile), arrays, meta)
        self._chunked = None
        self._times.clear()

    def store_constant(self, state: Dict[str, Quantity]) -> None:
        for name, quantity in state.items():
            a, dims = _host_array(quantity), list(quantity.dims)
            if dims[:1] != [c.TILE_DIM] and tuple(dims[:1]) not in GLOBAL_GRID_DIMS:
                a, dims = a[None], ["tile"] + dims
            self._write(self.CONSTANT_FILENAME_FORMAT.format(name=name, tile=self._tile), {name: a},
                        {name: {"dims": dims, "units": quantity.units}})

    def cleanup(self):
        self.flush()
