"""ValidationCheckpointer (util/pace/util/checkpointer/validation.py:14-143).

The reference opens the savepoint's netCDF file at every call and runs numpy.testing.assert_allclose twice per variable on
clipped host copies.  Here a call stages the slab [n_calls, rank] of every variable in one pinned buffer and makes ONE copy to
the device, ONE launch pair of pace_ckpt_validate (pace_amd/csrc/k_ckpt.hip; more only above 32 variables) and ONE transfer of
six doubles per variable; the fields are never copied, clipped or transposed.

Savepoint data: <savepoint_data_path>/<savepoint>.nc or .npz, holding per variable name an array [savepoint call, rank, ...].
A .nc file is read through whichever of xarray, netCDF4 and h5py imports, else through scipy.io.netcdf_file, which reads
NetCDF-3 only (a NetCDF-4 / HDF5 file then raises a ValueError that names the file and the format).  Where none of the three is
installed only the NetCDF-3 and the npz routes can be, and are, tested.  A file is opened once and kept.  Of an npz file the slabs of this rank are kept in host memory once read -- 8 B per element per
savepoint, call and variable, a third of a calibration's figure (thresholds.py) -- and the .nc routes read a slab per call.
"""
import collections
import contextlib
import ctypes as C
import math
import os.path
from typing import MutableMapping

import numpy as np
import torch

from ... import _launch, _lib
from ._device import DeviceSide
from .base import Checkpointer
from .thresholds import SavepointName, SavepointThresholds


def _clip_window(shape, target_shape):
    """The reference's clipping rule (validation.py:14-58) as (start, length) per axis of the handed array, or None where the
    clipped array would not have the target's shape: an odd difference in length drops the last point (the buffer point of a
    cell-centred axis), then half the remaining difference is clipped from each side."""
    if len(shape) != len(target_shape):
        return None
    window = []
    for array_len, target_len in zip(shape, target_shape):
        if (array_len - target_len) % 2 == 1:
            array_len -= 1
        n_halo_clip = (array_len - target_len) // 2
        if n_halo_clip < 0 or array_len - 2 * n_halo_clip != target_len or target_len < 1:
            return None
        window.append((n_halo_clip, target_len))
    return window


# ---- savepoint files -------------------------------------------------------------------------------------------------------------
class _NpzFile:
    def __init__(self, path):
        self.path = path
        self._file = np.load(path, allow_pickle=False)
        self._names = set(self._file.files)
        self._arrays = {}

    def __contains__(self, name):
        return name in self._names

    def slab(self, name, call, rank):
        if (name, rank) not in self._arrays:  # (a member of the archive is decoded once; only this rank's slabs are kept)
            self._arrays[name, rank] = np.ascontiguousarray(self._file[name][:, rank])
        return self._arrays[name, rank][call]


class _VariablesFile:
    """xarray, netCDF4, h5py and scipy.io.netcdf_file alike: a mapping of names to arrays that slice lazily."""

    def __init__(self, path, variables, values):
        self.path, self._variables, self._values = path, variables, values

    def __contains__(self, name):
        return name in self._variables

    def slab(self, name, call, rank):
        return np.asarray(self._values(self._variables[name], call, rank))

    def names(self):
        return list(self._variables.keys())

    def record(self, name, index=0):
        """Entry `index` of the variable's first axis (a restart file's one Time level) as a host array in the file's own type and
        byte order (pace_amd.util.open_restart)."""
        return np.asarray(np.ma.filled(self._variables[name][index], np.nan))


_HDF5_SIGNATURE = b"\x89HDF\r\n\x1a\n"


def _open_nc(path):
    try:
        import xarray

        return _VariablesFile(path, xarray.open_dataset(path), lambda v, c, r: v[c, r].values)
    except ImportError:
        pass
    try:
        import netCDF4

        return _VariablesFile(path, netCDF4.Dataset(path).variables, lambda v, c, r: np.ma.filled(v[c, r], np.nan))
    except ImportError:
        pass
    try:
        import h5py

        if h5py.is_hdf5(path):
            return _VariablesFile(path, h5py.File(path, "r"), lambda v, c, r: v[c, r])
    except ImportError:
        pass
    with open(path, "rb") as f:
        if f.read(len(_HDF5_SIGNATURE)) == _HDF5_SIGNATURE:
            raise ValueError(f"{path} is a NetCDF-4 / HDF5 file: reading it needs one of xarray, netCDF4 and h5py, and none of them "
                             "is installed (scipy.io.netcdf_file reads NetCDF-3 only)")
    import scipy.io

    return _VariablesFile(path, scipy.io.netcdf_file(path, "r", mmap=False).variables, lambda v, c, r: v[c, r])


def _open_savepoint(directory, savepoint_name):
    nc_file = os.path.join(directory, savepoint_name + ".nc")
    if os.path.exists(nc_file):
        return _open_nc(nc_file)
    npz_file = os.path.join(directory, savepoint_name + ".npz")
    if os.path.exists(npz_file):
        return _NpzFile(npz_file)
    raise FileNotFoundError(f"neither {nc_file} nor {npz_file} exists")


class ValidationCheckpointer(Checkpointer, DeviceSide):
    """
    Checkpointer which can be used to validate the output of a test.
    """

    def __init__(
        self,
        savepoint_data_path: str,
        thresholds: SavepointThresholds,
        rank: int,
        lib=None,
        device=None,
    ):
        """
        Args:
            savepoint_data_path: path to directory containing netcdf (or npz) savepoint data
            thresholds: thresholds to check against
            rank: rank of the process, needed to compare against
                the correct savepoint data
            lib, device: as pace_amd.driver.Driver takes them
        """
        DeviceSide.__init__(self, lib, device)
        self._savepoint_data_path = savepoint_data_path
        self._thresholds = thresholds
        self._rank = rank
        self._n_calls: MutableMapping[SavepointName, int] = collections.defaultdict(int)
        self._files = {}
        self._staging = None

    @contextlib.contextmanager
    def trial(self):
        """
        Context manager for a trial.

        When entered, resets reference data comparison back to the start of the data.

        A new context manager should entered before the code being tested is called,
        and exited at the end of code execution.
        """
        self._n_calls = collections.defaultdict(int)
        yield

    def _stage(self, total):
        """A host buffer of `total` doubles (pinned where there is a device) and the device's (on the CPU: itself); kept."""
        if self._staging is None or self._staging[0].numel() < total:
            self._staging = _launch.staging(total, torch.float64, self.device, alias_on_cpu=True)
        device, host = self._staging
        return host[:total], device[:total]

    def __call__(self, savepoint_name: str, **kwargs) -> None:
        """
        Checks the arrays passed as keyword arguments against thresholds specified.

        Args:
            savepoint_name: name of the savepoint
            **kwargs: array data for variables in that savepoint

        Raises:
            AssertionError: if the thresholds on any variable are not met
            ValueError: if a variable is not in the savepoint's file
        """
        if savepoint_name not in self._files:
            self._files[savepoint_name] = _open_savepoint(self._savepoint_data_path, savepoint_name)
        ds = self._files[savepoint_name]
        n_calls = self._n_calls[savepoint_name]
        var_thresholds = self._thresholds.savepoints[savepoint_name][n_calls]

        missing = None
        entries, total = [], 0  # (Variable, slab, window, offset into the staging buffer)
        for varname, array in kwargs.items():
            if varname not in ds:  # (raised below, after the variables before it have been judged: the reference's order)
                missing = varname
                break
            expected = ds.slab(varname, n_calls, self._rank)
            var = self.describe(varname, array)
            window = _clip_window(tuple(var.tensor.shape), expected.shape)
            if window is None:
                raise AssertionError(f"{varname}: {savepoint_name} call {n_calls}: an array of shape {tuple(var.tensor.shape)} "
                                     f"cannot be clipped to the expected shape {expected.shape}")
            entries.append((var, expected, window, total))
            total += expected.size

        if entries:
            host, device = self._stage(total)
            flat = host.numpy()
            for var, expected, _, offset in entries:
                np.copyto(flat[offset:offset + expected.size].reshape(expected.shape), expected, casting="same_kind")
            if self.device.type != "cpu":
                _launch.to_device(host, device)
            found = self._validate(entries, var_thresholds, device)
            for (var, expected, _, _), (nrel, nabs, max_abs, max_rel, first, compared) in zip(entries, found):
                if nrel > 0 or nabs > 0:
                    threshold = var_thresholds[var.name]
                    which, count, bound = (("relative", nrel, f"rtol={threshold.relative!r}") if nrel > 0 else
                                           ("absolute", nabs, f"atol={threshold.absolute!r}"))
                    index = tuple(int(x) for x in np.unravel_index(int(first), expected.shape))
                    raise AssertionError(
                        f"{var.name}: {savepoint_name} call {n_calls}, rank {self._rank}: not equal to the {which} tolerance {bound}\n"
                        f"Mismatched elements: {int(count)} / {int(compared)}\n"
                        f"Max absolute difference: {max_abs!r}\nMax relative difference: {max_rel!r}\n"
                        f"First mismatch at index {index} (flat {int(first)})")
        if missing is not None:
            raise ValueError(f"argument {missing} not in savepoint file {ds.path}")
        self._n_calls[savepoint_name] += 1

    def _validate(self, entries, var_thresholds, expected):
        """pace_ckpt_validate's six doubles per variable: a launch pair per 32 variables, ONE transfer."""
        out = torch.empty(6 * len(entries), dtype=torch.float64, device=self.device)
        chunks = []
        for start, chunk in _launch.chunks(entries, _lib.CKPT_MAX_ITEMS):
            items = (_lib.CkptItem * len(chunk))()
            for item, (var, slab, window, offset) in zip(items, chunk):
                var.fill(item)
                nd = len(window)
                steps = [math.prod(slab.shape[h + 1:]) for h in range(nd)]  # element strides of the dense C-ordered slab
                origin = [window[var.perm[a]][0] if a < nd else 0 for a in range(3)]
                extent = [window[var.perm[a]][1] if a < nd else 1 for a in range(3)]
                stride = [steps[var.perm[a]] if a < nd else 0 for a in range(3)]
                item.i0, item.j0, item.k0 = origin
                item.wi, item.wj, item.wk = extent
                item.ei, item.ej, item.ek = stride
                item.expected = expected.data_ptr() + 8 * offset
                item.rtol, item.atol = var_thresholds[var.name].relative, var_thresholds[var.name].absolute
            nbytes = int(self.lib.cdll.pace_ckpt_validate_workspace_bytes(items, len(chunk)))
            if nbytes <= 0:
                raise _lib.PaceError("pace_ckpt_validate_workspace_bytes: invalid items")
            chunks.append((start, items, len(chunk), nbytes))
        workspace = torch.empty(max(c[3] for c in chunks) // 8, dtype=torch.float64, device=self.device)
        for start, items, count, _ in chunks:
            self.lib.call("pace_ckpt_validate", items, count, C.c_void_p(workspace.data_ptr()),
                          C.c_void_p(out.data_ptr() + 48 * start), self.stream())
        return out.cpu().numpy().reshape(len(entries), 6).tolist()
