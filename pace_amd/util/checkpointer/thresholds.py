"""Threshold, SavepointThresholds and ThresholdCalibrationCheckpointer (util/pace/util/checkpointer/thresholds.py:23-162).

The reference folds numpy's minimum, maximum and abs of every handed array into host arrays.  Here a checkpoint call is ONE
launch of pace_ckpt_accumulate (pace_amd/csrc/k_ckpt.hip) for all its variables -- more only above 32 -- without a transfer or
a synchronisation, and `thresholds` is one launch pair of pace_ckpt_thresholds per 32 variables and ONE transfer of four
doubles per variable.

Memory: three doubles -- 24 B -- per element per savepoint, call and variable, whatever the field's type.  A checkpointed step
with k_split = 1, n_split = 2 hands over 166 variables, 162 whole 3-D fields and four 2-D ones: about 112 MB per tile at C12 x 79
(19 x 19 x 80 points a field) and about 12.3 GB at C192 x 79.
"""
import collections
import contextlib
import ctypes as C
import dataclasses
from typing import Dict, List

import torch

from ... import _launch, _lib
from ._device import DeviceSide
from .base import Checkpointer

SavepointName = str
VariableName = str


class InsufficientTrialsError(Exception):
    pass


@dataclasses.dataclass
class Threshold:
    relative: float
    absolute: float

    def merge(self, other: "Threshold") -> "Threshold":
        """
        Provide a threshold which is always satisfied
        if both input thresholds are satisfied.

        This is generally a less strict threshold than either input.
        """
        return Threshold(
            relative=max(self.relative, other.relative),
            absolute=max(self.absolute, other.absolute),
        )


@dataclasses.dataclass
class SavepointThresholds:
    savepoints: Dict[SavepointName, List[Dict[VariableName, Threshold]]]

    @classmethod
    def from_dict(cls, data) -> "SavepointThresholds":
        """The inverse of dataclasses.asdict (an extension: the reference rebuilds the class with dacite)."""
        return cls(savepoints={
            name: [{var: t if isinstance(t, Threshold) else Threshold(relative=float(t["relative"]), absolute=float(t["absolute"]))
                    for var, t in call.items()} for call in calls]
            for name, calls in data["savepoints"].items()})


class _Accumulators:
    """mn, mx, asum of one variable at one call of one savepoint: dense, storage order (x fastest)."""

    def __init__(self, var, device):
        self.perm, self.extents, self.shape = var.perm, var.extents, tuple(var.tensor.shape)
        self.mn, self.mx, self.asum = (torch.empty(var.count, dtype=torch.float64, device=device) for _ in range(3))
        self.folds = 0


class ThresholdCalibrationCheckpointer(Checkpointer, DeviceSide):
    """
    Calibrates thresholds to be used by a ValidationCheckpointer.

    Does this by recording the minimum and maximum values seen across trials,
    and using them to derive the maximum relative and absolute error one could
    have across any pair of trials, then multiplying this by a user-provided factor.

    The whole logical storage of a variable is covered, halos and the extra point included (the reference covers `.data`); the
    padding of a row is not.  See the module's docstring for the memory this takes: 24 B per element per savepoint, call and
    variable.
    """

    def __init__(self, factor: float = 1.0, lib=None, device=None):
        """
        Args:
            factor: set thresholds equal to this factor of the maximum error
                seen across trials
            lib, device: as pace_amd.driver.Driver takes them
        """
        DeviceSide.__init__(self, lib, device)
        self._factor = factor
        # dictionaries (over savepoint name) of lists (over call count) of dictionaries (over variable name)
        self._accumulators: Dict[SavepointName, List[Dict[VariableName, _Accumulators]]] = collections.defaultdict(list)
        self._n_trials = 0
        self._n_calls: Dict[SavepointName, int] = collections.defaultdict(int)

    def __call__(self, savepoint_name, **kwargs):
        """
        Record values for a savepoint.

        Args:
            savepoint_name: name of the savepoint
            **kwargs: data for the savepoint
        """
        i_call = self._n_calls[savepoint_name]
        if len(self._accumulators[savepoint_name]) < i_call + 1:
            self._accumulators[savepoint_name].append({})
        store = self._accumulators[savepoint_name][i_call]
        fresh, again = [], []  # (the first fold of a variable writes its accumulators: they are never initialised)
        for varname, array in kwargs.items():
            var = self.describe(varname, array)
            acc = store.get(varname)
            if acc is None:
                acc = store[varname] = _Accumulators(var, self.device)
            elif acc.extents != var.extents or acc.perm != var.perm:
                raise ValueError(f"{savepoint_name} call {i_call}: {varname} changed its shape or layout between trials")
            (fresh if acc.folds == 0 else again).append((var, acc))
            acc.folds += 1
        for group, first in ((fresh, 1), (again, 0)):
            for _, chunk in _launch.chunks(group, _lib.CKPT_MAX_ITEMS):
                items = (_lib.CkptItem * len(chunk))()
                for item, (var, acc) in zip(items, chunk):
                    var.fill(item)
                    item.mn, item.mx, item.asum = acc.mn.data_ptr(), acc.mx.data_ptr(), acc.asum.data_ptr()
                self.lib.call("pace_ckpt_accumulate", items, len(chunk), first, self.stream())
        self._n_calls[savepoint_name] += 1

    @contextlib.contextmanager
    def trial(self):
        """
        Context manager for a trial.

        A new context manager should entered each time the code being
        calibrated is called, and exited at the end of code execution.
        If each of these calls is done with slightly perturbed inputs,
        this calibrator will be able to estimate an error tolerance for
        each savepoint call.
        """
        for name in self._n_calls:
            self._n_calls[name] = 0
        yield
        self._n_trials += 1

    def accumulators(self, savepoint_name, i_call, varname):
        """(minimum, maximum, sum of magnitudes) so far, as float64 numpy arrays with the handed array's axes (a transfer)."""
        acc = self._accumulators[savepoint_name][i_call][varname]
        nd = len(acc.shape)
        order = [0] * nd
        for b in range(nd):
            order[acc.perm[nd - 1 - b]] = b
        return tuple(a.cpu().numpy().reshape(acc.extents[::-1][3 - nd:]).transpose(order) for a in (acc.mn, acc.mx, acc.asum))

    @property
    def thresholds(self) -> SavepointThresholds:
        if self._n_trials < 2:
            raise InsufficientTrialsError(
                "at least 2 trials required to generate thresholds"
            )
        entries = []  # (savepoint, call, variable, accumulators): the reference's order
        for savepoint_name in self._accumulators:
            for i_call in range(self._n_calls[savepoint_name]):
                for varname, acc in self._accumulators[savepoint_name][i_call].items():
                    entries.append((savepoint_name, i_call, varname, acc))
        found = self._reduce([e[3] for e in entries])
        savepoints: Dict[SavepointName, List[Dict[VariableName, Threshold]]] = {}
        for savepoint_name in self._accumulators:
            savepoints[savepoint_name] = [{} for _ in range(self._n_calls[savepoint_name])]
        for (savepoint_name, i_call, varname, _), (rel, absolute, all_zero, _) in zip(entries, found):
            relative = 0.0 if all_zero == 1.0 else self._factor * rel
            savepoints[savepoint_name][i_call][varname] = Threshold(relative=float(relative), absolute=float(self._factor * absolute))
        return SavepointThresholds(savepoints=savepoints)

    def _reduce(self, accs):
        """pace_ckpt_thresholds' four doubles per variable: a launch pair per 32 variables, ONE transfer."""
        if not accs:
            return []
        out = torch.empty(4 * len(accs), dtype=torch.float64, device=self.device)
        chunks = []
        for start, chunk in _launch.chunks(accs, _lib.CKPT_MAX_ITEMS):
            items = (_lib.CkptItem * len(chunk))()
            for item, acc in zip(items, chunk):
                item.ni, item.nj, item.nk = acc.extents
                item.mn, item.mx, item.asum = acc.mn.data_ptr(), acc.mx.data_ptr(), acc.asum.data_ptr()
            nbytes = int(self.lib.cdll.pace_ckpt_thresholds_workspace_bytes(items, len(chunk)))
            if nbytes <= 0:
                raise _lib.PaceError("pace_ckpt_thresholds_workspace_bytes: invalid items")
            chunks.append((start, items, len(chunk), nbytes))
        # (launches on one stream run in order: one workspace serves them all)
        workspace = torch.empty(max(c[3] for c in chunks) // 8, dtype=torch.float64, device=self.device)
        for start, items, count, _ in chunks:
            self.lib.call("pace_ckpt_thresholds", items, count, self._n_trials, C.c_void_p(workspace.data_ptr()),
                          C.c_void_p(out.data_ptr() + 32 * start), self.stream())
        return out.cpu().numpy().reshape(len(accs), 4).tolist()
