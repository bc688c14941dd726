"""SnapshotCheckpointer (util/pace/util/checkpointer/snapshots.py:22-72).

A stated departure: the reference builds an xarray Dataset and writes netCDF; neither library is a dependency here.  `dataset`
is a dict -- per variable an array [savepoint call, ...] and "<name>_savepoints", the list of savepoint names -- and `cleanup()`
writes it as comparison_rank<rank>.npz.  The copies are device clones (torch.clone); nothing here needs a kernel of the project's.
"""
import collections

import numpy as np
import torch

from .base import Checkpointer


class _Snapshots:
    def __init__(self):
        self._savepoints = collections.defaultdict(list)
        self._arrays = collections.defaultdict(list)

    def store(self, savepoint_name: str, variable_name: str, python_data):
        self._savepoints[variable_name].append(savepoint_name)
        self._arrays[variable_name].append(python_data)

    @property
    def dataset(self) -> dict:
        data_vars = {}
        for variable_name, savepoint_list in self._savepoints.items():
            data_vars[f"{variable_name}_savepoints"] = list(savepoint_list)
            arrays = [a.cpu().numpy() if torch.is_tensor(a) else a for a in self._arrays[variable_name]]
            data_vars[variable_name] = np.concatenate([array[None] for array in arrays], axis=0)
        return data_vars


class SnapshotCheckpointer(Checkpointer):
    """
    Checkpointer which can be used to save datasets showing the evolution
    of variables between checkpointer calls.
    """

    def __init__(self, rank: int):
        self._rank = rank
        self._snapshots = _Snapshots()

    def __call__(self, savepoint_name, **kwargs):
        for name, value in kwargs.items():
            data = value.data if hasattr(value, "dims") else value
            array_data = data.detach().clone() if torch.is_tensor(data) else np.copy(data)
            self._snapshots.store(savepoint_name, name, array_data)

    @property
    def dataset(self) -> dict:
        return self._snapshots.dataset

    def cleanup(self):
        np.savez(f"comparison_rank{self._rank}.npz",
                 **{k: (np.asarray(v, dtype=str) if k.endswith("_savepoints") else v) for k, v in self.dataset.items()})
