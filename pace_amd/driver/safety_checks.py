"""SafetyChecker -- the driver's per-step sanity check of the state (reference: driver/pace/driver/safety_checks.py:13-110).

The reference takes numpy's min and max of every registered variable and then looks for NaNs: three passes over each field
and a host synchronisation per number.  Here ONE launch pair (pace_state_extrema, pace_amd/csrc/k_driver.hip) reads every
registered variable once and leaves four doubles per variable on the device -- the minimum and the maximum of the values
that are no NaN, the number of NaNs in the window and in the compute domain -- and one transfer brings them to the host,
which then decides as the reference does, quirks included:

  * a bound that is None or 0 is not applied (the reference tests the bound's truthiness);
  * a NaN anywhere in the window suppresses both bound tests (numpy's min and max are NaN there, and every comparison with
    a NaN is false);
  * after the bound tests, a NaN in the compute domain raises "contains a NaN value".
"""
import ctypes as C
from typing import ClassVar, Dict, Optional

import torch

from .. import _launch, _lib


class VariableBounds:
    def __init__(self, minimum_value: Optional[float] = None, maximum_value: Optional[float] = None,
                 compute_domain_only: bool = False) -> None:
        self.minimum_value = minimum_value
        self.maximum_value = maximum_value
        self.compute_domain_only = compute_domain_only


def _field_tensor(var):
    return var.data if hasattr(var, "dims") else var


class SafetyChecker:
    """Safety-Checker that checks the state for sanity of variables

    Raises:
        NotImplementedError: Doubly-registered variables
        NotImplementedError: Variables not in the state
        RuntimeError: Variables outside the specified bounds
    """

    checks: ClassVar[Dict[str, VariableBounds]] = {}

    def __init__(self, lib=None):
        """lib: the library the state's fields belong to (default: the product library, loaded at the first check)."""
        self._lib = lib
        self._buffers = {}  # (device, n, nk, sj, sk) -> (Geom, workspace, results)

    @classmethod
    def register_variable(cls, name: str, minimum_value: Optional[float] = None, maximum_value: Optional[float] = None,
                          compute_domain_only: bool = False):
        """Register a variable in the checker: `name` is an attribute of the dycore state, the bounds are optional, and
        compute_domain_only says whether the compute domain or the whole storage is looked at.

        Raises:
            NotImplementedError: If variables are doubly-registered
        """
        if name in cls.checks:
            raise NotImplementedError("Can only register variables once")
        cls.checks[name] = VariableBounds(minimum_value, maximum_value, compute_domain_only)

    @classmethod
    def clear_all_checks(cls):
        """Clear all the registered checks"""
        cls.checks.clear()

    # ---- device side ------------------------------------------------------------------------------------------------------------
    def _plan(self, tensors):
        """The geometry the 3-D fields of the library's layout share, and the workspace and result buffers kept for it."""
        differ = "the safety check takes fields of one layout on one device"
        geom = _launch.geometry(
            tensors, lambda t: f"field of shape {tuple(t.shape)}, strides {tuple(t.stride())}: the safety check takes 3-D fields "
                               "allocated with pace_amd.util.QuantityFactory", differ, ndim=(3,))
        device = tensors[0].device
        if any(t.device != device for t in tensors):
            raise ValueError(differ)
        key = (device, geom.n, geom.nk, geom.sj, geom.sk)
        if key not in self._buffers:
            nbytes = int(self._lib.cdll.pace_state_extrema_workspace_bytes(C.byref(geom)))
            if nbytes <= 0:
                raise _lib.PaceError(f"pace_state_extrema_workspace_bytes: invalid geometry {key[1:]}")
            workspace = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
            results = torch.empty(4 * _lib.STATE_EXTREMA_MAX_FIELDS, dtype=torch.float64, device=device)
            self._buffers[key] = (geom, workspace, results)
        return key, self._buffers[key]

    def extrema(self, fields, compute_domain_only):
        """[minimum, maximum, NaNs in the window, NaNs in the compute domain] per field, as a (len(fields), 4) float64 numpy
        array: one launch pair per PACE_STATE_EXTREMA_MAX_FIELDS fields, one transfer (the only synchronisation)."""
        if self._lib is None:
            self._lib = _lib.load()
        tensors = [_field_tensor(f) for f in fields]
        if not tensors:
            return torch.empty((0, 4), dtype=torch.float64).numpy()
        key, (geom, workspace, results) = self._plan(tensors)
        device = tensors[0].device
        for dtype in {t.dtype for t in tensors}:
            _launch.check_library(self._lib, device, dtype)
        stream = _launch.stream_of(device)
        m = _lib.STATE_EXTREMA_MAX_FIELDS
        if len(tensors) > m and results.numel() < 4 * len(tensors):
            results = torch.empty(4 * len(tensors), dtype=torch.float64, device=device)
            self._buffers[key] = (geom, workspace, results)
        for first, chunk in _launch.chunks(tensors, m):
            table = (C.c_void_p * len(chunk))(*[t.data_ptr() for t in chunk])
            flags = (C.c_int * len(chunk))(*[int(bool(x)) for x in compute_domain_only[first:first + m]])
            self._lib.call("pace_state_extrema", C.byref(geom), table, flags, len(chunk), C.c_void_p(workspace.data_ptr()),
                           C.c_void_p(results.data_ptr() + 32 * first), stream)
        return results[:4 * len(tensors)].cpu().numpy().reshape(len(tensors), 4)

    # ---- the reference's decision -------------------------------------------------------------------------------------------------
    def check_state(self, state):
        """check the given dycore state with all the registered constraints

        Raises:
            NotImplementedError: If one of the registered variables are not in the state
            RuntimeError: If one of the variables exceeds its specified bounds
        """
        names, fields, flags = [], [], []
        missing = False
        for variable, variable_bounds in self.checks.items():
            try:
                var = getattr(state, variable)
            except AttributeError:
                missing = True  # (raised below, after the variables registered before it have been judged: the reference's order)
                break
            names.append(variable)
            fields.append(var)
            flags.append(variable_bounds.compute_domain_only)
        found = self.extrema(fields, flags)
        for variable, (min_value, max_value, nan_window, nan_compute) in zip(names, found):
            variable_bounds = self.checks[variable]
            comparable = nan_window == 0  # numpy's min / max of a window with a NaN are NaN: neither comparison holds
            if variable_bounds.minimum_value and comparable and min_value < variable_bounds.minimum_value:
                raise RuntimeError(f"Variable {variable} is outside of its specified bounds: "
                                   f"{variable_bounds.minimum_value} specified, {min_value} found")
            if variable_bounds.maximum_value and comparable and max_value > variable_bounds.maximum_value:
                raise RuntimeError(f"Variable {variable} is outside of its specified bounds: "
                                   f"{variable_bounds.maximum_value} specified, {max_value} found")
            if nan_compute > 0:
                raise RuntimeError(f"Variable {variable} contains a NaN value")
        if missing:
            raise NotImplementedError("Variable is not in the state")
