"""apply_nudging, get_nudging_tendencies -- the state relaxed toward a reference state (reference: util/pace/util/nudging.py).

    tendencies = apply_nudging(state, reference_state, {name: timedelta}, timestep, communicator=communicator)
    tendencies = get_nudging_tendencies(state, reference_state, {name: timedelta}, communicator=communicator)

For every name of `nudging_timescales`, on the compute domain of the state's quantity (D-grid staggering included):

    tendency = (reference - state) / timescale          state += tendency * timestep   (apply_nudging only)

ONE pace_nudge launch (pace_amd/csrc/k_nudge.hip) per 32 names, on the communicator's stream; no temporaries, no host
synchronisation.  In the float64 library the state and the tendencies have the reference's bits.  Stated departures: the
quantities are device storages, so the communicator (its library, device and stream) is a keyword; the tendencies are storages
of the state's layout whose `.view[:]` is what the reference returns (their halos hold zeros, or what a preallocated one held);
`tendencies=` takes preallocated ones, so that a step allocates nothing; and with `end_reference_state` and `weight` the
reference is `reference_state + (end_reference_state - reference_state) * weight`, a bracket of two analyses interpolated in
time.  All arithmetic is in double on the stored values; the float32 library rounds once on each store.
"""
import ctypes as C
from datetime import timedelta
from typing import Mapping, Optional

import torch

from .. import _launch, _lib
from .quantity import Quantity

__all__ = ["apply_nudging", "get_nudging_tendencies", "NO_TENDENCIES"]

NO_TENDENCIES = object()  # apply_nudging(..., tendencies=NO_TENDENCIES): the state is nudged, no tendency is stored; returns {}


def _like(quantity, units):
    """A zeroed storage of the quantity's layout."""
    base = torch.zeros_like(quantity._base)
    data = torch.as_strided(base, quantity.data.shape, quantity.data.stride(),
                            quantity.data.storage_offset() - quantity._base.storage_offset())
    return Quantity(data, quantity.dims, units, origin=quantity.origin, extent=quantity.extent, base=base)


def _nudge(state, reference_state, nudging_timescales, dt, apply, communicator, end_reference_state, weight, tendencies):
    weight = float(weight)
    if not 0.0 <= weight <= 1.0:
        raise ValueError(f"weight {weight} is outside [0, 1]")
    interpolate = end_reference_state is not None and weight != 0.0
    rows = []  # (name, state quantity, reference, end reference or None, tendency, seconds)
    result = {}
    for name, timescale in nudging_timescales.items():
        # (a missing name is the reference's KeyError: its ValueError in _apply_tendencies cannot be reached through apply_nudging,
        # which has looked every name up in the state by then)
        quantity = state[name]
        reference = reference_state[name]
        end = end_reference_state[name] if interpolate else None
        seconds = timescale.total_seconds()
        if not seconds > 0.0:
            raise ValueError(f"{name}: the nudging timescale is {seconds} s; it must be positive")
        if tendencies is NO_TENDENCIES:
            tendency = None
        else:
            tendency = _like(quantity, quantity.units + " s^-1") if tendencies is None else tendencies[name]
            result[name] = tendency
        rows.append((name, quantity, reference, end, tendency, seconds))
    if not rows:
        return result
    fields = [q for _, quantity, reference, end, tendency, _ in rows for q in (quantity, reference, end, tendency) if q is not None]
    geom = _launch.geometry(fields, lambda q: f"nudging: cannot nudge a quantity of dims {q.dims}",
                            "nudging: the state, the reference states and the tendencies do not share one storage layout")
    for name, quantity, reference, end, tendency, _ in rows:
        for other in (reference, end, tendency):
            if other is not None and (tuple(other.dims) != tuple(quantity.dims) or other.data.shape != quantity.data.shape):
                raise ValueError(f"{name}: dims {tuple(other.dims)} and shape {tuple(other.data.shape)} do not match the "
                                 f"state's {tuple(quantity.dims)}, {tuple(quantity.data.shape)}")
    lib = communicator.lib
    _launch.check_library(lib, fields[0].data.device, fields[0].data.dtype, "nudging")
    stream = communicator.stream()
    for _, chunk in _launch.chunks(rows, _lib.NUDGE_MAX_ITEMS):
        items = (_lib.NudgeItem * len(chunk))()
        for item, (_, quantity, reference, end, tendency, seconds) in zip(items, chunk):
            _launch.set_window(item, _launch.window_of(quantity))
            item.ref0, item.ref1 = reference.ptr, None if end is None else end.ptr
            item.tendency = None if tendency is None else tendency.ptr
            item.timescale = seconds
        lib.call("pace_nudge", C.byref(geom), items, len(chunk), weight, float(dt), int(apply), stream)
    return result


def apply_nudging(state, reference_state, nudging_timescales: Mapping[str, timedelta], timestep: timedelta, *, communicator,
                  end_reference_state: Optional[Mapping] = None, weight: float = 0.0, tendencies: Optional[Mapping] = None):
    """
    Nudge the given state towards the reference state according to the provided
    nudging timescales.

    Nudging is applied to the state in-place.

    Args:
        state (dict): A state dictionary.
        reference_state (dict): A reference state dictionary.
        nudging_timescales (dict): A dictionary whose keys are standard names and
            values are timedelta objects indicating the relaxation timescale for that
            variable.
        timestep (timedelta): length of the timestep
        communicator: gives the library, the device and the stream of the launch
        end_reference_state (dict, optional): the reference at the end of a bracket that
            begins at reference_state
        weight (float): where in that bracket the state is, 0 ... 1
        tendencies (dict, optional): preallocated quantities of the state's layout for the result

    Returns:
        nudging_tendencies (dict): A dictionary whose keys are standard names
            and values are Quantity objects indicating the nudging tendency
            of that standard name.
    """
    return _nudge(state, reference_state, nudging_timescales, timestep.total_seconds(), True, communicator, end_reference_state,
                  weight, tendencies)


def get_nudging_tendencies(state, reference_state, nudging_timescales: Mapping[str, timedelta], *, communicator,
                           end_reference_state: Optional[Mapping] = None, weight: float = 0.0,
                           tendencies: Optional[Mapping] = None):
    """
    Return the nudging tendency of the given state towards the reference state
    according to the provided nudging timescales.  The state is only read.

    Args:
        state (dict): A state dictionary.
        reference_state (dict): A reference state dictionary.
        nudging_timescales (dict): A dictionary whose keys are standard names and
            values are timedelta objects indicating the relaxation timescale for that
            variable.
        communicator, end_reference_state, weight, tendencies: as apply_nudging

    Returns:
        nudging_tendencies (dict): A dictionary whose keys are standard names
            and values are Quantity objects indicating the nudging tendency
            of that standard name.
    """
    return _nudge(state, reference_state, nudging_timescales, 0.0, False, communicator, end_reference_state, weight, tendencies)
