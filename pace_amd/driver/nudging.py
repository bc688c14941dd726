"""nudging_config -- the run held to a sequence of analyses (not in the reference's driver; fv3gfs-util's nudging, for which
pace.util.apply_nudging and open_restart were written).

    nudging_config:
      timescale_seconds: {u: 21600, v: 21600, pt: 21600, qvapor: 21600}   # DycoreState field names
      reference_paths: [ANL/2016080100, ANL/2016080106]                    # Fortran restart directories
      label: ""
      store_tendencies: false

Each directory's valid time is its coupler.res; the directories are ordered by it.  `Nudging` keeps TWO sets of the nudged fields
on the device, the ends of the bracket the model time is in, and fills a set (open_restart: one staging buffer, one copy, one
pace_state_unpack launch) only when the time enters a new bracket: a run that moves forward reads each directory once.  A step
is ONE pace_nudge launch (pace_amd.util.apply_nudging) toward the reference interpolated linearly in time to the END of the step;
before the first reference and after the last, the nearest one is held.

What is not done: ua / va stay as the step's last c2l_ord left them until the next step recomputes them; halos are not written
(the dycore's first halo updates refresh them); under comm_config.type cube each tile thread launches for its own tile.
delp, delz and phis are refused: pe, peln, pk, ps and pkz derive from the mass field and no stage after the nudging restores them.
"""
import dataclasses
import os
from datetime import datetime, timedelta
from typing import Dict, List

from ..fv3core.initialization.dycore_state import _FIELDS, FORTRAN_RESTART_FIELDS
from ..util.nudging import NO_TENDENCIES, apply_nudging
from ..util.restart import (RESTART_PROPERTIES, _open_nc, get_coupler_res_filename, get_current_date_from_coupler_res,
                            open_restart, restart_filenames)

_MASS_FIELDS = ("delp", "delz", "phis")


@dataclasses.dataclass
class NudgingConfig:
    """timescale_seconds: DycoreState field name -> relaxation timescale in seconds; reference_paths: directories of Fortran
    restart files, each with a coupler.res; label: prepended to the files' names; store_tendencies: keep the last step's
    tendencies as Driver.nudging_tendencies."""

    timescale_seconds: Dict[str, float] = dataclasses.field(default_factory=dict)
    reference_paths: List[str] = dataclasses.field(default_factory=list)
    label: str = ""
    store_tendencies: bool = False

    def __post_init__(self):
        if not isinstance(self.timescale_seconds, dict):
            raise ValueError(f"nudging_config.timescale_seconds = {self.timescale_seconds!r}: expected a mapping of field names")
        if not isinstance(self.reference_paths, (list, tuple)) or not all(isinstance(p, str) for p in self.reference_paths):
            raise ValueError(f"nudging_config.reference_paths = {self.reference_paths!r}: expected a list of directories")
        if len(self.timescale_seconds) < 1:
            raise ValueError("nudging_config.timescale_seconds names no field")
        for name, seconds in self.timescale_seconds.items():
            if name in _MASS_FIELDS:
                raise ValueError(f"nudging_config.timescale_seconds: {name} cannot be nudged: pe, peln, pk, ps and pkz derive from "
                                 "the mass field and would go stale, no stage after the nudging restores them (mass nudging is "
                                 "out of scope)")
            if name not in FORTRAN_RESTART_FIELDS or len(_FIELDS[name][0]) != 3:
                raise ValueError(f"nudging_config.timescale_seconds: {name!r} is no 3-D DycoreState field of a Fortran restart "
                                 f"({sorted(n for n in FORTRAN_RESTART_FIELDS if n not in _MASS_FIELDS)})")
            if isinstance(seconds, bool) or not isinstance(seconds, (int, float)) or not seconds > 0:
                raise ValueError(f"nudging_config.timescale_seconds.{name} = {seconds!r}: expected a positive number of seconds")
        if len(self.reference_paths) < 1:
            raise ValueError("nudging_config.reference_paths needs at least one directory")
        times = self.reference_times()
        if len(set(times)) != len(times):
            raise ValueError(f"nudging_config.reference_paths: two references are valid at the same time ({sorted(times)})")

    def reference_times(self) -> List[datetime]:
        """The valid time of each directory of reference_paths, in their order."""
        times = []
        for path in self.reference_paths:
            coupler_res = get_coupler_res_filename(path, self.label)
            if not os.path.isfile(coupler_res):
                raise ValueError(f"nudging_config.reference_paths: {coupler_res} is missing, the reference has no valid time")
            times.append(get_current_date_from_coupler_res(coupler_res))
        return times

    @classmethod
    def from_dict(cls, config) -> "NudgingConfig":
        from .config import _strict

        if isinstance(config, cls):
            return config
        values = dict(config or {})
        if isinstance(values.get("timescale_seconds"), dict):  # (a yaml integer is a number of seconds too)
            values["timescale_seconds"] = {name: float(s) if isinstance(s, int) and not isinstance(s, bool) else s
                                           for name, s in values["timescale_seconds"].items()}
        return _strict(cls, "nudging_config", values)


def bracket(times, t):
    """times ascending.  -> (index of the bracket's start, index of its end or None, weight): the references t lies between and
    where between them it is, in double from total_seconds(); before the first and after the last the nearest one is held.  A
    bracket is (t0, t1]: AT a later reference's time the weight is 1 in the bracket that ends there -- the interpolation's own
    expression, and the next directory is not read before the time has passed its predecessor's."""
    if t <= times[0]:
        return 0, None, 0.0
    if t > times[-1]:
        return len(times) - 1, None, 0.0
    start = max(m for m in range(len(times) - 1) if times[m] < t)
    weight = (t - times[start]).total_seconds() / (times[start + 1] - times[start]).total_seconds()
    return start, start + 1, weight


class Nudging:
    def __init__(self, config: NudgingConfig, quantity_factory, communicator):
        self.config = config
        self.communicator = communicator
        times = config.reference_times()
        order = sorted(range(len(times)), key=times.__getitem__)
        self.paths = [config.reference_paths[m] for m in order]
        self.times = [times[m] for m in order]
        self.names = list(config.timescale_seconds)
        self.timescales = {name: timedelta(seconds=float(config.timescale_seconds[name])) for name in self.names}
        self._check_shapes(quantity_factory)
        # two sets of the nudged fields; `held` says which reference each holds
        self.sets = [{name: quantity_factory.zeros(*_FIELDS[name], dtype=float) for name in self.names} for _ in range(2)]
        self.held = [None, None]
        self.tendencies = None
        if config.store_tendencies:
            self.tendencies = {name: quantity_factory.zeros(_FIELDS[name][0], _FIELDS[name][1] + " s^-1", dtype=float)
                               for name in self.names}

    def _check_shapes(self, quantity_factory):
        tile = self.communicator.partitioner.tile_index(self.communicator.rank)
        sizer = quantity_factory.sizer
        for path in self.paths:
            filenames = restart_filenames(path, tile, self.config.label)
            if not filenames:
                raise ValueError(f"nudging_config.reference_paths: no restart files found at {path}")
            shapes = {}
            for filename in filenames:
                file = _open_nc(filename)
                for restart_name in file.names():
                    shapes[restart_name] = (tuple(file._variables[restart_name].shape[1:]), filename)
            for name in self.names:
                restart_name = RESTART_PROPERTIES[FORTRAN_RESTART_FIELDS[name]]["restart_name"]
                if restart_name not in shapes:
                    raise ValueError(f"nudging_config.reference_paths: {path} has no variable {restart_name} (for {name})")
                want = tuple(sizer.get_extent(_FIELDS[name][0]))[::-1]
                if shapes[restart_name][0] != want:
                    raise ValueError(f"nudging_config.reference_paths: {restart_name} of {shapes[restart_name][1]} has shape "
                                     f"{shapes[restart_name][0]}, the run's is {want}")

    def _load(self, slot, index):
        to_state = {FORTRAN_RESTART_FIELDS[name]: self.sets[slot][name] for name in self.names}
        open_restart(self.paths[index], self.communicator, label=self.config.label, only_names=list(to_state), to_state=to_state)
        self.held[slot] = index

    def _slots_of(self, wanted):
        """The sets that hold the references `wanted` (one or two indices); one that neither set holds is read into a set that
        holds none of them, an empty one first."""
        free = sorted((slot for slot in (0, 1) if self.held[slot] not in wanted), key=lambda slot: self.held[slot] is not None)
        slots = []
        for index in wanted:
            if index not in self.held:
                self._load(free.pop(0), index)
            slots.append(self.held.index(index))
        return slots

    def __call__(self, dycore_state, valid_time: datetime, timestep: timedelta):
        """Nudge the fields of dycore_state toward the reference at valid_time, the end of the step: one launch.  -> the
        tendencies where they are stored, else None."""
        start, end, weight = bracket(self.times, valid_time)
        slots = self._slots_of([start] if end is None else [start, end])
        first, second = slots[0], (None if end is None else slots[1])
        state = {name: getattr(dycore_state, name) for name in self.names}
        apply_nudging(state, self.sets[first], self.timescales, timestep, communicator=self.communicator,
                      end_reference_state=None if second is None else self.sets[second], weight=weight,
                      tendencies=NO_TENDENCIES if self.tendencies is None else self.tendencies)
        return self.tendencies
