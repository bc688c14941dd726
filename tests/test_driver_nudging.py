"""The driver's nudging_config (pace_amd/driver/nudging.py): one tile of C12 x 63 from tests/golden/c12_restart on a NullComm.

Reference A is the fixture's directory (valid at its coupler.res time T); B and C are written in tmp_path by
DycoreState.to_fortran_restart from perturbed copies, valid at T + 450 s and T + 900 s; the configuration lists them out of order.

* two nudged steps (dt 225 s: weights 0.5 and 1.0 in the bracket A .. B) equal, bit for bit over the nudged fields' whole
  storage, an un-nudged Driver stepped one step at a time with the numpy restatement (tests/nudge_reference.py) applied on the
  host in between: the nudging has no transcendental and no contraction, so this holds on the GPU as well;
* one pace_nudge launch per step; open_restart once per directory; store_tendencies keeps the last step's tendencies;
* A LONE tile on a NullComm does not stay finite: its halos receive the fill value, delp = 0 there, and after the first step
  every nudged field is NaN (measured: 0 % of u, v, pt, qvapor finite after one step, with or without nudging).  The comparison of
  the stepped runs therefore holds the launches, the brackets, the reads and the NaN-ness together, not the arithmetic; fields are
  compared as bits where the expected value is no NaN and as NaN-ness where it is.  The arithmetic through the driver's path is
  held on FINITE data by the next item;
* the driver's Nudging called by hand on a fresh copy of the fixture's state against the restatement on a second copy, bit for
  bit, finite and moved after every call: the next bracket (B .. C, weight 0.5) reads the one new directory into the set that
  fell out of use, beyond the last reference the last one is held and before the first the first, without a second reference in
  the launch; the stored tendencies are the restatement's; without store_tendencies the launch stores none;
* a configuration without nudging_config makes no pace_nudge call;
* the refusals of from_dict and of the constructor, and restart_dict.
"""
import os
import sys
from datetime import timedelta

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import build_emu  # noqa: E402
import nudge_reference  # noqa: E402
import restart_helpers as rh  # noqa: E402

DT = rh.DT
TIMESCALES = {"u": 3600, "v": 7200.0, "pt": 1800, "qvapor": 900}
NAMES = tuple(TIMESCALES)


class SpyLib:
    """A library whose entry-point calls are counted; of a pace_nudge call also (items, second references passed, weight)."""

    def __init__(self, lib):
        self._lib, self.calls, self.nudges = lib, [], []

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def call(self, name, *args):
        self.calls.append(name)
        if name == "pace_nudge":
            items = args[1][:args[2]]
            self.nudges.append((args[2], [bool(x.ref1) for x in items], [bool(x.tendency) for x in items], args[3]))
        return self._lib.call(name, *args)


@pytest.fixture
def clean_checks():
    from pace_amd.driver import SafetyChecker

    saved = dict(SafetyChecker.checks)
    SafetyChecker.clear_all_checks()
    yield SafetyChecker
    SafetyChecker.clear_all_checks()
    SafetyChecker.checks.update(saved)


def _communicator(lib, device):
    from pace_amd.util import NullComm

    return rh.communicator_of(NullComm(rank=0, total_ranks=6, fill_value=0.0), lib, device)


def write_references(lib, device, tmp_path, time):
    """B and C: the fixture's state with the nudged fields moved, at time + 450 s and time + 900 s.  -> their directories."""
    from pace_amd.fv3core import DycoreState

    communicator = _communicator(lib, device)
    state = DycoreState.from_fortran_restart(quantity_factory=rh.factory(lib, device, rh.N, rh.NZ), communicator=communicator,
                                             path=rh.RESTART)
    paths = []
    for m, name in enumerate(("B", "C")):
        state.pt.view[:] = state.pt.view[:] * 1.002
        state.u.view[:] = state.u.view[:] + 1.5
        state.v.view[:] = state.v.view[:] * 0.97 - 0.75
        state.qvapor.view[:] = state.qvapor.view[:] * 0.9
        paths.append(str(tmp_path / name))
        state.to_fortran_restart(communicator=communicator, path=paths[-1], time=time + timedelta(seconds=450 * (m + 1)))
    return paths


def reference_arrays(lib, device, path):
    """name -> the nudged fields of a reference as [i, j, k] host arrays (zeros outside the compute domain)."""
    from pace_amd.fv3core import DycoreState

    state = DycoreState.from_fortran_restart(quantity_factory=rh.factory(lib, device, rh.N, rh.NZ),
                                             communicator=_communicator(lib, device), path=path)
    rh.sync(device)
    return {name: np.array(getattr(state, name).numpy()) for name in NAMES}


def settings(paths, store_tendencies=True, steps=2, **over):
    nudging = {"timescale_seconds": dict(TIMESCALES), "reference_paths": list(paths), "store_tendencies": store_tendencies}
    return rh.settings(stencil_config={}, minutes=0, seconds=int(steps * DT), nudging_config=nudging, **over)


def host_nudge(state, start, end, weight):
    """The restatement on the host over the nudged fields of a DycoreState, written back.  -> name -> the tendencies' storage."""
    tendencies = {}
    for name in NAMES:
        q = getattr(state, name)
        field = np.array(q.numpy())
        new, tendencies[name] = nudge_reference.nudge(field, start[name], None if end is None else end[name], q.origin + q.extent,
                                                      float(TIMESCALES[name]), weight, DT, 1, np.zeros_like(field))
        q.set(new)
    return tendencies


def bases(state):
    return {name: rh.base_of(getattr(state, name)) for name in NAMES}


def same(a, b, names=NAMES):
    """Bits where the expected value is no NaN, NaN-ness where it is."""
    for name in names:
        nan = np.isnan(b[name])
        if not (np.array_equal(np.isnan(a[name]), nan) and np.array_equal(a[name].view(np.uint64)[~nan], b[name].view(np.uint64)[~nan])):
            return False
    return True


def check_run(lib, device, tmp_path, monkeypatch):
    from pace_amd.driver import Driver, DriverConfig
    from pace_amd.driver import nudging as driver_nudging
    from pace_amd.fv3core import DycoreState
    from pace_amd.util import NullComm

    plain = DriverConfig.from_dict({k: v for k, v in settings([rh.RESTART]).items() if k != "nudging_config"})
    time = plain.start_time
    path_b, path_c = write_references(lib, device, tmp_path, time)
    ref_a, ref_b, ref_c = (reference_arrays(lib, device, p) for p in (rh.RESTART, path_b, path_c))
    opened = []
    real_open = driver_nudging.open_restart

    def counted_open(dirname, *args, **kwargs):
        opened.append(dirname)
        return real_open(dirname, *args, **kwargs)

    monkeypatch.setattr(driver_nudging, "open_restart", counted_open)
    # ---- two nudged steps
    spy = SpyLib(lib)
    nudged = Driver(DriverConfig.from_dict(settings([path_c, rh.RESTART, path_b])), comm=NullComm(rank=0, total_ranks=6, fill_value=0.0),
                    lib=spy, device=device)
    assert nudged.nudging.paths == [rh.RESTART, path_b, path_c] and opened == [] and nudged.nudging_tendencies is None
    assert nudged.nudging.times == [time, time + timedelta(seconds=450), time + timedelta(seconds=900)]
    nudged.step_all()
    rh.sync(device)
    assert nudged.time == time + timedelta(seconds=2 * DT)
    assert spy.calls.count("pace_nudge") == 2  # one launch per step
    assert spy.nudges == [(4, [True] * 4, [True] * 4, 0.5), (4, [True] * 4, [True] * 4, 1.0)]
    assert opened == [rh.RESTART, path_b]  # each directory once
    # ---- the same steps without nudging_config, one at a time, the restatement on the host in between
    spy_plain = SpyLib(lib)
    host = Driver(plain, comm=NullComm(rank=0, total_ranks=6, fill_value=0.0), lib=spy_plain, device=device)
    assert host.nudging is None
    for weight in (0.5, 1.0):
        host._critical_path_step_all(steps_count=1, timer=host.performance_collector.timestep_timer, dt=DT)
        rh.sync(device)
        last = host_nudge(host.state.dycore_state, ref_a, ref_b, weight)
    rh.sync(device)
    assert "pace_nudge" not in spy_plain.calls and host.nudging_tendencies is None
    got, want = bases(nudged.state.dycore_state), bases(host.state.dycore_state)
    assert same(got, want), [name for name in NAMES if not np.array_equal(got[name], want[name])]
    # store_tendencies: the last step's
    assert sorted(nudged.nudging_tendencies) == sorted(NAMES)
    for name in NAMES:
        t = nudged.nudging_tendencies[name]
        assert same({name: np.array(t.numpy())}, {name: last[name]}, (name,)), name
        assert t.units == getattr(nudged.state.dycore_state, name).units + " s^-1"
    # ---- by hand, on the FINITE state of the fixture (see the module's docstring): two copies of it, one nudged by the driver's
    # Nudging and one by the restatement.  The next bracket reads C alone, into the set that held A
    qf, communicator = nudged.quantity_factory, nudged.communicator
    state, mirror = (DycoreState.from_fortran_restart(quantity_factory=qf, communicator=communicator, path=rh.RESTART) for _ in "ab")
    step = timedelta(seconds=DT)

    def finite_and_moved(before):
        now = bases(state)
        assert same(now, bases(mirror))
        assert all(np.isfinite(a).all() for a in now.values()) and not any(np.array_equal(now[k], before[k]) for k in NAMES)
        return now

    del spy.nudges[:]
    tendencies = nudged.nudging(state, time + timedelta(seconds=675), step)
    last = host_nudge(mirror, ref_b, ref_c, 0.5)
    rh.sync(device)
    assert opened == [rh.RESTART, path_b, path_c] and sorted(nudged.nudging.held) == [1, 2]
    now = finite_and_moved(bases(DycoreState.from_fortran_restart(quantity_factory=qf, communicator=communicator, path=rh.RESTART)))
    for name in NAMES:  # zero outside the compute domains, the restatement's bits inside
        assert np.array_equal(np.array(tendencies[name].numpy()).view(np.uint64), last[name].view(np.uint64)), name
        assert np.abs(last[name]).max() > 0
    # beyond the last reference it is held; before the first, the first (read again: its set was given to C)
    nudged.nudging(state, time + timedelta(seconds=901), step)
    host_nudge(mirror, ref_c, None, 0.0)
    rh.sync(device)
    assert opened == [rh.RESTART, path_b, path_c]
    now = finite_and_moved(now)
    nudged.nudging(state, time - timedelta(hours=1), step)
    host_nudge(mirror, ref_a, None, 0.0)
    rh.sync(device)
    assert opened == [rh.RESTART, path_b, path_c, rh.RESTART]
    now = finite_and_moved(now)
    assert spy.nudges == [(4, [True] * 4, [True] * 4, 0.5), (4, [False] * 4, [True] * 4, 0.0), (4, [False] * 4, [True] * 4, 0.0)]
    # ---- without store_tendencies the launch stores none
    quiet = driver_nudging.Nudging(driver_nudging.NudgingConfig(timescale_seconds=dict(TIMESCALES), reference_paths=[path_b]),
                                   qf, communicator)
    del spy.nudges[:]
    assert quiet(state, time, step) is None
    host_nudge(mirror, ref_b, None, 0.0)
    rh.sync(device)
    assert spy.nudges == [(4, [False] * 4, [False] * 4, 0.0)]
    finite_and_moved(now)
    nudged.cleanup()
    host.cleanup()


def test_two_nudged_steps_are_the_steps_and_the_restatement_emulated(tmp_path, monkeypatch, clean_checks):
    from pace_amd import _lib

    check_run(_lib.Library(build_emu()), "cpu", tmp_path, monkeypatch)


@pytest.mark.gpu
def test_two_nudged_steps_are_the_steps_and_the_restatement_gpu(tmp_path, monkeypatch, clean_checks):
    from pace_amd import _lib

    check_run(_lib.load(), "cuda", tmp_path, monkeypatch)


def test_the_configuration(tmp_path):
    from pace_amd.driver import DriverConfig
    from pace_amd.driver.nudging import NudgingConfig

    config = DriverConfig.from_dict(settings([rh.RESTART], store_tendencies=False))
    assert isinstance(config.nudging_config, NudgingConfig) and config.nudging_config.label == ""
    assert config.nudging_config.timescale_seconds == {"u": 3600.0, "v": 7200.0, "pt": 1800.0, "qvapor": 900.0}
    assert config.nudging_config.store_tendencies is False and config.nudging_config.reference_paths == [rh.RESTART]
    # restart_dict carries the section on unchanged
    assert config.restart_dict(str(tmp_path))["nudging_config"] == settings([rh.RESTART], store_tendencies=False)["nudging_config"]
    # absent: no nudging
    assert DriverConfig.from_dict(rh.settings(stencil_config={})).nudging_config is None

    def refused(match, **changes):
        d = settings([rh.RESTART])
        d["nudging_config"].update(changes)
        with pytest.raises(ValueError, match=match):
            DriverConfig.from_dict(d)

    for name in ("delp", "delz", "phis"):
        refused("pe, peln, pk, ps and pkz", timescale_seconds={"pt": 3600, name: 3600})
    for name in ("ua", "pe", "qsgs_tke", "temperature"):  # no field of a Fortran restart, or no field at all
        refused("no 3-D DycoreState field of a Fortran restart", timescale_seconds={name: 3600})
    refused("names no field", timescale_seconds={})
    refused("no setting 'timescales'", timescales={"pt": 3600})
    refused("same time", reference_paths=[rh.RESTART, rh.RESTART])
    refused("at least one", reference_paths=[])
    refused("coupler.res is missing", reference_paths=[str(tmp_path)])
    for seconds in (0, -3600.0, "fast", True, float("nan")):
        refused("positive number of seconds", timescale_seconds={"pt": seconds})
    refused("expected bool", store_tendencies="yes")
    refused("expected a list", reference_paths=rh.RESTART)
    refused("expected a mapping", timescale_seconds=["pt"])


def test_a_reference_of_another_shape_is_refused(tmp_path):
    from pace_amd import _lib
    from pace_amd.driver.nudging import Nudging, NudgingConfig
    from pace_amd.fv3core import DycoreState

    lib = _lib.Library(build_emu())
    communicator = _communicator(lib, "cpu")
    config = NudgingConfig(timescale_seconds={"u": 3600.0}, reference_paths=[rh.RESTART])
    Nudging(config, rh.factory(lib, "cpu", rh.N, rh.NZ), communicator)
    with pytest.raises(ValueError, match=r"shape \(63, 13, 12\), the run's is \(5, 13, 12\)"):
        Nudging(config, rh.factory(lib, "cpu", rh.N, 5), communicator)
    with pytest.raises(ValueError, match="the run's is"):
        Nudging(config, rh.factory(lib, "cpu", 13, rh.NZ), communicator)
    # a directory with a coupler.res and no files
    small = DycoreState.init_zeros(rh.factory(lib, "cpu", rh.N, 5))
    small.to_fortran_restart(communicator=communicator, path=str(tmp_path / "small"), time=config.reference_times()[0])
    with pytest.raises(ValueError, match="the run's is"):
        Nudging(NudgingConfig(timescale_seconds={"u": 3600.0}, reference_paths=[str(tmp_path / "small")]),
                rh.factory(lib, "cpu", rh.N, rh.NZ), communicator)
    os.makedirs(tmp_path / "empty")
    with open(tmp_path / "empty" / "coupler.res", "w") as f, open(os.path.join(rh.RESTART, "coupler.res")) as g:
        f.write(g.read())
    with pytest.raises(ValueError, match="no restart files found"):
        Nudging(NudgingConfig(timescale_seconds={"u": 3600.0}, reference_paths=[str(tmp_path / "empty")]),
                rh.factory(lib, "cpu", rh.N, rh.NZ), communicator)
