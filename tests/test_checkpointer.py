"""pace_amd.util's checkpointers (pace_amd/util/checkpointer/, pace_amd/csrc/k_ckpt.hip) in both tiers: through the emulation
libraries (float64 and float32 storage) and on the device.

Calibration   against the reference's own run: tests/golden/checkpointer_thresholds.npz, which tools/make_golden_checkpointer.py
              writes by running the reference's ThresholdCalibrationCheckpointer on the inputs of tests/checkpointer_cases.py.
              relative and absolute are equal to the golden values bit for bit, or both NaN; after every trial the minimum, the
              maximum and the sum of magnitudes equal numpy's over the logical storage.
Validation    against numpy.testing.assert_allclose on host copies, the reference's two calls restated in np_validate below:
              the same pass / fail, and on a fail the same mismatch count and the same first index.  Every output field holds
              NaN and huge values everywhere outside its window (halo, extra point, row padding), so every point outside the
              window is a wrong one that must not be found.
Guard pages   the emulated cases again in a child pytest whose allocations lie against inaccessible pages.
End to end    six C12 tiles on threads: thresholds from two perturbed trials against a numpy restatement from two snapshots, a
              validation run that passes with all thresholds 0, and one that fails on one tile.
"""
import ctypes as C
import dataclasses
import functools
import os
import re
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import checkpointer_cases as cases  # noqa: E402
from helpers import GOLDEN, ROOT, build_emu, build_emu_f32  # noqa: E402

GUARDED = os.environ.get("PACE_GUARD_MODE")  # (a child run of test_checkpointers_with_guard_pages)
XYZI, XZIY, XY = ("x", "y", "z_interface"), ("x", "z_interface", "y"), ("x", "y")


@pytest.fixture(scope="module")
def emu_lib():
    from pace_amd import _lib

    return _lib.Library(build_emu())


@pytest.fixture(scope="module")
def emu_lib_f32():
    from pace_amd import _lib

    return _lib.Library(build_emu_f32())


@pytest.fixture(scope="module")
def lib():
    from pace_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def lib_f32():
    from pace_amd import _lib

    return _lib.load(32)


# ---- variables ------------------------------------------------------------------------------------------------------------------
def np_dtype(lib):
    return np.float32 if lib.real_bytes == 4 else np.float64


def factory(lib, device, n, nz):
    import torch

    from pace_amd.util import QuantityFactory, SubtileGridSizer

    sizer = SubtileGridSizer.from_tile_params(nx_tile=n, ny_tile=n, nz=nz, n_halo=3, extra_dim_lengths={}, layout=(1, 1))
    return QuantityFactory(sizer, device=device, dtype=torch.float32 if lib.real_bytes == 4 else torch.float64)


def quantity(qf, dims, array):
    """A Quantity holding `array` over its logical storage, NaN in the padding of its rows."""
    q = qf.zeros(list(dims), "u")
    assert q.shape == array.shape, (q.shape, array.shape)
    q._base[...] = float("nan")
    q.set(array)
    return q


def handed(lib, device, name, array):
    """The variable of tests/checkpointer_cases.py as a checkpoint call hands it over: Quantities of the C12 x 7 and C68 x 5
    storage, a 2-D one, an [x, z_interface, y] view of a 3-D one, a dense numpy vector."""
    if array.shape == (19, 19, 8):
        return quantity(factory(lib, device, 12, 7), XYZI, array)
    if array.shape == (75, 75, 6):
        return quantity(factory(lib, device, 68, 5), XYZI, array)
    if array.shape == (19, 19):
        return quantity(factory(lib, device, 12, 7), XY, array)
    if array.shape == (19, 8, 19):
        return quantity(factory(lib, device, 12, 7), XYZI, array.transpose(0, 2, 1)).transpose(XZIY)
    assert array.ndim == 1, (name, array.shape)
    return array.copy()


def bits(x):
    return struct.pack("<d", float(x))


def same_threshold(got, want):
    """equal bit for bit, or both NaN"""
    return bits(got) == bits(want) or (np.isnan(got) and np.isnan(want))


def same_arrays(got, want):
    """equal (NaNs in the same places), and the same bits wherever the value is no zero"""
    if got.shape != want.shape or not np.array_equal(got, want, equal_nan=True):
        return False
    plain = ~np.isnan(want) & (want != 0)
    return np.array_equal(got[plain].view(np.uint64), want[plain].view(np.uint64))


@functools.lru_cache(maxsize=None)
def calibration_inputs(dtype):
    return cases.calibration_inputs(dtype)  # (computed once per type, never written to)


def np_thresholds(trials, factor=1.0):
    """The reference's arithmetic (thresholds.py:106-161) over a list of arrays, one per trial."""
    mn, mx, asum = np.inf, -np.inf, 0.0
    with np.errstate(all="ignore"):
        for a in trials:
            mn, mx = np.minimum(mn, a), np.maximum(mx, a)
            asum = asum + np.abs(a)
        mean_abs = asum / len(trials)
        relative = 0.0 if np.all(mean_abs == 0.0) else factor * np.nanmax((mx - mn) / mean_abs)
        return float(relative), float(factor * np.max(mx - mn)), (mn, mx, asum)


# ---- calibration ----------------------------------------------------------------------------------------------------------------
def check_calibration_against_reference(lib, device):
    from pace_amd.util import SavepointThresholds, ThresholdCalibrationCheckpointer

    dtype = np_dtype(lib)
    inputs = calibration_inputs(dtype)
    golden = np.load(os.path.join(GOLDEN, "checkpointer_thresholds.npz"), allow_pickle=False)
    tag = "f32" if dtype == np.float32 else "f64"
    assert tuple(golden["names"]) == cases.NAMES
    calibration = ThresholdCalibrationCheckpointer(lib=lib, device=device)
    for trial in range(cases.N_TRIALS):
        with calibration.trial():
            for call in range(cases.N_CALLS):
                calibration(cases.SAVEPOINT, **{name: handed(lib, device, name, a) for name, a in inputs[trial][call].items()})
        # the accumulators after this trial, over the logical storage
        for call in range(cases.N_CALLS):
            for name in cases.NAMES:
                want = np_thresholds([inputs[t][call][name] for t in range(trial + 1)])[2]
                got = calibration.accumulators(cases.SAVEPOINT, call, name)
                for what, g, w in zip(("minimum", "maximum", "abs sum"), got, want):
                    assert same_arrays(g, np.broadcast_to(w, g.shape)), (trial, call, name, what)
    found = calibration.thresholds
    assert list(found.savepoints) == [cases.SAVEPOINT] and len(found.savepoints[cases.SAVEPOINT]) == cases.N_CALLS
    for call in range(cases.N_CALLS):
        assert list(found.savepoints[cases.SAVEPOINT][call]) == list(cases.NAMES)
        for v, name in enumerate(cases.NAMES):
            threshold = found.savepoints[cases.SAVEPOINT][call][name]
            want = (golden[f"relative_{tag}"][call, v], golden[f"absolute_{tag}"][call, v])
            assert same_threshold(threshold.relative, want[0]) and same_threshold(threshold.absolute, want[1]), (call, name, threshold, want)
    # the special values did what they are there for
    first = found.savepoints[cases.SAVEPOINT][0]
    assert first["zeros"].relative == 0.0 and first["zeros"].absolute == 0.0
    assert np.isnan(first["plane"].absolute) and np.isfinite(first["plane"].relative)
    assert first["c68"].absolute == np.inf and np.isfinite(first["c68"].relative)
    assert np.isnan(first["xzy"].absolute) and np.isfinite(first["c12"].relative)
    # asdict / from_dict round trip (the NaNs: compare the representation)
    assert repr(SavepointThresholds.from_dict(dataclasses.asdict(found))) == repr(found)


def check_variable_counts_and_factor(lib, device):
    """1, 32 and 33 variables in one call (one launch, one full launch, a second launch), with factor = 2.5, against numpy."""
    from pace_amd.util import ThresholdCalibrationCheckpointer

    dtype = np_dtype(lib)
    rng = np.random.default_rng(33)
    shapes = [(19, 19, 8), (5,), (19, 19), (19, 8, 19), (7, 3)]
    for count in (1, 32, 33):
        trials = [{f"v{m}": rng.normal(size=shapes[m % len(shapes)]).astype(dtype).astype(np.float64) for m in range(count)}
                  for _ in range(2)]
        plain, scaled = (ThresholdCalibrationCheckpointer(factor=f, lib=lib, device=device) for f in (1.0, 2.5))
        for arrays in trials:
            for calibration in (plain, scaled):
                with calibration.trial():
                    calibration("Many", **{name: handed(lib, device, name, a) if a.ndim != 2 or a.shape == (19, 19) else a.copy()
                                           for name, a in arrays.items()})
        for calibration, factor in ((plain, 1.0), (scaled, 2.5)):
            found = calibration.thresholds.savepoints["Many"]
            assert len(found) == 1 and list(found[0]) == [f"v{m}" for m in range(count)]
            for name, threshold in found[0].items():
                relative, absolute, _ = np_thresholds([t[name] for t in trials], factor)
                assert same_threshold(threshold.relative, relative) and same_threshold(threshold.absolute, absolute), (count, name)
                assert threshold.relative > 0.0 and threshold.absolute > 0.0


def check_bookkeeping(lib, device):
    from pace_amd.util import InsufficientTrialsError, ThresholdCalibrationCheckpointer

    calibration = ThresholdCalibrationCheckpointer(lib=lib, device=device)
    with pytest.raises(InsufficientTrialsError):
        calibration.thresholds
    a = np.arange(5.0)
    with calibration.trial():
        calibration("A", x=a)
        calibration("A", x=a + 1.0)
        calibration("B", y=a)
        assert dict(calibration._n_calls) == {"A": 2, "B": 1}
    with pytest.raises(InsufficientTrialsError):  # one trial is not enough
        calibration.thresholds
    with calibration.trial():
        assert dict(calibration._n_calls) == {"A": 0, "B": 0}  # trial() resets the counters
        calibration("A", x=a * 2.0)
        calibration("A", x=a + 1.0)
        calibration("B", y=a)
    found = calibration.thresholds.savepoints
    assert [len(found["A"]), len(found["B"])] == [2, 1]  # calls, not calls times trials
    assert found["A"][0]["x"].absolute == 4.0 and found["A"][0]["x"].relative == np_thresholds([a, a * 2.0])[0]
    assert found["A"][1]["x"].absolute == 0.0 and found["B"][0]["y"].relative == 0.0
    # an integer tensor and an integer array alike, a layout that changes between trials
    import torch

    with pytest.raises(TypeError):
        calibration("C", k=torch.arange(5, device=device))
    with pytest.raises(TypeError):
        calibration("C", k=np.arange(5))
    with calibration.trial():
        with pytest.raises(ValueError):
            calibration("A", x=np.arange(6.0))


def test_threshold_merge_and_exports():
    import pace_amd.util as util

    merged = util.Threshold(1.0, 5.0).merge(util.Threshold(2.0, 3.0))
    assert (merged.relative, merged.absolute) == (2.0, 5.0)
    for name in ("Checkpointer", "NullCheckpointer", "SnapshotCheckpointer", "ThresholdCalibrationCheckpointer",
                 "ValidationCheckpointer", "Threshold", "SavepointThresholds", "InsufficientTrialsError"):
        assert hasattr(util, name), name
    assert issubclass(util.NullCheckpointer, util.Checkpointer) and util.NullCheckpointer()("x", a=1) is None
    with pytest.raises(TypeError):
        util.Checkpointer()
    again = util.SavepointThresholds.from_dict(dataclasses.asdict(util.SavepointThresholds({"S": [{"v": util.Threshold(1.0, 2.0)}]})))
    assert again == util.SavepointThresholds({"S": [{"v": util.Threshold(1.0, 2.0)}]})


def test_perturb_is_roundoff():
    import torch

    from pace_amd.util import Quantity
    from pace_amd.util.testing import perturb

    a = np.linspace(1.0, 2.0, 1000)
    fill = np.full(4, 1.0e30)
    t = torch.linspace(1.0, 2.0, 1000, dtype=torch.float64)
    q = Quantity(t.clone().reshape(10, 10, 10), ("x", "y", "z"), "u")
    before = (a.copy(), t.clone(), q.data.clone())
    counts = np.arange(3)
    perturb({"a": a, "fill": fill, "t": t, "q": q, "counts": counts, "n": 3}, generator=torch.Generator().manual_seed(1))
    assert np.array_equal(fill, np.full(4, 1.0e30)) and np.array_equal(counts, np.arange(3))
    for now, was in ((a, before[0]), (t.numpy(), before[1].numpy()), (q.data.numpy(), before[2].numpy())):
        assert not np.array_equal(now, was) and np.abs(now / was - 1.0).max() <= 2.3e-16  # (one ulp below 1 is 1.1e-16)
    again = before[1].clone()
    perturb({"t": again}, generator=torch.Generator().manual_seed(1))
    perturb({"t": before[1]}, generator=torch.Generator().manual_seed(1))
    assert torch.equal(again, before[1])  # repeatable


def test_calibration_emulated(emu_lib, emu_lib_f32):
    check_calibration_against_reference(emu_lib, "cpu")
    check_calibration_against_reference(emu_lib_f32, "cpu")


def test_variable_counts_and_factor_emulated(emu_lib, emu_lib_f32):
    check_variable_counts_and_factor(emu_lib, "cpu")
    check_variable_counts_and_factor(emu_lib_f32, "cpu")


def test_bookkeeping_emulated(emu_lib, emu_lib_f32):
    check_bookkeeping(emu_lib, "cpu")
    check_bookkeeping(emu_lib_f32, "cpu")


# ---- validation -------------------------------------------------------------------------------------------------------------------
def clip(array, target_shape):
    """The reference's clipping (validation.py:14-58) in slices: drop the last point where the lengths differ by an odd
    number, then half the rest from each side."""
    selection = []
    for have, want in zip(array.shape, target_shape):
        have -= (have - want) % 2
        halo = (have - want) // 2
        selection.append(slice(halo, have - halo))
    return array[tuple(selection)]


def np_validate(output, expected, rtol, atol):
    """The yardstick: (passed, mismatch count, first index).  passed is what the reference's two assert_allclose calls
    (validation.py:122-142) decide.  The count is that of the first of the two tests that fails and the index is
    np.flatnonzero of the elements that fail either test, from assert_allclose's rules written as masks: NaNs match NaNs,
    an infinity matches only itself, anything else is compared as |a - d| <= atol + rtol * |d|.  Where numpy's message counts
    ("Mismatched elements: N / M") the count is checked against it."""
    not_zero = expected != 0
    message = None
    try:
        with np.errstate(all="ignore"):
            if not np.isnan(rtol):
                np.testing.assert_allclose(output[not_zero], expected[not_zero], rtol=rtol, atol=0.0)
            if not np.isnan(atol):
                np.testing.assert_allclose(output, expected, atol=atol, rtol=0.0)
    except AssertionError as e:
        message = str(e)

    def mask(rt, at, where):
        with np.errstate(all="ignore"):
            nan_a, nan_d = np.isnan(output), np.isnan(expected)
            special = np.isinf(output) | np.isinf(expected)
            close = np.abs(output - expected) <= at + rt * np.abs(expected)
            bad = np.where(nan_a | nan_d, nan_a != nan_d, np.where(special, output != expected, ~close))
        return bad & where

    everywhere = np.ones(expected.shape, dtype=bool)
    relative = mask(rtol, 0.0, not_zero) if not np.isnan(rtol) else ~everywhere
    absolute = mask(0.0, atol, everywhere) if not np.isnan(atol) else ~everywhere
    failed = relative | absolute
    assert (message is None) == (not failed.any()), message
    if message is None:
        return True, 0, -1
    count = int(relative.sum()) if relative.any() else int(absolute.sum())
    counted = re.search(r"Mismatched elements: (\d+) / (\d+)", message)
    if counted:
        assert int(counted.group(1)) == count, message
    return False, count, int(np.flatnonzero(failed)[0])


def garbage_around(array, shape, start, dtype):
    """`array` at `start` of an array of `shape` that holds NaN and huge values everywhere else."""
    huge = 3.0e38 if dtype == np.float32 else 1.0e300
    full = np.full(shape, np.nan)
    full.reshape(-1)[::3] = huge
    full.reshape(-1)[1::5] = -huge
    full[tuple(slice(s, s + e) for s, e in zip(start, array.shape))] = array
    return full


def window_start(shape, target_shape):
    return tuple(((have - (have - want) % 2) - want) // 2 for have, want in zip(shape, target_shape))


def validation_cases(dtype):
    """name -> (handed shape, expected, output inside the window, rtol, atol).  The output equals the expected values (which
    are float32 numbers where the fields are) except at the points a case is about."""
    rng = np.random.default_rng(7)
    eps = np.finfo(dtype).eps
    table = {}

    def base(target):
        expected = (rng.uniform(1.0, 50.0, target) * rng.choice([-1.0, 1.0], target)).astype(dtype).astype(np.float64)
        return expected, expected.copy()

    def up(x):  # the next number of the fields' type above x
        return float(np.nextafter(dtype(x), dtype(np.inf)))

    def add(name, shape, expected, output, rtol, atol):
        assert np.array_equal(output.astype(dtype).astype(np.float64), output, equal_nan=True), name
        table[name] = (shape, expected, output, rtol, atol)

    c12, compute = (19, 19, 8), (12, 12, 7)
    # an error exactly at the bound passes, one ulp above fails: d = 3, rtol = 2^-20, a - d = 3 * 2^-20 (exact in both types)
    for tag, rtol, atol, d, err in (("rtol", 2.0 ** -20, np.nan, 3.0, 3.0 * 2.0 ** -20), ("atol", np.nan, 2.0 ** -10, 1.0, 2.0 ** -10),
                                    ("rtol_with_atol", 2.0 ** -20, 1.0, 3.0, 3.0 * 2.0 ** -20), ("atol_with_rtol", 1.0, 2.0 ** -10, 1.0, 2.0 ** -10)):
        for how in ("at", "above"):
            expected, output = base(compute)
            expected[5, 6, 3] = d
            output[5, 6, 3] = d + err if how == "at" else up(d + err)
            add(f"{how}_{tag}", c12, expected, output, rtol, atol)
    # expected 0, output not: the relative test skips it, the absolute one catches it
    for tag, atol in (("skipped", np.nan), ("caught", 1.0e-6), ("allowed", 1.0e-2)):
        expected, output = base(compute)
        expected[0, 11, 6] = 0.0
        output[0, 11, 6] = 0.0009765625
        add(f"zero_expected_{tag}", c12, expected, output, 0.5, atol)
    # NaNs and infinities
    for tag, a, d in (("nan_both", np.nan, np.nan), ("nan_output", np.nan, 2.0), ("nan_expected", 2.0, np.nan),
                      ("inf_equal", np.inf, np.inf), ("inf_minus_equal", -np.inf, -np.inf), ("inf_unequal", np.inf, -np.inf),
                      ("inf_output", np.inf, 2.0), ("inf_expected", 2.0, -np.inf)):
        for tols, rtol, atol in (("both", 0.5, 1.0e300), ("rel", 0.5, np.nan), ("abs", np.nan, 1.0e300)):
            expected, output = base(compute)
            expected[11, 0, 0], output[11, 0, 0] = d, a
            add(f"{tag}_{tols}", c12, expected, output, rtol, atol)
    # expected 0 with a NaN or an infinite output: the relative test never sees the element, the absolute one fails on it
    for tag, a in (("nan", np.nan), ("inf", np.inf), ("minus_inf", -np.inf)):
        for tols, rtol, atol in (("both", 0.5, 1.0e300), ("rel", 0.5, np.nan), ("abs", np.nan, 1.0e300)):
            expected, output = base(compute)
            expected[6, 2, 4], output[6, 2, 4] = 0.0, a
            add(f"special_at_zero_{tag}_{tols}", c12, expected, output, rtol, atol)
    # a NaN tolerance skips its test: an error of 25 % passes rtol = NaN with atol = 100 and atol = NaN with rtol = 0.5
    for tag, rtol, atol in (("no_rtol", np.nan, 100.0), ("no_atol", 0.5, np.nan), ("neither", np.nan, np.nan), ("tight", 0.1, 100.0)):
        expected, output = base(compute)
        output[3, 3, 3] = float(dtype(expected[3, 3, 3] * 1.25))
        add(f"quarter_off_{tag}", c12, expected, output, rtol, atol)
    # the targets' shapes; one wrong element at each corner of the window (everything outside the window is wrong anyway)
    shapes = {"compute": (c12, compute), "halo": (c12, (18, 18, 7)), "staggered": (c12, (13, 12, 7)), "xzy": ((19, 8, 19), (12, 7, 12)),
              "plane": ((19, 19), (12, 12)), "c68": ((75, 75, 6), (68, 68, 5)), "c68_whole": ((75, 75, 6), (75, 75, 6)),
              "vector": ((5,), (5,)), "vector_inner": ((5,), (3,))}
    for tag, (shape, target) in shapes.items():
        expected, output = base(target)
        add(f"shape_{tag}_exact", shape, expected, output, 0.0, 0.0)
        for corner in np.ndindex(*(2,) * len(target)):
            expected, output = base(target)
            at = tuple((extent - 1) * c for extent, c in zip(target, corner))
            output[at] = up(output[at])
            add(f"shape_{tag}_corner{''.join(map(str, corner))}", shape, expected, output, eps / 4, np.nan)
    # several wrong elements: the count, and the first of them in the expected array's C order
    expected, output = base((68, 68, 5))
    for at in ((67, 67, 4), (40, 1, 0), (9, 66, 3), (9, 66, 4), (33, 33, 2)):
        output[at] = up(output[at])
    add("five_wrong", (75, 75, 6), expected, output, 0.0, 0.0)
    expected, output = base((12, 7, 12))
    for at in ((11, 6, 11), (2, 6, 0), (2, 5, 11)):
        output[at] = up(output[at])
    add("three_wrong_xzy", (19, 8, 19), expected, output, np.nan, 0.0)
    return table


@functools.lru_cache(maxsize=None)
def cached_validation_cases(dtype):
    return validation_cases(dtype)


def write_savepoint(directory, name, arrays, fmt):
    """arrays: name -> [savepoint call, rank, ...]; as <name>.npz or as NetCDF-3 classic <name>.nc written with scipy."""
    if fmt == "npz":
        np.savez(os.path.join(directory, name + ".npz"), **arrays)
        return
    import scipy.io

    with scipy.io.netcdf_file(os.path.join(directory, name + ".nc"), "w") as f:
        for var, a in arrays.items():
            dims = []
            for axis, extent in enumerate(a.shape):
                dims.append(f"{var}_dim{axis}")
                f.createDimension(dims[-1], extent)
            f.createVariable(var, "f8", tuple(dims))[:] = a


def parse_failure(message):
    count, compared = map(int, re.search(r"Mismatched elements: (\d+) / (\d+)", message).groups())
    return count, compared, int(re.search(r"\(flat (-?\d+)\)", message).group(1))


def check_validation_against_numpy(lib, device, directory, fmt="npz"):
    """(NetCDF-3 files: check_slabs_ranks_and_errors reads them)"""
    from pace_amd.util import SavepointThresholds, Threshold, ValidationCheckpointer

    dtype = np_dtype(lib)
    table = cached_validation_cases(dtype)
    os.makedirs(directory, exist_ok=True)
    write_savepoint(directory, "Cases", {name: case[1][None, None] for name, case in table.items()}, fmt)
    thresholds = SavepointThresholds({"Cases": [{name: Threshold(case[3], case[4]) for name, case in table.items()}]})
    validation = ValidationCheckpointer(directory, thresholds, 0, lib=lib, device=device)
    outcomes = {}
    for name, (shape, expected, output, rtol, atol) in table.items():
        full = garbage_around(output, shape, window_start(shape, expected.shape), dtype)
        variable = handed(lib, device, name, full)
        host = clip(full, expected.shape)
        assert np.array_equal(host, output, equal_nan=True), name
        want = np_validate(host, expected, rtol, atol)
        with validation.trial():
            try:
                validation("Cases", **{name: variable})
                got = (True, 0, -1)
                assert validation._n_calls["Cases"] == 1
            except AssertionError as e:
                assert str(e).startswith(name + ":"), (name, str(e))  # the message names the variable
                count, compared, first = parse_failure(str(e))
                assert compared == expected.size, (name, str(e))
                got = (False, count, first)
                assert validation._n_calls["Cases"] == 0  # the counter advances only after a passing call
        assert got == want, (name, got, want)
        outcomes[name] = got[0]
    # the table decided what it was written to decide
    for name, passed in outcomes.items():
        expect_pass = (name.startswith(("at_", "nan_both", "inf_equal", "inf_minus_equal", "quarter_off_no", "quarter_off_neither"))
                       or name.endswith("_exact") or name in ("zero_expected_skipped", "zero_expected_allowed")
                       or (name.startswith("special_at_zero_") and name.endswith("_rel")))
        assert passed == expect_pass, name
    assert len(validation._files) == 1  # one file, opened once
    # 33 variables in one call: a second launch; the first failing variable is the one reported
    many = [name for name in table if name.endswith("_exact") or name.startswith("at_")]
    many = (many * 3)[:32]
    arrays = {f"m{m}": table[name][1][None, None] for m, name in enumerate(many)}
    arrays["m32"] = table["five_wrong"][1][None, None]
    write_savepoint(directory, "Many", arrays, fmt)
    variables = {}
    for m, name in enumerate(many + ["five_wrong"]):
        shape, expected, output = table[name][:3]
        variables[f"m{m}"] = handed(lib, device, name, garbage_around(output, shape, window_start(shape, expected.shape), dtype))
    bounds = {f"m{m}": Threshold(table[name][3], table[name][4]) for m, name in enumerate(many)}
    bounds["m32"] = Threshold(1.0, 1.0)
    validation = ValidationCheckpointer(directory, SavepointThresholds({"Many": [bounds, bounds]}), 0, lib=lib, device=device)
    validation("Many", **variables)
    bounds["m32"] = Threshold(0.0, 0.0)
    with validation.trial():
        with pytest.raises(AssertionError, match=r"^m32: Many call 0") as e:
            validation("Many", **variables)
        assert parse_failure(str(e.value))[0] == 5


def check_slabs_ranks_and_errors(lib, device, directory, fmt):
    """Two calls read consecutive slabs, `rank` selects its slab, an unknown variable is a ValueError (after the variables
    before it have been judged), a savepoint without a file a FileNotFoundError."""
    from pace_amd.util import SavepointThresholds, Threshold, ValidationCheckpointer

    dtype = np_dtype(lib)
    rng = np.random.default_rng(11)
    data = rng.uniform(1.0, 2.0, (2, 3, 12, 12, 7)).astype(dtype).astype(np.float64)
    os.makedirs(directory, exist_ok=True)
    write_savepoint(directory, "Slabs", {"a": data, "b": data[:, :, :, :, 0]}, fmt)
    zero = {"a": Threshold(0.0, 0.0), "b": Threshold(0.0, 0.0), "c": Threshold(0.0, 0.0)}
    thresholds = SavepointThresholds({"Slabs": [zero, zero, zero], "Nowhere": [zero]})

    def fields(call, rank):
        return {"a": handed(lib, device, "a", garbage_around(data[call, rank], (19, 19, 8), (3, 3, 0), dtype)),
                "b": handed(lib, device, "b", garbage_around(data[call, rank, :, :, 0], (19, 19), (3, 3), dtype))}

    for rank in (0, 2):
        validation = ValidationCheckpointer(directory, thresholds, rank, lib=lib, device=device)
        validation("Slabs", **fields(0, rank))
        with pytest.raises(AssertionError, match="^a: Slabs call 1"):  # the second call reads the second slab
            validation("Slabs", **fields(0, rank))
        validation("Slabs", **fields(1, rank))
        assert validation._n_calls["Slabs"] == 2
        with validation.trial():
            with pytest.raises(AssertionError, match=f"^a: Slabs call 0, rank {rank}"):  # another rank's slab
                validation("Slabs", **fields(0, 1))
            with pytest.raises(ValueError, match="argument c not in"):
                validation("Slabs", c=fields(0, rank)["a"], **fields(0, rank))
            with pytest.raises(AssertionError, match="^b: Slabs"):  # b is judged before the missing c is reported
                validation("Slabs", b=fields(1, rank)["b"], c=fields(0, rank)["a"])
            with pytest.raises(AssertionError, match="cannot be clipped"):
                validation("Slabs", a=fields(0, rank)["b"])
            assert validation._n_calls["Slabs"] == 0
            with pytest.raises(FileNotFoundError):
                validation("Nowhere", a=fields(0, rank)["a"])
        assert len(validation._files) == 1


def test_validation_emulated(emu_lib, emu_lib_f32, tmp_path):
    check_validation_against_numpy(emu_lib, "cpu", str(tmp_path / "f64"))
    check_validation_against_numpy(emu_lib_f32, "cpu", str(tmp_path / "f32"))


@pytest.mark.parametrize("fmt", ["npz", "nc"])
def test_slabs_ranks_and_errors_emulated(emu_lib, emu_lib_f32, tmp_path, fmt):
    check_slabs_ranks_and_errors(emu_lib, "cpu", str(tmp_path / "f64"), fmt)
    check_slabs_ranks_and_errors(emu_lib_f32, "cpu", str(tmp_path / "f32"), fmt)


def test_snapshot_checkpointer(tmp_path, monkeypatch):
    import torch

    from pace_amd.util import SnapshotCheckpointer

    snapshot = SnapshotCheckpointer(rank=3)
    t = torch.arange(6.0, dtype=torch.float64).reshape(2, 3)
    snapshot("A", x=t, y=np.ones(2))
    t += 1.0  # (a clone was kept)
    snapshot("B", x=t)
    dataset = snapshot.dataset
    assert dataset["x_savepoints"] == ["A", "B"] and dataset["y_savepoints"] == ["A"]
    assert np.array_equal(dataset["x"], np.stack([np.arange(6.0).reshape(2, 3), np.arange(6.0).reshape(2, 3) + 1.0]))
    assert dataset["y"].shape == (1, 2)
    monkeypatch.chdir(tmp_path)
    snapshot.cleanup()
    written = np.load(tmp_path / "comparison_rank3.npz", allow_pickle=False)
    assert list(written["x_savepoints"]) == ["A", "B"] and np.array_equal(written["x"], dataset["x"])


# ---- argument errors, header and binding ------------------------------------------------------------------------------------------
def check_argument_errors(lib, device):
    import torch

    from pace_amd import _lib

    real = torch.float32 if lib.real_bytes == 4 else torch.float64
    field = torch.zeros(8 * 16 * 4, dtype=real, device=device)
    doubles = torch.zeros(3 * 5 * 4 * 3, dtype=torch.float64, device=device)
    work = torch.zeros(64, dtype=torch.float64, device=device)
    stream = None if device == "cpu" else C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def items(count=1, **over):
        table = (_lib.CkptItem * _lib.CKPT_MAX_ITEMS)()
        for item in table:
            item.field, item.ni, item.nj, item.nk, item.sj, item.sk = field.data_ptr(), 5, 4, 3, 8, 32
            item.mn, item.mx, item.asum = (doubles.data_ptr() + 480 * m for m in range(3))
            item.i0, item.j0, item.k0, item.wi, item.wj, item.wk = 1, 1, 0, 3, 2, 3
            item.expected, item.ei, item.ej, item.ek = doubles.data_ptr(), 6, 3, 1
            item.rtol, item.atol = 0.0, 0.0
            for key, value in over.items():
                setattr(item, key, value)
        return table

    wp, op = C.c_void_p(work.data_ptr()), C.c_void_p(work.data_ptr() + 256)
    lib.call("pace_ckpt_accumulate", items(), 1, 1, stream)
    lib.call("pace_ckpt_thresholds", items(), 1, 2, wp, op, stream)
    lib.call("pace_ckpt_validate", items(), 1, wp, op, stream)
    assert int(lib.cdll.pace_ckpt_thresholds_workspace_bytes(items(), 2)) == 2 * 32
    assert int(lib.cdll.pace_ckpt_validate_workspace_bytes(items(), 2)) == 2 * 48
    assert int(lib.cdll.pace_ckpt_validate_workspace_bytes(items(wi=6), 1)) == 0
    bad_everywhere = [dict(count=0), dict(count=_lib.CKPT_MAX_ITEMS + 1), dict(count=-1), dict(ni=0), dict(nj=0), dict(nk=-1)]
    bad_storage = [dict(field=None), dict(sj=4), dict(sk=8 * 3 + 4)]
    bad_accumulators = [dict(mn=None), dict(mx=None), dict(asum=None)]
    bad_window = [dict(expected=None), dict(i0=-1), dict(wi=0), dict(wi=5), dict(j0=3), dict(wj=0), dict(k0=1), dict(wk=4), dict(ei=-1)]
    for kwargs in bad_everywhere + bad_storage + bad_accumulators:
        count = kwargs.pop("count", 1)
        with pytest.raises(_lib.PaceError, match="invalid argument"):
            lib.call("pace_ckpt_accumulate", items(**kwargs), count, 0, stream)
        kwargs["count"] = count
    for kwargs in bad_everywhere + bad_accumulators:
        count = kwargs.pop("count", 1)
        with pytest.raises(_lib.PaceError, match="invalid argument"):
            lib.call("pace_ckpt_thresholds", items(**kwargs), count, 2, wp, op, stream)
        kwargs["count"] = count
    for kwargs in bad_everywhere + bad_storage + bad_window:
        count = kwargs.pop("count", 1)
        with pytest.raises(_lib.PaceError, match="invalid argument"):
            lib.call("pace_ckpt_validate", items(**kwargs), count, wp, op, stream)
        kwargs["count"] = count
    for args in (("pace_ckpt_accumulate", None, 1, 0), ("pace_ckpt_thresholds", items(), 1, 0, wp, op),
                 ("pace_ckpt_thresholds", items(), 1, 2, None, op), ("pace_ckpt_thresholds", items(), 1, 2, wp, None),
                 ("pace_ckpt_validate", items(), 1, None, op), ("pace_ckpt_validate", items(), 1, wp, None)):
        with pytest.raises(_lib.PaceError, match="invalid argument"):
            lib.call(*args, stream)


def test_argument_errors_emulated(emu_lib, emu_lib_f32):
    check_argument_errors(emu_lib, "cpu")
    check_argument_errors(emu_lib_f32, "cpu")


def test_header_and_binding_agree_on_the_entry_points():
    from pace_amd import _lib

    text = open(os.path.join(ROOT, "include", "pace_hip.h")).read()
    for name in ("pace_ckpt_accumulate", "pace_ckpt_thresholds_workspace_bytes", "pace_ckpt_thresholds",
                 "pace_ckpt_validate_workspace_bytes", "pace_ckpt_validate"):
        proto = re.search(rf"\b(?:int|int64_t) {name}\s*\(([^;]*)\);", text).group(1)
        assert len(proto.split(",")) == len(_lib._PROTOS[name][1]), name
        assert name in _lib.EXPORTED_SYMBOLS
    assert int(re.search(r"#define PACE_CKPT_MAX_ITEMS (\d+)", text).group(1)) == _lib.CKPT_MAX_ITEMS == 32
    body = re.search(r"typedef struct \{([^}]*)\} pace_ckpt_item_t;", text).group(1)
    names = re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", body))
    assert names == [name for name, _ in _lib.CkptItem._fields_]
    assert C.sizeof(_lib.CkptItem) == 136


# ---- guard pages ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["over", "under"])
def test_checkpointers_with_guard_pages(mode):
    """The emulated cases of both kinds in a child pytest whose every allocation -- the fields, the uploaded vectors, the
    accumulators, the expected values, the workspaces -- ends at (over) or starts right after (under) an inaccessible page
    (tests/guard.py, tests/test_guard_pages.py).  The accumulators and the expected buffer are allocated at their exact size:
    they have neither lead nor tail there."""
    if GUARDED:
        return  # (this IS the child)
    import test_guard_pages

    passed, tail = test_guard_pages._guarded_pytest(mode, ["test_checkpointer.py"])
    for case in ("test_calibration_emulated", "test_variable_counts_and_factor_emulated", "test_bookkeeping_emulated",
                 "test_validation_emulated", "test_slabs_ranks_and_errors_emulated[npz]", "test_slabs_ranks_and_errors_emulated[nc]",
                 "test_argument_errors_emulated"):
        assert any(t.endswith("::" + case) for t in passed), (case, tail)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def fan_out_class():
    from pace_amd.util import Checkpointer
    from pace_amd.util.testing import perturb

    class FanOut(Checkpointer):
        """Hands every call to several checkpointers.  With a generator it first perturbs, in place and once, the variables
        of the run's FIRST savepoint -- fields of the state itself, from before anything has been computed: the run's inputs."""

        def __init__(self, *targets, generator=None):
            self.targets, self.generator, self.calls = targets, generator, 0
            self.failure = None

        def __call__(self, savepoint_name, **kwargs):
            if self.calls == 0 and self.generator is not None:
                perturb(kwargs, generator=self.generator)
            self.calls += 1
            try:
                for target in self.targets:
                    target(savepoint_name, **kwargs)
            except AssertionError as e:
                self.failure = (savepoint_name, e)
                raise

    return FanOut


def occurrences(dataset):
    """(variable, savepoint, call of that savepoint, index into the variable's snapshots) of a SnapshotCheckpointer's dataset."""
    found = []
    for key, names in dataset.items():
        if key.endswith("_savepoints"):
            seen = {}
            for index, savepoint in enumerate(names):
                found.append((key[:-len("_savepoints")], savepoint, seen.get(savepoint, 0), index))
                seen[savepoint] = seen.get(savepoint, 0) + 1
    return found


def check_end_to_end(lib, device, directory, whole_step):
    import torch

    from helpers import run_acoustic_six_tiles, run_dycore_six_tiles
    from pace_amd.util import SavepointThresholds, SnapshotCheckpointer, Threshold, ThresholdCalibrationCheckpointer, ValidationCheckpointer

    FanOut = fan_out_class()
    run = (lambda cps: run_dycore_six_tiles(lib, device, checkpointers=cps)) if whole_step else \
        (lambda cps: run_acoustic_six_tiles(lib, device, checkpointers=cps))
    tiles = range(6)

    # 1. two perturbed trials: a snapshot and the calibration at once
    calibrations = [ThresholdCalibrationCheckpointer(lib=lib, device=device) for _ in tiles]
    snapshots = []
    for trial in range(2):
        snapshots.append([SnapshotCheckpointer(rank=t) for t in tiles])
        generators = [torch.Generator(device=device).manual_seed(100 * trial + t) for t in tiles]
        with contextlib_all([c.trial() for c in calibrations]):
            run([FanOut(snapshots[trial][t], calibrations[t], generator=generators[t]) for t in tiles])
    differ = 0
    for t in tiles:
        found = calibrations[t].thresholds.savepoints
        first, second = snapshots[0][t].dataset, snapshots[1][t].dataset
        listed = occurrences(first)
        assert listed == occurrences(second)
        assert sum(len(call) for calls in found.values() for call in calls) == len(listed)
        for variable, savepoint, call, index in listed:
            relative, absolute, _ = np_thresholds([first[variable][index], second[variable][index]])
            threshold = found[savepoint][call][variable]
            assert same_threshold(threshold.relative, relative) and same_threshold(threshold.absolute, absolute), (t, savepoint, call, variable)
            assert np.isfinite(relative) and np.isfinite(absolute) and relative >= 0.0 and absolute >= 0.0, (t, savepoint, call, variable)
            differ += absolute > 0.0
    assert differ > 0  # (the perturbation reached the savepoints)
    if whole_step:  # (k_split = 1, n_split = 2: 16 + 2 * 55 + 10 + the remapping's 18 + 12)
        assert len(listed) == 166
    del calibrations, snapshots

    # 2. an unperturbed run's snapshot as savepoint files; an unperturbed run validates against them with all thresholds 0
    plain = [SnapshotCheckpointer(rank=t) for t in tiles]
    run(plain)
    datasets = [s.dataset for s in plain]
    listed = occurrences(datasets[0])
    files, calls_of = {}, {}
    for variable, savepoint, call, index in listed:
        calls_of[savepoint] = max(calls_of.get(savepoint, 0), call + 1)
    for variable, savepoint, call, index in listed:
        shape = datasets[0][variable][index].shape
        slabs = files.setdefault(savepoint, {}).setdefault(variable, np.empty((calls_of[savepoint], 6) + shape))
        for t in tiles:
            slabs[call, t] = datasets[t][variable][index]
    os.makedirs(directory, exist_ok=True)
    for savepoint, arrays in files.items():
        write_savepoint(directory, savepoint, arrays, "npz")
    zero = SavepointThresholds({savepoint: [{variable: Threshold(0.0, 0.0) for variable in arrays} for _ in range(calls_of[savepoint])]
                                for savepoint, arrays in files.items()})
    validations = [ValidationCheckpointer(directory, zero, t, lib=lib, device=device) for t in tiles]
    run(validations)  # two runs are bit-identical at every savepoint
    for t in tiles:
        assert dict(validations[t]._n_calls) == calls_of

    # 3. one expected value of one D_SW-Out variable changed on one tile
    wrong_tile, wrong_call = 4, 0  # (the first substep: the run ends early)
    changed = dict(files["D_SW-Out"])
    changed["ptd"] = changed["ptd"].copy()
    changed["ptd"][wrong_call, wrong_tile, 9, 5, 40] *= 1.0 + 2.0 ** -40
    write_savepoint(directory, "D_SW-Out", changed, "npz")
    watchers = [FanOut(ValidationCheckpointer(directory, zero, t, lib=lib, device=device)) for t in tiles]
    with pytest.raises(RuntimeError, match=f"tile {wrong_tile} failed") as e:
        run(watchers)
    assert isinstance(e.value.__cause__, AssertionError) and str(e.value.__cause__).startswith(f"ptd: D_SW-Out call {wrong_call}, rank {wrong_tile}")
    count, _, flat = parse_failure(str(e.value.__cause__))
    assert count == 1 and flat == np.ravel_multi_index((9, 5, 40), changed["ptd"].shape[2:])
    for t in tiles:
        validation = watchers[t].targets[0]
        if t == wrong_tile:
            assert watchers[t].failure[0] == "D_SW-Out" and validation._n_calls["D_SW-Out"] == wrong_call
            assert validation._n_calls["D_SW-In"] == wrong_call + 1
        else:  # the other five passed every call they came to
            assert watchers[t].failure is None and watchers[t].calls == sum(validation._n_calls.values()) >= 1


class contextlib_all:
    """Several context managers as one."""

    def __init__(self, managers):
        self.managers = managers

    def __enter__(self):
        for m in self.managers:
            m.__enter__()

    def __exit__(self, *exc):
        for m in reversed(self.managers):
            m.__exit__(*exc)
        return False


def test_end_to_end_emulated(emu_lib, tmp_path):
    """AcousticDynamics alone on this tier: the whole DynamicalCore step takes the emulator minutes per run and this test makes
    five runs; the GPU tier runs the whole step."""
    if GUARDED:
        return  # (five six-tile runs under guard pages belong to tests/test_guard_pages.py's own lists, not to this child)
    check_end_to_end(emu_lib, "cpu", str(tmp_path), whole_step=False)


# ---- on the GPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_calibration_gpu(lib, lib_f32):
    check_calibration_against_reference(lib, "cuda")
    check_calibration_against_reference(lib_f32, "cuda")


@pytest.mark.gpu
def test_variable_counts_and_factor_gpu(lib, lib_f32):
    check_variable_counts_and_factor(lib, "cuda")
    check_variable_counts_and_factor(lib_f32, "cuda")


@pytest.mark.gpu
def test_bookkeeping_gpu(lib, lib_f32):
    check_bookkeeping(lib, "cuda")
    check_bookkeeping(lib_f32, "cuda")


@pytest.mark.gpu
def test_validation_gpu(lib, lib_f32, tmp_path):
    check_validation_against_numpy(lib, "cuda", str(tmp_path / "f64"))
    check_validation_against_numpy(lib_f32, "cuda", str(tmp_path / "f32"))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["npz", "nc"])
def test_slabs_ranks_and_errors_gpu(lib, lib_f32, tmp_path, fmt):
    check_slabs_ranks_and_errors(lib, "cuda", str(tmp_path / "f64"), fmt)
    check_slabs_ranks_and_errors(lib_f32, "cuda", str(tmp_path / "f32"), fmt)


@pytest.mark.gpu
def test_argument_errors_gpu(lib, lib_f32):
    check_argument_errors(lib, "cuda")
    check_argument_errors(lib_f32, "cuda")


@pytest.mark.gpu
def test_end_to_end_gpu(lib, tmp_path):
    check_end_to_end(lib, "cuda", str(tmp_path), whole_step=True)
