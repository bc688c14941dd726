"""pace_state_extrema (pace_amd/csrc/k_driver.hip) and pace_amd.driver.SafetyChecker against a numpy restatement written here.

The launch shape decides the sizes: a wave of stage one reads whole rows (lane l takes i = l, l + 64, ...), walks 8 consecutive
rows, and a workgroup has 4 waves, so a workgroup takes 32 rows of the window; stage two is ONE wave per field that folds
partials l, l + 64, ...  The workgroup count per field is that of the whole-storage window, (n + 7) * (nk + 1) rows:

    C12 x 7    19-wide rows (19 of 64 lanes), 152 rows -> 5 workgroups, the last with 24 rows; compute window 84 rows -> the last
               two workgroups hold no row of a compute-only field and write the identity
    C13 x 5    odd row length (20 and 13), 120 rows -> 4 workgroups, the last partial
    C68 x 5    75-wide rows: two passes of the 64 lanes, the second with 11; 450 rows -> 15 workgroups, 3 per level and a level's
               rows (75) no multiple of a wave's 8, so waves straddle levels
    C96 x 31   103 * 32 = 3296 rows -> 103 partials per field, more than the 64 lanes of stage two: lanes 0 .. 38 fold two
"""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import build_emu, build_emu_f32  # noqa: E402

SHAPES = ((12, 7), (13, 5), (68, 5), (96, 31))


@pytest.fixture(scope="module")
def emu_lib():
    from pace_amd import _lib

    return _lib.Library(build_emu())


@pytest.fixture(scope="module")
def emu_lib_f32():
    from pace_amd import _lib

    return _lib.Library(build_emu_f32())


# ---- the numpy restatement -----------------------------------------------------------------------------------------------------
def np_extrema(a, compute_only, n, nk):
    """[min of the non-NaN values (+inf if none), max (-inf if none), NaNs in the window, NaNs in the compute domain]."""
    compute = a[3:3 + n, 3:3 + n, :nk]
    window = compute if compute_only else a
    finite = window[~np.isnan(window)].astype(np.float64)
    mn = finite.min() if finite.size else np.inf
    mx = finite.max() if finite.size else -np.inf
    return [mn, mx, float(np.isnan(window).sum()), float(np.isnan(compute).sum())]


def np_check_state(state, checks, n, nk):
    """The decision of the reference's check_state (driver/pace/driver/safety_checks.py:80-110) in numpy: the exception it ends
    with as (type, message), or None."""
    for name, bounds in checks.items():
        if not hasattr(state, name):
            return NotImplementedError, "Variable is not in the state"
        a = getattr(state, name).numpy()
        window = a[3:3 + n, 3:3 + n, :nk] if bounds.compute_domain_only else a
        with np.errstate(all="ignore"):
            mn, mx = window.min(), window.max()  # NaN if the window holds one
        if bounds.minimum_value and mn < bounds.minimum_value:
            return RuntimeError, f"{bounds.minimum_value} specified, {mn} found"
        if bounds.maximum_value and mx > bounds.maximum_value:
            return RuntimeError, f"{bounds.maximum_value} specified, {mx} found"
        if np.isnan(a[3:3 + n, 3:3 + n, :nk]).any():
            return RuntimeError, f"Variable {name} contains a NaN value"
    return None


# ---- fields ------------------------------------------------------------------------------------------------------------------
class Fields:
    """Quantities of a C<n> x <nk> tile for `lib` on `device`; the row padding beyond n + 7 is filled with NaN / 1e300-sized
    garbage, which no result may show."""

    def __init__(self, lib, device, n, nk):
        import torch

        from pace_amd.util import QuantityFactory, SubtileGridSizer

        self.lib, self.n, self.nk = lib, n, nk
        self.dtype = np.float32 if lib.real_bytes == 4 else np.float64
        sizer = SubtileGridSizer.from_tile_params(nx_tile=n, ny_tile=n, nz=nk, n_halo=3, extra_dim_lengths={}, layout=(1, 1))
        self.qf = QuantityFactory(sizer, device=device, dtype=torch.float32 if lib.real_bytes == 4 else torch.float64)

    def base(self, seed):
        rng = np.random.default_rng(seed)
        return rng.uniform(-50.0, 50.0, (self.n + 7, self.n + 7, self.nk + 1)).astype(self.dtype)

    def quantity(self, array):
        q = self.qf.zeros(["x", "y", "z"], "")
        pad = q._base[:, :, self.n + 7:]
        pad[...] = float("nan")
        pad[:, ::2] = 3.0e38 if self.dtype == np.float32 else 1.0e300
        pad[:, 1::4] = -3.0e38 if self.dtype == np.float32 else -1.0e300
        q.set(np.asarray(array, dtype=self.dtype))
        return q


def run(lib, fields, flags):
    from pace_amd.driver import SafetyChecker

    return SafetyChecker(lib).extrema(fields, flags)


def assert_extrema(got, arrays, flags, n, nk, what=""):
    assert got.shape == (len(arrays), 4) and got.dtype == np.float64
    for m, (a, flag) in enumerate(zip(arrays, flags)):
        want = np_extrema(a, flag, n, nk)
        assert all(g == w for g, w in zip(got[m], want)), (what, m, flag, list(got[m]), want)


def planted_cases(f):
    """name -> (array, what the compute-only window must NOT show or None): one planted value per case."""
    n, nk = f.n, f.nk
    big, nan, inf = 1000.0, np.nan, np.inf
    cases = {}

    def case(name, seed, plant):
        a = f.base(seed)
        plant(a)
        cases[name] = a

    def first(a): a[0, 0, 0] = big
    def last(a): a[n + 6, n + 6, nk] = -big
    def last_compute(a): a[n + 2, n + 2, nk - 1] = big
    def halo(a): a[1, n + 4, min(2, nk - 1)] = -big
    def plus_inf(a): a[3 + n // 2, 4, 0] = inf
    def minus_inf(a): a[5, 3 + n // 2, nk - 1] = -inf
    def all_nan_compute(a): a[3:3 + n, 3:3 + n, :nk] = nan
    def all_nan(a): a[...] = nan
    def nan_halo(a): a[n + 3, 7, 1] = nan
    def nan_top(a): a[6, 6, nk] = nan
    def nan_compute(a): a[3, 3, 0] = nan; a[n + 2, n + 2, nk - 1] = nan
    def zeros(a): a[...] = 0.0; a[4, 4, 0] = -0.0

    for seed, plant in enumerate((first, last, last_compute, halo, plus_inf, minus_inf, all_nan_compute, all_nan, nan_halo, nan_top,
                                  nan_compute, zeros)):
        case(plant.__name__, 100 + seed, plant)
    return cases


def check_planted(lib, device, n, nk):
    f = Fields(lib, device, n, nk)
    cases = planted_cases(f)
    names = list(cases)
    arrays = [cases[k] for k in names for _ in (0, 1)]
    flags = [flag for _ in names for flag in (False, True)]
    fields = [f.quantity(a) for a in arrays]
    got = np.concatenate([run(lib, fields[s:s + 16], flags[s:s + 16]) for s in range(0, len(fields), 16)])
    assert_extrema(got, arrays, flags, n, nk, "planted")
    row = {(k, flag): got[2 * names.index(k) + int(flag)] for k in names for flag in (False, True)}
    # what the restatement implies, spelled out
    assert row["first", False][1] == 1000.0 and row["first", True][1] < 1000.0
    assert row["last", False][0] == -1000.0 and row["last", True][0] > -1000.0
    assert row["last_compute", False][1] == 1000.0 and row["last_compute", True][1] == 1000.0
    assert row["halo", False][0] == -1000.0 and row["halo", True][0] > -1000.0
    assert row["plus_inf", True][1] == np.inf and row["minus_inf", True][0] == -np.inf
    cells = n * n * nk
    assert list(row["all_nan_compute", True]) == [np.inf, -np.inf, cells, cells]
    assert list(row["all_nan", False]) == [np.inf, -np.inf, (n + 7) * (n + 7) * (nk + 1), cells]
    assert list(row["nan_halo", False][2:]) == [1, 0] and list(row["nan_halo", True][2:]) == [0, 0]
    assert list(row["nan_top", False][2:]) == [1, 0] and list(row["nan_top", True][2:]) == [0, 0]
    assert list(row["nan_compute", False][2:]) == [2, 2] and list(row["nan_compute", True][2:]) == [2, 2]
    assert list(row["zeros", True]) == [0.0, 0.0, 0, 0]


def check_counts(lib, device, n, nk, counts):
    """Field counts with mixed flags against numpy; then the workspace and the result buffer of ONE checker used for a large and a
    small call: the second result is what a fresh checker gives."""
    from pace_amd.driver import SafetyChecker

    f = Fields(lib, device, n, nk)
    arrays = [f.base(m) * (m + 1) for m in range(max(counts))]
    arrays[0][3 + n // 2, 3 + n // 3, nk // 2] = np.nan
    arrays[-1][0, 1, nk] = np.nan
    fields = [f.quantity(a) for a in arrays]
    flags = [bool((m * 5 // 3) % 2) for m in range(len(arrays))]
    checker = SafetyChecker(lib)
    for count in sorted(counts, reverse=True):
        got = checker.extrema(fields[:count], flags[:count])
        assert_extrema(got, arrays[:count], flags[:count], n, nk, f"{count} fields")
        assert np.array_equal(got, run(lib, fields[:count], flags[:count]))
    if len(counts) > 1:  # a small call with other fields and flags after the large ones
        got = checker.extrema([fields[-1]], [not flags[-1]])
        assert_extrema(got, [arrays[-1]], [not flags[-1]], n, nk, "after a larger call")


def check_seventeen(lib, device):
    from pace_amd import _lib
    from pace_amd.driver import SafetyChecker

    f = Fields(lib, device, 12, 7)
    q = f.quantity(f.base(0))
    checker = SafetyChecker(lib)
    checker.extrema([q], [True])
    (geom, workspace, results), = checker._buffers.values()
    assert _lib.STATE_EXTREMA_MAX_FIELDS == 16
    for count in (17, 0):
        table = (C.c_void_p * 17)(*[q.data.data_ptr()] * 17)
        flags = (C.c_int * 17)(*[1] * 17)
        with pytest.raises(_lib.PaceError, match="invalid argument"):
            lib.call("pace_state_extrema", C.byref(geom), table, flags, count, C.c_void_p(workspace.data_ptr()),
                     C.c_void_p(results.data_ptr()), None if device == "cpu" else checker_stream())
    got = checker.extrema([q] * 17, [True] * 17)  # the host class splits a longer list
    assert got.shape == (17, 4) and (got == got[0]).all()


def checker_stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- the emulated tier ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nk", SHAPES[:3])
def test_planted_values_emulated(emu_lib, emu_lib_f32, n, nk):
    check_planted(emu_lib, "cpu", n, nk)
    check_planted(emu_lib_f32, "cpu", n, nk)


@pytest.mark.parametrize("n,nk,counts", [(12, 7, (1, 4, 16)), (13, 5, (1, 4, 16)), (68, 5, (1, 4)), (96, 31, (1, 4))])
def test_field_counts_emulated(emu_lib, emu_lib_f32, n, nk, counts):
    check_counts(emu_lib, "cpu", n, nk, counts)
    check_counts(emu_lib_f32, "cpu", n, nk, counts[:1] if n == 96 else counts)  # (the emulation of the large shape is slow)


def test_seventeenth_field_is_refused_emulated(emu_lib):
    check_seventeen(emu_lib, "cpu")


def test_header_and_binding_agree_on_the_entry_point():
    import re

    from pace_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "pace_hip.h")).read()
    proto = re.search(r"\bint pace_state_extrema\s*\(([^;]*)\);", text).group(1)
    assert len(proto.split(",")) == len(_lib._PROTOS["pace_state_extrema"][1])
    assert int(re.search(r"#define PACE_STATE_EXTREMA_MAX_FIELDS (\d+)", text).group(1)) == _lib.STATE_EXTREMA_MAX_FIELDS


# ---- check_state ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def clean_checks():
    from pace_amd.driver import SafetyChecker

    saved = dict(SafetyChecker.checks)
    SafetyChecker.clear_all_checks()
    yield SafetyChecker
    SafetyChecker.clear_all_checks()
    SafetyChecker.checks.update(saved)


def check_state_cases(lib, device, SafetyChecker):
    n, nk = 12, 7
    f = Fields(lib, device, n, nk)
    cw = (slice(3, 3 + n), slice(3, 3 + n), slice(0, nk))

    def state(**planted):
        arrays = {"ua": f.base(1), "pt": f.base(2) + 250.0, "delp": np.abs(f.base(3)) + 1.0}
        for name, (index, value) in planted.items():
            arrays[name][index] = value
        return types.SimpleNamespace(**{k: f.quantity(v) for k, v in arrays.items()})

    def outcome(s):
        want = np_check_state(s, SafetyChecker.checks, n, nk)
        checker = SafetyChecker(lib)
        if want is None:
            checker.check_state(s)
            return None
        with pytest.raises(want[0]) as e:
            checker.check_state(s)
        assert want[1] in str(e.value), (want, str(e.value))
        return str(e.value)

    SafetyChecker.register_variable("ua", -200, 200, compute_domain_only=True)
    SafetyChecker.register_variable("pt", 100, 380, compute_domain_only=True)
    SafetyChecker.register_variable("delp", 0, 4000)  # whole storage; the lower bound 0 is not applied
    assert outcome(state()) is None
    # the two bound messages carry the bound and the planted value
    msg = outcome(state(ua=((5, 6, 2), -321.5)))
    assert "Variable ua is outside of its specified bounds" in msg and "-200 specified, -321.5 found" in msg
    msg = outcome(state(pt=((n + 2, n + 2, nk - 1), 1000.0)))
    assert "Variable pt is outside" in msg and "380 specified, 1000.0 found" in msg
    # outside the compute domain a compute-only variable may hold anything; a whole-storage one may not
    assert outcome(state(pt=((0, 0, 0), 1000.0), ua=((n + 6, n + 6, nk), -1e6))) is None
    msg = outcome(state(delp=((0, 0, nk), 5000.0)))
    assert "Variable delp is outside" in msg and "4000 specified, 5000.0 found" in msg
    # a bound of 0 is not applied
    assert outcome(state(delp=((4, 4, 1), -7.0))) is None
    # a NaN in the compute domain: the NaN message, even where a bound is also exceeded elsewhere in the field
    s = state(pt=((6, 6, 3), np.nan))
    s.pt.data[8, 8, 1] = 1000.0
    assert outcome(s) == "Variable pt contains a NaN value"
    # a NaN in the halo of a whole-storage variable silences its bounds and is itself no error
    s = state(delp=((1, 1, 0), np.nan))
    s.delp.data[7, 7, 2] = 5000.0
    assert outcome(s) is None
    # the first registered variable that fails decides
    msg = outcome(state(ua=((5, 6, 2), 300.0), pt=((5, 6, 2), np.nan)))
    assert "Variable ua is outside" in msg
    # an attribute that is not in the state
    SafetyChecker.register_variable("qfog")
    assert outcome(state()) == "Variable is not in the state"
    # double registration; clear_all_checks
    with pytest.raises(NotImplementedError, match="Can only register variables once"):
        SafetyChecker.register_variable("ua", -1, 1)
    SafetyChecker.clear_all_checks()
    assert SafetyChecker.checks == {}
    SafetyChecker(lib).check_state(state(ua=((5, 6, 2), 1e9)))
    SafetyChecker.register_variable("ua", -1, 1)
    assert "1 specified" in outcome(state())
    del cw


def test_check_state_emulated(emu_lib, clean_checks):
    check_state_cases(emu_lib, "cpu", clean_checks)


def test_check_state_emulated_f32(emu_lib_f32, clean_checks):
    check_state_cases(emu_lib_f32, "cpu", clean_checks)


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from pace_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def lib_f32():
    from pace_amd import _lib

    return _lib.load(32)


@pytest.mark.gpu
@pytest.mark.parametrize("n,nk", SHAPES)
def test_planted_values_gpu(lib, lib_f32, n, nk):
    check_planted(lib, "cuda", n, nk)
    check_planted(lib_f32, "cuda", n, nk)


@pytest.mark.gpu
@pytest.mark.parametrize("n,nk,counts", [(12, 7, (1, 4, 16)), (13, 5, (1, 4, 16)), (68, 5, (1, 4, 16)), (96, 31, (1, 4, 16))])
def test_field_counts_gpu(lib, lib_f32, n, nk, counts):
    check_counts(lib, "cuda", n, nk, counts)
    check_counts(lib_f32, "cuda", n, nk, counts)


@pytest.mark.gpu
def test_seventeenth_field_is_refused_gpu(lib):
    check_seventeen(lib, "cuda")


@pytest.mark.gpu
def test_check_state_gpu(lib, lib_f32, clean_checks):
    check_state_cases(lib, "cuda", clean_checks)
    clean_checks.clear_all_checks()
    check_state_cases(lib_f32, "cuda", clean_checks)
