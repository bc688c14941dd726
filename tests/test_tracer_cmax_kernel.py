"""pace_tracer_cmax, pace_tracer_subcycles, pace_tracer_divide_fluxes_levels and the three `_levels` stencils
(pace_amd/csrc/k_tracer.hip): the launches of the tracer advection's Courant-number sub-cycling.

Shapes: C12 x 2 (less than a wave of cells per row, every level in the widened form: 2 // 6 - 1 < 0), C13 x 7 (odd), C68 x 5 (two
workgroups per row), C12 x 19 (19 // 6 - 1 = 2: the levels 0 and 1 take the plain form, the others the widened one).

* pace_tracer_cmax BIT FOR BIT against the restatement (tests/tracer_subcycle_reference.py).  cx and cy hold small random values
  on the compute domain and HUGE ones everywhere else -- column ie + 1 of cx, row je + 1 of cy, every halo, the row padding,
  level nk; sin_sg5 is huge and negative outside its compute window: one cell read outside a window changes the maximum.  On top
  of that a maximum is planted, a different value per level: in each corner cell, in the last row and the last column away from
  the corners, in cx only, in cy only, as the negative value of largest magnitude; NaNs everywhere outside the windows (no
  effect), one NaN inside (in cx, in cy, in sin_sg5: it arrives, and only on its level(s)).  The float32 library: the restatement
  is fed what the storages hold, widened.  Inputs keep their bits; the doubles around cmax[0 .. nk - 1] keep theirs.
* Two runs, and six tiles' launches into ONE buffer in two orders, give the same bits (the launch keeps the larger of the old and
  the new value).
* pace_tracer_subcycles for one and six tables against the restatement AND against the literal counts: cmax of 0, 0.999,
  nextafter(1, 0) (1.0 + c rounds to 2.0: 2), 1.0, 2.5, max_subcycles - 1 (the largest count allowed), max_subcycles (refused), a
  NaN, an infinity; 70 levels (past a wave) with each level's maximum on a different tile, the tables in two orders; the integers
  around out[0 .. nk + 1] keep their bits.
* The divide kernel and the three `_levels` stencils bit for bit over the whole raw storage against the oracle's stencil
  (oracle/tracer.py) on the levels ksplt selects, every other cell keeping its bits, for ksplt all 1, all 3 and the mixed,
  non-contiguous 1, 3, 1, 2, 2, 1, ... and min_subcycles 1, 2, 3; the float32 library in the exact class of
  tests/test_tracer_stencils.py.
* Every PACE_ERR_ARG of the six wrappers, refused before any launch.
* The header and the ctypes binding agree on the new entry points.

Every check is a function of the device: the CPU tier calls it with the emulation libraries, the GPU tier with the product's."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import ROOT, build_emu, build_emu_f32  # noqa: E402
import tracer_subcycle_reference as ref  # noqa: E402

X, Y, Z = "x", "y", "z"
SHAPES = ((12, 2), (13, 7), (68, 5), (12, 19))
HUGE = 1.0e30
PAD = 4  # doubles / integers kept around an output to see that nothing but the output is written


def _libs(device):
    from pace_amd import _lib

    if device == "cpu":
        return [_lib.Library(build_emu()), _lib.Library(build_emu_f32())]
    return [_lib.load(), _lib.load(32)]


def _stream(device):
    if device == "cpu":
        return None
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sync(device):
    if device != "cpu":
        import torch

        torch.cuda.synchronize()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same(got, want):
    """Bits where the expected value is no NaN, NaN-ness where it is."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


class Fields:
    """Storages of one launch shape on the device; `host` keeps what each one holds, indexed [i, j(, k)] over the WHOLE base (row
    padding and level nk included)."""

    def __init__(self, lib, device, n, nk):
        import torch

        from pace_amd import _launch
        from pace_amd.util import QuantityFactory, SubtileGridSizer

        self.lib, self.device, self.n, self.nk = lib, device, n, nk
        self.np_real = np.float32 if lib.real_bytes == 4 else np.float64
        self.factory = QuantityFactory(SubtileGridSizer(n, n, nk), device, torch.float32 if lib.real_bytes == 4 else torch.float64)
        self.q, self.host = {}, {}
        probe = self.factory.zeros([X, Y, Z], "")
        self.geom = _launch.geometry([probe], str, "")
        self.s3 = tuple(probe._base.shape)[::-1]  # (padded row, n + 7, nk + 1)
        self.s2 = self.s3[:2]

    def put(self, name, a):
        import torch

        a = np.ascontiguousarray(np.asarray(a).astype(self.np_real))
        if name not in self.q:
            self.q[name] = self.factory.zeros([X, Y, Z] if a.ndim == 3 else [X, Y], "")
        self.q[name]._base.copy_(torch.as_tensor(np.ascontiguousarray(a.transpose(*range(a.ndim)[::-1]))))
        self.host[name] = a

    def raw(self, name):
        a = self.q[name]._base.detach().cpu().numpy().copy()
        return a.transpose(*range(a.ndim)[::-1])

    def wide(self, name):
        return self.host[name].astype(np.float64)

    def unchanged(self, names, where):
        for name in names:
            assert np.array_equal(_bits(self.raw(name)), _bits(self.host[name])), (name, "changed") + tuple(where)


# ---- pace_tracer_cmax ----------------------------------------------------------------------------------------------------------
def _outside(shape, n, value, di=0, dj=0):
    """An array of `value` with zeros on the window 3 .. n + 2 (+ di, + dj) of the levels 0 .. nk - 1 (3-D) or of the plane."""
    a = np.full(shape, value)
    if len(shape) == 3:
        a[3:3 + n + di, 3:3 + n + dj, :shape[2] - 1] = 0.0
    else:
        a[3:3 + n + di, 3:3 + n + dj] = 0.0
    return a


def cmax_inputs(f, seed, outside=HUGE):
    """Random Courant numbers below 0.4 and sines in 0.7 .. 1 on the compute windows, `outside` (with both signs) elsewhere."""
    n, nk = f.n, f.nk
    rng = np.random.default_rng(seed)
    inside3 = _outside(f.s3, n, 1.0) == 0.0
    inside2 = _outside(f.s2, n, 1.0) == 0.0
    sign = np.where(rng.random(f.s3) < 0.5, -1.0, 1.0)
    cx = np.where(inside3, rng.uniform(-0.4, 0.4, f.s3), outside * sign)
    cy = np.where(inside3, rng.uniform(-0.4, 0.4, f.s3), outside * sign[::-1])
    sin_sg5 = np.where(inside2, rng.uniform(0.7, 1.0, f.s2), -outside)
    return cx, cy, sin_sg5


def run_cmax(f, exact=True, zero=True, buffer=None):
    """One launch.  exact: cmax is a buffer of exactly nk doubles; else it lies inside a larger one whose other doubles must keep
    their bits.  -> (the nk doubles, the buffer)"""
    import torch

    nk = f.nk
    if buffer is None:
        buffer = torch.zeros(nk if exact else nk + 2 * PAD, dtype=torch.float64, device=f.device)
        if not exact:
            buffer.fill_(-7.25)
    off = 0 if buffer.numel() == nk else PAD
    if zero:
        buffer[off:off + nk] = 0.0
    f.lib.call("pace_tracer_cmax", C.byref(f.geom), f.q["cx"].ptr, f.q["cy"].ptr, f.q["sin_sg5"].ptr,
               C.c_void_p(buffer.data_ptr() + 8 * off), _stream(f.device))
    _sync(f.device)
    got = buffer.cpu().numpy().copy()
    if off:
        assert (got[:PAD] == -7.25).all() and (got[off + nk:] == -7.25).all(), ("written outside cmax", f.n, f.nk)
    return got[off:off + nk], buffer


def want_cmax(f):
    return ref.cmax(f.wide("cx"), f.wide("cy"), f.wide("sin_sg5"), f.n, f.nk)


def check_cmax(device, only=None):
    for which, lib in enumerate(_libs(device)):
        if only is not None and only != which:
            continue
        for seed, (n, nk) in enumerate(SHAPES):
            f = Fields(lib, device, n, nk)
            where = (n, nk, lib.real_bytes)
            base = cmax_inputs(f, 300 + seed)
            lo, hi, mid = 3, n + 2, 3 + n // 2
            # (name, field the maximum is planted in, cell, sign)
            plants = [("corner-sw", "cx", (lo, lo), 1), ("corner-se", "cy", (hi, lo), 1), ("corner-nw", "cx", (lo, hi), 1),
                      ("corner-ne", "cy", (hi, hi), 1), ("last-row", "cx", (mid, hi), 1), ("last-column", "cy", (hi, mid), 1),
                      ("cx-only", "cx", (mid, mid), 1), ("cy-only", "cy", (mid - 1, mid + 1), 1), ("negative", "cx", (mid + 1, lo + 1), -1)]
            for number, (name, field, (i, j), sign) in enumerate(plants):
                arrays = dict(zip(("cx", "cy", "sin_sg5"), (a.copy() for a in base)))
                for k in range(nk):
                    arrays[field][i, j, k] = sign * (0.9 + 0.01 * k)
                for key, a in arrays.items():
                    f.put(key, a)
                want = want_cmax(f)
                # the case is what it says: the maximum of every level is the planted cell's
                cells = ref.cell_values(f.wide("cx"), f.wide("cy"), f.wide("sin_sg5"), n, nk)
                assert np.array_equal(cells[i - 3, j - 3, :], want) and np.isfinite(want).all() and (want < 2.0).all(), (name,) + where
                assert (np.abs(f.wide(field)[i, j, :nk]) == np.abs(f.wide("cx" if field == "cy" else "cy")[i, j, :nk])).sum() == 0
                got, _ = run_cmax(f, exact=number % 2 == 0)
                assert np.array_equal(_bits(got), _bits(want)), (name,) + where + (got, want)
                f.unchanged(("cx", "cy", "sin_sg5"), (name,) + where)
            # the level split: the plain levels hold m itself, the others m + 1 - sin
            m = np.maximum(np.abs(f.wide("cx")), np.abs(f.wide("cy")))[3:3 + n, 3:3 + n, :nk]
            plain = max(0, nk // 6 - 1)
            assert np.array_equal(got[:plain], m.max(axis=(0, 1))[:plain]) and (got[plain:] != m.max(axis=(0, 1))[plain:]).all(), where
            assert plain == (2 if nk == 19 else 0)
            # ---- a second run: the same bits
            again, _ = run_cmax(f)
            assert np.array_equal(_bits(again), _bits(got)), where
            # ---- NaNs everywhere outside the windows: no effect
            nan_base = cmax_inputs(f, 300 + seed, outside=np.nan)
            for key, a in zip(("cx", "cy", "sin_sg5"), nan_base):
                f.put(key, a)
            want = want_cmax(f)
            assert np.isfinite(want).all()
            got, _ = run_cmax(f, exact=False)
            assert np.array_equal(_bits(got), _bits(want)), ("nan outside",) + where
            # ---- a NaN inside arrives, on its level only (a plane's: on every level that reads the plane)
            for field, cell in (("cx", (hi, mid, nk - 1)), ("cy", (lo, hi, 0)), ("sin_sg5", (mid, lo))):
                a = {"cx": base[0], "cy": base[1], "sin_sg5": base[2]}[field].copy()
                a[cell] = np.nan
                f.put(field, a)
                want = want_cmax(f)
                hit = np.isnan(want)
                if field == "sin_sg5":
                    assert np.array_equal(hit, np.arange(nk) >= plain)
                else:
                    assert np.array_equal(hit, np.arange(nk) == cell[2])
                got, _ = run_cmax(f)
                assert same(got, want), ("nan inside", field) + where + (got, want)
                f.put(field, {"cx": base[0], "cy": base[1], "sin_sg5": base[2]}[field])


def check_order(device, only=None):
    """Six tiles' launches into one buffer, in two orders, and their tables through pace_tracer_subcycles in two orders."""
    import torch

    for which, lib in enumerate(_libs(device)):
        if only is not None and only != which:
            continue
        n, nk = 13, 7
        tiles, tables = [], []
        for t in range(6):
            f = Fields(lib, device, n, nk)
            cx, cy, sin_sg5 = cmax_inputs(f, 400 + t)
            cx[3 + t, 3 + 2 * t, t] = 1.3 + 0.2 * t  # level t's maximum over the six is tile t's
            for key, a in zip(("cx", "cy", "sin_sg5"), (cx, cy, sin_sg5)):
                f.put(key, a)
            tiles.append(f)
            table, _ = run_cmax(f)
            assert np.array_equal(_bits(table), _bits(want_cmax(f)))
            tables.append(table)
        want = np.maximum.reduce(tables)
        assert [int(np.argmax([tb[k] for tb in tables])) for k in range(6)] == list(range(6))
        for order in (range(6), (4, 1, 5, 0, 3, 2)):
            buffer = torch.zeros(nk, dtype=torch.float64, device=device)
            for t in order:
                got, buffer = run_cmax(tiles[t], zero=False, buffer=buffer)
            assert np.array_equal(_bits(got), _bits(want)), (tuple(order), got, want)
        expected = ref.subcycles(tables, 16)
        assert expected[1] == 0 and set(expected[2:]) == {1, 2, 3}, expected
        for order in (range(6), (4, 1, 5, 0, 3, 2)):
            got = run_subcycles(lib, device, [tables[t] for t in order], 16)
            assert np.array_equal(got, expected), (tuple(order), got, expected)


# ---- pace_tracer_subcycles -----------------------------------------------------------------------------------------------------
def run_subcycles(lib, device, tables, max_subcycles, exact=True):
    import torch

    nk = len(tables[0])
    buffers = [torch.as_tensor(np.ascontiguousarray(t, dtype=np.float64), device=device) for t in tables]
    out = torch.full((nk + 2 + (0 if exact else 2 * PAD),), -77, dtype=torch.int32, device=device)
    off = 0 if exact else PAD
    table = (C.c_void_p * len(buffers))(*[b.data_ptr() for b in buffers])
    lib.call("pace_tracer_subcycles", table, len(buffers), nk, max_subcycles, C.c_void_p(out.data_ptr() + 4 * off), _stream(device))
    _sync(device)
    got = out.cpu().numpy().copy()
    if off:
        assert (got[:PAD] == -77).all() and (got[off + nk + 2:] == -77).all(), "written outside out"
    for b, t in zip(buffers, tables):
        assert same(b.cpu().numpy(), np.asarray(t, dtype=np.float64))  # the launch only reads the tables
    return got[off:off + nk + 2]


def check_subcycles(device, only=None):
    for which, lib in enumerate(_libs(device)):
        if only is not None and only != which:
            continue
        below_one = np.nextafter(1.0, 0.0)
        assert 1.0 + below_one == 2.0  # the sum rounds: the count is 2
        values = [0.0, 0.999, below_one, 1.0, 2.5, 15.0, 15.5, 16.0, np.nan, np.inf, 0.3]
        literal = [1, 1, 2, 2, 3, 16, 16, 0, 0, 0, 1]
        for exact in (True, False):
            got = run_subcycles(lib, device, [values], 16, exact=exact)
            assert list(got) == [16, 3] + literal, got
            assert np.array_equal(got, ref.subcycles([values], 16))
        got = run_subcycles(lib, device, [values], 3)
        assert list(got) == [3, 5, 1, 1, 2, 2, 3, 0, 0, 0, 0, 0, 1] and np.array_equal(got, ref.subcycles([values], 3)), got
        got = run_subcycles(lib, device, [[0.0]], 1)
        assert list(got) == [1, 0, 1]
        got = run_subcycles(lib, device, [[1.0]], 1)
        assert list(got) == [0, 1, 0]
        # ---- six tables, 70 levels (past one wave of levels), each level's maximum on a different tile
        nk = 70
        rng = np.random.default_rng(77)
        tables = [rng.uniform(0.0, 0.5, nk) for _ in range(6)]
        peak = rng.uniform(0.6, 3.4, nk)
        for k in range(nk):
            tables[(k * 5 + 1) % 6][k] = peak[k]
        tables[2][11], tables[5][40], tables[0][69] = np.nan, np.inf, 15.99  # (NaN and infinity beside smaller values)
        want = ref.subcycles(tables, 16)
        assert want[1] == 2 and want[0] == 16 and want[2 + 11] == 0 and want[2 + 40] == 0 and set(want[2:]) >= {1, 2, 3, 4, 16}
        for order in (range(6), (3, 0, 5, 2, 1, 4)):
            got = run_subcycles(lib, device, [tables[t] for t in order], 16, exact=False)
            assert np.array_equal(got, want), (tuple(order), got, want)
        got = run_subcycles(lib, device, tables[:1], 16)
        assert np.array_equal(got, ref.subcycles(tables[:1], 16))


# ---- the divide kernel and the three _levels stencils ----------------------------------------------------------------------------
def ksplt_patterns(nk):
    mixed = ([1, 3, 1, 2, 2, 1, 3, 3, 1, 2] * ((nk + 9) // 10))[:nk]
    return {"ones": [1] * nk, "threes": [3] * nk, "mixed": mixed}


def check_levels(device, only=None):
    import torch

    import opchain
    from helpers import oracle_grid
    from oracle import tracer
    from pace_amd import synthetic
    from pace_amd.tile import Env

    for which, lib in enumerate(_libs(device)):
        if only is not None and only != which:
            continue
        f32 = lib.real_bytes == 4
        for seed, (n, nk) in enumerate(SHAPES):
            metrics = synthetic.tile_metrics(n, nk)
            if f32:
                metrics = opchain.f32_dict(metrics)
            g = oracle_grid(metrics, n, nk)
            env = Env(lib, device, metrics, n, nk)
            met = env.grid_data.c_struct()
            f = Fields(lib, device, n, nk)
            rng = np.random.default_rng(500 + seed)
            area, dp = float(np.asarray(metrics["area"])[3:3 + n, 3:3 + n].mean()), 1000.0
            st = _stream(device)

            def fill(name, lo, hi):
                f.put(name, rng.uniform(lo, hi, f.s3))

            def logical(name):
                """What the oracle sees of a storage: [i, j, k] without the row padding."""
                return f.wide(name)[:n + 7]

            def expect(name, new, levels, window):
                """The raw storage after a launch wrote `new` (float64, the oracle's) on `window` of the levels `levels`."""
                a = f.host[name].copy()
                for k in levels:
                    a[window + (k,)] = new[window + (k,)].astype(f.np_real)
                return a

            compute = (slice(3, 3 + n), slice(3, 3 + n))
            for pattern, ksplt in ksplt_patterns(nk).items():
                where = (n, nk, lib.real_bytes, pattern)
                kdev = torch.as_tensor(np.array(ksplt, dtype=np.int32), device=device)
                kptr = C.c_void_p(kdev.data_ptr())
                # ---- divide: the whole storage plane (n + 7 points a row; not the row padding) of the levels with ksplt > 1
                names = ("cxd", "xfx", "mfxd", "cyd", "yfx", "mfyd")
                for name in names:
                    fill(name, -0.6 * area, 0.6 * area)
                want = {}
                for name in names:
                    a = f.host[name].copy()
                    for k in range(nk):
                        if ksplt[k] > 1:
                            plane = [logical(name)[:, :, k:k + 1].copy()]
                            tracer.divide_fluxes(plane, ksplt[k], 1)
                            a[:n + 7, :, k] = plane[0][:, :, 0].astype(f.np_real)
                    want[name] = a
                lib.call("pace_tracer_divide_fluxes_levels", C.byref(f.geom), *[f.q[name].ptr for name in names], kptr, st)
                _sync(device)
                for name in names:
                    assert np.array_equal(_bits(f.raw(name)), _bits(want[name])), ("divide", name) + where
                if pattern == "ones":
                    f.unchanged(names, ("divide",) + where)
                for min_subcycles in (1, 2, 3):
                    levels = [k for k in range(nk) if ksplt[k] >= min_subcycles]
                    tag = where + (min_subcycles,)
                    # ---- apply_mass_flux
                    fill("dp1", 0.8 * dp, 1.2 * dp)
                    fill("dp2", 0.8 * dp, 1.2 * dp)
                    fill("mfx", -0.1 * area * dp, 0.1 * area * dp)
                    fill("mfy", -0.1 * area * dp, 0.1 * area * dp)
                    new = logical("dp2").copy()
                    tracer.apply_mass_flux(g, logical("dp1"), logical("mfx"), logical("mfy"), new, nk)
                    full = f.wide("dp2")
                    full[:n + 7] = new
                    want_dp2 = expect("dp2", full, levels, compute)
                    lib.call("pace_apply_mass_flux_levels", C.byref(f.geom), C.byref(met), f.q["dp1"].ptr, f.q["mfx"].ptr,
                             f.q["mfy"].ptr, f.q["dp2"].ptr, kptr, min_subcycles, st)
                    _sync(device)
                    assert np.array_equal(_bits(f.raw("dp2")), _bits(want_dp2)), ("apply_mass_flux",) + tag
                    f.unchanged(("dp1", "mfx", "mfy"), ("apply_mass_flux",) + tag)
                    # ---- apply_tracer_flux
                    fill("q", 1.0e-4, 1.0e-2)
                    fill("fx", -1.0e-3 * area * dp, 1.0e-3 * area * dp)
                    fill("fy", -1.0e-3 * area * dp, 1.0e-3 * area * dp)
                    f.put("dp2", f.host["dp2"])  # (the random one again: every level positive)
                    new = logical("q").copy()
                    tracer.apply_tracer_flux(g, new, logical("dp1"), logical("fx"), logical("fy"), logical("dp2"), nk)
                    full = f.wide("q")
                    full[:n + 7] = new
                    want_q = expect("q", full, levels, compute)
                    lib.call("pace_apply_tracer_flux_levels", C.byref(f.geom), C.byref(met), f.q["q"].ptr, f.q["dp1"].ptr,
                             f.q["fx"].ptr, f.q["fy"].ptr, f.q["dp2"].ptr, kptr, min_subcycles, st)
                    _sync(device)
                    assert np.array_equal(_bits(f.raw("q")), _bits(want_q)), ("apply_tracer_flux",) + tag
                    f.unchanged(("dp1", "fx", "fy", "dp2"), ("apply_tracer_flux",) + tag)
                    # ---- swap_dp
                    want_1 = expect("dp1", f.wide("dp2"), levels, compute)
                    want_2 = expect("dp2", f.wide("dp1"), levels, compute)
                    lib.call("pace_swap_dp_levels", C.byref(f.geom), f.q["dp1"].ptr, f.q["dp2"].ptr, kptr, min_subcycles, st)
                    _sync(device)
                    assert np.array_equal(_bits(f.raw("dp1")), _bits(want_1)), ("swap_dp dp1",) + tag
                    assert np.array_equal(_bits(f.raw("dp2")), _bits(want_2)), ("swap_dp dp2",) + tag
                    if levels:
                        assert not np.array_equal(_bits(want_1), _bits(f.host["dp1"]))
                    else:
                        assert pattern != "threes" and np.array_equal(_bits(want_1), _bits(f.host["dp1"]))
                assert kdev.cpu().tolist() == ksplt


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def check_refusals(device):
    import torch

    from pace_amd import _lib
    from pace_amd import synthetic
    from pace_amd.tile import Env

    lib = _libs(device)[0]
    n, nk = 12, 5
    f = Fields(lib, device, n, nk)
    env = Env(lib, device, synthetic.tile_metrics(n, nk), n, nk)
    met = C.byref(env.grid_data.c_struct())
    rng = np.random.default_rng(9)
    names = ("cx", "cy", "a", "b", "c", "d", "e")
    for name in names:
        f.put(name, rng.uniform(-0.4, 0.4, f.s3))
    f.put("sin_sg5", rng.uniform(0.7, 1.0, f.s2))
    st = _stream(device)
    geom = C.byref(f.geom)
    cmax = torch.full((nk,), 5.5, dtype=torch.float64, device=device)
    out = torch.full((nk + 2,), -3, dtype=torch.int32, device=device)
    ksplt = torch.full((nk,), 3, dtype=torch.int32, device=device)
    P = {name: f.q[name].ptr for name in f.q}
    cm, kp, op = C.c_void_p(cmax.data_ptr()), C.c_void_p(ksplt.data_ptr()), C.c_void_p(out.data_ptr())
    invalid = pytest.raises(_lib.PaceError, match="invalid argument")

    def refused(name, good, bad_args):
        for position, value in bad_args:
            args = list(good)
            args[position] = value
            with invalid:
                lib.call(name, *args, st)

    # ---- pace_tracer_cmax
    good = [geom, P["cx"], P["cy"], P["sin_sg5"], cm]
    refused("pace_tracer_cmax", good, [(p, None) for p in range(5)] + [(4, C.c_void_p(P[x])) for x in ("cx", "cy", "sin_sg5")] +
            [(0, C.byref(_lib.Geom(0, nk, f.geom.sj, 0, f.geom.sk)))])
    # ---- pace_tracer_subcycles
    table = (C.c_void_p * 1)(cmax.data_ptr())
    none = (C.c_void_p * 1)(None)
    alias = (C.c_void_p * 1)(out.data_ptr())
    many = (C.c_void_p * (_lib.TRACER_MAX_TILES + 1))(*[cmax.data_ptr()] * (_lib.TRACER_MAX_TILES + 1))
    good = [table, 1, nk, 16, op]
    refused("pace_tracer_subcycles", good, [(0, None), (0, none), (0, alias), (4, None), (1, 0), (1, -1), (2, 0), (2, -1),
                                            (2, _lib.TRACER_MAX_LEVELS + 1), (3, 0), (3, -1), (3, _lib.TRACER_MAX_SUBCYCLES + 1)])
    with invalid:
        lib.call("pace_tracer_subcycles", many, _lib.TRACER_MAX_TILES + 1, nk, 16, op, st)
    # ---- pace_tracer_divide_fluxes_levels
    good = [geom] + [P[x] for x in ("cx", "a", "b", "cy", "c", "d")] + [kp]
    refused("pace_tracer_divide_fluxes_levels", good, [(p, None) for p in range(8)] + [(7, C.c_void_p(P["a"]))])
    # ---- the three stencils
    good = [geom, met, P["a"], P["b"], P["c"], P["d"], kp, 1]
    refused("pace_apply_mass_flux_levels", good, [(p, None) for p in range(7)] + [(7, 0), (7, -2)] +
            [(5, P[x]) for x in ("a", "b", "c")] + [(6, C.c_void_p(P["d"]))])
    good = [geom, met, P["a"], P["b"], P["c"], P["d"], P["e"], kp, 1]
    refused("pace_apply_tracer_flux_levels", good, [(p, None) for p in range(8)] + [(8, 0), (8, -2)] +
            [(2, P[x]) for x in ("b", "c", "d", "e")] + [(7, C.c_void_p(P["a"]))])
    good = [geom, P["a"], P["b"], kp, 1]
    refused("pace_swap_dp_levels", good, [(p, None) for p in range(4)] + [(4, 0), (4, -2), (2, P["a"]), (3, C.c_void_p(P["a"])),
                                                                           (3, C.c_void_p(P["b"]))])
    # refused before any launch: nothing is written
    _sync(device)
    f.unchanged(names + ("sin_sg5",), ("refusals",))
    assert (cmax.cpu().numpy() == 5.5).all() and (out.cpu().numpy() == -3).all() and (ksplt.cpu().numpy() == 3).all()


# ---- the CPU tier ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_cmax_against_numpy_emulated(library):
    check_cmax("cpu", library)


@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_order_independence_emulated(library):
    check_order("cpu", library)


@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_subcycles_emulated(library):
    check_subcycles("cpu", library)


@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_levels_stencils_emulated(library):
    check_levels("cpu", library)


def test_refusals_emulated():
    check_refusals("cpu")


def test_header_and_binding_agree_on_the_entry_points():
    from pace_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pace_hip.h")).read(), flags=re.S)
    for name, count in (("pace_tracer_cmax", 6), ("pace_tracer_subcycles", 6), ("pace_tracer_divide_fluxes_levels", 9),
                        ("pace_apply_mass_flux_levels", 9), ("pace_apply_tracer_flux_levels", 10), ("pace_swap_dp_levels", 6)):
        assert name in _lib.EXPORTED_SYMBOLS
        proto = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", text).group(1)
        assert len(proto.split(",")) == len(_lib._PROTOS[name][1]) == count, name
    for macro, value in (("TILES", _lib.TRACER_MAX_TILES), ("LEVELS", _lib.TRACER_MAX_LEVELS), ("SUBCYCLES", _lib.TRACER_MAX_SUBCYCLES)):
        assert int(re.search(r"#define PACE_TRACER_MAX_" + macro + r" (\d+)", text).group(1)) == value


# ---- the GPU tier ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_cmax_against_numpy_on_the_gpu(library):
    check_cmax("cuda", library)


@pytest.mark.gpu
@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_order_independence_on_the_gpu(library):
    check_order("cuda", library)


@pytest.mark.gpu
@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_subcycles_on_the_gpu(library):
    check_subcycles("cuda", library)


@pytest.mark.gpu
@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_levels_stencils_on_the_gpu(library):
    check_levels("cuda", library)


@pytest.mark.gpu
def test_refusals_on_the_gpu():
    check_refusals("cuda")
