"""pace_diag_pack (pace_amd/csrc/k_diag.hip), pace_amd.driver.MonitorDiagnostics / NpzMonitor and the Driver's diagnostics against
a numpy restatement written here: the window slice cast to the output type, and the column integral as an explicit ascending-k
loop in float64 times RGRAV.  Kernel results are compared bit for bit.

The launch shape decides the sizes: a workgroup takes a tile of 64 points in i by 32 in the output's fastest axis -- k for a 3-D
item (TK = 32), j for a plane; 64 by 4 for a column integral -- and finds its item in a prefix table of per-item tile counts:

    C12 x 7    windows narrower than one wave (12 of 64 lanes), fewer levels than a tile
    C13 x 5    odd extents; dims (x_interface, y, z), (x, y_interface, z), (x, y, z_interface): extents 14 and 6; a 2-D field;
               a column integral's last tile holds one row
    C12 x 32   nk = TK; the z_interface field has TK + 1
    C68 x 33   a second i tile 4 wide; 33 levels = TK + 1
    C96 x 79   the model's level count (tiles of 32, 32, 15); 33 items of mixed kinds: a second launch, and items whose
               workgroups lie anywhere in the prefix table (the emulation runs a fiber per thread, so its tier has this
               shape as the 33-item case and pt_z65 only; the GPU tier runs everything at every shape)
"""
import ctypes as C
import datetime
import json
import os
import re
import sys
import types
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import GOLDEN, ROOT, build_emu, build_emu_f32  # noqa: E402

SHAPES = ((12, 7), (13, 5), (12, 32), (68, 33), (96, 79))
TK = 32
RGRAV = 1.0 / 9.80665
SENTINEL = -12345.0
WINDOW3D, PLANE, COLUMN = 0, 1, 2
XYZ, XIYZ, XYIZ, XYZI, XY = (("x", "y", "z"), ("x_interface", "y", "z"), ("x", "y_interface", "z"), ("x", "y", "z_interface"),
                             ("x", "y"))
YAML = os.path.join(GOLDEN, "driver_baroclinic_c12.yaml")


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


# ---- fields ------------------------------------------------------------------------------------------------------------------
class Fields:
    """Quantities of a C<n> x <nk> tile for `lib` on `device`.  A field holds distinct values inside `window` (default: its
    compute domain) and NaN / 1e300-sized garbage everywhere else: the halo, the levels outside the window, the row padding."""

    def __init__(self, lib, device, n, nk):
        import torch

        from pace_amd import _lib
        from pace_amd.util import QuantityFactory, SubtileGridSizer

        self.lib, self.device, self.n, self.nk = lib, device, n, nk
        self.dtype = np.float32 if lib.real_bytes == 4 else np.float64
        self.huge = 3.0e38 if self.dtype == np.float32 else 1.0e300
        sizer = SubtileGridSizer.from_tile_params(nx_tile=n, ny_tile=n, nz=nk, n_halo=3, extra_dim_lengths={}, layout=(1, 1))
        self.qf = QuantityFactory(sizer, device=device, dtype=torch.float32 if lib.real_bytes == 4 else torch.float64)
        self.geom = _lib.Geom(n, nk, self.qf.row_stride, 0, self.qf.level_stride)
        self.rng = np.random.default_rng(1000 * n + nk)

    def garbage(self, shape):
        a = np.full(shape, np.nan, dtype=self.dtype)
        flat = a.reshape(-1)
        flat[::3] = self.huge
        flat[1::5] = -self.huge
        return a

    def quantity(self, dims, values=None, window=None, units="u"):
        """(Quantity, the numpy array of its logical storage).  values: a function of the window's shape."""
        q = self.qf.zeros(list(dims), units)
        q._base[...] = float("nan")  # (the row padding included)
        q._base[..., ::2] = self.huge
        a = self.garbage(q.shape)
        if window is None:
            window = tuple(slice(o, o + e) for o, e in zip(q.origin, q.extent))
        shape = a[window].shape
        a[window] = (values(shape) if values is not None else self.rng.uniform(-50.0, 50.0, shape)).astype(self.dtype)
        q.set(a)
        return q, a

    def special(self, a, window):
        """A few values beyond float32's range and a few exactly halfway between two float32 values (float64 storage only)."""
        if self.dtype != np.float64:
            return
        w = a[window]
        vals = [1.0e39, -1.0e300, 3.5e38,
                float(np.float32(1.5)) + 2.0 ** -24,                                   # a tie, even below: rounds down
                float(np.nextafter(np.float32(1.5), np.float32(2.0))) + 2.0 ** -24,    # a tie, even above: rounds up
                -(float(np.float32(1024.0)) + 2.0 ** -14), float(np.finfo(np.float32).max) + 2.0 ** 103]  # the last tie is +inf
        idx = np.linspace(0, w.size - 1, len(vals)).astype(int)
        pos = np.unravel_index(idx, w.shape)
        w[pos] = vals


def window_of(q):
    return tuple(q.origin) + (0,) * (3 - len(q.origin)) + tuple(q.extent) + (1,) * (3 - len(q.extent))


# ---- the numpy restatement -----------------------------------------------------------------------------------------------------
def np_item(kind, a, w, win, out_dtype, level=0):
    i0, j0, k0, ni, nj, nk = win
    with np.errstate(over="ignore"):  # (values beyond float32's range become +-inf: that is asked for)
        if kind == WINDOW3D:
            return np.ascontiguousarray(a[i0:i0 + ni, j0:j0 + nj, k0:k0 + nk]).astype(out_dtype)
        if kind == PLANE:
            plane = a[:, :, level] if a.ndim == 3 else a
            return np.ascontiguousarray(plane[i0:i0 + ni, j0:j0 + nj]).astype(out_dtype)
        acc = np.zeros((ni, nj), dtype=np.float64)
        for k in range(k0, k0 + nk):
            acc = acc + a[i0:i0 + ni, j0:j0 + nj, k].astype(np.float64) * w[i0:i0 + ni, j0:j0 + nj, k].astype(np.float64)
        return (RGRAV * acc).astype(out_dtype)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def run_items(f, specs, out_is_double, gap=5, tail=77):
    """specs: (kind, (Quantity, array), (weight Quantity, array) or None, window, level).  Packs them with gaps between the items
    and a tail in a sentinel-filled buffer, PACE_DIAG_MAX_ITEMS per call, and compares the WHOLE buffer with the restatement."""
    import torch

    from pace_amd import _lib

    out_dtype = np.float64 if out_is_double else np.float32
    offsets, total = [], 3
    for kind, _, _, win, _ in specs:
        offsets.append(total)
        total += int(np.prod(win[3:] if kind == WINDOW3D else win[3:5])) + gap
    total += tail
    out = torch.full((total,), SENTINEL, dtype=torch.float64 if out_is_double else torch.float32, device=f.device)
    want = np.full(total, SENTINEL, dtype=out_dtype)
    stream = None if f.device == "cpu" else C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for first in range(0, len(specs), _lib.DIAG_MAX_ITEMS):
        chunk = specs[first:first + _lib.DIAG_MAX_ITEMS]
        items = (_lib.DiagItem * len(chunk))()
        for item, (kind, (q, a), weight, win, level), offset in zip(items, chunk, offsets[first:]):
            item.field = q.ptr + level * f.geom.sk * f.lib.real_bytes
            item.weight = weight[0].ptr if weight is not None else None
            item.kind = kind
            item.i0, item.j0, item.k0, item.ni, item.nj, item.nk = win
            item.out_offset = offset
            expect = np_item(kind, a, weight[1] if weight is not None else None, win, out_dtype, level)
            want[offset:offset + expect.size] = expect.reshape(-1)
        f.lib.call("pace_diag_pack", C.byref(f.geom), items, len(chunk), int(out_is_double), C.c_void_p(out.data_ptr()), stream)
    got = out.cpu().numpy()
    same = bits(got) == bits(want)
    assert same.all(), (f.n, f.nk, out_dtype, int((~same).sum()), np.flatnonzero(~same)[:8], got[~same][:4], want[~same][:4])


def standard_specs(f):
    """One item of every kind and dims for the shape; planes at level 0, nk - 1 and an interior one (65 of 79 levels)."""
    n, nk = f.n, f.nk
    specs = []
    fields = {}
    for dims in (XYZ, XIYZ, XYIZ, XYZI):
        q, a = f.quantity(dims)
        if dims == XYZ:
            cw = tuple(slice(o, o + e) for o, e in zip(q.origin, q.extent))
            f.special(a, cw)
            q.set(a)
        fields[dims] = (q, a)
        specs.append((WINDOW3D, (q, a), None, window_of(q), 0))
    q2 = f.quantity(XY)
    specs.append((PLANE, q2, None, window_of(q2[0]), 0))
    interior = 65 if nk == 79 else nk // 2
    for level in (0, nk - 1, interior):
        # the level's plane holds values, every other level garbage
        q, a = f.quantity(XYZ, window=(slice(3, 3 + n), slice(3, 3 + n), slice(level, level + 1)))
        specs.append((PLANE, (q, a), None, (3, 3, 0, n, n, 1), level))
    # column integrals: a tracer with both signs, and a positive one, with a positive weight; levels outside 0 .. nk - 1 are garbage
    delp = f.quantity(XYZ, values=lambda s: f.rng.uniform(50.0, 1500.0, s))
    specs.append((COLUMN, f.quantity(XYZ, values=lambda s: f.rng.uniform(-1e-2, 2e-2, s)), delp, (3, 3, 0, n, n, nk), 0))
    specs.append((COLUMN, f.quantity(XYZ, values=lambda s: f.rng.uniform(1e-6, 2e-2, s)), delp, (3, 3, 0, n, n, nk), 0))
    if nk > 2:  # a window of levels inside the column, and a 3-D window that is no compute domain
        lo, hi = 1, nk - 1
        w = (slice(3, 3 + n), slice(3, 3 + n), slice(lo, hi))
        dw = f.quantity(XYZ, values=lambda s: f.rng.uniform(50.0, 1500.0, s), window=w)
        specs.append((COLUMN, f.quantity(XYZ, window=w), dw, (3, 3, lo, n, n, hi - lo), 0))
        w = (slice(1, n + 6), slice(2, 5), slice(lo, hi))
        specs.append((WINDOW3D, f.quantity(XYZ, window=w), None, (1, 2, lo, n + 5, 3, hi - lo), 0))
    return specs


def many_specs(f, count=33):
    """`count` items of mixed kinds over a handful of fields: 5 3-D windows (the emulation runs a fiber per thread: they are what
    takes time), the rest planes and column integrals."""
    n, nk = f.n, f.nk
    vols = [f.quantity(dims) for dims in (XYZ, XIYZ, XYIZ, XYZI)]
    f.special(vols[0][1], (slice(3, 3 + n), slice(3, 3 + n), slice(0, nk)))
    vols[0][0].set(vols[0][1])
    full = f.quantity(XYZI, window=(slice(0, n + 7), slice(0, n + 7), slice(0, nk + 1)))  # values everywhere: any window is legal
    delp = f.quantity(XYZ, values=lambda s: f.rng.uniform(50.0, 1500.0, s))
    tracer = f.quantity(XYZ, values=lambda s: f.rng.uniform(-1e-2, 2e-2, s))
    plane = f.quantity(XY)
    specs = []
    for m in range(count):
        if m % 4 == 0 and m < 20:
            q = vols[(m // 4) % 4] if m < 16 else full
            win = window_of(q[0]) if m < 16 else (m % 7, m % 5, m % 3, n + 7 - m % 7 - m % 11, n - m % 9, nk + 1 - m % 3 - m % 2)
            specs.append((WINDOW3D, q, None, win, 0))
        elif m % 4 == 1:
            specs.append((COLUMN, tracer, delp, (3, 3, 0, n, n, nk), 0))
        elif m % 4 == 2:
            specs.append((PLANE, full, None, (m % 5, m % 3, 0, n + 7 - m % 5, n + 7 - m % 3 - m % 4, 1), (m * 7) % (nk + 1)))
        else:
            specs.append((PLANE, plane, None, window_of(plane[0]), 0))
    return specs


def check_shape(lib, device, n, nk, out_is_double):
    f = Fields(lib, device, n, nk)
    run_items(f, standard_specs(f), out_is_double)


def check_many(lib, device, n, nk, out_is_double):
    f = Fields(lib, device, n, nk)
    specs = many_specs(f)
    assert len(specs) == 33
    run_items(f, specs, out_is_double)


# ---- the kernel, emulated ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nk", SHAPES[:4])
def test_pack_emulated(emu_lib, emu_lib_f32, n, nk):
    for out_is_double in (False, True):
        check_shape(emu_lib, "cpu", n, nk, out_is_double)
        check_shape(emu_lib_f32, "cpu", n, nk, out_is_double)


def test_pack_thirty_three_items_emulated(emu_lib, emu_lib_f32):
    check_many(emu_lib, "cpu", 96, 79, False)
    check_many(emu_lib_f32, "cpu", 96, 79, True)


def test_pt_z65_emulated(emu_lib):
    """The example file's level selection, at the model's level count: pt at level 65 of 79."""
    f = Fields(emu_lib, "cpu", 12, 79)
    specs = [s for s in standard_specs(f) if s[0] == PLANE and s[4] == 65]
    assert len(specs) == 1
    run_items(f, specs, False)


# ---- the column integral against the reference's expression ---------------------------------------------------------------------
def ulps_apart(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def check_column_integral(lib, device, n=24, nk=79):
    """The reference (diagnostics.py:228-253) takes RGRAV * np.sum(q * delp, axis=2) on (x, y, z) C-ordered data, numpy's pairwise
    order, and the monitor narrows it to float32.  Any order of at most 128 positive terms differs by at most 127 * 2^-53 =
    1.4e-14 relative in float64, so only a value that close to a float32 rounding boundary can land on the neighbour: the float32
    results agree to one ulp, and at least 99 % of the columns bit for bit.  The two numpy orders are held to that first."""
    f = Fields(lib, device, n, nk)
    q = f.quantity(XYZ, values=lambda s: f.rng.uniform(1e-6, 2e-2, s))
    delp = f.quantity(XYZ, values=lambda s: f.rng.uniform(50.0, 1500.0, s))
    cw = (slice(3, 3 + n), slice(3, 3 + n), slice(0, nk))
    qc = np.ascontiguousarray(q[1][cw]).astype(np.float64)
    dc = np.ascontiguousarray(delp[1][cw]).astype(np.float64)
    reference = (RGRAV * np.sum(qc * dc, axis=2)).astype(np.float32)
    loop = np_item(COLUMN, q[1], delp[1], (3, 3, 0, n, n, nk), np.float32)
    assert ulps_apart(reference, loop).max() <= 1 and (bits(reference) == bits(loop)).mean() >= 0.99
    import torch

    from pace_amd import _lib

    out = torch.full((n * n,), SENTINEL, dtype=torch.float32, device=device)
    item = (_lib.DiagItem * 1)()
    item[0].field, item[0].weight, item[0].kind = q[0].ptr, delp[0].ptr, COLUMN
    item[0].i0, item[0].j0, item[0].k0, item[0].ni, item[0].nj, item[0].nk = 3, 3, 0, n, n, nk
    stream = None if device == "cpu" else C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.call("pace_diag_pack", C.byref(f.geom), item, 1, 0, C.c_void_p(out.data_ptr()), stream)
    got = out.cpu().numpy().reshape(n, n)
    apart = ulps_apart(reference, got)
    equal = (bits(reference) == bits(got)).mean()
    print(f"column integral C{n} x {nk}: max {apart.max()} ulp from the reference's expression, {100 * equal:.2f} % bit-equal")
    assert apart.max() <= 1 and equal >= 0.99


def test_column_integral_against_the_reference_expression_emulated(emu_lib, emu_lib_f32):
    check_column_integral(emu_lib, "cpu")
    check_column_integral(emu_lib_f32, "cpu")


# ---- argument errors ------------------------------------------------------------------------------------------------------------
def check_argument_errors(lib, device):
    import torch

    from pace_amd import _lib

    n, nk = 12, 7
    f = Fields(lib, device, n, nk)
    q, _ = f.quantity(XYZ)
    out = torch.full((4 * (n + 7) * (n + 7) * (nk + 1),), SENTINEL, dtype=torch.float32, device=device)
    stream = None if device == "cpu" else C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(count, kind=WINDOW3D, win=(3, 3, 0, n, n, nk), weight=None, offset=0):
        items = (_lib.DiagItem * _lib.DIAG_MAX_ITEMS)()
        for item in items:
            item.field, item.weight, item.kind, item.out_offset = q.ptr, weight, kind, offset
            item.i0, item.j0, item.k0, item.ni, item.nj, item.nk = win
        lib.call("pace_diag_pack", C.byref(f.geom), items, count, 0, C.c_void_p(out.data_ptr()), stream)

    call(1)  # the table itself is fine
    call(1, win=(0, 0, 0, n + 7, n + 7, nk + 1))  # the whole storage is a window
    call(1, kind=COLUMN, weight=q.ptr)
    bad = [dict(count=0), dict(count=_lib.DIAG_MAX_ITEMS + 1), dict(count=-1),
           dict(count=1, win=(0, 0, 0, n + 8, n, nk)), dict(count=1, win=(8, 3, 0, n, n, nk)), dict(count=1, win=(3, 8, 0, n, n, nk)),
           dict(count=1, win=(3, 3, 0, n, n + 5, nk)), dict(count=1, win=(3, 3, 0, n, n, nk + 2)), dict(count=1, win=(3, 3, 2, n, n, nk)),
           dict(count=1, win=(-1, 3, 0, n, n, nk)), dict(count=1, win=(3, -1, 0, n, n, nk)), dict(count=1, win=(3, 3, -1, n, n, nk)),
           dict(count=1, win=(3, 3, 0, 0, n, nk)), dict(count=1, win=(3, 3, 0, n, 0, nk)), dict(count=1, win=(3, 3, 0, n, n, 0)),
           dict(count=1, kind=PLANE, win=(3, 3, 0, n, n, 2)), dict(count=1, kind=PLANE, win=(3, 3, 0, n, n + 5, 1)),
           dict(count=1, kind=COLUMN), dict(count=1, kind=COLUMN, win=(3, 3, 0, n, n, nk + 2), weight=q.ptr),
           dict(count=1, kind=3), dict(count=1, offset=-1)]
    for kwargs in bad:
        with pytest.raises(_lib.PaceError, match="invalid argument"):
            call(**kwargs)
    with pytest.raises(_lib.PaceError, match="invalid argument"):
        lib.call("pace_diag_pack", C.byref(f.geom), None, 1, 0, C.c_void_p(out.data_ptr()), stream)


def test_argument_errors_emulated(emu_lib):
    check_argument_errors(emu_lib, "cpu")


def test_header_and_binding_agree_on_the_entry_point():
    from pace_amd import _lib

    text = open(os.path.join(ROOT, "include", "pace_hip.h")).read()
    proto = re.search(r"\bint pace_diag_pack\s*\(([^;]*)\);", text).group(1)
    assert len(proto.split(",")) == len(_lib._PROTOS["pace_diag_pack"][1])
    assert int(re.search(r"#define PACE_DIAG_MAX_ITEMS (\d+)", text).group(1)) == _lib.DIAG_MAX_ITEMS
    kinds = re.search(r"enum \{ PACE_DIAG_WINDOW3D = (\d), PACE_DIAG_PLANE = (\d), PACE_DIAG_COLUMN_INTEGRAL = (\d) \}", text).groups()
    assert tuple(int(k) for k in kinds) == (_lib.DIAG_WINDOW3D, _lib.DIAG_PLANE, _lib.DIAG_COLUMN_INTEGRAL) == (WINDOW3D, PLANE, COLUMN)
    body = re.search(r"typedef struct \{([^}]*)\} pace_diag_item_t;", text).group(1)
    names = re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", body))
    assert names == [name for name, _ in _lib.DiagItem._fields_]
    assert C.sizeof(_lib.DiagItem) == 56


# ---- MonitorDiagnostics ---------------------------------------------------------------------------------------------------------
class RecordingMonitor:
    def __init__(self):
        self.stored, self.constants, self.cleaned = [], [], 0

    def store(self, state):
        self.stored.append({k: (v if k == "time" else (v.dims, v.units, v.view[:].numpy().copy(), v.view[:].is_contiguous()))
                            for k, v in state.items()})

    def store_constant(self, state):
        self.constants.append({k: (v.dims, v.units, v.view[:].numpy().copy()) for k, v in state.items()})

    def cleanup(self):
        self.cleaned += 1


class CountingLib:
    """A library whose entry-point calls are counted."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def call(self, name, *args):
        self.calls.append(name)
        return self._lib.call(name, *args)


def counting_diagnostics(lib, names, derived=(), z_select=()):
    from pace_amd.driver import MonitorDiagnostics

    counting = CountingLib(lib)
    diag = MonitorDiagnostics(RecordingMonitor(), list(names), list(derived), list(z_select), lib=counting)
    copies = []
    to_host = diag._to_host

    def counted(packed, host):
        copies.append(packed.numel())
        to_host(packed, host)

    diag._to_host = counted
    return diag, counting, copies


def small_state(f):
    """(state, arrays): a dycore state with fields of four dims and a 2-D one, a physics state with one field of its own."""
    made = {"pt": f.quantity(XYZ, units="degK"), "u": f.quantity(XYIZ, units="m/s"), "v": f.quantity(XIYZ, units="m/s"),
            "pe": f.quantity(XYZI, units="Pa"), "phis": f.quantity(XY, units="m^2 s^-2"),
            "delp": f.quantity(XYZ, values=lambda s: f.rng.uniform(50.0, 1500.0, s), units="Pa"),
            "qliquid": f.quantity(XYZ, values=lambda s: f.rng.uniform(-1e-3, 2e-2, s), units="kg/kg")}
    physics = {"prsi": f.quantity(XYZI, units="Pa"), "pt": f.quantity(XYZ, units="never looked at")}
    state = types.SimpleNamespace(dycore_state=types.SimpleNamespace(**{k: v[0] for k, v in made.items()}),
                                  physics_state=types.SimpleNamespace(**{k: v[0] for k, v in physics.items()}))
    arrays = {k: v[1] for k, v in made.items()}
    arrays["prsi"] = physics["prsi"][1]
    return state, arrays


def compute(a, q):
    return a[tuple(slice(o, o + e) for o, e in zip(q.origin, q.extent))]


def check_monitor_diagnostics(lib, device):
    from pace_amd.driver import ZSelect

    n, nk = 13, 5
    f = Fields(lib, device, n, nk)
    state, arrays = small_state(f)
    names = ["pt", "u", "v", "pe", "phis", "prsi"]
    diag, counting, copies = counting_diagnostics(lib, names, ["column_integrated_qliquid"], [ZSelect(level=3, names=["pt"])])
    time = datetime.datetime(2000, 1, 1, 0, 3, 45)
    diag.store(time, state)
    assert counting.calls == ["pace_diag_pack"] and len(copies) == 1
    (got,) = diag.monitor.stored
    assert list(got) == ["time"] + names + ["column_integrated_qliquid", "pt_z3"] and got["time"] == time
    for name in names:  # prsi comes from the physics state, pt from the dycore's
        q = getattr(state.physics_state if name == "prsi" else state.dycore_state, name)
        dims, units, data, contiguous = got[name]
        assert dims == q.dims and units == q.units and contiguous and data.dtype == np.float32 and data.shape == tuple(q.extent)
        assert np.array_equal(bits(data), bits(compute(arrays[name], q).astype(np.float32))), name
    dims, units, data, _ = got["column_integrated_qliquid"]
    assert dims == ("x", "y") and units == "kg/m**2"
    assert np.array_equal(bits(data), bits(np_item(COLUMN, arrays["qliquid"], arrays["delp"], (3, 3, 0, n, n, nk), np.float32)))
    dims, units, data, _ = got["pt_z3"]
    assert dims == ("x", "y") and units == "degK" and np.array_equal(data, arrays["pt"][3:3 + n, 3:3 + n, 3].astype(np.float32))
    # swap_storage replaces the storage of pt: the next store shows the new contents, with one pack and one copy again
    other, other_array = f.quantity(XYZ, units="degK")
    state.dycore_state.pt.swap_storage(other)
    diag.store(time, state)
    assert counting.calls == ["pace_diag_pack"] * 2 and len(copies) == 2
    latest = diag.monitor.stored[1]
    assert np.array_equal(bits(latest["pt"][2]), bits(other_array[3:3 + n, 3:3 + n, :nk].astype(np.float32)))
    assert np.array_equal(latest["pt_z3"][2], other_array[3:3 + n, 3:3 + n, 3].astype(np.float32))
    assert not np.array_equal(latest["pt"][2], got["pt"][2]) and np.array_equal(latest["u"][2], got["u"][2])
    # more than PACE_DIAG_MAX_ITEMS variables: two launches, still one copy
    many, counting, copies = counting_diagnostics(lib, ["pt", "u", "phis"] * 11)
    assert many.pack(many._requests(state)).keys() == {"pt", "u", "phis"}  # (same names: the dictionary keeps one of each)
    assert counting.calls == ["pace_diag_pack"] * 2 and len(copies) == 1
    # store_grid: device Quantities go through the pack in float64, host arrays are cut on the host
    lat, lat_array = f.quantity(("x_interface", "y_interface"), units="radians")
    host_lon = np.arange((n + 7.0) * (n + 7)).reshape(n + 7, n + 7) / 7.0
    grid = types.SimpleNamespace(lat=lat, lon=host_lon, lon_agrid=host_lon + 1.0, lat_agrid=f.quantity(XY, units="radians")[0])
    diag.store_grid(grid)
    constants = {k: v for entry in diag.monitor.constants for k, v in entry.items()}
    assert [list(entry) for entry in diag.monitor.constants] == [["lat"], ["lon"], ["lon_agrid"], ["lat_agrid"]]
    assert constants["lat"][0] == ("x_interface", "y_interface") and constants["lat"][2].dtype == np.float64
    assert np.array_equal(bits(constants["lat"][2]), bits(lat_array[3:4 + n, 3:4 + n].astype(np.float64)))
    assert np.array_equal(constants["lon"][2], host_lon[3:4 + n, 3:4 + n]) and constants["lon"][0] == ("x_interface", "y_interface")
    assert np.array_equal(constants["lon_agrid"][2], host_lon[3:3 + n, 3:3 + n] + 1.0) and constants["lon_agrid"][0] == ("x", "y")
    assert constants["lat_agrid"][2].shape == (n, n)
    diag.cleanup()
    assert diag.monitor.cleaned == 1


def test_monitor_diagnostics_emulated(emu_lib, emu_lib_f32):
    check_monitor_diagnostics(emu_lib, "cpu")
    check_monitor_diagnostics(emu_lib_f32, "cpu")


def test_monitor_diagnostics_refusals_emulated(emu_lib):
    from pace_amd.driver import MonitorDiagnostics, ZSelect

    f = Fields(emu_lib, "cpu", 12, 7)
    state, _ = small_state(f)
    now = datetime.datetime(2000, 1, 1)

    def diagnostics(names=(), derived=(), z_select=()):
        return MonitorDiagnostics(RecordingMonitor(), list(names), list(derived), list(z_select), lib=emu_lib)

    with pytest.raises(ValueError, match="Invalid state variable prsi for level select"):  # (the physics state is not searched)
        diagnostics(z_select=[ZSelect(level=1, names=["prsi"])]).store(now, state)
    with pytest.raises(ValueError, match="z_select only works for state variables with dimension"):  # the reference's quirk
        diagnostics(z_select=[ZSelect(level=1, names=["pe"])]).store(now, state)
    with pytest.raises(AttributeError):
        diagnostics(names=["qfog"]).store(now, state)
    with pytest.raises(NotImplementedError, match="z-dimension"):
        diagnostics(derived=["column_integrated_pe"]).store(now, state)
    diag = diagnostics(names=["pt"], derived=["total_lightning", "column_integrated_qliquid"])
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        diag.store(now, state)
    assert [str(w.message) for w in seen] == ["total_lightning is not a supported diagnostic variable."]
    assert list(diag.monitor.stored[0]) == ["time", "pt", "column_integrated_qliquid"]
    # ZSelect.select_data keeps the reference's form: 2-D Quantities over the state's own storage
    picked = ZSelect(level=2, names=["pt"]).select_data(state.dycore_state)
    assert list(picked) == ["pt_z2"] and picked["pt_z2"].dims == ("x", "y") and picked["pt_z2"].extent == (12, 12)
    assert np.array_equal(picked["pt_z2"].view[:].numpy(), state.dycore_state.pt.view[:][:, :, 2].numpy())
    # NullDiagnostics does nothing, whatever it is given
    from pace_amd.driver import NullDiagnostics

    null = NullDiagnostics()
    assert null.store(now, None) is None and null.store_grid(None) is None and null.cleanup() is None


# ---- NpzMonitor -----------------------------------------------------------------------------------------------------------------
def host_quantity(array, dims, units):
    import torch

    from pace_amd.util import Quantity

    return Quantity(torch.from_numpy(np.ascontiguousarray(array)), dims, units)


def load(path):
    with np.load(path, allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


def test_npz_monitor_chunks(tmp_path):
    from pace_amd.driver import NpzMonitor

    rng = np.random.default_rng(5)
    monitor = NpzMonitor(str(tmp_path), tile=3, time_chunk_size=2)
    start = datetime.datetime(2000, 1, 1)
    states = []
    for m in range(5):
        states.append({"pt": rng.uniform(-1, 1, (4, 3, 2)).astype(np.float32), "ps": rng.uniform(-1, 1, (4, 3)).astype(np.float32)})
        monitor.store({"time": start + m * datetime.timedelta(seconds=225), "pt": host_quantity(states[m]["pt"], XYZ, "degK"),
                       "ps": host_quantity(states[m]["ps"], XY, "Pa")})
        assert sorted(os.listdir(tmp_path)) == [f"state_{chunk:04d}_tile3.npz" for chunk in range((m + 1) // 2)]
    monitor.cleanup()
    assert sorted(os.listdir(tmp_path)) == [f"state_{chunk:04d}_tile3.npz" for chunk in range(3)]
    for chunk, members in enumerate(((0, 1), (2, 3), (4,))):
        d = load(tmp_path / f"state_{chunk:04d}_tile3.npz")
        assert sorted(d) == ["__meta__", "ps", "pt", "time"]
        assert d["time"].dtype == np.dtype("datetime64[us]")
        assert list(d["time"]) == [np.datetime64(start + m * datetime.timedelta(seconds=225), "us") for m in members]
        assert d["pt"].shape == (len(members), 1, 4, 3, 2) and d["pt"].dtype == np.float32 and d["ps"].shape == (len(members), 1, 4, 3)
        for at, m in enumerate(members):
            assert np.array_equal(d["pt"][at, 0], states[m]["pt"]) and np.array_equal(d["ps"][at, 0], states[m]["ps"])
        meta = json.loads(str(d["__meta__"]))
        assert meta["pt"] == {"dims": ["time", "tile", "x", "y", "z"], "units": "degK"}
        assert meta["ps"] == {"dims": ["time", "tile", "x", "y"], "units": "Pa"} and meta["time"]["dims"] == ["time"]
    monitor.cleanup()  # nothing left to write
    assert len(os.listdir(tmp_path)) == 3


def test_npz_monitor_keys_times_and_constants(tmp_path):
    from pace_amd.driver import NpzMonitor

    a = np.arange(6, dtype=np.float32).reshape(3, 2)
    monitor = NpzMonitor(str(tmp_path), tile=0, time_chunk_size=2)
    monitor.store({"time": datetime.timedelta(seconds=225), "ps": host_quantity(a, XY, "Pa")})
    with pytest.raises(ValueError, match="state keys must be the same each time store is called"):
        monitor.store({"time": datetime.timedelta(seconds=450), "ps": host_quantity(a, XY, "Pa"), "pt": host_quantity(a, XY, "K")})
    with pytest.raises(ValueError, match="state keys must be the same"):
        monitor.store({"time": datetime.timedelta(seconds=450)})
    # the dimensions may come in another order than in the chunk's first state: they are put back
    monitor.store({"time": datetime.timedelta(seconds=450), "ps": host_quantity(2 * a.T, ("y", "x"), "Pa")})
    d = load(tmp_path / "state_0000_tile0.npz")
    assert d["time"].dtype == np.dtype("timedelta64[us]")
    assert list(d["time"]) == [np.timedelta64(225_000_000, "us"), np.timedelta64(450_000_000, "us")]
    assert np.array_equal(d["ps"][0, 0], a) and np.array_equal(d["ps"][1, 0], 2 * a)
    # an existing file is replaced
    again = NpzMonitor(str(tmp_path), tile=0, time_chunk_size=1)
    again.store({"time": datetime.timedelta(seconds=1), "ps": host_quantity(a + 1, XY, "Pa")})
    d = load(tmp_path / "state_0000_tile0.npz")
    assert d["ps"].shape == (1, 1, 3, 2) and np.array_equal(d["ps"][0, 0], a + 1)
    lat = np.linspace(-1.0, 1.0, 12).reshape(4, 3)
    monitor.store_constant({"lat": host_quantity(lat, ("x_interface", "y_interface"), "radians")})
    d = load(tmp_path / "constants_lat_tile0.npz")
    assert sorted(d) == ["__meta__", "lat"] and d["lat"].dtype == np.float64 and np.array_equal(d["lat"][0], lat)
    assert json.loads(str(d["__meta__"]))["lat"] == {"dims": ["tile", "x_interface", "y_interface"], "units": "radians"}


# ---- the configuration ----------------------------------------------------------------------------------------------------------
def test_diagnostics_config(tmp_path):
    from pace_amd.driver import DiagnosticsConfig, MonitorDiagnostics, NpzMonitor, NullDiagnostics
    from pace_amd.util.partitioner import CubedSpherePartitioner

    with pytest.raises(ValueError, match="path must be given"):
        DiagnosticsConfig(names=["pt"])
    with pytest.raises(ValueError, match="path must be given"):
        DiagnosticsConfig(derived_names=["column_integrated_qliquid"])
    with pytest.raises(ValueError, match="output_format must be one of"):
        DiagnosticsConfig(path=str(tmp_path), output_format="grib")
    communicator = types.SimpleNamespace(rank=4, partitioner=CubedSpherePartitioner())
    target = tmp_path / "deep" / "er"
    for output_format in ("zarr", "netcdf"):
        config = DiagnosticsConfig(path=str(target), output_format=output_format, names=["pt"])
        assert isinstance(config.diagnostics_factory(communicator), NullDiagnostics) and not target.exists()
    assert isinstance(DiagnosticsConfig().diagnostics_factory(communicator), NullDiagnostics)
    config = DiagnosticsConfig.from_dict({"path": str(target), "output_format": "npz", "names": ["pt"], "time_chunk_size": 3,
                                          "z_select": [{"level": 65, "names": ["pt"]}]})
    diag = config.diagnostics_factory(communicator, lib="the library")
    assert isinstance(diag, MonitorDiagnostics) and isinstance(diag.monitor, NpzMonitor) and target.is_dir()
    assert (diag.names, diag.z_select[0].level, diag._lib, diag.monitor._tile, diag.monitor._time_chunk_size) == \
        (["pt"], 65, "the library", 4, 3)


# ---- the Driver -------------------------------------------------------------------------------------------------------------------
EXAMPLE_NAMES = ("u", "v", "ua", "va", "pt", "delp", "qvapor", "qliquid", "qice", "qrain", "qsnow", "qgraupel")


def settings(**over):
    import yaml

    with open(YAML) as f:
        d = yaml.safe_load(f)
    d.update(over)
    return d


@pytest.fixture
def clean_checks():
    from pace_amd.driver import SafetyChecker

    saved = dict(SafetyChecker.checks)
    SafetyChecker.clear_all_checks()
    yield SafetyChecker
    SafetyChecker.clear_all_checks()
    SafetyChecker.checks.update(saved)


def driver_settings(path, output_format, steps):
    base = settings()
    diagnostics = dict(base["diagnostics_config"], path=str(path), output_format=output_format, time_chunk_size=2)
    assert tuple(diagnostics["names"]) == EXAMPLE_NAMES and diagnostics["z_select"] == [{"level": 65, "names": ["pt"]}]
    return settings(dycore_only=True, diagnostics_config=diagnostics, output_initial_state=True, minutes=0, seconds=225 * steps)


def state_arrays(driver):
    out = {}
    for name in EXAMPLE_NAMES:
        q = getattr(driver.state.dycore_state, name)
        out[name] = q.view[:].cpu().numpy().astype(np.float32)
    out["pt_z65"] = driver.state.dycore_state.pt.view[:][:, :, 65].cpu().numpy().astype(np.float32)
    return out


def check_driver(lib, tmp_path, steps):
    from pace_amd.driver import Driver, DriverConfig, MonitorDiagnostics
    from pace_amd.util import NullComm

    out = tmp_path / "diagnostics"
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        driver = Driver(DriverConfig.from_dict(driver_settings(out, "npz", steps)), comm=NullComm(0, 6), lib=lib)
    assert not [w for w in seen if "no diagnostics are written" in str(w.message)]
    assert isinstance(driver.diagnostics, MonitorDiagnostics)
    initial = state_arrays(driver)
    driver.step_all()
    final = state_arrays(driver)
    driver.cleanup()
    times = steps + 1
    chunks = [load(out / f"state_{chunk:04d}_tile0.npz") for chunk in range((times + 1) // 2)]
    assert sorted(os.listdir(out)) == sorted([f"state_{chunk:04d}_tile0.npz" for chunk in range(len(chunks))]
                                             + [f"constants_{name}_tile0.npz" for name in ("lat", "lon", "lon_agrid", "lat_agrid")])
    stamps = np.concatenate([d["time"] for d in chunks])
    assert list(stamps) == [np.datetime64(datetime.datetime(2000, 1, 1) + m * datetime.timedelta(seconds=225), "us") for m in range(times)]
    assert sorted(chunks[0]) == sorted(("__meta__", "time", "pt_z65") + EXAMPLE_NAMES)
    meta = json.loads(str(chunks[0]["__meta__"]))
    for name in EXAMPLE_NAMES + ("pt_z65",):
        series = np.concatenate([d[name] for d in chunks])
        extent = {"u": (12, 13, 79), "v": (13, 12, 79), "pt_z65": (12, 12)}.get(name, (12, 12, 79))
        assert series.shape == (times, 1) + extent and series.dtype == np.float32, name
        assert np.array_equal(bits(series[-1, 0]), bits(final[name])), name
        assert np.array_equal(bits(series[0, 0]), bits(initial[name])), name
        assert meta[name]["dims"][:2] == ["time", "tile"] and len(meta[name]["dims"]) == 2 + len(extent)
    assert meta["u"] == {"dims": ["time", "tile", "x", "y_interface", "z"], "units": driver.state.dycore_state.u.units}
    assert not np.array_equal(final["pt"], initial["pt"])
    grid = driver.state.grid_data
    for name, extent in (("lat", 13), ("lon", 13), ("lon_agrid", 12), ("lat_agrid", 12)):
        d = load(out / f"constants_{name}_tile0.npz")
        assert d[name].dtype == np.float64 and np.array_equal(d[name][0], np.asarray(getattr(grid, name))[3:3 + extent, 3:3 + extent])
    return initial


def test_driver_writes_diagnostics_emulated(emu_lib, clean_checks, tmp_path):
    """Two steps of the C12 example, dycore only, with output_format npz: three times in chunks of two, the last the final
    state, the first a second driver's initial state; that second driver has the same configuration with netcdf, which
    writes nothing -- no initial state, no constants -- and says so."""
    from pace_amd.driver import Driver, DriverConfig, NullDiagnostics
    from pace_amd.util import NullComm

    initial = check_driver(emu_lib, tmp_path, steps=2)
    ignored = tmp_path / "ignored"
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        second = Driver(DriverConfig.from_dict(driver_settings(ignored, "netcdf", 2)), comm=NullComm(0, 6), lib=emu_lib)
    assert len([w for w in seen if "no diagnostics are written" in str(w.message)]) == 1
    assert isinstance(second.diagnostics, NullDiagnostics)
    fresh = state_arrays(second)
    for name, a in initial.items():
        assert np.array_equal(bits(a), bits(fresh[name])), name
    second.cleanup()
    assert not ignored.exists()


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,nk", SHAPES)
def test_pack_gpu(lib, lib_f32, n, nk):
    for out_is_double in (False, True):
        check_shape(lib, "cuda", n, nk, out_is_double)
        check_shape(lib_f32, "cuda", n, nk, out_is_double)


@pytest.mark.gpu
def test_pack_thirty_three_items_gpu(lib, lib_f32):
    for out_is_double in (False, True):
        check_many(lib, "cuda", 96, 79, out_is_double)
        check_many(lib_f32, "cuda", 96, 79, out_is_double)


@pytest.mark.gpu
def test_column_integral_against_the_reference_expression_gpu(lib, lib_f32):
    check_column_integral(lib, "cuda")
    check_column_integral(lib_f32, "cuda")


@pytest.mark.gpu
def test_argument_errors_gpu(lib):
    check_argument_errors(lib, "cuda")


@pytest.mark.gpu
def test_monitor_diagnostics_gpu(lib, lib_f32):
    check_monitor_diagnostics(lib, "cuda")
    check_monitor_diagnostics(lib_f32, "cuda")


@pytest.mark.gpu
def test_driver_writes_diagnostics_gpu(lib, clean_checks, tmp_path):
    check_driver(lib, tmp_path, steps=1)
