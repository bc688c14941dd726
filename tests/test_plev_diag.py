"""pace_plev_diag (pace_amd/csrc/k_plev.hip), `p_select` of pace_amd.driver.MonitorDiagnostics / DiagnosticsConfig and the
Driver's pressure-level output against tests/plev_reference.py, the numpy restatement of the definitions in include/pace_hip.h.
Kernel results are compared bit for bit, NaNs included (no test generates a NaN: the one a column holds is propagated, which
keeps its bits), over the WHOLE output buffer, which holds a sentinel before, between and after the items.

The launch shape decides the sizes: a workgroup takes a tile of 64 columns in i by 4 rows in j, one row per wave:

    C12 x 2    the smallest column: the layers' bracket search is empty
    C12 x 7    12 of 64 lanes, three row tiles
    C13 x 5    the last row tile holds one row
    C68 x 33   a second i tile 4 lanes wide
    C96 x 79   the model's level count

The columns: surface pressure 50000 ... 103000 Pa changing from lane to lane, so that 850 hPa lies in different brackets in
neighbouring lanes and under the ground in some; targets above pm[0], below pm[nz - 1], above peln[0] and below peln[nz]; exact
ties lp == pm[k], pm[0], pm[nz - 1], peln[k], taken from the stored peln; a column with a negative delp and one with a NaN.
"""
import ctypes as C
import datetime
import json
import math
import os
import re
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plev_reference as ref  # noqa: E402
import test_diagnostics as td  # noqa: E402  (Fields, the dims, the library fixtures, the recording monitor)
from helpers import GOLDEN, ROOT  # noqa: E402

SHAPES = ((12, 2), (12, 7), (13, 5), (68, 33), (96, 79))
LAYER, HEIGHT = 0, 1
SENTINEL = td.SENTINEL
PTOP = 300.0
GUARDED = os.environ.get("PACE_GUARD_MODE")  # (a child run of test_plev_diag_with_guard_pages)
YAML = os.path.join(GOLDEN, "driver_baroclinic_c12_plev.yaml")
XYZ, XYIZ, XYZI, XY = td.XYZ, td.XYIZ, td.XYZI, td.XY

emu_lib, emu_lib_f32, lib, lib_f32 = td.emu_lib, td.emu_lib_f32, td.lib, td.lib_f32
clean_checks = td.clean_checks


# ---- the columns ---------------------------------------------------------------------------------------------------------------
class Columns:
    """peln, two delz, phis and three layer fields of a C<n> x <nz> tile, with values over the WHOLE horizontal storage (any
    window is legal) and garbage in the level below the layers and in the row padding.  Made once per shape and library and only
    read; the restatement's planes are computed once each and kept."""

    NEGATIVE_DELP, HOLDS_NAN = (4, 6), (7, 5)

    def __init__(self, lib, device, n, nz):
        f = self.f = td.Fields(lib, device, n, nz)
        side = n + 7
        i, j = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
        self.ps = 50000.0 + 53000.0 * ((5 * i + 3 * j) % side) / (side - 1)  # (neighbouring lanes are far apart)
        assert (self.ps > 85000.0).any() and (self.ps < 85000.0).any()
        peln = np.log(PTOP + (self.ps[..., None] - PTOP) * (np.arange(nz + 1) / nz) ** 1.5)
        k = nz // 2
        peln[self.NEGATIVE_DELP + ([k, k + 1],)] = peln[self.NEGATIVE_DELP + ([k + 1, k],)]
        peln[self.HOLDS_NAN + (k,)] = np.nan
        layers, interfaces = (slice(0, side), slice(0, side), slice(0, nz)), (slice(0, side), slice(0, side), slice(0, nz + 1))
        self.peln = f.quantity(XYZI, values=lambda s: peln, window=interfaces, units="ln(Pa)")
        self.phis = f.quantity(XY, values=lambda s: f.rng.uniform(0.0, 2.0e4, s), window=layers[:2], units="m^2 s^-2")
        self.fields = {name: f.quantity(XYZ, window=layers, units=units) for name, units in (("pt", "degK"), ("ua", "m/s"), ("va", "m/s"))}
        for name in ("delz", "delz2"):
            self.fields[name] = f.quantity(XYZ, values=lambda s: -f.rng.uniform(20.0, 900.0, s), window=layers, units="m")
        self._planes = {}

    def ties(self):
        """Eight levels: 850 hPa; 1 hPa (above peln[0]) and 1100 hPa (below every peln[nz]); just below the model top (above
        every pm[0]); lp == pm[k], pm[0], pm[nz - 1] and peln[k] of four columns, from the stored values."""
        a, nz = self.peln[1].astype(np.float64), self.f.nk
        k = nz // 2

        def pm(i, j, k):
            return float(0.5 * (a[i, j, k] + a[i, j, k + 1]))

        log_p = [math.log(85000.0), math.log(100.0), math.log(110000.0), float(a[0, 0, 0]) + 1.0e-3,
                 pm(5, 4, k), pm(6, 9, 0), pm(9, 3, nz - 1), float(a[10, 10, k])]
        assert log_p[1] < a[..., 0].min() and log_p[2] > np.nanmax(a[..., nz]) and a[0, 0, 0] < log_p[3] < pm(0, 0, 0)
        return log_p

    def plane(self, kind, name, lp, window):
        key = (kind, name, lp, window)
        if key not in self._planes:
            i0, j0, ni, nj = window
            w = (slice(i0, i0 + ni), slice(j0, j0 + nj))
            if kind == HEIGHT:
                self._planes[key] = ref.height(self.fields[name][1][w], self.phis[1][w], self.peln[1][w], lp, self.f.nk)
            else:
                self._planes[key] = ref.layer(self.fields[name][1][w], self.peln[1][w], lp, self.f.nk)
            self._planes[key].setflags(write=False)
        return self._planes[key]


_columns = {}


def columns(lib, device, n, nz):
    key = (lib.path, device, n, nz)
    if key not in _columns:
        _columns[key] = Columns(lib, device, n, nz)
    return _columns[key]


def run(cols, log_p, specs, window, out_is_double):
    """specs: (kind, field name, index into log_p).  One call with the items at gaps in a sentinel-filled buffer (under guard
    pages: no lead, no gaps, no tail); the WHOLE buffer is compared with the restatement, bit for bit."""
    import torch

    from pace_amd import _lib

    f = cols.f
    out_dtype = np.float64 if out_is_double else np.float32
    lead, gap, tail = (0, 0, 0) if GUARDED else (3, 5, 77)
    size = window[2] * window[3]
    offsets = [lead + m * (size + gap) for m in range(len(specs))]
    total = lead + len(specs) * (size + gap) - gap + tail
    out = torch.full((total,), SENTINEL, dtype=torch.float64 if out_is_double else torch.float32, device=f.device)
    want = np.full(total, SENTINEL, dtype=out_dtype)
    items = (_lib.PlevItem * len(specs))()
    for item, (kind, name, level), offset in zip(items, specs, offsets):
        item.field = cols.fields[name][0].ptr
        item.surface = cols.phis[0].ptr if kind == HEIGHT else None
        item.kind, item.level, item.out_offset = kind, level, offset
        with np.errstate(over="ignore"):
            want[offset:offset + size] = cols.plane(kind, name, log_p[level], window).astype(out_dtype).reshape(-1)
    stream = None if f.device == "cpu" else C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f.lib.call("pace_plev_diag", C.byref(f.geom), cols.peln[0].ptr, (C.c_double * len(log_p))(*log_p), len(log_p), items, len(specs),
               *window, int(out_is_double), C.c_void_p(out.data_ptr()), stream)
    got = out.cpu().numpy()
    same = td.bits(got) == td.bits(want)
    assert same.all(), (f.n, f.nk, f.dtype, out_dtype, window, int((~same).sum()), np.flatnonzero(~same)[:8], got[~same][:4], want[~same][:4])


def check_shape(lib, device, n, nz):
    """Eight levels with 21 items in mixed order -- layer fields and heights alternate, a second delz comes between the heights
    of the first -- and one level with two items; the compute domain and an off-origin window that reaches into the halo; both
    output types."""
    cols = columns(lib, device, n, nz)
    log_p = cols.ties()
    specs = []
    for p in range(8):
        specs += [(LAYER, ("pt", "ua", "va")[p % 3], p), (HEIGHT, "delz", p)]
    specs += [(LAYER, "ua", 0), (HEIGHT, "delz2", 0), (LAYER, "pt", 7), (HEIGHT, "delz2", 5), (HEIGHT, "delz", 2)]
    compute, off_origin = (3, 3, n, n), (1, 2, n + 3, n + 1)
    run(cols, log_p, specs, compute, False)
    run(cols, log_p, specs, off_origin, True)
    one = [math.log(50000.0)]
    run(cols, one, [(LAYER, "pt", 0), (HEIGHT, "delz", 0)], compute, True)
    run(cols, one, [(HEIGHT, "delz", 0), (LAYER, "va", 0)], off_origin, False)
    if not GUARDED:
        # the columns are what they are meant to be: 850 hPa lies in many brackets and under the ground in some columns, and the
        # NaN reaches the output of its column alone
        w = (slice(3, 3 + n), slice(3, 3 + n))
        a = cols.peln[1][w].astype(np.float64)
        below = (a <= log_p[0]).sum(axis=-1)
        assert len(np.unique(below)) >= (3 if nz >= 33 else 2) and (below == nz + 1).any() and (below < nz + 1).any()
        assert all(np.isnan(plane).sum() <= 1 for plane in cols._planes.values())


@pytest.mark.parametrize("n,nz", SHAPES)
def test_plev_emulated(emu_lib, emu_lib_f32, n, nz):
    check_shape(emu_lib, "cpu", n, nz)
    check_shape(emu_lib_f32, "cpu", n, nz)


@pytest.mark.parametrize("mode", ["over", "under"])
def test_plev_diag_with_guard_pages(mode):
    """The emulated cases of this file in a child pytest whose every allocation -- the fields, peln, the output -- ends at
    (over) or starts right after (under) an inaccessible page (tests/guard.py, tests/test_guard_pages.py): there the output has
    neither lead nor tail nor gaps, so a store before the first or past the last item's elements ends the child, as does a
    read past a field's last row or level.  (The driver runs are not repeated there.)"""
    if GUARDED:
        return  # (this IS the child)
    import test_guard_pages

    passed, tail = test_guard_pages._guarded_pytest(mode, ["test_plev_diag.py"])
    for case in ["test_plev_emulated[%d-%d]" % shape for shape in SHAPES] + ["test_host_path_emulated", "test_argument_errors_emulated"]:
        assert any(t.endswith("::" + case) for t in passed), (case, tail)


# ---- against the expression ------------------------------------------------------------------------------------------------------
# Where the two bounds come from.  In an isothermal hydrostatic column delz[k] = -(Rd T / g) (peln[k + 1] - peln[k]), so the
# interface heights are linear in log p and the interpolation -- and both extrapolations -- reproduce phis / g + (Rd T / g)
# ln(ps / p) but for rounding: of every delz as it is stored (half an ulp of a layer's depth), of the nz subtractions that sum
# them (each half an ulp of the height reached), of the interpolation's five operations, and under the ground of the lowest
# layer's depth, a difference of two rounded heights, times t -- up to 40 where 1050 hPa is sought under a 500 hPa surface
# through a layer 0.019 deep in log p.  With U the spacing of doubles at the column's largest height, zi[0], the sums alone are
# at most about nz / 2 U were every rounding to go the same way, and a few U as they go in practice.  The restatement's own
# error on exactly these inputs, against the expression in extended precision, was measured on the CPU (C24 x 79, the five
# pressures below): 4.79 U for the height, and 0.88 spacings of the field's largest value for the linear field.  The bounds are
# those figures and a few ulps: the kernel, which equals the restatement bit for bit, has to meet them on the GPU too.
HEIGHT_BOUND_ULPS = 8.0
LINEAR_BOUND_ULPS = 3.0
T_ISOTHERMAL = 250.0


def check_expression(lib, device, n=24, nz=79):
    import torch

    from pace_amd import _lib
    from pace_amd.util import constants

    assert lib.real_bytes == 8
    f = td.Fields(lib, device, n, nz)
    side = n + 7
    rng = np.random.default_rng(7)
    everywhere = (slice(0, side), slice(0, side))
    ps = rng.uniform(50000.0, 103000.0, (side, side))
    peln = np.log(PTOP + (ps[..., None] - PTOP) * (np.arange(nz + 1) / nz) ** 1.5)
    scale = constants.RDGAS * T_ISOTHERMAL / constants.GRAV
    delz = -scale * (peln[..., 1:] - peln[..., :-1])
    pm = 0.5 * (peln[..., 1:] + peln[..., :-1])
    linear = 220.0 + 11.0 * pm
    q_peln = f.quantity(XYZI, values=lambda s: peln, window=everywhere + (slice(0, nz + 1),))
    q_delz = f.quantity(XYZ, values=lambda s: delz, window=everywhere + (slice(0, nz),))
    q_linear = f.quantity(XYZ, values=lambda s: linear, window=everywhere + (slice(0, nz),))
    q_phis = f.quantity(XY, values=lambda s: rng.uniform(0.0, 3.0e4, s), window=everywhere)
    # 1 hPa (above the model top) and 1050 hPa (under every ground) are extrapolations of the height; the linear field is
    # compared where it is interpolated: between pm[0] and pm[nz - 1] of every column
    pressures = [85000.0, 50000.0, 20000.0, 100.0, 105000.0]
    log_p = [math.log(p) for p in pressures]
    items = (_lib.PlevItem * (2 * len(log_p)))()
    size = side * side
    for p in range(len(log_p)):
        items[2 * p].field, items[2 * p].surface, items[2 * p].kind = q_delz[0].ptr, q_phis[0].ptr, HEIGHT
        items[2 * p + 1].field, items[2 * p + 1].kind = q_linear[0].ptr, LAYER
        for m in (2 * p, 2 * p + 1):
            items[m].level, items[m].out_offset = p, m * size
    out = torch.full((len(items) * size,), SENTINEL, dtype=torch.float64, device=device)
    stream = None if device == "cpu" else C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.call("pace_plev_diag", C.byref(f.geom), q_peln[0].ptr, (C.c_double * len(log_p))(*log_p), len(log_p), items, len(items),
             0, 0, side, side, 1, C.c_void_p(out.data_ptr()), stream)
    got = out.cpu().numpy().reshape(len(items), side, side)
    wide = np.longdouble
    surface = q_phis[1].astype(wide) / wide(constants.GRAV)
    z_top = surface + wide(scale) * (peln[..., nz].astype(wide) - peln[..., 0].astype(wide))
    worst_height = worst_linear = 0.0
    for p, lp in enumerate(log_p):
        exact = surface + wide(scale) * (peln[..., nz].astype(wide) - wide(lp))
        worst_height = max(worst_height, float(np.max(np.abs(got[2 * p].astype(wide) - exact) / np.spacing(z_top.astype(np.float64)))))
        assert np.array_equal(td.bits(got[2 * p]), td.bits(ref.height(q_delz[1], q_phis[1], q_peln[1], lp, nz)))
        inside = (lp > pm[..., 0]) & (lp < pm[..., nz - 1])
        if pressures[p] in (85000.0, 50000.0, 20000.0):
            assert inside.mean() > 0.25, (pressures[p], inside.mean())  # (the comparison below is not empty)
        if inside.any():
            exact = wide(220.0) + wide(11.0) * wide(lp)
            error = np.abs(got[2 * p + 1].astype(wide) - exact)[inside] / np.spacing(np.abs(linear).max())
            worst_linear = max(worst_linear, float(error.max()))
    print(f"isothermal column C{n} x {nz}: height {worst_height:.2f} spacings of zi[0] from the expression, "
          f"linear field {worst_linear:.2f} spacings of its largest value")
    assert worst_height <= HEIGHT_BOUND_ULPS and worst_linear <= LINEAR_BOUND_ULPS


def test_against_the_expression_emulated(emu_lib):
    check_expression(emu_lib, "cpu")


# ---- argument errors ------------------------------------------------------------------------------------------------------------
def check_argument_errors(lib, device):
    import torch

    from pace_amd import _lib

    n, nz = 12, 7
    cols = columns(lib, device, n, nz)
    f = cols.f
    out = torch.full((2 * (n + 7) * (n + 7),), SENTINEL, dtype=torch.float32, device=device)
    stream = None if device == "cpu" else C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pt, delz, phis, peln = cols.fields["pt"][0].ptr, cols.fields["delz"][0].ptr, cols.phis[0].ptr, cols.peln[0].ptr
    present = dict(peln=peln, log_p=True, items=True, out=out.data_ptr())

    def call(nitems=2, nlevels=2, kind=LAYER, level=1, field=pt, surface=None, window=(3, 3, n, n), offset=0, geom=f.geom, **pointers):
        p = {**present, **pointers}
        items = (_lib.PlevItem * (_lib.PLEV_MAX_ITEMS + 1))()
        for item in items:
            item.field, item.surface, item.kind, item.level, item.out_offset = field, surface, kind, level, offset
        log_p = (C.c_double * (_lib.PLEV_MAX_LEVELS + 1))(*[math.log(50000.0 + 1000.0 * m) for m in range(_lib.PLEV_MAX_LEVELS + 1)])
        lib.call("pace_plev_diag", C.byref(geom), p["peln"], log_p if p["log_p"] else None, nlevels, items if p["items"] else None,
                 nitems, *window, 0, None if p["out"] is None else C.c_void_p(p["out"]), stream)

    call()  # the table itself is fine
    call(_lib.PLEV_MAX_ITEMS, _lib.PLEV_MAX_LEVELS, level=_lib.PLEV_MAX_LEVELS - 1)
    call(kind=HEIGHT, field=delz, surface=phis, window=(0, 0, n + 7, n + 7))  # the whole storage is a window
    before = out.clone()
    one_layer = _lib.Geom(n, 1, f.geom.sj, 0, f.geom.sk)
    bad = [dict(nlevels=0), dict(nlevels=_lib.PLEV_MAX_LEVELS + 1), dict(nlevels=-1),
           dict(nitems=0), dict(nitems=_lib.PLEV_MAX_ITEMS + 1), dict(nitems=-1),
           dict(kind=2), dict(kind=-1), dict(level=2), dict(level=-1), dict(kind=HEIGHT, field=delz), dict(field=None),
           dict(geom=one_layer),
           dict(window=(3, 3, 0, n)), dict(window=(3, 3, n, 0)), dict(window=(-1, 3, n, n)), dict(window=(3, -1, n, n)),
           dict(window=(8, 3, n, n)), dict(window=(3, 8, n, n)), dict(window=(0, 0, n + 8, n)), dict(window=(0, 0, n, n + 8)),
           dict(window=(n + 7, 3, 1, 1)), dict(offset=-1),
           dict(peln=None), dict(log_p=False), dict(items=False), dict(out=None)]
    for kwargs in bad:
        with pytest.raises(_lib.PaceError, match="invalid argument"):
            call(**kwargs)
    # a refused call wrote nothing: the output is what the accepted calls above left
    assert torch.equal(out, before) and not (before == SENTINEL).all()


def test_argument_errors_emulated(emu_lib, emu_lib_f32):
    check_argument_errors(emu_lib, "cpu")
    check_argument_errors(emu_lib_f32, "cpu")


def test_header_and_binding_agree_on_the_entry_point():
    from pace_amd import _lib

    text = open(os.path.join(ROOT, "include", "pace_hip.h")).read()
    proto = re.search(r"\bint pace_plev_diag\s*\(([^;]*)\);", text).group(1)
    assert len(proto.split(",")) == len(_lib._PROTOS["pace_plev_diag"][1]) == 13
    assert int(re.search(r"#define PACE_PLEV_MAX_ITEMS (\d+)", text).group(1)) == _lib.PLEV_MAX_ITEMS == 32
    assert int(re.search(r"#define PACE_PLEV_MAX_LEVELS (\d+)", text).group(1)) == _lib.PLEV_MAX_LEVELS == 8
    kinds = re.search(r"enum \{ PACE_PLEV_LAYER = (\d), PACE_PLEV_HEIGHT = (\d) \}", text).groups()
    assert tuple(int(k) for k in kinds) == (_lib.PLEV_LAYER, _lib.PLEV_HEIGHT) == (LAYER, HEIGHT)
    body = re.search(r"typedef struct \{([^}]*)\} pace_plev_item_t;", text).group(1)
    names = re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", body))
    assert names == [name for name, _ in _lib.PlevItem._fields_]
    assert C.sizeof(_lib.PlevItem) == 32
    assert "pace_plev_diag" in _lib.EXPORTED_SYMBOLS
    assert re.search(r"\bpace_\*;", open(os.path.join(ROOT, "pace_amd", "csrc", "exports.map")).read())


# ---- MonitorDiagnostics ---------------------------------------------------------------------------------------------------------
def plev_state(cols):
    f = cols.f
    dycore = {name: q for name, (q, _) in cols.fields.items()}
    dycore.update(peln=cols.peln[0], phis=cols.phis[0], u=f.quantity(XYIZ, units="m/s")[0], pe=f.quantity(XYZI, units="Pa")[0])
    return types.SimpleNamespace(dycore_state=types.SimpleNamespace(**dycore), physics_state=types.SimpleNamespace())


def counting_diagnostics(lib, p_select, names=(), z_select=()):
    from pace_amd.driver import MonitorDiagnostics

    counting = td.CountingLib(lib)
    diag = MonitorDiagnostics(td.RecordingMonitor(), list(names), [], list(z_select), lib=counting, p_select=p_select)
    copies = []
    to_host = diag._to_host

    def counted(packed, host):
        copies.append(packed.numel())
        to_host(packed, host)

    diag._to_host = counted
    return diag, counting, copies


NINE = (85000.0, 50000.0, 20000.0, 100.0, 110000.0, 70000.0, 30000.0, 92500.0, 1000.0)
NINE_SUFFIXES = ("850", "500", "200", "1", "1100", "700", "300", "925", "10")


def check_host_path(lib, device):
    """33 planes on 9 pressures after a volume and a level: one pace_diag_pack, two pace_plev_diag, ONE transfer; names, dims,
    units, order; the values are the restatement's on the state's arrays, narrowed."""
    from pace_amd.driver import PSelect, ZSelect

    n, nz = 13, 5
    cols = columns(lib, device, n, nz)
    state = plev_state(cols)
    four = ["pt", "ua", "height", "va"]
    p_select = [PSelect(pressure=p, names=list(four)) for p in NINE[:8]] + [PSelect(pressure=NINE[8], names=["pt"])]
    diag, counting, copies = counting_diagnostics(lib, p_select, names=["pt"], z_select=[ZSelect(level=3, names=["ua"])])
    time = datetime.datetime(2000, 1, 1, 0, 3, 45)
    diag.store(time, state)
    assert counting.calls == ["pace_diag_pack", "pace_plev_diag", "pace_plev_diag"] and len(copies) == 1
    (got,) = diag.monitor.stored
    expected = [f"{name}_p{suffix}" for suffix in NINE_SUFFIXES[:8] for name in four] + ["pt_p10"]
    assert len(expected) == 33 and list(got) == ["time", "pt", "ua_z3"] + expected
    assert copies == [n * n * nz + n * n + 33 * n * n]
    window = (3, 3, n, n)
    for p, suffix in zip(NINE, NINE_SUFFIXES):
        for name in four if p != NINE[8] else ["pt"]:
            dims, units, data, contiguous = got[f"{name}_p{suffix}"]
            assert dims == ("x", "y") and contiguous and data.dtype == np.float32 and data.shape == (n, n)
            assert units == ("m" if name == "height" else cols.fields[name][0].units)
            kind, field = (HEIGHT, "delz") if name == "height" else (LAYER, name)
            want = cols.plane(kind, field, math.log(p), window).astype(np.float32)
            assert np.array_equal(td.bits(data), td.bits(want)), (name, suffix)
    assert np.array_equal(td.bits(got["pt"][2]), td.bits(cols.fields["pt"][1][3:3 + n, 3:3 + n, :nz].astype(np.float32)))
    # a second store: the plan is kept, the counts are the same again
    diag.store(time, state)
    assert counting.calls == ["pace_diag_pack", "pace_plev_diag", "pace_plev_diag"] * 2 and len(copies) == 2
    # pressure levels alone: one launch, one transfer, no pace_diag_pack
    diag, counting, copies = counting_diagnostics(lib, [PSelect(50000.0, ["height", "pt"])])
    diag.store(time, state)
    assert counting.calls == ["pace_plev_diag"] and copies == [2 * n * n]
    assert list(diag.monitor.stored[0]) == ["time", "height_p500", "pt_p500"]


def test_host_path_emulated(emu_lib, emu_lib_f32):
    check_host_path(emu_lib, "cpu")
    check_host_path(emu_lib_f32, "cpu")


def test_refusals_and_configuration_emulated(emu_lib, tmp_path):
    from pace_amd.driver import DiagnosticsConfig, MonitorDiagnostics, NullDiagnostics, PSelect
    from pace_amd.util.partitioner import CubedSpherePartitioner

    state = plev_state(columns(emu_lib, "cpu", 13, 5))
    now = datetime.datetime(2000, 1, 1)
    for name, message in (("u", "u has dimension"), ("pe", "pe has dimension"), ("qfog", "Invalid state variable qfog"),
                          ("phis", "phis has dimension")):
        diag = MonitorDiagnostics(td.RecordingMonitor(), [], [], [], lib=emu_lib, p_select=[PSelect(85000.0, ["pt", name])])
        with pytest.raises(ValueError, match=message):
            diag.store(now, state)
        assert diag.monitor.stored == []
    for pressure in (0.0, -85000.0, float("nan")):
        with pytest.raises(ValueError, match="p_select of pt: the pressure must be positive"):
            PSelect(pressure, ["pt"])
    block = [{"pressure": 85000, "names": ["pt", "ua"]}, {"pressure": 500.5e2, "names": ["height"]}]
    with pytest.raises(ValueError, match="path must be given"):
        DiagnosticsConfig(p_select=[PSelect(85000.0, ["pt"])])
    with pytest.raises(ValueError, match="path must be given"):
        DiagnosticsConfig.from_dict({"p_select": block})
    with pytest.raises(ValueError, match="diagnostics_config.p_select has no setting 'level'"):
        DiagnosticsConfig.from_dict({"path": str(tmp_path), "p_select": [{"pressure": 85000, "names": ["pt"], "level": 3}]})
    with pytest.raises(ValueError, match="diagnostics_config.p_select.pressure"):
        DiagnosticsConfig.from_dict({"path": str(tmp_path), "p_select": [{"pressure": "850 hPa", "names": ["pt"]}]})
    with pytest.raises(ValueError, match="the pressure must be positive"):
        DiagnosticsConfig.from_dict({"path": str(tmp_path), "p_select": [{"pressure": -1, "names": ["pt"]}]})
    target = tmp_path / "out"
    config = DiagnosticsConfig.from_dict({"path": str(target), "output_format": "npz", "p_select": block})
    assert [(p.pressure, p.names) for p in config.p_select] == [(85000.0, ["pt", "ua"]), (50050.0, ["height"])]
    assert [p.output_name(name) for p in config.p_select for name in p.names] == ["pt_p850", "ua_p850", "height_p500.5"]
    communicator = types.SimpleNamespace(rank=2, partitioner=CubedSpherePartitioner())
    diag = config.diagnostics_factory(communicator, lib="the library")
    assert isinstance(diag, MonitorDiagnostics) and diag.p_select == config.p_select and diag.names == []
    for output_format in ("zarr", "netcdf"):  # (a per-rank communicator: nothing is written, as before)
        config = DiagnosticsConfig.from_dict({"path": str(tmp_path / output_format), "output_format": output_format, "p_select": block})
        assert isinstance(config.diagnostics_factory(communicator), NullDiagnostics) and not (tmp_path / output_format).exists()
    assert DiagnosticsConfig().p_select == []


# ---- the Driver -------------------------------------------------------------------------------------------------------------------
PLEV_OUTPUTS = (("pt_p850", LAYER, "pt", 85000.0), ("ua_p850", LAYER, "ua", 85000.0), ("va_p850", LAYER, "va", 85000.0),
                ("height_p500", HEIGHT, "delz", 50000.0), ("pt_p500", LAYER, "pt", 50000.0))


def driver_settings(path, output_format, **over):
    import yaml

    with open(YAML) as f:
        d = yaml.safe_load(f)
    block = d["diagnostics_config"]["p_select"]
    assert block == [{"pressure": 85000, "names": ["pt", "ua", "va"]}, {"pressure": 50000, "names": ["height", "pt"]}]
    d["diagnostics_config"] = dict(d["diagnostics_config"], path=str(path), output_format=output_format, time_chunk_size=1)
    d.update(dycore_only=True, output_initial_state=False, minutes=0, seconds=225, **over)
    return d


def restated(driver):
    """The five planes of the file's p_select block from the driver's state, by the restatement."""
    state = driver.state.dycore_state
    a = {name: getattr(state, name).data.cpu().numpy()[3:15, 3:15] for name in ("pt", "ua", "va", "delz", "phis", "peln")}
    out = {}
    for name, kind, field, pressure in PLEV_OUTPUTS:
        if kind == HEIGHT:
            out[name] = ref.height(a["delz"], a["phis"], a["peln"], math.log(pressure), 79).astype(np.float32)
        else:
            out[name] = ref.layer(a[field], a["peln"], math.log(pressure), 79).astype(np.float32)
    return out


def same_planes(got, want):
    """Bit for bit where the restatement has a value, NaN where it has a NaN.  (A lone tile's halo is never filled, so after a
    step its state holds NaNs of either sign; which of two different NaNs an addition returns is the processor's choice of
    operand, not part of the definition.)"""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(td.bits(got)[~nan], td.bits(want)[~nan])


def check_driver(lib, tmp_path):
    """One step of the C12 example with its p_select block, dycore only, npz: the file's planes are the restatement's on the
    driver's final state (a lone tile: what its unfilled halo has reached is NaN in both); where the wave is computed, 850 hPa
    temperature and 500 hPa height are what they are for this case."""
    from pace_amd.driver import Driver, DriverConfig
    from pace_amd.util import NullComm

    out = tmp_path / "diagnostics"
    driver = Driver(DriverConfig.from_dict(driver_settings(out, "npz")), comm=NullComm(0, 6), lib=lib)
    driver.step_all()
    want = restated(driver)
    driver.cleanup()
    d = td.load(out / "state_0000_tile0.npz")
    meta = json.loads(str(d["__meta__"]))
    assert list(meta)[-6:] == ["pt_z65"] + [name for name, _, _, _ in PLEV_OUTPUTS]
    for name, kind, field, _ in PLEV_OUTPUTS:
        assert d[name].shape == (1, 1, 12, 12) and d[name].dtype == np.float32, name
        assert same_planes(d[name][0, 0], want[name]), name
        units = "m" if kind == HEIGHT else getattr(driver.state.dycore_state, field).units
        assert meta[name] == {"dims": ["time", "tile", "x", "y"], "units": units}
    assert np.isfinite(d["pt_p850"]).sum() >= 16 and np.isfinite(d["height_p500"]).sum() >= 16
    assert 200.0 < np.nanmin(d["pt_p850"]) and np.nanmax(d["pt_p850"]) < 320.0
    assert 4000.0 < np.nanmin(d["height_p500"]) and np.nanmax(d["height_p500"]) < 6200.0


def test_driver_writes_pressure_levels_emulated(emu_lib, clean_checks, tmp_path):
    if GUARDED:
        return  # (a driver step under guard pages belongs to tests/test_guard_pages.py's own lists)
    check_driver(emu_lib, tmp_path)


def test_whole_cube_writes_pressure_levels_emulated(emu_lib, clean_checks, tmp_path):
    """The same step under run_cube_driver with netcdf: every rank packs its planes (one pace_plev_diag each), the root stores
    them with a tile axis of 6; tile by tile they are the restatement's on that tile's final state."""
    if GUARDED:
        return
    from scipy.io import netcdf_file

    from pace_amd.driver import DriverConfig, run_cube_driver

    out = tmp_path / "globe"
    counting = td.CountingLib(emu_lib)
    settings = driver_settings(out, "netcdf", stencil_config={}, comm_config={"type": "cube"}, days=0, hours=0)
    drivers = run_cube_driver(DriverConfig.from_dict(settings), device="cpu", lib=counting)
    assert counting.calls.count("pace_plev_diag") == 6 and counting.calls.count("pace_cube_gather") == 1
    with netcdf_file(str(out / "state_0000_tile0.nc"), "r", mmap=False) as f:
        got = {name: f.variables[name][:].copy() for name, _, _, _ in PLEV_OUTPUTS}
        dims = {name: f.variables[name].dimensions for name in got}
        units = {name: f.variables[name].units.decode() for name in got}
    assert len(drivers) == 6
    for name, kind, field, _ in PLEV_OUTPUTS:
        assert got[name].shape == (1, 6, 12, 12) and got[name].dtype.itemsize == 4 and dims[name] == ("time", "tile", "x", "y")
        assert units[name] == ("m" if kind == HEIGHT else getattr(drivers[0].state.dycore_state, field).units)
    for t, driver in enumerate(drivers):
        want = restated(driver)
        for name in got:
            assert np.array_equal(td.bits(got[name][0, t].astype(np.float32)), td.bits(want[name])), (name, t)
    # the whole globe has its halos: every value is there, and is what this case has at 850 and 500 hPa
    assert np.isfinite(got["pt_p850"]).all() and 200.0 < got["pt_p850"].min() and got["pt_p850"].max() < 320.0
    assert np.isfinite(got["height_p500"]).all() and 4000.0 < got["height_p500"].min() and got["height_p500"].max() < 6200.0
    assert not np.array_equal(got["pt_p850"][0, 0], got["pt_p850"][0, 2])


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,nz", SHAPES)
def test_plev_gpu(lib, lib_f32, n, nz):
    check_shape(lib, "cuda", n, nz)
    check_shape(lib_f32, "cuda", n, nz)


@pytest.mark.gpu
def test_against_the_expression_gpu(lib):
    check_expression(lib, "cuda")


@pytest.mark.gpu
def test_argument_errors_gpu(lib, lib_f32):
    check_argument_errors(lib, "cuda")
    check_argument_errors(lib_f32, "cuda")


@pytest.mark.gpu
def test_host_path_gpu(lib, lib_f32):
    check_host_path(lib, "cuda")
    check_host_path(lib_f32, "cuda")


@pytest.mark.gpu
def test_driver_writes_pressure_levels_gpu(lib, clean_checks, tmp_path):
    check_driver(lib, tmp_path)
