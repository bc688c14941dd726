"""pace_state_unpack (pace_amd/csrc/k_state.hip) against a numpy restatement written here: a slice assignment with astype,
compared bit for bit over the WHOLE raw storage of every field, row padding included -- so a write outside a window shows as
well as a wrong value inside it.

The launch shape decides the sizes, as in tests/test_diagnostics.py (whose field factory this file shares): a workgroup takes a
tile of 64 points in i by 32 in the source's fastest axis -- k for a 3-D item, j for a plane -- and finds its item in a prefix
table of per-item tile counts:

    C12 x 7    windows narrower than one wave, fewer levels than a tile
    C13 x 5    odd extents and the three staggered dims
    C12 x 32   nk equal to the tile; the z_interface windows have one more
    C68 x 33   a second i tile 4 wide (the n + 2 and n + 7 wide windows: 6 and 11), one level over the tile
    C96 x 79   tiles of 32, 32, 15 (the emulation runs a fiber per thread of a transposing workgroup: its tier has this shape
               as the 32-item launch only; the GPU tier runs everything at every shape)
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_diagnostics as td  # noqa: E402  (Fields, bits and the shapes)
from helpers import ROOT  # noqa: E402

SHAPES = td.SHAPES
WINDOW3D, PLANE = 0, 1
ZFAST, XFAST = 0, 1
XYZ, XIYZ, XYIZ, XYZI, XY = td.XYZ, td.XIYZ, td.XYIZ, td.XYZI, td.XY
GUARDED = os.environ.get("PACE_GUARD_MODE")  # (a child run of test_unpack_with_guard_pages)

emu_lib, emu_lib_f32, lib, lib_f32 = td.emu_lib, td.emu_lib_f32, td.lib, td.lib_f32


def spec(field, dims, win, order=ZFAST, kind=WINDOW3D, step=1, level=0):
    return dict(field=field, dims=dims, win=win, order=order, kind=kind, step=step, level=level)


def specials():
    """Values beyond float32's range and exactly halfway between two float32 values: the float32 library narrows them as
    astype(np.float32) does (round to nearest even, overflow to +-inf); the float64 library keeps them."""
    return [1.0e39, -1.0e300, 3.5e38,
            float(np.float32(1.5)) + 2.0 ** -24,                                   # a tie, even below: rounds down
            float(np.nextafter(np.float32(1.5), np.float32(2.0))) + 2.0 ** -24,    # a tie, even above: rounds up
            -(float(np.float32(1024.0)) + 2.0 ** -14), float(np.finfo(np.float32).max) + 2.0 ** 103]  # the last tie is +inf


def run_unpack(f, specs, species=()):
    """specs: items of their own; species: (window, seven field names) -- seven ZFAST items with in_step = 7 over ONE C-ordered
    (ni, nj, nk, 7) block.  One launch.  The source has garbage before, between (and, with in_step > 1, inside) and after the
    items' elements; under guard pages it has neither lead nor tail, so the first and the last item lie against the pages."""
    import torch

    from pace_amd import _lib

    dtype = f.dtype
    fields = {}

    def field(name, dims):
        if name not in fields:
            q = f.qf.zeros(list(dims), "u")
            q._base[...] = float("nan")  # (the row padding included)
            q._base[..., ::2] = f.huge
            q._base[..., 1::5] = -f.huge
            want = q._base.cpu().numpy().copy()
            fields[name] = (q, want, want.transpose(2, 1, 0) if want.ndim == 3 else want.transpose(1, 0))
        return fields[name]

    def shape_of(s):
        return tuple(s["win"][3:]) if s["kind"] == WINDOW3D else tuple(s["win"][3:5])

    # the source buffer: every item's elements, in its order and with its step
    lead, gap, tail = (0, 0, 0) if GUARDED else (3, 5, 77)
    entries, total = [], lead  # (spec, offset, values)
    for s in specs:
        values = f.rng.uniform(-50.0, 50.0, shape_of(s))
        entries.append((s, total, values))
        total += (values.size - 1) * s["step"] + 1 + gap
    for win, names in species:
        block = f.rng.uniform(-50.0, 50.0, tuple(win[3:]) + (len(names),))
        for t, name in enumerate(names):
            entries.append((spec(name, XYZ, win, ZFAST, step=len(names)), total + t, block[..., t]))
        total += block.size + gap
    total += tail - (gap if entries else 0)
    first = next((e for e in entries if e[0]["kind"] == WINDOW3D), entries[0])
    flat = first[2].reshape(-1)
    flat[np.linspace(0, flat.size - 1, len(specials())).astype(int)] = specials()
    source = f.garbage((total,)).astype(np.float64)
    source[np.isfinite(source)] = np.sign(source[np.isfinite(source)]) * 1.0e300
    for s, offset, values in entries:
        elements = values.reshape(-1, order="F" if s["order"] == XFAST else "C")
        source[offset:offset + (elements.size - 1) * s["step"] + 1:s["step"]] = elements
    assert len(entries) <= _lib.UNPACK_MAX_ITEMS
    device_source = torch.full((total,), 0.0, dtype=torch.float64, device=f.device)
    device_source.copy_(torch.from_numpy(source))

    items = (_lib.UnpackItem * len(entries))()
    for item, (s, offset, values) in zip(items, entries):
        q, _, view = field(s["field"], s["dims"])
        i0, j0, k0, ni, nj, nk = s["win"]
        item.field = q.ptr + s["level"] * f.geom.sk * f.lib.real_bytes
        item.kind, item.order, item.in_step, item.in_offset = s["kind"], s["order"], s["step"], offset
        item.i0, item.j0, item.k0, item.ni, item.nj, item.nk = s["win"]
        with np.errstate(over="ignore"):  # (values beyond float32's range become +-inf: that is asked for)
            # the restatement: a slice assignment with astype
            if s["kind"] == WINDOW3D:
                view[i0:i0 + ni, j0:j0 + nj, k0:k0 + nk] = values.astype(dtype)
            elif view.ndim == 3:
                view[i0:i0 + ni, j0:j0 + nj, s["level"]] = values.astype(dtype)
            else:
                view[i0:i0 + ni, j0:j0 + nj] = values.astype(dtype)
    stream = None if f.device == "cpu" else C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f.lib.call("pace_state_unpack", C.byref(f.geom), items, len(entries), C.c_void_p(device_source.data_ptr()), stream)
    for name, (q, want, _) in fields.items():
        got = q._base.cpu().numpy()
        same = td.bits(got) == td.bits(want)
        assert same.all(), (f.n, f.nk, dtype, name, int((~same).sum()), np.argwhere(~same)[:6], got[~same][:4], want[~same][:4])
    assert np.array_equal(td.bits(device_source.cpu().numpy()), td.bits(source))  # (the source is only read)
    if f.lib.real_bytes == 8:
        # the round trip: pace_diag_pack(out_is_double) over the same windows returns the source's bits
        sizes = [values.size for _, _, values in entries]
        offsets = np.concatenate(([0], np.cumsum(sizes)))
        out = torch.full((int(offsets[-1]),), td.SENTINEL, dtype=torch.float64, device=f.device)
        back = (_lib.DiagItem * len(entries))()
        for item, unpacked, offset in zip(back, items, offsets):
            item.field, item.weight, item.kind, item.out_offset = unpacked.field, None, unpacked.kind, int(offset)
            item.i0, item.j0, item.k0, item.ni, item.nj, item.nk = (unpacked.i0, unpacked.j0, unpacked.k0, unpacked.ni, unpacked.nj,
                                                                    unpacked.nk)
        f.lib.call("pace_diag_pack", C.byref(f.geom), back, len(entries), 1, C.c_void_p(out.data_ptr()), stream)
        got = out.cpu().numpy()
        for (s, _, values), offset, size in zip(entries, offsets, sizes):
            assert np.array_equal(td.bits(got[offset:offset + size]), td.bits(values.reshape(-1))), (f.n, f.nk, s)


def standard_specs(f):
    """3-D items and planes in both orders; the wrapper's own windows -- the compute domain, the staggered ones, the compute
    domain +- 1 in i and j with nk + 1 levels -- a plane that is one level of a 3-D field, a window that is no compute domain, the
    whole storage, in_step = 2 on the path without LDS; and seven species of one interleaved block."""
    n, nk = f.n, f.nk
    compute = (3, 3, 0, n, n, nk)
    specs = [spec("z", XYZ, compute, ZFAST), spec("x", XYZ, compute, XFAST),
             spec("u", XYIZ, (3, 3, 0, n, n + 1, nk), XFAST), spec("v", XIYZ, (3, 3, 0, n + 1, n, nk), ZFAST),
             spec("uc", XIYZ, (3, 3, 0, n + 1, n, nk), XFAST), spec("vc", XYIZ, (3, 3, 0, n, n + 1, nk), ZFAST),
             spec("pk", XYZI, (3, 3, 0, n, n, nk + 1), ZFAST), spec("peln", XYZI, (3, 3, 0, n, n, nk + 1), XFAST),
             spec("pe", XYZI, (2, 2, 0, n + 2, n + 2, nk + 1), ZFAST), spec("pe_x", XYZI, (2, 2, 0, n + 2, n + 2, nk + 1), XFAST),
             spec("ps", XY, (3, 3, 0, n, n, 1), ZFAST, PLANE), spec("phis", XY, (3, 3, 0, n, n, 1), XFAST, PLANE),
             spec("levels", XYZ, (3, 3, 0, n, n, 1), ZFAST, PLANE, level=nk - 1),
             spec("levels", XYZ, (1, 2, 0, n + 5, 3, 1), XFAST, PLANE, level=0),
             spec("strip", XY, (0, 1, 0, n + 7, n + 5, 1), ZFAST, PLANE, step=3),
             spec("whole", XYZI, (0, 0, 0, n + 7, n + 7, nk + 1), XFAST),
             spec("stepped", XYZ, compute, XFAST, step=2)]
    if nk > 2:
        specs.append(spec("inner", XYZ, (1, 2, 1, n + 5, 3, nk - 2), ZFAST))
        specs.append(spec("inner_x", XYZ, (4, 1, 1, n - 2, n + 6, nk - 2), XFAST))
    return specs, [(compute, [f"q{t}" for t in range(7)])]


def many_specs(f):
    """32 items of mixed kind and order in one launch: 4 3-D windows, planes on levels of 3-D fields (distinct levels:
    the windows do not overlap) and on 2-D fields."""
    n, nk = f.n, f.nk
    specs = []
    for m in range(32):
        if m % 8 == 0:
            dims = (XYZ, XIYZ, XYIZ, XYZI)[m // 8]
            win = (3, 3, 0, n + (dims == XIYZ), n + (dims == XYIZ), nk + (dims == XYZI))
            specs.append(spec(f"vol{m}", dims, win, (m // 8) % 2))
        elif m % 2 == 1:
            specs.append(spec(f"full{(m // 2) // (nk + 1)}", XYZI, (m % 5, m % 3, 0, n + 7 - m % 5, n + 7 - m % 3 - m % 4, 1),
                              (m // 2) % 2, PLANE, level=((m // 2) * 7) % (nk + 1), step=1 + m % 3))
        else:
            specs.append(spec(f"plane{m}", XY, (3, 3, 0, n, n, 1), (m // 2) % 2, PLANE))
    assert len({(s["field"], s["level"]) for s in specs if s["field"].startswith("full")}) == 16
    return specs


def check_shape(lib, device, n, nk):
    f = td.Fields(lib, device, n, nk)
    specs, species = standard_specs(f)
    run_unpack(f, specs, species)


def check_many(lib, device, n, nk):
    f = td.Fields(lib, device, n, nk)
    specs = many_specs(f)
    assert len(specs) == 32
    run_unpack(f, specs)


# ---- the kernel, emulated ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nk", SHAPES[:4])
def test_unpack_emulated(emu_lib, emu_lib_f32, n, nk):
    check_shape(emu_lib, "cpu", n, nk)
    check_shape(emu_lib_f32, "cpu", n, nk)


def test_unpack_thirty_two_items_emulated(emu_lib, emu_lib_f32):
    check_many(emu_lib, "cpu", 96, 79)
    check_many(emu_lib_f32, "cpu", 96, 79)


@pytest.mark.parametrize("mode", ["over", "under"])
def test_unpack_with_guard_pages(mode):
    """The emulated cases of this file in a child pytest whose every allocation -- the fields and the source -- ends at (over)
    or starts right after (under) an inaccessible page (tests/guard.py, tests/test_guard_pages.py): there the source has
    neither lead nor tail, so a read before the first or past the last item's elements ends the child, as does a write past a
    field's last row."""
    if GUARDED:
        return  # (this IS the child)
    import test_guard_pages

    passed, tail = test_guard_pages._guarded_pytest(mode, ["test_state_unpack.py"])
    for case in ["test_unpack_emulated[%d-%d]" % shape for shape in SHAPES[:4]] + ["test_unpack_thirty_two_items_emulated"]:
        assert any(t.endswith("::" + case) for t in passed), (case, tail)


# ---- argument errors ------------------------------------------------------------------------------------------------------------
def check_argument_errors(lib, device):
    import torch

    from pace_amd import _lib

    n, nk = 12, 7
    f = td.Fields(lib, device, n, nk)
    q, _ = f.quantity(XYZ)
    source = torch.full((4 * (n + 7) * (n + 7) * (nk + 1),), 1.0, dtype=torch.float64, device=device)
    stream = None if device == "cpu" else C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(count, kind=WINDOW3D, win=(3, 3, 0, n, n, nk), order=ZFAST, step=1, offset=0, field=q.ptr):
        items = (_lib.UnpackItem * _lib.UNPACK_MAX_ITEMS)()
        for item in items:
            item.field, item.kind, item.order, item.in_step, item.in_offset = field, kind, order, step, offset
            item.i0, item.j0, item.k0, item.ni, item.nj, item.nk = win
        lib.call("pace_state_unpack", C.byref(f.geom), items, count, C.c_void_p(source.data_ptr()), stream)

    call(1)  # the table itself is fine
    call(1, win=(0, 0, 0, n + 7, n + 7, nk + 1), order=XFAST)  # the whole storage is a window
    call(1, kind=PLANE, win=(3, 3, 0, n, n, 1), step=2)
    bad = [dict(count=0), dict(count=_lib.UNPACK_MAX_ITEMS + 1), dict(count=-1),
           dict(count=1, win=(0, 0, 0, n + 8, n, nk)), dict(count=1, win=(8, 3, 0, n, n, nk)), dict(count=1, win=(3, 8, 0, n, n, nk)),
           dict(count=1, win=(3, 3, 0, n, n + 5, nk)), dict(count=1, win=(3, 3, 0, n, n, nk + 2)), dict(count=1, win=(3, 3, 2, n, n, nk)),
           dict(count=1, win=(-1, 3, 0, n, n, nk)), dict(count=1, win=(3, -1, 0, n, n, nk)), dict(count=1, win=(3, 3, -1, n, n, nk)),
           dict(count=1, win=(3, 3, 0, 0, n, nk)), dict(count=1, win=(3, 3, 0, n, 0, nk)), dict(count=1, win=(3, 3, 0, n, n, 0)),
           dict(count=1, kind=PLANE, win=(3, 3, 0, n, n, 2)), dict(count=1, kind=PLANE, win=(3, 3, 0, n, n + 5, 1)),
           dict(count=1, kind=PLANE, win=(3, 3, 1, n, n, 1)),
           dict(count=1, kind=2), dict(count=1, kind=3), dict(count=1, kind=-1),  # (a column integral is no destination)
           dict(count=1, order=2), dict(count=1, order=-1), dict(count=1, step=0), dict(count=1, step=-7),
           dict(count=1, offset=-1), dict(count=1, field=None)]
    for kwargs in bad:
        with pytest.raises(_lib.PaceError, match="invalid argument"):
            call(**kwargs)
    items = (_lib.UnpackItem * 1)()
    for args in ((None, items, 1, C.c_void_p(source.data_ptr())), (C.byref(f.geom), None, 1, C.c_void_p(source.data_ptr())),
                 (C.byref(f.geom), items, 1, None)):
        with pytest.raises(_lib.PaceError, match="invalid argument"):
            lib.call("pace_state_unpack", *args, stream)


def test_argument_errors_emulated(emu_lib, emu_lib_f32):
    check_argument_errors(emu_lib, "cpu")
    check_argument_errors(emu_lib_f32, "cpu")


def test_header_and_binding_agree_on_the_entry_point():
    from pace_amd import _lib

    text = open(os.path.join(ROOT, "include", "pace_hip.h")).read()
    proto = re.search(r"\bint pace_state_unpack\s*\(([^;]*)\);", text).group(1)
    assert len(proto.split(",")) == len(_lib._PROTOS["pace_state_unpack"][1])
    assert int(re.search(r"#define PACE_UNPACK_MAX_ITEMS (\d+)", text).group(1)) == _lib.UNPACK_MAX_ITEMS == 32
    orders = re.search(r"enum \{ PACE_ORDER_ZFAST = (\d), PACE_ORDER_XFAST = (\d) \}", text).groups()
    assert tuple(int(k) for k in orders) == (_lib.ORDER_ZFAST, _lib.ORDER_XFAST) == (ZFAST, XFAST)
    assert (_lib.DIAG_WINDOW3D, _lib.DIAG_PLANE) == (WINDOW3D, PLANE)
    body = re.search(r"typedef struct \{([^}]*)\} pace_unpack_item_t;", text).group(1)
    names = re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", body))
    assert names == [name for name, _ in _lib.UnpackItem._fields_]
    assert C.sizeof(_lib.UnpackItem) == 56
    assert "pace_state_unpack" in _lib.EXPORTED_SYMBOLS


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,nk", SHAPES)
def test_unpack_gpu(lib, lib_f32, n, nk):
    check_shape(lib, "cuda", n, nk)
    check_shape(lib_f32, "cuda", n, nk)


@pytest.mark.gpu
def test_unpack_thirty_two_items_gpu(lib, lib_f32):
    for n, nk in SHAPES:
        check_many(lib, "cuda", n, nk)
        check_many(lib_f32, "cuda", n, nk)


@pytest.mark.gpu
def test_argument_errors_gpu(lib, lib_f32):
    check_argument_errors(lib, "cuda")
    check_argument_errors(lib_f32, "cuda")
