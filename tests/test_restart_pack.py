"""pace_restart_pack (pace_amd/csrc/k_restart.hip) against a numpy restatement written here:

    q[window].transpose(2, 1, 0).astype('>f8' | '>f4').tobytes()          the bytes of an item
    (the same, native-endian).view(uint64 | uint32).sum(dtype=uint64)     its sum, which wraps

compared bit for bit over the WHOLE output buffer, whose bytes before, between and after the items hold a sentinel.

The launch shape decides the sizes.  The launch is indexed by output element: an item is cut into 16-byte slots (2 doubles or 4
floats) counted from the 16-byte boundary below its first byte, a workgroup takes 1024 slots, a thread 4 of them, and the slots
at an item's two ends that it does not fill are stored element by element:

    C12 x 63   the restart fixture's shape: rows of 12 and 13, 5 and 6 workgroups per 3-D item
    C13 x 7    odd element counts: every item after the first starts 8 (4) bytes off a 16-byte boundary
    C65 x 5    a row longer than a wave
    C24 x 1    one level
    C96 x 79   (GPU only) 728 064 elements per item: 356 workgroups, the combine's lanes fold 5 and 6 partials each

An item of 2 x 1 x 1 is one slot or two halves of two; 32 items fill the table; 33 go through the host layer's two launches.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_diagnostics as td  # noqa: E402  (Fields, the dims and the library fixtures)
from helpers import ROOT  # noqa: E402

SHAPES = ((12, 63), (13, 7), (65, 5), (24, 1))
GPU_SHAPES = SHAPES + ((96, 79),)
WINDOW3D, PLANE = 0, 1
BE_F64, BE_F32 = 0, 1
XYZ, XIYZ, XYIZ, XYZI, XY = td.XYZ, td.XIYZ, td.XYIZ, td.XYZI, td.XY
GUARDED = os.environ.get("PACE_GUARD_MODE")  # (a child run of test_restart_pack_with_guard_pages)
SENTINEL = 0xA5
SENTINEL_WORD = int(np.array([SENTINEL] * 4, dtype=np.uint8).view(np.int32)[0])

emu_lib, emu_lib_f32, lib, lib_f32 = td.emu_lib, td.emu_lib_f32, td.lib, td.lib_f32

NAN_WITH_PAYLOAD = np.array([0x7FF800000BADC0DE], dtype=np.uint64).view(np.float64)[0]


def specials(dtype):
    """-0.0, denormals, +-inf, a NaN with a payload; for float64 storage also values above FLT_MAX, a float32 denormal and ties
    of the narrowing."""
    if dtype == np.float32:
        nan = np.array([0x7FC00ABC], dtype=np.uint32).view(np.float32)[0]
        return np.array([-0.0, 1.0e-45, -3.0e-39, np.inf, -np.inf, nan, 3.4028235e38], dtype=np.float32)
    return np.array([-0.0, 5.0e-324, -1.0e-310, np.inf, -np.inf, NAN_WITH_PAYLOAD, 1.0e39, -1.0e300, 3.5e38, 1.0e-40,
                     float(np.float32(1.5)) + 2.0 ** -24, float(np.nextafter(np.float32(1.5), np.float32(2.0))) + 2.0 ** -24,
                     float(np.finfo(np.float32).max) + 2.0 ** 103], dtype=np.float64)


def spec(field, dims, win, kind=WINDOW3D, level=0):
    return dict(field=field, dims=dims, win=win, kind=kind, level=level)


def standard_specs(n, nk):
    """The compute window, both staggered windows, the whole logical storage, a plane of a 2-D field, a plane at level nk - 1 of
    a 3-D field, an item of 2 x 1 x 1."""
    return [spec("c", XYZ, (3, 3, 0, n, n, nk)), spec("v", XIYZ, (3, 3, 0, n + 1, n, nk)), spec("u", XYIZ, (3, 3, 0, n, n + 1, nk)),
            spec("whole", XYZI, (0, 0, 0, n + 7, n + 7, nk + 1)), spec("phis", XY, (3, 3, 0, n, n, 1), PLANE),
            spec("c", XYZ, (3, 3, 0, n, n, 1), PLANE, level=nk - 1), spec("tiny", XYZ, (4, 5, nk - 1, 2, 1, 1)),
            spec("phis", XY, (2, 1, 0, n + 5, 3, 1), PLANE)]


def many_specs(n, nk, count):
    """`count` items of mixed kind: four 3-D windows, planes on levels of 3-D fields and on 2-D fields."""
    specs = []
    for m in range(count):
        if m % 8 == 0:
            dims = (XYZ, XIYZ, XYIZ, XYZI)[(m // 8) % 4]
            specs.append(spec(f"vol{m}", dims, (3, 3, 0, n + (dims == XIYZ), n + (dims == XYIZ), nk + (dims == XYZI))))
        elif m % 2 == 1:
            specs.append(spec("full", XYZI, (m % 5, m % 3, 0, n + 7 - m % 5, n + 7 - m % 3 - m % 4, 1), PLANE, level=(m * 7) % (nk + 1)))
        else:
            specs.append(spec(f"plane{m % 6}", XY, (3, 3, 0, n - m % 3, n, 1), PLANE))
    return specs


class Packer:
    """The fields of one shape and library (made once, only read) and the runs over them."""

    def __init__(self, lib, device, n, nk):
        self.f = td.Fields(lib, device, n, nk)
        self.fields = {}

    def field(self, name, dims):
        if name not in self.fields:
            f = self.f
            q, a = f.quantity(dims, window=tuple(slice(0, s) for s in f.qf.sizer.get_shape(dims)))
            flat = a.reshape(-1)
            values = specials(f.dtype)
            flat[np.linspace(0, flat.size - 1, len(values)).astype(int)] = values
            # (through a view of integers: a NaN's payload must arrive in the storage as it is here)
            import torch

            as_int = torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if f.dtype == np.float32 else np.int64)).to(f.device)
            q.data.view(as_int.dtype)[...] = as_int
            a.setflags(write=False)
            self.fields[name] = (q, a)
        return self.fields[name]

    def expected(self, s, out_type):
        """(big-endian bytes, native bit patterns as uint64) of an item."""
        _, a = self.field(s["field"], s["dims"])
        i0, j0, k0, ni, nj, nk = s["win"]
        if s["kind"] == WINDOW3D:
            w = a[i0:i0 + ni, j0:j0 + nj, k0:k0 + nk].transpose(2, 1, 0)
        else:
            w = (a[:, :, s["level"]] if a.ndim == 3 else a)[i0:i0 + ni, j0:j0 + nj].transpose(1, 0)
        with np.errstate(over="ignore", under="ignore"):
            file = np.ascontiguousarray(w).astype(">f8" if out_type == BE_F64 else ">f4")
        native = file.astype(file.dtype.newbyteorder("=")).view(np.uint64 if out_type == BE_F64 else np.uint32).reshape(-1)
        return file.tobytes(), native.astype(np.uint64), np.isnan(file).reshape(-1)

    def run(self, specs, out_type, with_out=True, with_sums=True, through_host=False):
        import torch

        from pace_amd import _lib
        from pace_amd.util import restart

        f = self.f
        esize = 8 if out_type == BE_F64 else 4
        exact_nan = out_type == BE_F64 and f.lib.real_bytes == 8  # float64 -> BE_F64 moves bits: payloads are asserted
        expected = [self.expected(s, out_type) for s in specs]
        # the items one after the other; without guard pages a lead, gaps and a tail of sentinel bytes, whose sizes put the items
        # at every alignment an element offset can have
        offsets, total = [], 0
        for m, (data, _, _) in enumerate(expected):
            if not GUARDED:  # a gap of at least one element, up to the next offset that is (m + 1) elements past a 16-byte boundary
                total += esize
                total += (esize * (m + 1) - total) % 16
            offsets.append(total)
            total += len(data)
        total += 0 if GUARDED else 40
        # (int32: a type the guard pages' allocator knows; every size here is a multiple of 4 bytes)
        out = torch.full((total // 4,), SENTINEL_WORD, dtype=torch.int32, device=f.device)
        sums = torch.full((len(specs) + 2,), -77, dtype=torch.int64, device=f.device)
        if with_out and not GUARDED and len(specs) > 3:
            alignments = {(out.data_ptr() + o) % 16 for o in offsets}
            assert alignments >= ({0, 8} if esize == 8 else {0, 4, 8, 12}), alignments
        windows = []
        for s in specs:
            q, _ = self.field(s["field"], s["dims"])
            windows.append((q.ptr + s["level"] * f.geom.sk * f.lib.real_bytes, s["kind"]) + tuple(s["win"]))
        stream = None if f.device == "cpu" else C.c_void_p(torch.cuda.current_stream().cuda_stream)
        out_ptr = out.data_ptr() if with_out else None
        sums_ptr = sums.data_ptr() + 8 if with_sums else None
        if through_host:
            workspace = restart._pack(f.lib, f.geom, windows, offsets, out_type, out_ptr, sums_ptr, f.device, stream)
        else:
            assert len(specs) <= _lib.RESTART_MAX_ITEMS
            items = (_lib.RestartItem * len(specs))()
            for item, window, offset in zip(items, windows, offsets):
                item.field, item.kind, item.i0, item.j0, item.k0, item.ni, item.nj, item.nk = window
                item.out_offset = offset
            need = int(f.lib.cdll.pace_restart_pack_workspace_bytes(C.byref(f.geom), items, len(specs)))
            assert need >= 8 * len(specs)
            assert need % 8 == 0
            workspace = torch.full((need // 8 if with_sums else 1,), -1, dtype=torch.int64, device=f.device)  # (exactly: guarded)
            f.lib.call("pace_restart_pack", C.byref(f.geom), items, len(specs), out_type, None if out_ptr is None else C.c_void_p(out_ptr),
                       None if sums_ptr is None else C.c_void_p(sums_ptr),
                       C.c_void_p(workspace.data_ptr()) if with_sums else None, stream)
        got = out.cpu().numpy().view(np.uint8)
        got_sums = sums.cpu().numpy().view(np.uint64)
        del workspace
        want = np.full(total, SENTINEL, dtype=np.uint8)
        if with_out:
            for offset, (data, _, nans) in zip(offsets, expected):
                want[offset:offset + len(data)] = np.frombuffer(data, dtype=np.uint8)
                if not exact_nan and nans.any():
                    # a NaN that is widened or narrowed stays a NaN; which payload it keeps is the converter's
                    elements = got[offset:offset + len(data)].view(">f8" if esize == 8 else ">f4")
                    assert np.isnan(elements[nans]).all(), (f.n, f.nk, out_type)
                    keep = np.repeat(nans, esize)
                    want[offset:offset + len(data)][keep] = got[offset:offset + len(data)][keep]
        same = got == want
        assert same.all(), (f.n, f.nk, f.dtype, out_type, int((~same).sum()), np.flatnonzero(~same)[:8], got[~same][:8], want[~same][:8])
        minus77 = np.array([-77], dtype=np.int64).view(np.uint64)[0]
        assert got_sums[0] == minus77 and got_sums[-1] == minus77
        if not with_sums:
            assert (got_sums == minus77).all()
            return
        for m, (offset, (data, native, nans)) in enumerate(zip(offsets, expected)):
            if not exact_nan and nans.any():
                if not with_out:
                    continue  # (nothing to take the NaNs' patterns from)
                native = native.copy()
                view = got[offset:offset + len(data)].view(">f8" if esize == 8 else ">f4")
                native[nans] = view.astype(view.dtype.newbyteorder("=")).view(np.uint64 if esize == 8 else np.uint32)[nans]
            assert got_sums[1 + m] == native.sum(dtype=np.uint64), (f.n, f.nk, f.dtype, out_type, m, specs[m])


def check_shape(lib, device, n, nk):
    p = Packer(lib, device, n, nk)
    specs = standard_specs(n, nk)
    for out_type in (BE_F64, BE_F32):
        p.run(specs, out_type)
        p.run(specs, out_type, with_sums=False)
        p.run(specs, out_type, with_out=False)
    if lib.real_bytes == 8:
        # the payload arrived: the item that holds the NaN, through the kernel alone
        s = spec("c", XYZ, (0, 0, 0, n + 7, n + 7, nk + 1))
        data, _, nans = p.expected(s, BE_F64)
        assert nans.any() and np.frombuffer(data, dtype=">u8")[nans].min() == 0x7FF800000BADC0DE
        p.run([s], BE_F64)


def check_many(lib, device, n, nk):
    p = Packer(lib, device, n, nk)
    for out_type in (BE_F64, BE_F32):
        p.run(many_specs(n, nk, 32), out_type)
        p.run(many_specs(n, nk, 33), out_type, through_host=True)


# ---- the kernel, emulated ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nk", SHAPES)
def test_restart_pack_emulated(emu_lib, emu_lib_f32, n, nk):
    check_shape(emu_lib, "cpu", n, nk)
    check_shape(emu_lib_f32, "cpu", n, nk)


def test_restart_pack_many_items_emulated(emu_lib, emu_lib_f32):
    check_many(emu_lib, "cpu", 13, 7)
    check_many(emu_lib_f32, "cpu", 13, 7)


@pytest.mark.parametrize("mode", ["over", "under"])
def test_restart_pack_with_guard_pages(mode):
    """The emulated cases of this file in a child pytest whose every allocation -- the fields, the output, the sums' workspace --
    ends at (over) or starts right after (under) an inaccessible page (tests/guard.py, tests/test_guard_pages.py): there the
    output has neither lead nor tail nor gaps, so a store before the first or past the last item's bytes ends the child, as
    does a read past a field's last row."""
    if GUARDED:
        return  # (this IS the child)
    import test_guard_pages

    passed, tail = test_guard_pages._guarded_pytest(mode, ["test_restart_pack.py"])
    for case in ["test_restart_pack_emulated[%d-%d]" % shape for shape in SHAPES] + ["test_restart_pack_many_items_emulated"]:
        assert any(t.endswith("::" + case) for t in passed), (case, tail)


# ---- argument errors ------------------------------------------------------------------------------------------------------------
def check_argument_errors(lib, device):
    import torch

    from pace_amd import _lib

    n, nk = 12, 7
    f = td.Fields(lib, device, n, nk)
    q, _ = f.quantity(XYZ)
    out = torch.zeros((n + 7) * (n + 7) * (nk + 1) + 8, dtype=torch.int64, device=device)
    sums = torch.zeros(_lib.RESTART_MAX_ITEMS, dtype=torch.int64, device=device)
    workspace = torch.zeros(1 << 13, dtype=torch.int64, device=device)
    stream = None if device == "cpu" else C.c_void_p(torch.cuda.current_stream().cuda_stream)
    everything = dict(out=out.data_ptr(), sums=sums.data_ptr(), workspace=workspace.data_ptr())

    def call(count, kind=WINDOW3D, win=(3, 3, 0, n, n, nk), offset=0, field=q.ptr, out_type=BE_F64, **pointers):
        p = {**everything, **pointers}
        items = (_lib.RestartItem * (_lib.RESTART_MAX_ITEMS + 1))()
        for item in items:
            item.field, item.kind, item.out_offset = field, kind, offset
            item.i0, item.j0, item.k0, item.ni, item.nj, item.nk = win
        lib.call("pace_restart_pack", C.byref(f.geom), items, count, out_type, *[None if p[k] is None else C.c_void_p(p[k])
                                                                                   for k in ("out", "sums", "workspace")], stream)

    call(1)  # the table itself is fine
    call(1, win=(0, 0, 0, n + 7, n + 7, nk + 1))  # the whole storage is a window
    call(1, kind=PLANE, win=(3, 3, 0, n, n, 1), offset=4, out_type=BE_F32)
    call(1, offset=8, out=None)
    call(1, sums=None, workspace=None)
    out_before, sums_before = out.clone(), sums.clone()
    bad = [dict(count=0), dict(count=_lib.RESTART_MAX_ITEMS + 1), dict(count=-1),
           dict(count=1, win=(0, 0, 0, n + 8, n, nk)), dict(count=1, win=(8, 3, 0, n, n, nk)), dict(count=1, win=(3, 8, 0, n, n, nk)),
           dict(count=1, win=(3, 3, 0, n, n + 5, nk)), dict(count=1, win=(3, 3, 0, n, n, nk + 2)), dict(count=1, win=(3, 3, 2, n, n, nk)),
           dict(count=1, win=(-1, 3, 0, n, n, nk)), dict(count=1, win=(3, -1, 0, n, n, nk)), dict(count=1, win=(3, 3, -1, n, n, nk)),
           dict(count=1, win=(3, 3, 0, 0, n, nk)), dict(count=1, win=(3, 3, 0, n, 0, nk)), dict(count=1, win=(3, 3, 0, n, n, 0)),
           dict(count=1, kind=PLANE, win=(3, 3, 0, n, n, 2)), dict(count=1, kind=PLANE, win=(3, 3, 1, n, n, 1)),
           dict(count=1, kind=2), dict(count=1, kind=3), dict(count=1, kind=-1),  # (a column integral is no restart variable)
           dict(count=1, out_type=2), dict(count=1, out_type=-1),
           dict(count=1, offset=-8), dict(count=1, offset=4), dict(count=1, offset=12), dict(count=1, offset=2, out_type=BE_F32),
           dict(count=1, field=None), dict(count=1, out=None, sums=None), dict(count=1, out=None, sums=None, workspace=None)]
    for kwargs in bad:
        with pytest.raises(_lib.PaceError, match="invalid argument"):
            call(**kwargs)
    items = (_lib.RestartItem * 1)()
    for args in ((None, items, 1), (C.byref(f.geom), None, 1)):
        with pytest.raises(_lib.PaceError, match="invalid argument"):
            lib.call("pace_restart_pack", *args, BE_F64, C.c_void_p(out.data_ptr()), C.c_void_p(sums.data_ptr()),
                     C.c_void_p(workspace.data_ptr()), stream)
    assert lib.cdll.pace_restart_pack_workspace_bytes(C.byref(f.geom), items, 1) == 0  # (an empty window)
    assert lib.cdll.pace_restart_pack_workspace_bytes(C.byref(f.geom), None, 1) == 0
    # a refused call wrote nothing: the output and the sums are what the accepted calls above left
    assert torch.equal(out, out_before) and torch.equal(sums, sums_before) and not (out_before == 0).all()


def test_argument_errors_emulated(emu_lib, emu_lib_f32):
    check_argument_errors(emu_lib, "cpu")
    check_argument_errors(emu_lib_f32, "cpu")


def test_header_and_binding_agree_on_the_entry_point():
    from pace_amd import _lib

    text = open(os.path.join(ROOT, "include", "pace_hip.h")).read()
    proto = re.search(r"\bint pace_restart_pack\s*\(([^;]*)\);", text).group(1)
    assert len(proto.split(",")) == len(_lib._PROTOS["pace_restart_pack"][1])
    assert int(re.search(r"#define PACE_RESTART_MAX_ITEMS (\d+)", text).group(1)) == _lib.RESTART_MAX_ITEMS == 32
    types = re.search(r"enum \{ PACE_RESTART_BE_F64 = (\d), PACE_RESTART_BE_F32 = (\d) \}", text).groups()
    assert tuple(int(k) for k in types) == (_lib.RESTART_BE_F64, _lib.RESTART_BE_F32) == (BE_F64, BE_F32)
    body = re.search(r"typedef struct \{([^}]*)\} pace_restart_item_t;", text).group(1)
    names = re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", body))
    assert names == [name for name, _ in _lib.RestartItem._fields_]
    assert C.sizeof(_lib.RestartItem) == 48
    assert {"pace_restart_pack", "pace_restart_pack_workspace_bytes"} <= set(_lib.EXPORTED_SYMBOLS)


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,nk", GPU_SHAPES)
def test_restart_pack_gpu(lib, lib_f32, n, nk):
    check_shape(lib, "cuda", n, nk)
    check_shape(lib_f32, "cuda", n, nk)


@pytest.mark.gpu
def test_restart_pack_many_items_gpu(lib, lib_f32):
    for n, nk in ((13, 7), (96, 79)):
        check_many(lib, "cuda", n, nk)
        check_many(lib_f32, "cuda", n, nk)


@pytest.mark.gpu
def test_argument_errors_gpu(lib, lib_f32):
    check_argument_errors(lib, "cuda")
    check_argument_errors(lib_f32, "cuda")
