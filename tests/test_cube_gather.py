"""pace_cube_gather / pace_cube_scatter (pace_amd/csrc/k_gather.hip): one launch moves windows of any number of fields of six
storages between the fields and one dense buffer in (x, y, z) C order.

* both kernels bit for bit against a numpy slice restatement, over the WHOLE dense buffer and the WHOLE raw storages (sentinels
  everywhere else): C12, C13 (13 + 1 interface points: a partial 64-wide tile) and C68 (two tiles in i, one partial); 1, 7, 33
  and 79 levels (a partial and full 32-level tiles); centred, x-, y- and z-interface windows, planes of a 2-D field and of one
  level, a window that starts in the halo, and 40 items in one call spread over the six storages; both libraries and both dense
  types; -0.0, NaN (with a payload), inf and a denormal; and the whole storages of six C68 x 79 fields, 2700 tiles for a grid
  capped at 2048 workgroups, so that 652 workgroups take a second tile and reuse their LDS;
* scatter after gather is the identity on the windows;
* what the host refuses (pace_amd.util.gather.check_cube_items) and what the entry point refuses.

Every check is a function of the device; the CPU tier calls it with the emulation libraries, the GPU tier in a child process
with a time limit, as tests/test_halo_cube.py does."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import ROOT, build_emu, build_emu_f32  # noqa: E402

SENTINEL = -12345.0
X, Y, Z, ZI = "x", "y", "z", "z_interface"
CASES = ((12, 79), (13, 7), (13, 1), (68, 33))  # (n, levels)


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


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def special_values(dtype):
    """-0.0, a NaN with a payload, +inf, -inf, the smallest denormal."""
    dtype = np.dtype(dtype)
    nan = np.array([0x7FF8000000ABCDEF], np.uint64).view(np.float64) if dtype == np.float64 else np.array([0x7FC0ABCD], np.uint32).view(np.float32)
    return np.array([-0.0, nan[0], np.inf, -np.inf, np.finfo(dtype).smallest_subnormal], dtype=dtype)


class Storages:
    """Six 3-D fields and one 2-D field of one geometry whose whole raw storage is the sentinel (values=False), or random
    values with the special ones planted in the halo corner and in the compute domain."""

    def __init__(self, lib, device, n, nz, seed, values=True):
        import torch

        from pace_amd import _lib
        from pace_amd.util import QuantityFactory, SubtileGridSizer

        self.n, self.nz, self.lib, self.device = n, nz, lib, device
        self.tdtype = torch.float64 if lib.real_bytes == 8 else torch.float32
        self.dtype = np.float64 if lib.real_bytes == 8 else np.float32
        qf = QuantityFactory(SubtileGridSizer(n, n, nz), device, self.tdtype)
        rng = np.random.default_rng(seed)
        self.q = [qf.zeros([X, Y, ZI], "") for _ in range(6)] + [qf.zeros([X, Y], "")]
        for q in self.q:
            q._base[...] = SENTINEL
            if values:
                a = (rng.random(q.shape) - 0.5).astype(self.dtype)
                a.reshape(-1)[:5] = special_values(self.dtype)  # (0, 0, 0 .. 4): the halo corner
                a[(4, slice(5, 10)) + (0,) * (a.ndim - 2)] = special_values(self.dtype)  # ... and the compute domain
                q.data[...] = torch.as_tensor(a, device=device)
        self.geom = _lib.Geom(n, nz, qf.row_stride, 0, qf.level_stride)

    def raw(self):
        return [q._base.detach().cpu().numpy().copy() for q in self.q]

    def arrays(self):
        """The fields indexed [i, j, k] (2-D: [i, j, 0]), row padding excluded."""
        out = [q.data.detach().cpu().numpy() for q in self.q]
        return [a if a.ndim == 3 else a[:, :, None] for a in out]


def item_list(s, many=False):
    """(storage index, level of a PLANE's plane or None, kind, window) -- no two windows of one storage overlap."""
    from pace_amd import _lib

    n, nz = s.n, s.nz
    W, P = _lib.DIAG_WINDOW3D, _lib.DIAG_PLANE
    if many == "whole":  # the whole storage of each 3-D field: at C68 x 79, 2 x 3 x 75 = 450 tiles each, 2700 past the grid's 2048
        return [(f, None, W, (0, 0, 0, n + 7, n + 7, nz + 1)) for f in range(6)]
    if many:  # 40 items, past the old cap of 32 of the by-value tables: rows of two, seven per storage
        out = []
        for m in range(40):
            f, q = m % 6, m // 6
            out.append((f, None, W, (q % 3, 2 * q, 0, n + 7 - q % 3 - q % 2, 2, nz + (q % 2))))
        return out
    kk = min(nz, 3)
    return [
        (0, None, W, (3, 3, 0, n, n, nz)),          # centred
        (1, None, W, (3, 3, 0, n + 1, n, nz)),      # x-interface
        (2, None, W, (3, 3, 0, n, n + 1, nz)),      # y-interface
        (3, None, W, (3, 3, 0, n, n, nz + 1)),      # z-interface
        (4, None, W, (1, 0, 0, n + 2, 5, kk)),      # starts in the halo
        (4, nz, P, (3, 3, 0, n, n, 1)),             # one level's plane (the interface level the window above leaves alone)
        (5, None, W, (0, 0, 0, n + 7, n + 7, nz + 1)),  # the whole storage
        (6, None, P, (3, 3, 0, n + 1, n + 1, 1)),   # a 2-D field, both interfaces
    ]


def make_items(s, spec, gap=3):
    """The table entries with `gap` unused dense elements in front of every item; returns (items, dense elements)."""
    from pace_amd import _lib

    items, offset = [], 0
    for f, level, kind, (i0, j0, k0, ni, nj, nk) in spec:
        x = _lib.CubeItem()
        x.field = s.q[f].ptr + (0 if level is None else level * s.geom.sk * s.lib.real_bytes)
        x.kind, x.i0, x.j0, x.k0, x.ni, x.nj, x.nk = kind, i0, j0, k0, ni, nj, nk
        offset += gap
        x.offset = offset
        offset += ni * nj * nk
        items.append(x)
    return items, offset + gap


def window_of(arrays, f, level, w):
    i0, j0, k0, ni, nj, nk = w
    if level is not None:
        k0 = level
    return arrays[f][i0:i0 + ni, j0:j0 + nj, k0:k0 + nk]


def launch(s, name, items, dense, scatter):
    from pace_amd import _lib
    from pace_amd.util import gather, halo

    buf = gather.build_cube_table(s.geom, items, scatter=scatter)
    keep = halo._upload_table(buf, dense.device)
    code = _lib.DENSE_F64 if dense.element_size() == 8 else _lib.DENSE_F32
    s.lib.call(name, C.byref(s.geom), C.c_void_p(keep[0].data_ptr()), len(items), code, C.c_void_p(dense.data_ptr()), _stream(s.device))
    if s.device != "cpu":
        import torch

        torch.cuda.synchronize()
    return keep


def kernel_case(lib, device, n, nz, dense_dtype, many, seed):
    import torch

    tdense = torch.float64 if dense_dtype == np.float64 else torch.float32
    # gather: dense is the sentinel outside the items, the cast windows inside; the storages are not touched
    s = Storages(lib, device, n, nz, seed)
    spec = item_list(s, many)
    items, total = make_items(s, spec)
    before = s.raw()
    dense = torch.full((total,), SENTINEL, dtype=tdense, device=device)
    launch(s, "pace_cube_gather", items, dense, False)
    want = np.full(total, SENTINEL, dtype=dense_dtype)
    arrays = s.arrays()
    with np.errstate(over="ignore", under="ignore"):
        for x, (f, level, _, w) in zip(items, spec):
            want[x.offset:x.offset + x.ni * x.nj * x.nk] = window_of(arrays, f, level, w).astype(dense_dtype).reshape(-1)
    got = dense.cpu().numpy()
    same = s.dtype == dense_dtype
    assert np.array_equal(_bits(got), _bits(want)) if same else np.array_equal(got, want, equal_nan=True), (n, nz, dense_dtype, many)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(before, s.raw()))
    # scatter: the storages are the sentinel outside the windows, the cast dense values inside; dense is not touched
    t = Storages(lib, device, n, nz, seed, values=False)
    items, total = make_items(t, spec)
    rng = np.random.default_rng(seed + 1000)
    src = (rng.random(total) - 0.5).astype(dense_dtype)
    src[items[0].offset:items[0].offset + 5] = special_values(dense_dtype)
    dense = torch.empty(total, dtype=tdense, device=device)
    dense.copy_(torch.from_numpy(src))
    launch(t, "pace_cube_scatter", items, dense, True)
    assert np.array_equal(_bits(dense.cpu().numpy()), _bits(src))
    want_fields = [np.full(a.shape, SENTINEL, dtype=t.dtype) for a in t.arrays()]
    with np.errstate(over="ignore", under="ignore"):
        for x, (f, level, _, w) in zip(items, spec):
            window_of(want_fields, f, level, w)[...] = src[x.offset:x.offset + x.ni * x.nj * x.nk].astype(t.dtype).reshape(x.ni, x.nj, x.nk)
    for f, (got_f, want_f) in enumerate(zip(t.arrays(), want_fields)):
        assert np.array_equal(_bits(got_f), _bits(want_f)) if same else np.array_equal(got_f, want_f, equal_nan=True), (n, nz, f)
    for q, raw in zip(t.q, t.raw()):  # the row padding behind the fields' points
        pad = raw.reshape((-1,) + raw.shape[-2:])[:, :, q.shape[0]:]
        assert (pad == SENTINEL).all()
    return len(items)


def check_kernel(device, only=None):
    seed = 0
    for which, lib in enumerate(_libs(device)):
        for dense_dtype in (np.float64, np.float32):
            if only is not None and only != (which, dense_dtype):
                continue
            for n, nz in CASES:
                seed += 1
                assert kernel_case(lib, device, n, nz, dense_dtype, False, seed) == 8
            assert kernel_case(lib, device, 12, 7, dense_dtype, True, seed) == 40
            assert kernel_case(lib, device, 68, 33, dense_dtype, True, seed) == 40
            assert kernel_case(lib, device, 68, 79, dense_dtype, "whole", seed) == 6


def check_round_trip(device):
    """scatter after gather is the identity on the windows: gather, overwrite the windows, scatter the dense buffer back."""
    import torch

    for lib in _libs(device):
        for many in (False, True):
            s = Storages(lib, device, 13, 33, 7)
            spec = item_list(s, many)
            items, total = make_items(s, spec)
            before = s.raw()
            dense = torch.full((total,), SENTINEL, dtype=s.tdtype, device=device)
            launch(s, "pace_cube_gather", items, dense, False)
            for (f, level, _, (i0, j0, k0, ni, nj, nk)) in spec:
                k0 = k0 if level is None else level
                idx = (slice(i0, i0 + ni), slice(j0, j0 + nj)) + ((slice(k0, k0 + nk),) if f < 6 else ())
                s.q[f].data[idx] = 1.0e30
            assert not all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(before, s.raw()))
            launch(s, "pace_cube_scatter", items, dense, True)
            assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(before, s.raw()))


def check_refusals(device):
    import torch

    from pace_amd import _lib
    from pace_amd.util.gather import build_cube_table, check_cube_items, cube_tiles

    lib = _libs(device)[0]
    s = Storages(lib, device, 12, 7, 1)
    geom = s.geom

    def item(**kw):
        x = _lib.CubeItem()
        x.field, x.kind, x.i0, x.j0, x.k0, x.ni, x.nj, x.nk, x.offset = s.q[0].ptr, _lib.DIAG_WINDOW3D, 3, 3, 0, 12, 12, 7, 0
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    check_cube_items(geom, [item()])
    check_cube_items(geom, [item(), item()])  # gather may read one window twice
    check_cube_items(geom, [item(), item(j0=15, nj=4, offset=2000)], scatter=True)
    for bad in (dict(i0=8), dict(j0=8), dict(k0=2), dict(i0=-1), dict(nk=9), dict(ni=0), dict(nj=0), dict(nk=0), dict(field=0),
                dict(offset=-1), dict(kind=2), dict(kind=_lib.DIAG_PLANE), dict(kind=_lib.DIAG_PLANE, nk=1, k0=1)):
        with pytest.raises(ValueError):
            check_cube_items(geom, [item(), item(**bad)])
    with pytest.raises(ValueError, match="overlap"):
        check_cube_items(geom, [item(), item(i0=14, j0=14, k0=6, ni=2, nj=2, nk=2, offset=5000)], scatter=True)
    check_cube_items(geom, [item(), item(field=s.q[1].ptr)], scatter=True)  # the same window of another field
    with pytest.raises(ValueError, match="items"):
        check_cube_items(geom, [])
    with pytest.raises(ValueError, match="items"):
        check_cube_items(geom, [item()] * (_lib.CUBE_MAX_ITEMS + 1))
    with pytest.raises(ValueError):
        build_cube_table(geom, [item(i0=8)])
    # the prefix table behind the items
    items = [item(), item(kind=_lib.DIAG_PLANE, nk=1, ni=13, nj=13), item(ni=19, nj=2, nk=8, i0=0)]
    assert [cube_tiles(x) for x in items] == [12, 1, 2]
    buf = bytes(build_cube_table(geom, items))
    assert len(buf) % 8 == 0 and C.sizeof(_lib.CubeItem) == 48
    assert list(np.frombuffer(buf, np.int32, 4, 3 * 48)) == [0, 12, 13, 15]
    # the entry point: what it can see
    dense = torch.zeros(64, dtype=torch.float64, device=device)
    table = torch.zeros(64, dtype=torch.int64, device=device)
    g, st = C.byref(geom), _stream(device)
    for name in ("pace_cube_gather", "pace_cube_scatter"):
        for args in ((g, C.c_void_p(table.data_ptr()), 0, _lib.DENSE_F64, C.c_void_p(dense.data_ptr()), st),
                     (g, C.c_void_p(table.data_ptr()), -1, _lib.DENSE_F64, C.c_void_p(dense.data_ptr()), st),
                     (g, C.c_void_p(table.data_ptr()), _lib.CUBE_MAX_ITEMS + 1, _lib.DENSE_F64, C.c_void_p(dense.data_ptr()), st),
                     (g, C.c_void_p(table.data_ptr()), 1, 2, C.c_void_p(dense.data_ptr()), st),
                     (g, None, 1, _lib.DENSE_F64, C.c_void_p(dense.data_ptr()), st),
                     (g, C.c_void_p(table.data_ptr()), 1, _lib.DENSE_F64, None, st),
                     (None, C.c_void_p(table.data_ptr()), 1, _lib.DENSE_F64, C.c_void_p(dense.data_ptr()), st)):
            with pytest.raises(_lib.PaceError, match="invalid argument"):
                lib.call(name, *args)


@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
@pytest.mark.parametrize("dense_dtype", [np.float64, np.float32], ids=["dense64", "dense32"])
def test_kernels_against_numpy_emulated(library, dense_dtype):
    check_kernel("cpu", (library, dense_dtype))


def test_round_trip_emulated():
    check_round_trip("cpu")


def test_refusals_emulated():
    check_refusals("cpu")


def test_header_and_binding_agree_on_the_entry_points():
    import re

    from pace_amd import _lib

    text = open(os.path.join(ROOT, "include", "pace_hip.h")).read()
    for name in ("pace_cube_gather", "pace_cube_scatter"):
        proto = re.search(rf"\bint {name}\s*\(([^;]*)\);", text).group(1)
        assert len(proto.split(",")) == len(_lib._PROTOS[name][1]) == 6, name
        assert name in _lib.EXPORTED_SYMBOLS
    assert int(re.search(r"#define PACE_CUBE_MAX_ITEMS (\d+)", text).group(1)) == _lib.CUBE_MAX_ITEMS == 4096
    codes = re.search(r"enum \{ PACE_DENSE_F64 = (\d), PACE_DENSE_F32 = (\d) \}", text).groups()
    assert tuple(int(x) for x in codes) == (_lib.DENSE_F64, _lib.DENSE_F32)
    body = re.search(r"typedef struct \{([^}]*)\} pace_cube_item_t;", text).group(1)
    names = re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", body))
    assert names == [name for name, _ in _lib.CubeItem._fields_]
    assert C.sizeof(_lib.CubeItem) == 48
    # the tile of the prefix table behind the items: the kernel's constants (csrc/wgmap.h) and their Python mirror
    from types import SimpleNamespace

    from pace_amd.util import gather

    maps = open(os.path.join(ROOT, "pace_amd", "csrc", "wgmap.h")).read()
    ti, ts = (int(re.search(rf"^#define {name} (\d+)$", maps, re.M).group(1)) for name in ("WT_TI", "WT_TS"))
    assert (ti, ts) == (gather.CUBE_TILE_I, gather.CUBE_TILE_S) == (64, 32)
    for n, nz in CASES + ((68, 79),):
        for many in (False, True, "whole"):
            for _, _, kind, (_, _, _, ni, nj, nk) in item_list(SimpleNamespace(n=n, nz=nz), many):
                x = _lib.CubeItem()
                x.kind, x.ni, x.nj, x.nk = kind, ni, nj, nk
                volume = kind == _lib.DIAG_WINDOW3D
                want = ((ni + ti - 1) // ti) * (((nk if volume else nj) + ts - 1) // ts) * (nj if volume else 1)
                assert gather.cube_tiles(x) == want, (n, nz, many, kind, ni, nj, nk)
    assert sum(gather.cube_tiles(SimpleNamespace(kind=_lib.DIAG_WINDOW3D, ni=75, nj=75, nk=80)) for _ in range(6)) == 2700 > 2048


# ---- the GPU tier: each check in a child process with a time limit --------------------------------------------------------------
def _in_child(what, timeout=300):
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); "
            f"import test_cube_gather; test_cube_gather.check_{what}('cuda')")
    p = subprocess.run([sys.executable, "-X", "faulthandler", "-c", code], capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-6000:])


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["kernel", "round_trip", "refusals"])
def test_on_the_gpu(what):
    _in_child(what)
