"""pace_cube_regrid (pace_amd/csrc/k_regrid.hip): one launch regrids any number of variables of six storages to a list of points,
three weighted sources each, into one dense buffer.

* bit for bit against the numpy restatement of the contract (tests/latlon_reference.py) over the WHOLE dense buffer (sentinels
  between the items) and with the raw storages unchanged afterwards: C12, C13 and C68 (padded rows); 1, 7, 33 and 79 levels (a
  partial and full 32-level tiles); 40 points (less than one 64-point tile), 288 (four tiles and a partial one) and 72 x 36
  points x 79 levels x 18 items = 2214 tiles for a grid capped at 2048 workgroups, so that 166 workgroups take a second tile and
  reuse their LDS; tables built by pace_amd.util.latlon and synthetic ones (all three sources in one cell, three different
  tiles, a weight of exactly 0, rows in random order, weights that do not sum to 1): the kernel assumes nothing about the table
  beyond the contract; 3-D items with k0 > 0, planes of a 2-D field and of one level, and more items than one launch takes
  (the host wrapper cuts them); both libraries and both dense types;
* -0.0, a NaN, +-inf and a denormal planted in sources: a NaN or an inf source with weight 0 still yields NaN; compared as bits
  where the result is not NaN, as NaN-ness where it is;
* what the host refuses (check_regrid_items) and what the entry point refuses.

Every check is a function of the device; the CPU tier calls it with the emulation libraries, the GPU tier in a child process
with a time limit, as tests/test_cube_gather.py does."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import ROOT, build_emu, build_emu_f32  # noqa: E402
import latlon_reference  # noqa: E402

SENTINEL = -12345.0
H = 3
X, Y, ZI = "x", "y", "z_interface"
SPECIAL_CELLS = [(4, 5 + s) for s in range(5)]  # storage (i, j) of -0.0, NaN, +inf, -inf, the smallest denormal: every tile, every level


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
    dtype = np.dtype(dtype)
    return np.array([-0.0, np.nan, np.inf, -np.inf, np.finfo(dtype).smallest_subnormal], dtype=dtype)


class Cube:
    """Two 3-D variables and one 2-D variable of six tiles each; the raw storages are the sentinel outside the fields' points,
    random values inside with the special ones planted in the compute domain."""

    def __init__(self, lib, device, n, nz, seed):
        import torch

        from pace_amd import _lib
        from pace_amd.util import QuantityFactory, SubtileGridSizer

        self.n, self.nz, self.lib, self.device = n, nz, lib, device
        self.tdtype = torch.float64 if lib.real_bytes == 8 else torch.float32
        self.dtype = np.float64 if lib.real_bytes == 8 else np.float32
        qf = QuantityFactory(SubtileGridSizer(n, n, nz), device, self.tdtype)
        rng = np.random.default_rng(seed)
        self.vars = [[qf.zeros([X, Y, ZI], "") for _ in range(6)] for _ in range(2)] + [[qf.zeros([X, Y], "") for _ in range(6)]]
        for q in self.all():
            q._base[...] = SENTINEL
            a = (rng.random(q.shape) - 0.5).astype(self.dtype)
            for (i, j), v in zip(SPECIAL_CELLS, special_values(self.dtype)):
                a[i, j] = v
            q.data[...] = torch.as_tensor(a, device=device)
        self.geom = _lib.Geom(n, nz, qf.row_stride, 0, qf.level_stride)

    def all(self):
        return [q for v in self.vars for q in v]

    def raw(self):
        return [q._base.detach().cpu().numpy().copy() for q in self.all()]

    def arrays(self, v):
        return [q.data.detach().cpu().numpy() for q in self.vars[v]]


def synthetic_table(n, npoints, seed):
    """Rows the geometry would never give: sources anywhere in the compute domain, weights of any size, in random order; the
    first rows aim at the special cells."""
    from pace_amd.util import latlon

    rng = np.random.default_rng(seed)
    tile = rng.integers(0, 6, (npoints, 3))
    i = rng.integers(H + 2, H + n, (npoints, 3))  # (i >= 5: none of the random rows reads a special cell, at i = 4)
    j = rng.integers(H, H + n, (npoints, 3))
    w = rng.random((npoints, 3)) * 2.0 - 0.5
    neg0, nan, pinf, ninf, den = SPECIAL_CELLS
    rows = [
        ([2, 2, 2], [7, 7, 7], [9, 9, 9], [0.25, 0.25, 0.5]),                    # all three sources in one cell
        ([5, 0, 3], [6, 7, 8], [3, 4, 5], [1 / 3, 1 / 3, 1 / 3]),                # three different tiles
        ([0, 1, 2], [8, nan[0], 9], [8, nan[1], 9], [0.5, 0.0, 0.5]),            # a NaN source with weight 0: NaN
        ([0, 1, 2], [8, 8, pinf[0]], [8, 8, pinf[1]], [0.5, 0.5, 0.0]),          # +inf with weight 0: NaN
        ([3, 3, 3], [ninf[0], 9, 9], [ninf[1], 9, 10], [0.0, 1.0, 0.0]),         # -inf with weight 0: NaN
        ([0, 4, 5], [neg0[0]] * 3, [neg0[1]] * 3, [0.5, 0.25, 0.25]),            # -0.0 from every source: -0.0
        ([1, 1, 2], [den[0], 9, 9], [den[1], 9, 10], [1.0, 0.0, 0.0]),           # a denormal and exact zeros
        ([1, 2, 3], [pinf[0], ninf[0], 9], [pinf[1], ninf[1], 9], [1.0, 1.0, 1.0]),  # inf - inf: NaN
        ([4, 4, 4], [pinf[0], 9, 10], [pinf[1], 9, 10], [2.0, 0.5, 0.5]),        # inf
        ([0, 0, 0], [9, 10, 11], [9, 9, 9], [1.0, 0.0, 0.0]),                    # a weight of exactly 0 on finite sources
    ]
    at = rng.permutation(npoints)[:len(rows)]  # ... anywhere in the list
    for p, (t_, i_, j_, w_) in zip(at, rows):
        tile[p], i[p], j[p], w[p] = t_, i_, j_, w_
    return latlon.RegridTable(tile, i, j, w)


_built = {}


def built_table(n, grid):
    from pace_amd.util import gridgen, latlon

    if (n, grid) not in _built:
        t = gridgen.tiles(n, 7)
        lon = np.stack([x["lon_agrid"][H:H + n, H:H + n] for x in t])
        lat = np.stack([x["lat_agrid"][H:H + n, H:H + n] for x in t])
        _built[n, grid] = latlon.build_regrid_table(lon, lat, *latlon.LatLonGrid(*grid).targets())
    return _built[n, grid]


def item_list(nz, many=None):
    """(variable, level of a PLANE's plane or None, kind, k0, nk)"""
    from pace_amd import _lib

    W, P = _lib.DIAG_WINDOW3D, _lib.DIAG_PLANE
    if many:
        return [(m % 2, None, W, 0, nz) if many > 0 else (m % 3, m % (nz + 1) if m % 3 < 2 else None, P, 0, 1) for m in range(abs(many))]
    k0 = min(2, nz - 1)
    return [
        (0, None, W, 0, nz),                # every layer
        (1, None, W, 0, nz + 1),            # ... and the interface level
        (0, None, W, k0, nz + 1 - k0),      # k0 > 0, up to the storage's last level
        (1, None, W, nz // 2, 1),           # one level as a window
        (2, None, P, 0, 1),                 # a 2-D field
        (1, nz, P, 0, 1),                   # one level's plane
        (0, 0, P, 0, 1),
    ]


def make_items(s, spec, npoints, gap=3):
    """The items with `gap` unused dense elements between them (the buffer starts and ends with an item: under guard pages
    its first and last elements are the ones next to the inaccessible page); returns (items, dense elements)."""
    from pace_amd.util import latlon

    items, offset = [], 0
    for v, level, kind, k0, nk in spec:
        step = 0 if level is None else level * s.geom.sk * s.lib.real_bytes
        items.append(latlon.regrid_item([q.ptr + step for q in s.vars[v]], kind, k0, nk, offset))
        offset += npoints * nk + gap
    return items, offset - gap


def _guardable(buf, device):
    """The bytes of a table as a tensor on the device, through torch.as_tensor: tests/guard.py puts it next to an inaccessible
    page."""
    import torch

    return torch.as_tensor(np.frombuffer(bytes(buf), dtype=np.int64).copy(), device=device)


def expected(s, spec, items, table, total, dense_dtype):
    want = np.full(total, SENTINEL, dtype=dense_dtype)
    arrays = [s.arrays(v) for v in range(3)]
    for x, (v, level, _, k0, nk) in zip(items, spec):
        fields = arrays[v] if level is None else [a[:, :, level] for a in arrays[v]]
        ref = latlon_reference.regrid(fields, table.tile, table.i, table.j, table.w, k0, nk, dense_dtype)
        want[x.offset:x.offset + table.npoints * nk] = ref.reshape(-1)
    return want


def same(got, want):
    """Bits where the expected value is no NaN, NaN-ness where it is."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def kernel_case(lib, device, n, nz, dense_dtype, table, spec, seed, wrapper=False):
    import torch

    from pace_amd import _lib
    from pace_amd.util import latlon

    tdense = torch.float64 if dense_dtype == np.float64 else torch.float32
    s = Cube(lib, device, n, nz, seed)
    items, total = make_items(s, spec, table.npoints)
    before = s.raw()
    dense = torch.full((total,), SENTINEL, dtype=tdense, device=device)
    latlon.check_regrid_table(s.geom, table)
    points = _guardable(table.points().tobytes(), device)
    if wrapper:  # the host wrapper: one launch per PACE_REGRID_MAX_ITEMS items
        keep = latlon.launch_regrid(lib, s.geom, points, table.npoints, items, dense, _stream(device))
        assert len(keep) == -(-len(items) // _lib.REGRID_MAX_ITEMS)
    else:
        keep = _guardable(latlon.build_item_table(s.geom, table.npoints, items), device)
        lib.call("pace_cube_regrid", C.byref(s.geom), C.c_void_p(points.data_ptr()), table.npoints, C.c_void_p(keep.data_ptr()),
                 len(items), _lib.DENSE_F64 if dense_dtype == np.float64 else _lib.DENSE_F32, C.c_void_p(dense.data_ptr()),
                 _stream(device))
    if device != "cpu":
        torch.cuda.synchronize()
    got = dense.cpu().numpy()
    want = expected(s, spec, items, table, total, dense_dtype)
    assert same(got, want), (n, nz, dense_dtype, table.npoints, len(items), int((_bits(got) != _bits(want)).sum()))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(before, s.raw()))
    return got, want


def check_kernel(device, only=None, big=True):
    from pace_amd import _lib

    seed = 0
    for which, lib in enumerate(_libs(device)):
        for dense_dtype in (np.float64, np.float32):
            if only is not None and only != (which, dense_dtype):
                continue
            seed += 10
            kernel_case(lib, device, 12, 79, dense_dtype, built_table(12, (8, 5)), item_list(79), seed)
            kernel_case(lib, device, 13, 7, dense_dtype, built_table(13, (24, 12)), item_list(7), seed + 1)
            kernel_case(lib, device, 13, 1, dense_dtype, synthetic_table(13, 288, seed), item_list(1), seed + 2)
            kernel_case(lib, device, 68, 33, dense_dtype, built_table(68, (24, 12)), item_list(33), seed + 3)
            got, want = kernel_case(lib, device, 68, 33, dense_dtype, synthetic_table(68, 40, seed), item_list(33), seed + 4)
            assert np.isnan(want).sum() >= 4 * 33 and (np.signbit(want) & (want == 0)).any() and np.isinf(want).any()
            kernel_case(lib, device, 12, 7, dense_dtype, synthetic_table(12, 40, seed), item_list(7, many=-(_lib.REGRID_MAX_ITEMS + 6)),
                        seed + 5, wrapper=True)
            if big:  # 41 x 3 tiles per item, 18 items: 2214 tiles on 2048 workgroups
                kernel_case(lib, device, 12, 79, dense_dtype, built_table(12, (72, 36)), item_list(79, many=18), seed + 6)


def check_refusals(device):
    import torch

    from pace_amd import _lib
    from pace_amd.util import latlon

    lib = _libs(device)[0]
    s = Cube(lib, device, 12, 7, 1)
    geom = s.geom
    ptrs = [q.ptr for q in s.vars[0]]

    def item(**kw):
        x = latlon.regrid_item(ptrs, _lib.DIAG_WINDOW3D, 0, 7, 0)
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    latlon.check_regrid_items(geom, 40, [item(), item(k0=1, nk=7), item(kind=_lib.DIAG_PLANE, nk=1)])
    nullfield = item()
    nullfield.field[4] = None
    for bad in (item(kind=2), item(k0=-1), item(nk=0), item(k0=2), item(nk=9), item(offset=-1), item(kind=_lib.DIAG_PLANE),
                item(kind=_lib.DIAG_PLANE, nk=1, k0=1), nullfield):
        with pytest.raises(ValueError):
            latlon.check_regrid_items(geom, 40, [item(), bad])
    with pytest.raises(ValueError, match="items"):
        latlon.check_regrid_items(geom, 40, [])
    with pytest.raises(ValueError, match="items"):
        latlon.check_regrid_items(geom, 40, [item()] * (_lib.REGRID_MAX_ITEMS + 1))
    # the prefix table behind the items
    items = [item(), item(kind=_lib.DIAG_PLANE, nk=1), item(k0=0, nk=8)]
    assert [latlon.regrid_tiles(288, x) for x in items] == [5, 5, 5] and latlon.regrid_tiles(2592, item(nk=79)) == 123
    geom79 = _lib.Geom(12, 79, geom.sj, 0, geom.sk)
    buf = bytes(latlon.build_item_table(geom79, 65, [item(), item(kind=_lib.DIAG_PLANE, nk=1), item(nk=33)]))
    assert len(buf) % 8 == 0 and C.sizeof(_lib.RegridItem) == 72
    assert list(np.frombuffer(buf, np.int32, 4, 3 * 72)) == [0, 2, 4, 8]
    # the entry point: what it can see
    dense = torch.zeros(64, dtype=torch.float64, device=device)
    table = torch.zeros(64, dtype=torch.int64, device=device)
    g, st = C.byref(geom), _stream(device)
    t, d = C.c_void_p(table.data_ptr()), C.c_void_p(dense.data_ptr())
    for args in ((g, t, 0, t, 1, _lib.DENSE_F64, d, st), (g, t, -1, t, 1, _lib.DENSE_F64, d, st),
                 (g, t, 1, t, 0, _lib.DENSE_F64, d, st), (g, t, 1, t, -1, _lib.DENSE_F64, d, st),
                 (g, t, 1, t, _lib.REGRID_MAX_ITEMS + 1, _lib.DENSE_F64, d, st), (g, t, 1, t, 1, 2, d, st), (g, t, 1, t, 1, -1, d, st),
                 (None, t, 1, t, 1, _lib.DENSE_F64, d, st), (g, None, 1, t, 1, _lib.DENSE_F64, d, st),
                 (g, t, 1, None, 1, _lib.DENSE_F64, d, st), (g, t, 1, t, 1, _lib.DENSE_F64, None, st)):
        with pytest.raises(_lib.PaceError, match="invalid argument"):
            lib.call("pace_cube_regrid", *args)


@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
@pytest.mark.parametrize("dense_dtype", [np.float64, np.float32], ids=["dense64", "dense32"])
def test_kernel_against_numpy_emulated(library, dense_dtype):
    check_kernel("cpu", (library, dense_dtype))


def test_refusals_emulated():
    check_refusals("cpu")


def test_header_and_binding_agree_on_the_entry_point():
    from pace_amd import _lib
    from pace_amd.util import latlon

    text = open(os.path.join(ROOT, "include", "pace_hip.h")).read()
    proto = re.search(r"\bint pace_cube_regrid\s*\(([^;]*)\);", text).group(1)
    assert len(proto.split(",")) == len(_lib._PROTOS["pace_cube_regrid"][1]) == 8
    assert "pace_cube_regrid" in _lib.EXPORTED_SYMBOLS
    assert int(re.search(r"#define PACE_REGRID_MAX_ITEMS (\d+)", text).group(1)) == _lib.REGRID_MAX_ITEMS == 1024
    for struct, cls, size in (("pace_regrid_point_t", _lib.RegridPoint, 64), ("pace_regrid_item_t", _lib.RegridItem, 72)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, text).group(1)
        fields = re.findall(r"(\w+)(?:\[(\d)\])?\s*[;,]", re.sub(r"/\*.*?\*/", "", body))
        assert [(name, int(count or 1)) for name, count in fields] == [(name, getattr(t, "_length_", 1)) for name, t in cls._fields_], struct
        assert C.sizeof(cls) == size
    assert latlon.POINT_DTYPE.itemsize == 64 and [latlon.POINT_DTYPE.fields[name][1] for name, _ in _lib.RegridPoint._fields_] == [
        getattr(_lib.RegridPoint, name).offset for name, _ in _lib.RegridPoint._fields_]
    maps = open(os.path.join(ROOT, "pace_amd", "csrc", "wgmap.h")).read()
    ti, ts = (int(re.search(rf"^#define {name} (\d+)$", maps, re.M).group(1)) for name in ("WT_TI", "WT_TS"))
    assert (ti, ts) == (latlon.REGRID_TILE_P, latlon.REGRID_TILE_S) == (64, 32)
    cap = int(re.search(r"#define RG_MAX_GRID (\d+)", open(os.path.join(ROOT, "pace_amd", "csrc", "k_regrid.hip")).read()).group(1))
    assert 18 * latlon.regrid_tiles(72 * 36, _lib.RegridItem(kind=_lib.DIAG_WINDOW3D, nk=79)) == 2214 > cap == 2048


# ---- the GPU tier: each check in a child process with a time limit --------------------------------------------------------------
def _in_child(what, timeout=300):
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); "
            f"import test_cube_regrid; test_cube_regrid.check_{what}('cuda')")
    p = subprocess.run([sys.executable, "-X", "faulthandler", "-c", code], capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-6000:])


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["kernel", "refusals"])
def test_on_the_gpu(what):
    _in_child(what)
