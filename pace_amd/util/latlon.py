"""Regridding the cubed sphere to a regular latitude-longitude grid: the table (host, numpy + scipy) and the launches of
``pace_cube_regrid`` (pace_amd/csrc/k_regrid.hip) that apply it.  The reference has no such operator; this is the horizontal
counterpart of ``p_select``: reduce on the device to what the user looks at, ship a fraction of the bytes.

Method: piecewise-linear interpolation on the spherical Delaunay triangulation of the 6 n^2 cell centres.  The triangulation is
the facets of the convex hull of their unit vectors (points on a sphere: every point is a hull vertex and the hull's facets are
the Delaunay triangles); it needs no knowledge of the cube's topology, the edges and the eight three-tile corners come out of
it.  A target's weights are the barycentric coordinates of its central projection onto its triangle's plane.

A table row names three source cells (tile, i, j) in STORAGE indices (the halo origin added), sorted ascending, and three float64
weights; the device applies ``(w0 * f0 + w1 * f1) + w2 * f2`` in float64 in this order (include/pace_hip.h).
"""
import ctypes as C

import numpy as np

from .. import _launch, _lib
from . import constants as c

REGRID_TILE_P, REGRID_TILE_S = 64, 32  # pace_amd/csrc/wgmap.h WT_TI, WT_TS: the points and levels of a workgroup's tile
NEIGHBOURS = 12  # candidate triangles per target: those with the nearest centroids
INSIDE = -1e-9  # the smallest barycentric coordinate a containing triangle may have (rounding at an edge or vertex)


class LatLonGrid:
    """Cell-centred targets of a regular grid, so that none lies at a pole: lon[i] = (i + 0.5) 2 pi / nlon,
    lat[j] = -pi / 2 + (j + 0.5) pi / nlat, point p = i * nlat + j ((lon, lat) in C order)."""

    def __init__(self, nlon: int, nlat: int):
        if int(nlon) < 1 or int(nlat) < 1:
            raise ValueError(f"a lat-lon grid has at least one point each way, not {nlon} x {nlat}")
        self.nlon, self.nlat = int(nlon), int(nlat)
        self.lon = (np.arange(self.nlon) + 0.5) * (2.0 * np.pi / self.nlon)
        self.lat = -0.5 * np.pi + (np.arange(self.nlat) + 0.5) * (np.pi / self.nlat)

    @property
    def npoints(self) -> int:
        return self.nlon * self.nlat

    def targets(self):
        """(lon, lat) of every point, in the points' order."""
        lon, lat = np.meshgrid(self.lon, self.lat, indexing="ij")
        return lon.reshape(-1), lat.reshape(-1)

    def __eq__(self, other):
        return isinstance(other, LatLonGrid) and (self.nlon, self.nlat) == (other.nlon, other.nlat)

    def __hash__(self):
        return hash((self.nlon, self.nlat))


class RegridTable:
    """npoints rows: tile, i, j (int32 [npoints, 3], storage indices) and w (float64 [npoints, 3])."""

    def __init__(self, tile, i, j, w):
        self.tile, self.i, self.j = (np.ascontiguousarray(a, dtype=np.int32) for a in (tile, i, j))
        self.w = np.ascontiguousarray(w, dtype=np.float64)
        if not (self.tile.shape == self.i.shape == self.j.shape == self.w.shape and self.w.ndim == 2 and self.w.shape[1] == 3):
            raise ValueError("a regrid table has [npoints, 3] tiles, i, j and weights")

    @property
    def npoints(self) -> int:
        return self.w.shape[0]

    def points(self):
        """The rows as the kernel reads them: a numpy view of pace_regrid_point_t[npoints]."""
        out = np.zeros(self.npoints, dtype=POINT_DTYPE)
        out["tile"], out["i"], out["j"], out["w"] = self.tile, self.i, self.j, self.w
        return out


POINT_DTYPE = np.dtype([("tile", "<i4", 3), ("i", "<i4", 3), ("j", "<i4", 3), ("pad_", "<i4"), ("w", "<f8", 3)])
assert POINT_DTYPE.itemsize == C.sizeof(_lib.RegridPoint) == 64


def unit_vectors(lon, lat):
    lon, lat = np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64)
    return np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], axis=-1)


def triangulate(lon_agrid6, lat_agrid6):
    """(unit vectors [6 n^2, 3] in (tile, i, j) C order, triangles [2 V - 4, 3] of point numbers).  Raises ValueError unless the
    hull has exactly 2 V - 4 facets (Euler's formula for a triangulated sphere with every point a vertex)."""
    from scipy.spatial import ConvexHull

    r = unit_vectors(np.asarray(lon_agrid6), np.asarray(lat_agrid6)).reshape(-1, 3)
    hull = ConvexHull(r)
    want = 2 * r.shape[0] - 4
    if hull.simplices.shape[0] != want or np.unique(hull.simplices).size != r.shape[0]:
        raise ValueError(f"the convex hull of the {r.shape[0]} cell centres has {hull.simplices.shape[0]} facets over "
                         f"{np.unique(hull.simplices).size} of them, not {want} over all: the centres are not distinct points of a "
                         "sphere")
    return r, hull.simplices


def build_regrid_table(lon_agrid6, lat_agrid6, lon_t, lat_t, origin=c.N_HALO_DEFAULT) -> RegridTable:
    """The table that regrids cell-centre fields of six tiles to the targets (lon_t, lat_t).

    lon_agrid6, lat_agrid6: [6, n, n] cell-centre coordinates of the compute domains [radians]; `origin` is added to the
    sources' (i, j): the compute domain's first cell in the storage.  No target is ever dropped: one without a containing
    triangle among the candidates raises ValueError naming it."""
    from scipy.spatial import cKDTree

    lon_agrid6, lat_agrid6 = np.asarray(lon_agrid6, dtype=np.float64), np.asarray(lat_agrid6, dtype=np.float64)
    if lon_agrid6.ndim != 3 or lon_agrid6.shape[0] != 6 or lon_agrid6.shape[1] != lon_agrid6.shape[2] or lat_agrid6.shape != lon_agrid6.shape:
        raise ValueError(f"the cell centres are two [6, n, n] arrays, not {lon_agrid6.shape} and {lat_agrid6.shape}")
    n = lon_agrid6.shape[1]
    r, tri = triangulate(lon_agrid6, lat_agrid6)
    p = unit_vectors(np.asarray(lon_t).reshape(-1), np.asarray(lat_t).reshape(-1))
    centroids = r[tri].sum(axis=1)
    centroids /= np.linalg.norm(centroids, axis=1, keepdims=True)
    k = min(NEIGHBOURS, tri.shape[0])
    _, near = cKDTree(centroids).query(p, k=k)
    near = near.reshape(p.shape[0], k)
    # [r0 r1 r2] w = p for every candidate, w /= sum(w): the barycentric coordinates of the central projection
    m = np.swapaxes(r[tri[near]], -1, -2)  # [points, candidates, 3 (xyz), 3 (vertices)]
    w = np.linalg.solve(m, np.broadcast_to(p[:, None, :, None], m.shape[:3] + (1,)))[..., 0]
    w /= w.sum(axis=-1, keepdims=True)
    best = np.argmax(w.min(axis=-1), axis=1)
    rows = np.arange(p.shape[0])
    w, vertices = w[rows, best], tri[near[rows, best]]
    bad = np.flatnonzero(~(w.min(axis=1) >= INSIDE))
    if bad.size:
        t = int(bad[0])
        raise ValueError(f"target {t} (lon {float(np.asarray(lon_t).reshape(-1)[t])!r}, lat {float(np.asarray(lat_t).reshape(-1)[t])!r}) "
                         f"lies in none of its {k} candidate triangles (smallest weight {w[t].min()!r}); {bad.size} such targets")
    w = np.maximum(w, 0.0)
    w /= w.sum(axis=1, keepdims=True)
    # the order of the sum must not depend on qhull's vertex order: ascending point number = ascending (tile, i, j)
    order = np.argsort(vertices, axis=1, kind="stable")
    vertices, w = np.take_along_axis(vertices, order, 1), np.take_along_axis(w, order, 1)
    tile, rest = np.divmod(vertices, n * n)
    i, j = np.divmod(rest, n)
    return RegridTable(tile, i + origin, j + origin, w)


def compute_domain(a, n, origin=c.N_HALO_DEFAULT):
    """The [n, n] compute domain of a tile's cell-centre array: the array itself, or the cut of a whole storage (a host array,
    or a Quantity on any device)."""
    a = a.data if hasattr(a, "dims") else a
    a = np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float64)
    if a.shape == (n, n):
        return a
    if a.ndim != 2 or min(a.shape) < origin + n:
        raise ValueError(f"the cell centres of a C{n} tile are [{n}, {n}] or a storage with a halo of {origin}, not {a.shape}")
    return a[origin:origin + n, origin:origin + n]


def levels_of(name, q, n):
    """(kind, k0, nk) of what regrid_state is handed under `name`: a Quantity with dims (x, y) or (x, y, z) over its compute
    domain, or a gather Window of such a field -- one level's plane, or a range of levels.  Anything else (staggered fields,
    interface fields) raises ValueError naming the variable and its dims."""
    centred = tuple(q.dims) in ((c.X_DIM, c.Y_DIM), (c.X_DIM, c.Y_DIM, c.Z_DIM))
    if not centred or tuple(q.origin[:2]) != (c.N_HALO_DEFAULT,) * 2 or tuple(q.extent[:2]) != (n, n):
        raise ValueError(f"{name} has dimensions {tuple(q.dims)} (origin {tuple(q.origin)}, extent {tuple(q.extent)}): regridding takes "
                         "cell-centre variables with dimensions (x, y) or (x, y, z) over the compute domain")
    if hasattr(q, "kind"):  # a gather Window
        return (q.kind, q.window[2], q.window[5]) if q.kind == _lib.DIAG_WINDOW3D else (q.kind, 0, 1)
    if len(q.dims) == 3:
        return _lib.DIAG_WINDOW3D, int(q.origin[2]), int(q.extent[2])
    return _lib.DIAG_PLANE, 0, 1


def check_regrid_table(geom, table: RegridTable):
    """The host checks of a pace_cube_regrid point table, before the upload (the entry point sees device memory only): at least
    one point, every tile 0 .. 5, every source inside the compute domain of the storage (a halo cell of a diagnostics step holds
    whatever the last exchange left there), every weight finite.  Raises ValueError."""
    if table.npoints < 1:
        raise ValueError("a regrid table holds at least one point")
    lo, hi = c.N_HALO_DEFAULT, c.N_HALO_DEFAULT + geom.n
    for name, a, first, last in (("tile", table.tile, 0, 6), ("i", table.i, lo, hi), ("j", table.j, lo, hi)):
        bad = np.argwhere((a < first) | (a >= last))
        if bad.size:
            p, m = (int(x) for x in bad[0])
            what = "is not one of the six tiles" if name == "tile" else f"lies outside the compute domain {lo} .. {hi - 1} of the storage"
            raise ValueError(f"regrid table point {p}, source {m}: {name} = {int(a[p, m])} {what}")
    bad = np.argwhere(~np.isfinite(table.w))
    if bad.size:
        p, m = (int(x) for x in bad[0])
        raise ValueError(f"regrid table point {p}, source {m}: the weight {float(table.w[p, m])!r} is not finite")


def regrid_tiles(npoints, item) -> int:
    """Workgroup tiles of one item (include/pace_hip.h: the prefix table behind the items counts these)."""
    nk = item.nk if item.kind == _lib.DIAG_WINDOW3D else 1
    return -(-npoints // REGRID_TILE_P) * -(-nk // REGRID_TILE_S)


def check_regrid_items(geom, npoints, items):
    """The host checks of a pace_cube_regrid item table of ONE launch: the count, the kind, a level range inside the storage's
    nk + 1 levels (a plane: k0 = 0, nk = 1), no NULL field, no negative offset, fewer than 2^31 tiles.  Raises ValueError."""
    if len(items) < 1 or len(items) > _lib.REGRID_MAX_ITEMS:
        raise ValueError(f"a regrid launch takes 1 .. {_lib.REGRID_MAX_ITEMS} items, not {len(items)}")
    tiles = 0
    for t, x in enumerate(items):
        if x.kind not in (_lib.DIAG_WINDOW3D, _lib.DIAG_PLANE):
            raise ValueError(f"regrid item {t}: kind {x.kind} is neither a 3-D window nor a plane")
        if not all(x.field[r] for r in range(6)):
            raise ValueError(f"regrid item {t}: null field")
        if x.offset < 0:
            raise ValueError(f"regrid item {t}: negative offset {x.offset}")
        if x.kind == _lib.DIAG_PLANE and (x.k0 != 0 or x.nk != 1):
            raise ValueError(f"regrid item {t}: a plane has k0 = 0 and nk = 1")
        if x.k0 < 0 or x.nk < 1 or x.k0 + x.nk > geom.nk + 1:
            raise ValueError(f"regrid item {t}: the levels {x.k0} + {x.nk} lie outside the storage's {geom.nk + 1}")
        tiles += regrid_tiles(npoints, x)
    if tiles >= 2 ** 31:
        raise ValueError(f"{tiles} tiles in one regrid launch")


def build_item_table(geom, npoints, items):
    """The bytes of one launch's item table as the kernel reads it: the items, then int32 first[n + 1], the prefix sums of their
    tile counts (padded to 8-byte units for the upload).  Checks the items first."""
    check_regrid_items(geom, npoints, items)
    n = len(items)
    item_bytes = C.sizeof(_lib.RegridItem) * n
    buf = (C.c_uint8 * ((item_bytes + 4 * (n + 1) + 7) // 8 * 8))()
    C.memmove(buf, (_lib.RegridItem * n)(*items), item_bytes)
    first = np.zeros(n + 1, dtype=np.int32)
    first[1:] = np.cumsum([regrid_tiles(npoints, x) for x in items])
    C.memmove(C.addressof(buf) + item_bytes, first.ctypes.data, first.nbytes)
    return buf


def upload_points(geom, table: RegridTable, device):
    """The checked point table on the device: the tensors to keep alive with it (device copy first)."""
    check_regrid_table(geom, table)
    pts = table.points()
    return _launch.upload_table((C.c_uint8 * pts.nbytes).from_buffer(pts), device)


def regrid_item(pointers, kind, k0, nk, offset):
    """One variable -- its six tiles' pointers (a plane's: at the plane) -- as an item at `offset` elements of the dense
    buffer."""
    x = _lib.RegridItem()
    for r, ptr in enumerate(pointers):
        x.field[r] = ptr
    x.kind, x.k0, x.nk, x.offset = kind, int(k0), int(nk), int(offset)
    return x


def launch_regrid(lib, geom, points_on_device, npoints, items, dense, stream, tables=None):
    """ONE pace_cube_regrid launch per PACE_REGRID_MAX_ITEMS items into `dense` (a float64 or float32 tensor on the tables'
    device).  `tables`: uploaded item tables of an earlier call with the same items, to use again; returns them (keep them
    alive until the launches have run)."""
    code = _lib.DENSE_F64 if dense.element_size() == 8 else _lib.DENSE_F32
    if tables is None:
        tables = [(_launch.upload_table(build_item_table(geom, npoints, chunk), dense.device), len(chunk))
                  for _, chunk in _launch.chunks(items, _lib.REGRID_MAX_ITEMS)]
    for keep, n in tables:
        lib.call("pace_cube_regrid", C.byref(geom), C.c_void_p(points_on_device.data_ptr()), int(npoints),
                 C.c_void_p(keep[0].data_ptr()), n, code, C.c_void_p(dense.data_ptr()), stream)
    return tables
