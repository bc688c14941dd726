"""The regridding table of the lat-lon diagnostics (pace_amd/util/latlon.py): the host geometry, on the CPU.

* the spherical Delaunay triangulation of the cell centres at C12 and C13: 2 V - 4 facets (1724 and 2024), exactly 8 triangles
  that span three tiles (the cube's corners) and 24 (n - 1) that span two (264 and 288);
* every target of a 90 x 45 and a 72 x 36 grid finds a triangle; all weights >= 0, every row sums to 1 within 4e-16, the sources
  lie in the compute domain and are sorted by (tile, i, j);
* targets at the eight cube corners get three different tiles with weights 1/3 (within 1e-12), targets at cell centres -- an
  interior cell, one on a tile edge, one at a tile corner -- weight 1 on that cell (within 1e-12: machine epsilon times the
  triangle matrix's condition number, about 1 / h^2 = 60 at C12, is 1.3e-14; the rest is margin);
* a field linear in Cartesian coordinates, f = a . r, comes back with |result - a . p| <= |a| (1 - cos delta_p) + 1e-15, where
  delta_p is the largest angle between the target and its three sources -- derived, not measured: the weighted sum of the sources
  is s p with cos delta_p <= s <= 1; a constant field comes back within 2 ulp;
* what is refused: a hull with the wrong facet count (a duplicated centre), and by check_regrid_table a source in the halo,
  tile 6 and a NaN weight."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import ROOT  # noqa: E402,F401
import latlon_reference  # noqa: E402

H = 3  # the halo: the compute domain's first cell in the storage
GRIDS = ((90, 45), (72, 36))
_cache = {}


def centres(n):
    """(lon_agrid6, lat_agrid6, the six tiles' metric terms) of Cn."""
    from pace_amd.util import gridgen

    if n not in _cache:
        t = gridgen.tiles(n, 7)
        _cache[n] = (np.stack([x["lon_agrid"][H:H + n, H:H + n] for x in t]), np.stack([x["lat_agrid"][H:H + n, H:H + n] for x in t]), t)
    return _cache[n]


def table_of(n, grid):
    from pace_amd.util import latlon

    key = (n, grid)
    if key not in _cache:
        lon, lat, _ = centres(n)
        _cache[key] = latlon.build_regrid_table(lon, lat, *latlon.LatLonGrid(*grid).targets())
    return _cache[key]


def source_vectors(n, table):
    """The unit vectors [npoints, 3, 3] of a table's sources."""
    from pace_amd.util import latlon

    lon, lat, _ = centres(n)
    return latlon.unit_vectors(lon, lat)[table.tile, table.i - H, table.j - H]


def test_the_grid():
    from pace_amd.util import latlon

    g = latlon.LatLonGrid(8, 5)
    assert g.npoints == 40 and g.lon.shape == (8,) and g.lat.shape == (5,)
    assert np.allclose(g.lon, (np.arange(8) + 0.5) * 2 * np.pi / 8, rtol=0, atol=1e-15)
    assert np.allclose(g.lat, -np.pi / 2 + (np.arange(5) + 0.5) * np.pi / 5, rtol=0, atol=1e-15)
    assert np.abs(g.lat).max() < np.pi / 2  # no target at a pole
    lon, lat = g.targets()
    assert lon[1 * 5 + 2] == g.lon[1] and lat[1 * 5 + 2] == g.lat[2]  # p = i * nlat + j
    with pytest.raises(ValueError):
        latlon.LatLonGrid(0, 5)


@pytest.mark.parametrize("n,facets,two", [(12, 1724, 264), (13, 2024, 288)])
def test_triangulation(n, facets, two):
    from pace_amd.util import latlon

    lon, lat, _ = centres(n)
    r, tri = latlon.triangulate(lon, lat)
    assert r.shape == (6 * n * n, 3) and tri.shape == (facets, 3) and facets == 2 * 6 * n * n - 4
    tiles = np.sort(tri // (n * n), axis=1)
    spans = 1 + (tiles[:, 0] != tiles[:, 1]) + (tiles[:, 1] != tiles[:, 2])
    assert (spans == 3).sum() == 8
    assert (spans == 2).sum() == two == 24 * (n - 1)


@pytest.mark.parametrize("n", [12, 13])
@pytest.mark.parametrize("grid", GRIDS, ids=["90x45", "72x36"])
def test_table_properties(n, grid):
    t = table_of(n, grid)
    assert t.npoints == grid[0] * grid[1]  # no target left out
    assert t.w.dtype == np.float64 and t.tile.dtype == t.i.dtype == t.j.dtype == np.int32
    assert (t.w >= 0).all()
    assert np.abs(t.w.sum(axis=1) - 1.0).max() <= 4e-16
    assert t.tile.min() >= 0 and t.tile.max() <= 5
    assert min(t.i.min(), t.j.min()) >= H and max(t.i.max(), t.j.max()) < H + n
    key = (t.tile.astype(np.int64) * 1000 + t.i) * 1000 + t.j
    assert (np.diff(key, axis=1) > 0).all()  # sorted by (tile, i, j), three different cells


@pytest.mark.parametrize("n", [12, 13])
def test_targets_at_the_cube_corners(n):
    from pace_amd.util import latlon

    lon, lat, terms = centres(n)
    at = [(x["lon"][a, b], x["lat"][a, b]) for x in terms for a in (H, H + n) for b in (H, H + n)]
    p = latlon.unit_vectors(*np.array(at).T)
    corners = []
    for v in p:  # 24 tile corners: 8 different points
        if not any(np.linalg.norm(v - u) < 1e-9 for u in corners):
            corners.append(v)
    assert len(corners) == 8
    corners = np.array(corners)
    t = latlon.build_regrid_table(lon, lat, np.arctan2(corners[:, 1], corners[:, 0]), np.arcsin(corners[:, 2]))
    assert all(len(set(row)) == 3 for row in t.tile)
    print("corner weights: largest deviation from 1/3:", np.abs(t.w - 1 / 3).max())
    assert np.abs(t.w - 1 / 3).max() <= 1e-12


@pytest.mark.parametrize("n", [12, 13])
def test_targets_at_cell_centres(n):
    from pace_amd.util import latlon

    lon, lat, _ = centres(n)
    cells = [(2, 5, 6), (0, 0, 5), (4, n - 1, n - 1), (1, 0, 0), (3, 7, n - 1)]  # interior, tile edge, tile corner, ...
    t = latlon.build_regrid_table(lon, lat, [lon[c] for c in cells], [lat[c] for c in cells])
    for p, (tile, i, j) in enumerate(cells):
        hit = (t.tile[p] == tile) & (t.i[p] == i + H) & (t.j[p] == j + H)
        assert hit.sum() == 1, (cells[p], t.tile[p], t.i[p], t.j[p])
        print("cell", cells[p], "weight - 1:", t.w[p][hit][0] - 1)
        assert abs(t.w[p][hit][0] - 1.0) <= 1e-12 and np.abs(t.w[p][~hit]).max() <= 1e-12


@pytest.mark.parametrize("n", [12, 13, 96])
def test_linear_and_constant_fields(n):
    from pace_amd.util import latlon

    lon, lat, _ = centres(n)
    grid = GRIDS[0]
    if n == 96:
        t = latlon.build_regrid_table(lon, lat, *latlon.LatLonGrid(*grid).targets())
    else:
        t = table_of(n, grid)
    r = latlon.unit_vectors(lon, lat)  # [6, n, n, 3]
    p = latlon.unit_vectors(*latlon.LatLonGrid(*grid).targets())
    cos_delta = np.clip(np.einsum("pmc,pc->pm", source_vectors(n, t), p), -1.0, 1.0).min(axis=1)
    rng = np.random.default_rng(n)
    for _ in range(3):
        a = rng.normal(size=3)
        fields = [np.pad(r[tile] @ a, H) for tile in range(6)]  # storage indices: the halo in front
        got = latlon_reference.regrid(fields, t.tile, t.i, t.j, t.w)
        bound = np.linalg.norm(a) * (1.0 - cos_delta) + 1e-15
        assert (np.abs(got - p @ a) <= bound).all(), (n, np.abs(got - p @ a).max(), bound.max())
    const = 287.15
    got = latlon_reference.regrid([np.full((n + 7, n + 7), const)] * 6, t.tile, t.i, t.j, t.w)
    assert np.abs(got - const).max() <= 2 * np.spacing(const)


def test_refusals():
    from pace_amd import _lib
    from pace_amd.util import latlon

    lon, lat, _ = centres(12)
    lon2, lat2 = lon.copy(), lat.copy()
    lon2[0, 0, 1], lat2[0, 0, 1] = lon2[0, 0, 0], lat2[0, 0, 0]  # a duplicated centre: the hull loses a vertex and two facets
    with pytest.raises(ValueError, match="facets"):
        latlon.build_regrid_table(lon2, lat2, [1.0], [0.5])
    with pytest.raises(ValueError):
        latlon.build_regrid_table(lon[:5], lat[:5], [1.0], [0.5])
    geom = _lib.Geom(12, 7, 24, 0, 24 * 19)
    good = table_of(12, GRIDS[1])
    latlon.check_regrid_table(geom, good)

    def changed(**kw):
        cols = {name: getattr(good, name).copy() for name in ("tile", "i", "j", "w")}
        for name, value in kw.items():
            cols[name][17, 1] = value
        return latlon.RegridTable(cols["tile"], cols["i"], cols["j"], cols["w"])

    for bad, word in ((dict(i=2), "compute domain"), (dict(j=15), "compute domain"), (dict(i=-1), "compute domain"),
                      (dict(tile=6), "tiles"), (dict(tile=-1), "tiles"), (dict(w=np.nan), "finite"), (dict(w=np.inf), "finite")):
        with pytest.raises(ValueError, match=f"point 17, source 1.*{word}"):
            latlon.check_regrid_table(geom, changed(**bad))
    with pytest.raises(ValueError):
        latlon.check_regrid_table(geom, latlon.RegridTable(*(np.zeros((0, 3)),) * 4))
