// Exhaustive check of the workgroup maps of pace_amd/csrc/wgmap.h (stand-alone host program; test infrastructure).
//
// For every launch shape in the ranges below: the image of the launch's workgroups under the map is EXACTLY the set of the
// launch's pieces of work, each once -- none skipped, none repeated, none outside.  For the padded launch of the flux preparation
// the pieces are the nblocks real blocks of every chunk: each is taken once, and the other workgroups of the launch -- exactly
// (padded - nblocks) per chunk -- get block numbers in [nblocks, padded), whose points lie past the plane's last row, so the
// kernel's box test returns them (k_fxadv.hip; fxadv_block_is_padding is that comparison by name, nothing more).  For the window
// tiles of the pack kernels the pieces are the points (i, j, s) of the window: the tiles 0 .. window_tiles - 1 cover each once and
// stay inside it.  table_find is held against a linear scan of the prefix table.  Prints the
// first offending shape and workgroup and exits 1; prints one summary line per map and exits 0 otherwise.
//
//   wgmap_check            the full ranges
//   wgmap_check --quick    a tenth of the level counts (for a first look; the test-suite runs the full ranges)
//   wgmap_check --fv b gx gy nlev    prints the (tile x, tile y, level) of workgroup b of a gx x gy x nlev transport launch
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../../pace_amd/csrc/wgmap.h"

namespace {

long long g_workgroups = 0;
std::vector<unsigned char> g_seen;  // (sized per shape; its bounds are what AddressSanitizer watches)

// ---- transport: gx x gy tiles x nlev levels ----
bool check_fv(int gx, int gy, int nlev) {
  const int total = gx * gy * nlev;
  g_seen.assign((size_t)total, 0);
  for (int b = 0; b < total; ++b) {
    const FvTile t = fv_tile_of_linear(b, gx, gy, nlev);
    const bool inside = t.bx >= 0 && t.bx < gx && t.by >= 0 && t.by < gy && t.bz >= 0 && t.bz < nlev;
    if (!inside) {
      std::printf("fv_tile_of_linear: gx %d gy %d nlev %d: workgroup %d -> (%d, %d, %d) is outside the launch\n", gx, gy, nlev, b, t.bx,
                  t.by, t.bz);
      return false;
    }
    unsigned char& s = g_seen[(size_t)t.bx + (size_t)gx * ((size_t)t.by + (size_t)gy * (size_t)t.bz)];
    if (s) {
      std::printf("fv_tile_of_linear: gx %d gy %d nlev %d: workgroup %d -> (%d, %d, %d) is taken twice\n", gx, gy, nlev, b, t.bx, t.by,
                  t.bz);
      return false;
    }
    s = 1;
  }
  g_workgroups += total;
  return true;  // total distinct images among total places: nothing is skipped
}

// ---- d_sw's kinetic energy + vorticity: nbx blocks x nlev chunks of levels ----
bool check_ke(int nbx, int nlev) {
  const int total = nbx * nlev;
  g_seen.assign((size_t)total, 0);
  for (int lin = 0; lin < total; ++lin) {
    const KeBlock t = ke_block_of_linear(lin, nbx, nlev);
    if (!(t.bx >= 0 && t.bx < nbx && t.bz >= 0 && t.bz < nlev)) {
      std::printf("ke_block_of_linear: nbx %d nlev %d: workgroup %d -> (%d, %d) is outside the launch\n", nbx, nlev, lin, t.bx, t.bz);
      return false;
    }
    unsigned char& s = g_seen[(size_t)t.bx + (size_t)nbx * (size_t)t.bz];
    if (s) {
      std::printf("ke_block_of_linear: nbx %d nlev %d: workgroup %d -> (%d, %d) is taken twice\n", nbx, nlev, lin, t.bx, t.bz);
      return false;
    }
    s = 1;
  }
  g_workgroups += total;
  return true;
}

// ---- the flux preparation's interior: nblocks real blocks, padded to a multiple of eight, x nchunks chunks of levels ----
bool check_fx(int nblocks, int nchunks) {
  const int nbx = fxadv_padded_blocks(nblocks);
  if (nbx < nblocks || nbx % 8 != 0 || nbx - nblocks > 7) {
    std::printf("fxadv_padded_blocks: %d blocks -> %d\n", nblocks, nbx);
    return false;
  }
  const int total = nbx * nchunks;
  g_seen.assign((size_t)nblocks * (size_t)nchunks, 0);
  int real = 0, padding = 0;
  for (int b = 0; b < total; ++b) {
    const FxBlock t = fxadv_block_of_workgroup(b, nbx);
    if (!(t.block >= 0 && t.block < nbx && t.chunk >= 0 && t.chunk < nchunks)) {
      std::printf("fxadv_block_of_workgroup: blocks %d chunks %d: workgroup %d -> (%d, %d) is outside the padded launch\n", nblocks,
                  nchunks, b, t.block, t.chunk);
      return false;
    }
    if (fxadv_block_is_padding(t, nblocks)) {  // (in [nblocks, nbx) by the test above: past the plane)
      ++padding;
      continue;
    }
    unsigned char& s = g_seen[(size_t)t.block + (size_t)nblocks * (size_t)t.chunk];
    if (s) {
      std::printf("fxadv_block_of_workgroup: blocks %d chunks %d: workgroup %d -> (%d, %d) is taken twice\n", nblocks, nchunks, b, t.block,
                  t.chunk);
      return false;
    }
    s = 1;
    ++real;
  }
  if (real != nblocks * nchunks || padding != (nbx - nblocks) * nchunks) {
    std::printf("fxadv_block_of_workgroup: blocks %d chunks %d: %d real and %d padding workgroups, expected %d and %d\n", nblocks, nchunks,
                real, padding, nblocks * nchunks, (nbx - nblocks) * nchunks);
    return false;
  }
  g_workgroups += total;
  return true;
}

// ---- the pack kernels' window tiles: ni x nj x ns points (a plane: nj = 1 rows of its own, s = j), `rows` per tile in s ----
bool check_window(int ni, int nj, int ns, bool vol, int rows) {
  // (a plane's s axis is its nj, and its nk is 1)
  const int wnj = vol ? nj : ns, wnk = vol ? ns : 1;
  const long count = window_tiles(ni, wnj, wnk, vol, rows);
  g_seen.assign((size_t)ni * (size_t)nj * (size_t)ns, 0);
  long points = 0;
  for (int t = 0; t < (int)count; ++t) {
    const WindowTile w = window_tile_of_linear(t, ni, wnj, wnk, vol, rows);
    const bool inside = w.wi >= 1 && w.wi <= WT_TI && w.ws >= 1 && w.ws <= rows && w.ib >= 0 && w.ib + w.wi <= ni && w.sb >= 0 &&
                        w.sb + w.ws <= ns && w.j >= 0 && w.j < nj;
    if (!inside) {
      std::printf("window_tile_of_linear: ni %d nj %d ns %d 3-D %d rows %d: tile %d -> sb %d ib %d j %d wi %d ws %d leaves the window\n", ni,
                  nj, ns, (int)vol, rows, t, w.sb, w.ib, w.j, w.wi, w.ws);
      return false;
    }
    for (int i = w.ib; i < w.ib + w.wi; ++i)
      for (int s = w.sb; s < w.sb + w.ws; ++s) {
        unsigned char& seen = g_seen[(size_t)s + (size_t)ns * ((size_t)w.j + (size_t)nj * (size_t)i)];
        if (seen) {
          std::printf("window_tile_of_linear: ni %d nj %d ns %d 3-D %d rows %d: tile %d takes (%d, %d, %d) again\n", ni, nj, ns, (int)vol,
                      rows, t, i, w.j, s);
          return false;
        }
        seen = 1;
        ++points;
      }
  }
  if (points != (long)ni * nj * ns) {
    std::printf("window_tiles: ni %d nj %d ns %d 3-D %d rows %d: %ld tiles hold %ld of %ld points\n", ni, nj, ns, (int)vol, rows, count,
                points, (long)ni * nj * ns);
    return false;
  }
  g_workgroups += count;
  return true;
}

// ---- the table search: n items with counts >= 1 from a fixed generator; every b below the total against a linear scan ----
bool check_find(int n, unsigned seed) {
  std::vector<int> first((size_t)n + 1, 0);
  for (int m = 0; m < n; ++m) {
    seed = seed * 1664525u + 1013904223u;
    const int count = 1 + (int)((seed >> 16) % ((seed >> 8) % 3 == 0 ? 40u : 3u));  // mostly 1 .. 3, a third up to 40
    first[(size_t)m + 1] = first[(size_t)m] + count;
  }
  for (int b = 0; b < first[(size_t)n]; ++b) {
    int want = 0;
    while (first[(size_t)want + 1] <= b) ++want;
    const int got = table_find(first.data(), n, b);
    if (got != want) {
      std::printf("table_find: %d items, seed %u: workgroup %d -> item %d, a linear scan gives %d\n", n, seed, b, got, want);
      return false;
    }
  }
  g_workgroups += first[(size_t)n];
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 6 && std::strcmp(argv[1], "--fv") == 0) {  // one workgroup of one transport launch: "bx by bz"
    const FvTile t = fv_tile_of_linear(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]));
    std::printf("%d %d %d\n", t.bx, t.by, t.bz);
    return 0;
  }
  const int step = (argc > 1 && std::strcmp(argv[1], "--quick") == 0) ? 10 : 1;
  // transport: every gx in 1 .. 13, gy in 1 .. 16, nlev in 1 .. 130 ...
  long long shapes = 0;
  for (int gx = 1; gx <= 13; ++gx)
    for (int gy = 1; gy <= 16; ++gy)
      for (int nlev = 1; nlev <= 130; nlev += step, ++shapes)
        if (!check_fv(gx, gy, nlev)) return 1;
  // ... and, outside that box, every grid a launcher makes of some n in 12 .. 384, with every nlev 1 .. 130: the general kernel's
  // (ceil(n / 32), ceil(n / 24)), the three-planes-high launch of d_sw's three scalars (the same with 3 ceil(n / 24)), and the
  // lean kernels' n / 32 x n / 24 and n / 16 x n / 24 where the tile divides n (k_fvt.hip covers: the 16 x 24 shape takes the
  // multiples of 48 that are no multiples of 32 -- C48, C144, C240: 15 x 10, C336: 21 x 14)
  std::vector<std::pair<int, int>> done;
  const auto extra = [&](int gx, int gy) {
    if (gx <= 13 && gy <= 16) return true;
    for (const auto& d : done)
      if (d.first == gx && d.second == gy) return true;
    done.emplace_back(gx, gy);
    for (int nlev = 1; nlev <= 130; nlev += step, ++shapes)
      if (!check_fv(gx, gy, nlev)) return false;
    return true;
  };
  for (int n = 12; n <= 384; ++n) {
    const int gx = (n + 31) / 32, gy = (n + 23) / 24;
    if (!extra(gx, gy) || !extra(gx, 3 * gy)) return 1;
    if (n % 24 == 0 && n % 32 == 0 && !extra(n / 32, n / 24)) return 1;
    if (n % 24 == 0 && n % 16 == 0 && !extra(n / 16, n / 24)) return 1;
  }
  std::printf("fv_tile_of_linear: %lld launch shapes, every (tile, level) once\n", shapes);
  // kinetic energy + vorticity (blocks x chunks of one or two levels; C12: 11 blocks, C384: about 1 300): every block count
  // 1 .. 64 with every level count 1 .. 130, every block count 65 .. 1400 with the level counts at both ends and around the
  // multiples of eight (the map's only dependence on the level count is nlev / 8 and nlev % 8)
  shapes = 0;
  for (int nbx = 1; nbx <= 64; ++nbx)
    for (int nlev = 1; nlev <= 130; nlev += step, ++shapes)
      if (!check_ke(nbx, nlev)) return 1;
  for (int nbx = 65; nbx <= 1400; nbx += step)
    for (int nlev : {1, 7, 8, 9, 79, 127, 128}) {
      ++shapes;
      if (!check_ke(nbx, nlev)) return 1;
    }
  std::printf("ke_block_of_linear: %lld launch shapes, every (block, chunk) once\n", shapes);
  // flux preparation: every block count 1 .. 160 (C384: 153) with every chunk count 1 .. 130 (a small tile takes one level per
  // chunk)
  shapes = 0;
  for (int nblocks = 1; nblocks <= 160; ++nblocks)
    for (int nchunks = 1; nchunks <= 130; nchunks += step, ++shapes)
      if (!check_fx(nblocks, nchunks)) return 1;
  std::printf("fxadv_block_of_workgroup: %lld launch shapes, every real (block, chunk) once, the rest past the last block\n", shapes);
  // window tiles: every ni 1 .. 200 (three tiles and a partial fourth) with every ns 1 .. 100, 32 and 4 rows per tile; a plane,
  // and a 3-D item of 1 .. 3 rows j (per j identical: three rows catch a wrong carry between ib and j)
  shapes = 0;
  for (int rows : {WT_TS, WT_TS_COLUMN})
    for (int ni = 1; ni <= 200; ++ni)
      for (int ns = 1; ns <= 100; ns += step)
        for (int nj = 0; nj <= 3; ++nj, ++shapes)  // 0: the plane
          if (!check_window(ni, nj == 0 ? 1 : nj, ns, nj != 0, rows)) return 1;
  std::printf("window_tile_of_linear: %lld windows, every point once, every tile inside\n", shapes);
  // the table search: every item count 1 .. 33 with eight tables each
  shapes = 0;
  for (int n = 1; n <= 33; ++n)
    for (unsigned seed = 1; seed <= 8; ++seed, ++shapes)
      if (!check_find(n, seed * 2654435761u + (unsigned)n)) return 1;
  std::printf("table_find: %lld tables, every workgroup as a linear scan\n", shapes);
  std::printf("wgmap_check ok: %lld workgroups\n", g_workgroups);
  return 0;
}
