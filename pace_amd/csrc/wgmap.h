// Workgroup maps: which piece of the work a workgroup of a launch takes, as pure functions of its place in the launch.
//
// Workgroups are handed to the eight XCDs round-robin in launch order, and every XCD has an L2 of its own, so the kernels that
// re-read their neighbours' lines renumber their workgroups to keep neighbours on one XCD.  Each map must be a bijection of the
// launch's workgroups onto its pieces of work (a piece skipped is never computed; a piece taken twice is accumulated twice where
// the kernel accumulates).  The maps have no HIP dependency: the device build, the CPU emulation build and the stand-alone
// exhaustive check (tests/emu/wgmap_check.cpp) compile this one text.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WGMAP_FN __host__ __device__ __forceinline__
#else
#define WGMAP_FN inline
#endif

// ---- the transport kernels (k_fvt.hip, k_fvtp2d.hip): linear workgroup of a gx x gy x nlev launch -> (tile, level) ----------
// With the plain (x, y, z) order, neighbouring tiles of a level land on DIFFERENT XCDs and every line of their overlapping
// footprints is fetched from memory once per XCD (measured: 1.9 x the algorithmic bytes).  Here a level belongs to ONE XCD: XCD x
// works through levels x, x + 8, x + 16, ... tile by tile, so the halo lines shared by neighbouring tiles are L2 hits.  (Affinity
// only: nothing depends on where a workgroup really runs.)
struct FvTile {
  int bx, by, bz;
};
WGMAP_FN FvTile fv_tile_of_linear(int b, int gx, int gy, int nlev) {
  const int tpl = gx * gy;
  const int full = (nlev / 8) * 8;  // levels that can be dealt out eight at a time
  int lev, t;
  if (b < full * tpl) {
    const int xcd = b & 7, slot = b >> 3;
    lev = (slot / tpl) * 8 + xcd;
    t = slot - (slot / tpl) * tpl;
  } else {
    lev = b / tpl;
    t = b - lev * tpl;
  }
  // within a level: the four corner tiles first, then the edge tiles, then the interior ones -- the corner and edge forms take
  // 1.2 - 2 x as long as the straight-line interior code, and the workgroups that start last should not be the longest ones
  if (gx >= 3 && gy >= 3) {
    if (t < 4) return FvTile{(t & 1) ? gx - 1 : 0, (t & 2) ? gy - 1 : 0, lev};
    t -= 4;
    const int nsn = 2 * (gx - 2), nwe = 2 * (gy - 2);
    if (t < nsn) return FvTile{1 + (t >> 1), (t & 1) ? gy - 1 : 0, lev};
    t -= nsn;
    if (t < nwe) return FvTile{(t & 1) ? gx - 1 : 0, 1 + (t >> 1), lev};
    t -= nwe;
    return FvTile{1 + t % (gx - 2), 1 + t / (gx - 2), lev};
  }
  return FvTile{t % gx, t / gx, lev};
}

// ---- d_sw's kinetic energy + vorticity launch (k_dsw.hip k_ke_vorticity): linear workgroup of an nbx x 1 x nlev launch ----
// A point re-reads rows of its j-neighbours: the blocks of a level (of a chunk of levels) run on ONE XCD -- XCD x works through
// levels x, x + 8, ...
struct KeBlock {
  int bx, bz;
};
WGMAP_FN KeBlock ke_block_of_linear(int lin, int nbx, int nlev) {
  const int full = (nlev / 8) * 8;
  if (lin < full * nbx) {
    const int slot = lin >> 3;
    return KeBlock{slot - (slot / nbx) * nbx, (slot / nbx) * 8 + (lin & 7)};
  }
  const int bz = lin / nbx;
  return KeBlock{lin - bz * nbx, bz};
}

// ---- the interior box of the flux preparation (k_fxadv.hip): workgroup b of the nbx_padded x nchunks interior workgroups --------
// The plane's flattened rows are cut into `nblocks` blocks of FX_NT points; the launch pads that to a multiple of eight
// (fxadv_padded_blocks) so that XCD x takes the x-th eighth of the (padded) blocks -- contiguous rows -- of every chunk of levels
// and only the seams between the eighths are fetched by two L2s (with the plain order: 324 MB for 233 algorithmic).  A padding
// workgroup gets a block number >= nblocks: all its points lie past the plane's last row, it holds nothing.
struct FxBlock {
  int block, chunk;
};
WGMAP_FN int fxadv_padded_blocks(int nblocks) { return (nblocks + 7) / 8 * 8; }
WGMAP_FN FxBlock fxadv_block_of_workgroup(int b, int nbx_padded) {
  const int seg = nbx_padded / 8;
  const int chunk = b / nbx_padded, r = b - chunk * nbx_padded;
  return FxBlock{(r & 7) * seg + (r >> 3), chunk};
}
WGMAP_FN bool fxadv_block_is_padding(const FxBlock& w, int nblocks) { return w.block >= nblocks; }

// ---- the window tiles of the table-driven pack kernels (k_diag.hip, k_state.hip, k_gather.hip) -------------------------------
// A window of a field ([k][j][i], i fastest) moves to or from a dense array whose fastest axis, called s, is never i: k of a 3-D
// item (`vol`), j of a plane.  It is cut into tiles of WT_TI points in i by `ts` points in s (WT_TS; WT_TS_COLUMN for a column
// integral, one row per wave), a 3-D item at one j per tile, numbered with the s tiles fastest, then the i tiles, then the rows j.
// The host's tile count and the kernels' decomposition are these two functions and nothing else.
//
// The tile is transposed through LDS as tile[s][i] at a pitch of WT_PITCH = 65 elements (MI355X_MICROARCH.md, LDS: 64 banks of
// 4 B; b32 goes in groups of 32 lanes, b64 in groups of 16 for writes).  The field side is rows of 64 consecutive elements:
// conflict-free in both directions.  The dense side is s = 0 .. 31 at one i, element 65 s + i:
//   reads (pack, gather)      ds_read_b32: bank (s + i) mod 32; ds_read_b64: 2 ((s + i) mod 32) of 64 -- 32 different banks;
//   writes (unpack, scatter)  ds_write_b32: bank (s + i) mod 32 -- 32 different banks; ds_write_b64, s = 0 .. 15 (16 .. 31):
//                             dword 130 s + 2 i, banks (2 s + 2 i) mod 32 and the one after it -- 16 different pairs.
// A pitch of 64 would put a whole group on one bank (pair).  A tile narrower than 32 in s (the last 15 of 79 levels) mixes two
// or three i in a group and takes up to 3 lanes per bank.
#define WT_TI 64
#define WT_TS 32
#define WT_WAVES 4
#define WT_TS_COLUMN WT_WAVES
#define WT_PITCH (WT_TI + 1)

WGMAP_FN long window_tiles(int ni, int nj, int nk, bool vol, int ts) {
  const int ns = vol ? nk : nj;
  const long per_row = (long)((ni + WT_TI - 1) / WT_TI) * ((ns + ts - 1) / ts);
  return vol ? per_row * nj : per_row;
}
struct WindowTile {
  int sb, ib;  // the tile's first point in s and in i, within the window
  int j;       // the row of a 3-D item's tile; 0 for a plane
  int wi, ws;  // its points in i (1 .. WT_TI) and in s (1 .. ts)
};
WGMAP_FN WindowTile window_tile_of_linear(int t, int ni, int nj, int nk, bool vol, int ts) {
  const int ns = vol ? nk : nj;
  const int nts = (ns + ts - 1) / ts, nti = (ni + WT_TI - 1) / WT_TI;
  const int sb = (t % nts) * ts;
  t /= nts;
  const int ib = (t % nti) * WT_TI;
  return WindowTile{sb, ib, t / nti, ni - ib < WT_TI ? ni - ib : WT_TI, ns - sb < ts ? ns - sb : ts};
}

// ---- the item of a workgroup: m with first[m] <= b < first[m + 1] in a prefix table first[0 .. n] of per-item counts >= 1 ------
// (b is the same for a whole workgroup and first[] is read-only: scalar loads and scalar branches, ceil(log2 n) of them)
WGMAP_FN int table_find(const int* first, int n, int b) {
  int m = 0, hi = n;  // first[m] <= b < first[hi]
  while (hi - m > 1) {
    const int mid = (m + hi) >> 1;
    if (b >= first[mid]) m = mid;
    else hi = mid;
  }
  return m;
}
