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
