// A host model's arrays into the state (fv3core/pace/fv3core/initialization/geos_wrapper.py:207-270): the inverse of k_diag_pack.
// Up to PACE_UNPACK_MAX_ITEMS windows of fields are filled by ONE launch from one packed device buffer of float64, narrowed to
// the storage type on the way.
//
// Fields are stored [k][j][i], i fastest, rows padded (IDX3).  An item's source elements are in_step apart (7: one species of a
// C-ordered (x, y, z, 7) array) and ordered either
//   ZFAST  e = (i * nj + j) * nk + k   a C-ordered numpy array: the fastest axis of the source, called s below, is k for a 3-D
//                                      item and j for a plane, and never i, so the tile is transposed on its way;
//   XFAST  e = i + ni * (j + nj * k)   Fortran order, which is the device's own: nothing to transpose.
//
//   k_state_unpack  1-D grid, 256 threads = 4 waves.  A workgroup takes one window tile (wgmap.h: 64 points in i by 32 in s) of
//                   the item that table_find gives it; the table travels by value (pack_table.h).  The branch on the order is
//                   per item, hence workgroup-uniform.
//                   ZFAST  read    wt_runs_to_lds: runs of up to 32 contiguous doubles per i (256 B; with in_step = 7 every
//                                  seventh double of a run of 1792 B).
//                          LDS     tile[s][i] of the STORAGE type (narrowed before it is staged) at wgmap.h's pitch: here the
//                                  transposed accesses are the writes.
//                          write   wave w takes s = w, w + 4, ...; lane l writes i = l of that row: 64 contiguous elements.
//                   XFAST  no LDS: wave w takes s = w, w + 4, ...; lane l reads and writes i = l: contiguous runs of up to 64
//                          elements on both sides (in_step = 1).
//
// Nothing outside an item's window is written (not the halo, not the levels outside k0 .. k0 + nk - 1, not the row padding), and
// nothing outside its ni * nj * nk (ni * nj) source elements is read.  No atomics, no workspace.  The narrowing is a plain cast:
// round to nearest even, overflow to +-inf, as ndarray.astype(np.float32).  Two items whose windows overlap on one field: the
// result is undefined (their workgroups run in any order).
//
//   k_pe_peln_from_delp  the interface pressures a Fortran restart does not hold (driver/pace/driver/initialization.py:422-442):
//                   pe(i, j, k) = ptop + sum of delp(i, j, l) over l < k and peln = log(pe), k = 0 .. nk, on every column of the
//                   WHOLE storage (n + 7) x (n + 7), halo and stagger row included, as the reference writes .data.  One thread
//                   per column; the plane is flattened over its padded rows, so lane l of a wave reads and writes element l of a
//                   512-byte (float32: 256-byte) aligned run at every level; the lanes of the row padding return before they
//                   touch memory.  One double accumulator in ascending k, pe = ptop + s, then s += delp: additions only, the
//                   order of a sequential numpy cumsum.  peln = lean_log of that double (lean_math.h: <= 0.546 ulp); both are
//                   narrowed on the store only.  nk loads and 2 (nk + 1) stores per column, no LDS, no atomics, no workspace.
#include "common.h"
#include "kernels.h"
#include "lean_math.h"
#include "pack_table.h"

typedef PackTable<pace_unpack_item_t, PACE_UNPACK_MAX_ITEMS> UnpackTable;

__global__ void __launch_bounds__(64 * WT_WAVES) k_state_unpack(Geo g, UnpackTable tab, const double* __restrict__ in) {
  const int b = (int)blockIdx.x;
  const int m = table_find(tab.first, tab.nitems, b);
  const pace_unpack_item_t& it = tab.item[m];
  const bool vol = it.kind == PACE_DIAG_WINDOW3D;
  const WindowTile wt = window_tile_of_linear(b - tab.first[m], it.ni, it.nj, it.nk, vol, WT_TS);
  const int sb = wt.sb, ib = wt.ib, j = wt.j, wi = wt.wi, ws = wt.ws;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const long step = it.in_step;
  const double* __restrict__ src = in + it.in_offset;
  real* __restrict__ q = it.field;

  if (it.order == PACE_ORDER_XFAST) {
    if (lane >= wi) return;
    // source elements between s and s + 1 (a 3-D item: levels; a plane: rows), and the tile's first element
    const long sstride = vol ? (long)it.ni * it.nj : (long)it.ni;
    const long e0 = (vol ? (long)it.ni * j : 0L) + ib + lane;
    for (int s = wave; s < ws; s += WT_WAVES) {
      const real v = (real)src[(e0 + sstride * (sb + s)) * step];
      if (vol) q[IDX3(g, it.i0 + ib + lane, it.j0 + j, it.k0 + sb + s)] = v;
      else q[IDX2(g, it.i0 + ib + lane, it.j0 + sb + s)] = v;
    }
    return;
  }

  __shared__ real tile[WT_TS * WT_PITCH];
  const long istride = vol ? (long)it.nj * it.nk : (long)it.nj;  // source elements between i and i + 1
  const long e0 = (vol ? (long)j * it.nk : 0L) + sb + (long)ib * istride;
  wt_runs_to_lds(tile, src + e0 * step, istride, step, wi, ws);
  __syncthreads();
  if (lane < wi) {
    const int i = it.i0 + ib + lane;
    for (int s = wave; s < ws; s += WT_WAVES) {
      const real v = tile[s * WT_PITCH + lane];
      if (vol) q[IDX3(g, i, it.j0 + j, it.k0 + sb + s)] = v;
      else q[IDX2(g, i, it.j0 + sb + s)] = v;
    }
  }
}

int launch_state_unpack(const Geo& g, const pace_unpack_item_t* items, int nitems, const double* in, hipStream_t st) {
  UnpackTable tab{};
  tab.nitems = nitems;
  for (int m = 0; m < nitems; ++m) tab.item[m] = items[m];
  const int rc = pack_table_fill_first(tab, [](const pace_unpack_item_t& it) {
    return window_tiles(it.ni, it.nj, it.nk, it.kind == PACE_DIAG_WINDOW3D, WT_TS);
  });
  if (rc != PACE_OK) return rc;
  const dim3 grid((unsigned)tab.first[nitems]), block(64 * WT_WAVES);
  hipLaunchKernelGGL(k_state_unpack, grid, block, 0, st, g, tab, in);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}

__global__ void __launch_bounds__(64) k_pe_peln_from_delp(Geo g, const real* __restrict__ delp, double ptop, real* __restrict__ pe,
                                                          real* __restrict__ peln) {
  const long p = (long)blockIdx.x * 64 + threadIdx.x;
  const int j = (int)(p / g.sj);
  const int i = (int)(p - (long)j * g.sj);
  if (j >= g.nj || i >= g.ni) return;
  long c = IDX2(g, i, j);
  double s = 0.0;
  for (int k = 0; k < g.nk; ++k, c += g.sk) {
    const double v = ptop + s;
    pe[c] = (real)v;
    peln[c] = (real)lean_log(v);
    s += (double)delp[c];
  }
  const double v = ptop + s;
  pe[c] = (real)v;
  peln[c] = (real)lean_log(v);
}

int launch_pe_peln_from_delp(const Geo& g, const real* delp, double ptop, real* pe, real* peln, hipStream_t st) {
  const dim3 grid((unsigned)(((long)g.sj * g.nj + 63) / 64)), block(64);
  hipLaunchKernelGGL(k_pe_peln_from_delp, grid, block, 0, st, g, delp, ptop, pe, peln);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
