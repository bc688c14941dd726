// Gather and scatter across the cube (util/pace/util/communicator.py:111-329): windows of any number of fields of any of the six
// tiles' storages of one geometry, moved between the fields (x fastest, padded rows: IDX3) and ONE dense buffer in the
// reference's axis order ((x, y, z) in C order, z fastest) by one launch, with the cast between the storage type and the dense
// type on the way.  pace_cube_gather: dense[offset + (i * nj + j) * nk + k] = field(i0 + i, j0 + j, k0 + k); pace_cube_scatter is
// the inverse.  A PLANE item (a 2-D field, or one level of a 3-D one) is the same with nk = 1 and j the fastest dense axis.
//
// The work decomposition is the window tile of wgmap.h (64 points in i by 32 in s, the fastest axis of the dense side), staged
// through LDS at its pitch; the dense-side phases are pack_table.h's.
//
//   the table   lies in DEVICE memory (a whole cube's output step is 84 items and more: no by-value batch holds them):
//               n items, and behind them the prefix table int32 first[n + 1] of the items' tile counts, first[n] = all tiles.  Both
//               are the same for a whole workgroup and const __restrict__, so they are fetched by scalar loads.
//   the grid    the host cannot read first[n] without a synchronisation, so the grid is not the tile count: it is
//               min(n * (the most tiles an item of this geometry can have), CG_MAX_GRID) workgroups, each of which takes the
//               tiles b, b + gridDim.x, ... below first[n].  A workgroup past the last tile leaves after one scalar load.
//   gather      read: wave w takes s = w, w + 4, ...; lane l reads i = l of that row (64 contiguous elements).  write: runs of
//               up to 32 contiguous dense elements per i.
//   scatter     the same two phases in the other order: dense runs into LDS, then rows of 64 contiguous field elements out.
//
// Nothing outside an item's window is read or written on the field side (not the halo, not the row padding, not other levels),
// nothing outside its ni * nj * nk elements on the dense side.  No atomics, no workspace, no host synchronisation.  The
// conversion is a plain cast; where the storage type is the dense type the value moves through registers and LDS as it is:
// -0.0, NaN payloads and denormals arrive unchanged.
#include "common.h"
#include "kernels.h"
#include "pack_table.h"

#define CG_MAX_GRID 2048  // 256 CUs x 8 workgroups of 4 waves

template <typename DT, bool SCATTER>
__global__ void __launch_bounds__(64 * WT_WAVES) k_cube_xfer(Geo g, const pace_cube_item_t* __restrict__ items,
                                                              const int* __restrict__ first, int n, DT* dense) {
  __shared__ DT tile[WT_TS * WT_PITCH];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int total = first[n];
  for (int b = (int)blockIdx.x; b < total; b += (int)gridDim.x) {
    const int m = table_find(first, n, b);
    const pace_cube_item_t it = items[m];
    const bool vol = it.kind == PACE_DIAG_WINDOW3D;
    const WindowTile wt = window_tile_of_linear(b - first[m], it.ni, it.nj, it.nk, vol, WT_TS);
    const int sb = wt.sb, ib = wt.ib, j = wt.j, wi = wt.wi, ws = wt.ws;
    const long dstride = vol ? (long)it.nj * it.nk : (long)it.nj;  // dense elements between i and i + 1
    DT* d = dense + it.offset + (vol ? (long)j * it.nk : 0L) + sb + (long)ib * dstride;
    real* q = (real*)it.field;
    // the field element of (lane, s) of this tile
    const long f0 = vol ? IDX3(g, it.i0 + ib + lane, it.j0 + j, it.k0 + sb) : IDX2(g, it.i0 + ib + lane, it.j0 + sb);
    const long fs = vol ? g.sk : (long)g.sj;
    if (!SCATTER) {
      if (lane < wi)
        for (int s = wave; s < ws; s += WT_WAVES) tile[s * WT_PITCH + lane] = (DT)q[f0 + s * fs];
      __syncthreads();
      wt_lds_to_runs(d, tile, dstride, wi, ws);
    } else {
      wt_runs_to_lds(tile, d, dstride, 1L, wi, ws);
      __syncthreads();
      if (lane < wi)
        for (int s = wave; s < ws; s += WT_WAVES) q[f0 + s * fs] = (real)tile[s * WT_PITCH + lane];
    }
    __syncthreads();  // the next tile of this workgroup reuses the LDS
  }
}

int launch_cube_xfer(const Geo& g, const pace_cube_item_t* table_on_device, int n, int dense_is_double, void* dense, int scatter,
                     hipStream_t st) {
  const long bound = window_tiles(g.ni, g.nj, g.nk + 1, true, WT_TS) * n;  // a whole field's tiles per item at the most
  const dim3 grid((unsigned)(bound < CG_MAX_GRID ? bound : CG_MAX_GRID)), block(64 * WT_WAVES);
  const int* first = (const int*)(table_on_device + n);
  if (dense_is_double) {
    if (scatter) hipLaunchKernelGGL((k_cube_xfer<double, true>), grid, block, 0, st, g, table_on_device, first, n, (double*)dense);
    else hipLaunchKernelGGL((k_cube_xfer<double, false>), grid, block, 0, st, g, table_on_device, first, n, (double*)dense);
  } else {
    if (scatter) hipLaunchKernelGGL((k_cube_xfer<float, true>), grid, block, 0, st, g, table_on_device, first, n, (float*)dense);
    else hipLaunchKernelGGL((k_cube_xfer<float, false>), grid, block, 0, st, g, table_on_device, first, n, (float*)dense);
  }
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
