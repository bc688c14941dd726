// Regridding the cube to a list of points (the lat-lon diagnostics; no counterpart in the reference): every target point is the
// weighted sum of three cells of the six tiles' storages (pace_amd/util/latlon.py: the spherical Delaunay triangle around it),
// any number of variables by one launch into ONE dense buffer, point-major with z fastest like every other output here.
//   dense[offset + p * nk + k] = (DT)((w0 * f_0(k0 + k) + w1 * f_1(k0 + k)) + w2 * f_2(k0 + k))
// in double, products then adds in this order (the build has -ffp-contract=off: no FMA), the sources widened to double first.
//
// The work decomposition is the window tile of wgmap.h with the POINT LIST as the 64-wide axis and the levels as the 32-deep
// one (an item is a "window" of npoints x 1 x nk, a plane of npoints x 1 x 1), staged through LDS at its pitch; the dense-side
// phase is pack_table.h's.
//
//   the tables  lie in DEVICE memory: npoints points of 64 bytes; n items and behind them the prefix table int32 first[n + 1] of
//               their tile counts.  The item of a workgroup is found by scalar loads; a lane loads ITS point once per tile (four
//               16-byte loads, 64 consecutive points are 4 KiB in a row) and the three tile pointers it names from the item.
//   the grid    min(n * (the most tiles an item can have), RG_MAX_GRID) workgroups, each of which takes the tiles b,
//               b + gridDim.x, ... below first[n], as k_cube_xfer does (the host cannot read first[n] without a synchronisation).
//   read        wave w takes the levels s = w, w + 4, ...; lane l does three loads per level for its point, each sk elements
//               behind the last level's.  Neighbouring targets mostly name neighbouring cells along x, so the gathers are partly
//               coalesced (supposed, not measured).
//   write       runs of up to 32 contiguous dense elements per point.
//
// Only the three named elements per point and level are read, nothing is written outside an item's npoints * nk dense elements,
// the storages are not written.  No atomics, no workspace, no host synchronisation.
#include "common.h"
#include "kernels.h"
#include "pack_table.h"

#define RG_MAX_GRID 2048  // 256 CUs x 8 workgroups of 4 waves

template <typename DT>
__global__ void __launch_bounds__(64 * WT_WAVES) k_cube_regrid(Geo g, const pace_regrid_point_t* __restrict__ points, int npoints,
                                                               const pace_regrid_item_t* __restrict__ items,
                                                               const int* __restrict__ first, int n, DT* dense) {
  __shared__ DT tile[WT_TS * WT_PITCH];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int total = first[n];
  for (int b = (int)blockIdx.x; b < total; b += (int)gridDim.x) {
    const int m = table_find(first, n, b);
    const pace_regrid_item_t* it = items + m;  // (its members one by one: the pointers are indexed per lane, from memory)
    const bool vol = it->kind == PACE_DIAG_WINDOW3D;
    const int nk = vol ? it->nk : 1, k0 = vol ? it->k0 : 0;
    const WindowTile wt = window_tile_of_linear(b - first[m], npoints, 1, nk, true, WT_TS);
    const int sb = wt.sb, ib = wt.ib, wi = wt.wi, ws = wt.ws;
    DT* d = dense + it->offset + (long)ib * nk + sb;
    if (lane < wi) {
      const pace_regrid_point_t p = points[ib + lane];
      const long level = (long)(k0 + sb) * g.sk;  // (a plane: 0)
      const real* q0 = (const real*)it->field[p.tile[0]] + IDX2(g, p.i[0], p.j[0]) + level;
      const real* q1 = (const real*)it->field[p.tile[1]] + IDX2(g, p.i[1], p.j[1]) + level;
      const real* q2 = (const real*)it->field[p.tile[2]] + IDX2(g, p.i[2], p.j[2]) + level;
      for (int s = wave; s < ws; s += WT_WAVES) {
        const long o = s * g.sk;
        const double a0 = p.w[0] * (double)q0[o], a1 = p.w[1] * (double)q1[o], a2 = p.w[2] * (double)q2[o];
        tile[s * WT_PITCH + lane] = (DT)((a0 + a1) + a2);
      }
    }
    __syncthreads();
    wt_lds_to_runs(d, tile, (long)nk, wi, ws);
    __syncthreads();  // the next tile of this workgroup reuses the LDS
  }
}

int launch_cube_regrid(const Geo& g, const pace_regrid_point_t* points_on_device, int npoints,
                       const pace_regrid_item_t* items_on_device, int n, int dense_is_double, void* dense, hipStream_t st) {
  const long bound = window_tiles(npoints, 1, g.nk + 1, true, WT_TS) * n;  // a whole field's levels per item at the most
  const dim3 grid((unsigned)(bound < RG_MAX_GRID ? bound : RG_MAX_GRID)), block(64 * WT_WAVES);
  const int* first = (const int*)(items_on_device + n);
  if (dense_is_double)
    hipLaunchKernelGGL((k_cube_regrid<double>), grid, block, 0, st, g, points_on_device, npoints, items_on_device, first, n,
                       (double*)dense);
  else
    hipLaunchKernelGGL((k_cube_regrid<float>), grid, block, 0, st, g, points_on_device, npoints, items_on_device, first, n,
                       (float*)dense);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
