// Gather and scatter across the cube (util/pace/util/communicator.py:111-329): windows of any number of fields of any of the six
// tiles' storages of one geometry, moved between the fields (x fastest, padded rows: IDX3) and ONE dense buffer in the
// reference's axis order ((x, y, z) in C order, z fastest) by one launch, with the cast between the storage type and the dense
// type on the way.  pace_cube_gather: dense[offset + (i * nj + j) * nk + k] = field(i0 + i, j0 + j, k0 + k); pace_cube_scatter is
// the inverse.  A PLANE item (a 2-D field, or one level of a 3-D one) is the same with nk = 1 and j the fastest dense axis.
//
// The work decomposition is k_diag.hip's: a tile is CG_TI = 64 points in i by CG_TS = 32 points in s, the fastest axis of the
// dense side (k of a 3-D item, at one j; j of a plane), staged through LDS at a pitch of 65 elements so that both the rows
// (64 consecutive elements: conflict-free) and the transposed accesses (s = 0 .. 31 at one i: element 65 * s + i, 32 different
// banks for 4-byte and for 8-byte elements -- MI355X_MICROARCH.md, LDS) are conflict-free for a full tile.
//
//   the table   lies in DEVICE memory (a whole cube's output step is 84 items and more: no by-value batch holds them):
//               n items, and behind them the prefix table int32 first[n + 1] of the items' tile counts, first[n] = all tiles.  Both
//               are the same for a whole workgroup and const __restrict__, so they are fetched by scalar loads; the bisection of
//               first[] is ceil(log2 n) dependent scalar loads and scalar branches.
//   the grid    the host cannot read first[n] without a synchronisation, so the grid is not the tile count: it is
//               min(n * (the most tiles an item of this geometry can have), CG_MAX_GRID) workgroups, each of which takes the
//               tiles b, b + gridDim.x, ... below first[n].  A workgroup past the last tile leaves after one scalar load.
//   gather      read: wave w takes s = w, w + 4, ...; lane l reads i = l of that row (64 contiguous elements).  write: the tile's
//               points flattened with s fastest over the 256 threads: runs of up to 32 contiguous dense elements per i.
//   scatter     the same two phases in the other order: dense runs into LDS (transposed, conflict-free as above), then rows
//               of 64 contiguous field elements out.
//
// Nothing outside an item's window is read or written on the field side (not the halo, not the row padding, not other levels),
// nothing outside its ni * nj * nk elements on the dense side.  No atomics, no workspace, no host synchronisation.  The
// conversion is a plain cast; where the storage type is the dense type the value moves through registers and LDS as it is:
// -0.0, NaN payloads and denormals arrive unchanged.
#include "common.h"
#include "kernels.h"

#define CG_TI 64
#define CG_TS 32
#define CG_WAVES 4
#define CG_PITCH (CG_TI + 1)
#define CG_MAX_GRID 2048  // 256 CUs x 8 workgroups of 4 waves

template <typename DT, bool SCATTER>
__global__ void __launch_bounds__(64 * CG_WAVES) k_cube_xfer(Geo g, const pace_cube_item_t* __restrict__ items,
                                                              const int* __restrict__ first, int n, DT* dense) {
  __shared__ DT tile[CG_TS * CG_PITCH];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int total = first[n];
  for (int b = (int)blockIdx.x; b < total; b += (int)gridDim.x) {
    int m = 0, hi = n;  // first[m] <= b < first[hi]
    while (hi - m > 1) {
      const int mid = (m + hi) >> 1;
      if (b >= first[mid]) m = mid;
      else hi = mid;
    }
    const pace_cube_item_t it = items[m];
    const bool vol = it.kind == PACE_DIAG_WINDOW3D;
    const int ns = vol ? it.nk : it.nj;
    const int nts = (ns + CG_TS - 1) / CG_TS, nti = (it.ni + CG_TI - 1) / CG_TI;
    int t = b - first[m];
    const int sb = (t % nts) * CG_TS;
    t /= nts;
    const int ib = (t % nti) * CG_TI;
    const int j = t / nti;  // the row of a 3-D item's tile; 0 for a plane
    const int wi = it.ni - ib < CG_TI ? it.ni - ib : CG_TI;
    const int ws = ns - sb < CG_TS ? ns - sb : CG_TS;
    const long dstride = vol ? (long)it.nj * it.nk : (long)it.nj;  // dense elements between i and i + 1
    DT* d = dense + it.offset + (vol ? (long)j * it.nk : 0L) + sb + (long)ib * dstride;
    real* q = (real*)it.field;
    // the field element of (lane, s) of this tile
    const long f0 = vol ? IDX3(g, it.i0 + ib + lane, it.j0 + j, it.k0 + sb) : IDX2(g, it.i0 + ib + lane, it.j0 + sb);
    const long fs = vol ? g.sk : (long)g.sj;
    if (!SCATTER) {
      if (lane < wi)
        for (int s = wave; s < ws; s += CG_WAVES) tile[s * CG_PITCH + lane] = (DT)q[f0 + s * fs];
      __syncthreads();
      for (int f = (int)threadIdx.x; f < wi * ws; f += 64 * CG_WAVES) {
        const int li = f / ws, s = f - li * ws;
        d[(long)li * dstride + s] = tile[s * CG_PITCH + li];
      }
    } else {
      for (int f = (int)threadIdx.x; f < wi * ws; f += 64 * CG_WAVES) {
        const int li = f / ws, s = f - li * ws;
        tile[s * CG_PITCH + li] = d[(long)li * dstride + s];
      }
      __syncthreads();
      if (lane < wi)
        for (int s = wave; s < ws; s += CG_WAVES) q[f0 + s * fs] = (real)tile[s * CG_PITCH + lane];
    }
    __syncthreads();  // the next tile of this workgroup reuses the LDS
  }
}

int launch_cube_xfer(const Geo& g, const pace_cube_item_t* table_on_device, int n, int dense_is_double, void* dense, int scatter,
                     hipStream_t st) {
  const long most = (long)((g.ni + CG_TI - 1) / CG_TI) * ((g.nk + 1 + CG_TS - 1) / CG_TS) * g.nj;  // tiles of a whole field
  const long bound = most * n;
  const dim3 grid((unsigned)(bound < CG_MAX_GRID ? bound : CG_MAX_GRID)), block(64 * CG_WAVES);
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
