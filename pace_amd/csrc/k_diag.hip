// The driver's diagnostics (driver/pace/driver/diagnostics.py:144-253): everything a diagnostics step asks for -- compute windows
// of 3-D fields, planes (2-D fields and single levels), column integrals -- gathered, TRANSPOSED to the files' axis order,
// narrowed to the output type and written to ONE packed device buffer by one launch per PACE_DIAG_MAX_ITEMS items, so that the
// host gets it all with one transfer and one synchronisation.
//
// Fields are stored [k][j][i], i fastest, rows padded (IDX3); the reference's files hold (x, y, z) in C order, z fastest.  An
// item's output is therefore out[(i * nj + j) * nk + k] (WINDOW3D) or out[i * nj + j] (PLANE, COLUMN_INTEGRAL): the fastest
// axis of the output, called s below, is k for a 3-D item and j for a plane, and never i.
//
//   k_diag_pack   1-D grid, 256 threads = 4 waves.  A workgroup takes one window tile (wgmap.h: 64 points in i by 32 in s, so 32
//                 levels of a 3-D item) of the item that table_find gives it; the table travels by value (pack_table.h).
//                   read    wave w takes s = w, w + 4, ...; lane l reads i = l of that row: 64 contiguous elements.  A column
//                           integral's lane walks its column there, k ascending, one double accumulator, product then add;
//                           its tile is only WT_TS_COLUMN = 4 rows in s (one per wave) and its workgroups come first in the
//                           grid: with 32 rows a C192 plane was 18 workgroups of 8 columns per lane, the longest of the launch.
//                   LDS     tile[s][i] of the OUTPUT type at wgmap.h's pitch: the transposed accesses are the reads.
//                   write   wt_lds_to_runs: runs of up to 32 contiguous output elements per i (128 B of float32).
//
// Nothing outside an item's window is read (not the halo, not the levels outside k0 .. k0 + nk - 1, not the row padding), and
// nothing outside its ni * nj * nk (ni * nj) output elements is written.  No atomics, no workspace.  The narrowing is a plain
// cast: round to nearest even, overflow to +-inf, as ndarray.astype(np.float32).
#include "common.h"
#include "kernels.h"
#include "pack_table.h"
#include "thermo.h"

typedef PackTable<pace_diag_item_t, PACE_DIAG_MAX_ITEMS> DiagTable;
__host__ __device__ __forceinline__ int diag_tile_rows(int kind) { return kind == PACE_DIAG_COLUMN_INTEGRAL ? WT_TS_COLUMN : WT_TS; }

template <typename OutT>
__global__ void __launch_bounds__(64 * WT_WAVES) k_diag_pack(Geo g, DiagTable tab, OutT* __restrict__ out) {
  const int b = (int)blockIdx.x;
  const int m = table_find(tab.first, tab.nitems, b);
  const pace_diag_item_t& it = tab.item[m];
  const bool vol = it.kind == PACE_DIAG_WINDOW3D;
  const WindowTile wt = window_tile_of_linear(b - tab.first[m], it.ni, it.nj, it.nk, vol, diag_tile_rows(it.kind));
  const int sb = wt.sb, ib = wt.ib, j = wt.j, wi = wt.wi, ws = wt.ws;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;

  __shared__ OutT tile[WT_TS * WT_PITCH];
  const real* __restrict__ q = it.field;
  if (lane < wi) {
    const int i = it.i0 + ib + lane;
    for (int s = wave; s < ws; s += WT_WAVES) {
      OutT v;
      if (vol) {
        v = (OutT)q[IDX3(g, i, it.j0 + j, it.k0 + sb + s)];
      } else if (it.kind == PACE_DIAG_PLANE) {
        v = (OutT)q[IDX2(g, i, it.j0 + sb + s)];
      } else {
        const real* __restrict__ w = it.weight;
        const long c = IDX3(g, i, it.j0 + sb + s, it.k0);
        double acc = 0.0;
#pragma unroll 4  // (the loads of four levels in flight; the sum keeps its order)
        for (int k = 0; k < it.nk; ++k) {
          const double p = (double)q[c + k * g.sk] * (double)w[c + k * g.sk];
          acc = acc + p;
        }
        v = (OutT)(phys::RGRAV * acc);
      }
      tile[s * WT_PITCH + lane] = v;
    }
  }
  __syncthreads();
  const long ostride = vol ? (long)it.nj * it.nk : (long)it.nj;  // output elements between i and i + 1
  wt_lds_to_runs(out + it.out_offset + (vol ? (long)j * it.nk : 0L) + sb + (long)ib * ostride, tile, ostride, wi, ws);
}

int launch_diag_pack(const Geo& g, const pace_diag_item_t* items, int nitems, int out_is_double, void* out, hipStream_t st) {
  DiagTable tab{};
  tab.nitems = nitems;
  // the column integrals first: their lanes walk whole columns, the longest a workgroup of this launch runs, so they start
  // with the launch and the windows' workgroups fill the machine beside them (an item says where its output goes: any order)
  int m = 0;
  for (int column = 1; column >= 0; --column)
    for (int r = 0; r < nitems; ++r)
      if ((items[r].kind == PACE_DIAG_COLUMN_INTEGRAL) == (column == 1)) tab.item[m++] = items[r];
  const int rc = pack_table_fill_first(tab, [](const pace_diag_item_t& it) {
    return window_tiles(it.ni, it.nj, it.nk, it.kind == PACE_DIAG_WINDOW3D, diag_tile_rows(it.kind));
  });
  if (rc != PACE_OK) return rc;
  const dim3 grid((unsigned)tab.first[nitems]), block(64 * WT_WAVES);
  if (out_is_double) hipLaunchKernelGGL(k_diag_pack<double>, grid, block, 0, st, g, tab, (double*)out);
  else hipLaunchKernelGGL(k_diag_pack<float>, grid, block, 0, st, g, tab, (float*)out);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
