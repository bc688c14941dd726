// The driver's diagnostics (driver/pace/driver/diagnostics.py:144-253): everything a diagnostics step asks for -- compute windows
// of 3-D fields, planes (2-D fields and single levels), column integrals -- gathered, TRANSPOSED to the files' axis order,
// narrowed to the output type and written to ONE packed device buffer by one launch per PACE_DIAG_MAX_ITEMS items, so that the
// host gets it all with one transfer and one synchronisation.
//
// Fields are stored [k][j][i], i fastest, rows padded (IDX3); the reference's files hold (x, y, z) in C order, z fastest.  An
// item's output is therefore out[(i * nj + j) * nk + k] (WINDOW3D) or out[i * nj + j] (PLANE, COLUMN_INTEGRAL): the fastest
// axis of the output, called s below, is k for a 3-D item and j for a plane, and never i.
//
//   k_diag_pack   1-D grid, 256 threads = 4 waves.  A workgroup takes one tile of DG_TI = 64 points in i by DG_TS = 32 points in s
//                 (a 3-D item: at one j; so TK = 32 levels), and finds its item by a bisection of the prefix table of per-item tile
//                 counts, which travels by value with the items (workgroup-uniform: scalar loads and scalar branches only).
//                   read    wave w takes s = w, w + 4, ...; lane l reads i = l of that row: 64 contiguous elements.  A column
//                           integral's lane walks its column there, k ascending, one double accumulator, product then add;
//                           its tile is only 4 rows in s (one per wave) and its workgroups come first in the grid: with
//                           32 rows a C192 plane was 18 workgroups of 8 columns per lane, the longest of the launch.
//                   LDS     tile[s][i] of the OUTPUT type, pitch DG_PITCH = 65 elements.  The row writes are 64 consecutive
//                           elements: conflict-free.  The transposed reads of a 32-lane group are s = 0 .. 31 at one i: element
//                           address 65 * s + i, bank (s + i) mod 32 for ds_read_b32 and 2 * ((s + i) mod 32) of 64 for
//                           ds_read_b64 -- 32 different banks (MI355X_MICROARCH.md, LDS: 64 banks of 4 B, groups of 32 lanes).
//                           A pitch of 64 would put all 32 on one bank.  A tile narrower than 32 in s (the last 15 of 79 levels)
//                           mixes two or three i in a group and takes up to 3 lanes per bank.
//                   write   the tile's points flattened with s fastest over the 256 threads: runs of up to 32 contiguous output
//                           elements per i (128 B of float32), 8 points per thread.
//
// Nothing outside an item's window is read (not the halo, not the levels outside k0 .. k0 + nk - 1, not the row padding), and
// nothing outside its ni * nj * nk (ni * nj) output elements is written.  No atomics, no workspace.  The narrowing is a plain
// cast: round to nearest even, overflow to +-inf, as ndarray.astype(np.float32).
#include "common.h"
#include "kernels.h"
#include "thermo.h"

#define DG_TI 64
#define DG_TS 32  // = TK, the k tile of a 3-D item
#define DG_WAVES 4
#define DG_TS_COLUMN DG_WAVES  // rows of a column integral's tile: one per wave
#define DG_PITCH (DG_TI + 1)

struct DiagTable {
  pace_diag_item_t item[PACE_DIAG_MAX_ITEMS];
  int first[PACE_DIAG_MAX_ITEMS + 1];  // first tile of each item; first[nitems] = the grid
  int nitems;
};

// tiles of an item: s tiles fastest, then i tiles, then (3-D) the rows j
static inline int diag_tiles(const pace_diag_item_t& it) {
  const int ns = it.kind == PACE_DIAG_WINDOW3D ? it.nk : it.nj;
  const int ts = it.kind == PACE_DIAG_COLUMN_INTEGRAL ? DG_TS_COLUMN : DG_TS;
  const int per_row = ((it.ni + DG_TI - 1) / DG_TI) * ((ns + ts - 1) / ts);
  return it.kind == PACE_DIAG_WINDOW3D ? per_row * it.nj : per_row;
}

template <typename OutT>
__global__ void __launch_bounds__(64 * DG_WAVES) k_diag_pack(Geo g, DiagTable tab, OutT* __restrict__ out) {
  const int b = (int)blockIdx.x;
  int m = 0, hi = tab.nitems;  // first[m] <= b < first[hi]
  while (hi - m > 1) {
    const int mid = (m + hi) >> 1;
    if (b >= tab.first[mid]) m = mid;
    else hi = mid;
  }
  const pace_diag_item_t& it = tab.item[m];
  const bool vol = it.kind == PACE_DIAG_WINDOW3D;
  const int ns = vol ? it.nk : it.nj;
  const int ts = it.kind == PACE_DIAG_COLUMN_INTEGRAL ? DG_TS_COLUMN : DG_TS;
  const int nts = (ns + ts - 1) / ts, nti = (it.ni + DG_TI - 1) / DG_TI;
  int t = b - tab.first[m];
  const int sb = (t % nts) * ts;
  t /= nts;
  const int ib = (t % nti) * DG_TI;
  const int j = t / nti;  // the row of a 3-D item's tile; 0 for a plane
  const int wi = it.ni - ib < DG_TI ? it.ni - ib : DG_TI;
  const int ws = ns - sb < ts ? ns - sb : ts;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;

  __shared__ OutT tile[DG_TS * DG_PITCH];
  const real* __restrict__ q = it.field;
  if (lane < wi) {
    const int i = it.i0 + ib + lane;
    for (int s = wave; s < ws; s += DG_WAVES) {
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
      tile[s * DG_PITCH + lane] = v;
    }
  }
  __syncthreads();
  const long ostride = vol ? (long)it.nj * it.nk : (long)it.nj;  // output elements between i and i + 1
  OutT* __restrict__ o = out + it.out_offset + (vol ? (long)j * it.nk : 0L) + sb + (long)ib * ostride;
  for (int f = (int)threadIdx.x; f < wi * ws; f += 64 * DG_WAVES) {
    const int li = f / ws, s = f - li * ws;
    o[(long)li * ostride + s] = tile[s * DG_PITCH + li];
  }
}

int launch_diag_pack(const Geo& g, const pace_diag_item_t* items, int nitems, int out_is_double, void* out, hipStream_t st) {
  DiagTable tab{};
  tab.nitems = nitems;
  // the column integrals first: their lanes walk whole columns, the longest a workgroup of this launch runs, so they start
  // with the launch and the windows' workgroups fill the machine beside them (an item says where its output goes: any order)
  long tiles = 0;
  int m = 0;
  for (int column = 1; column >= 0; --column)
    for (int r = 0; r < nitems; ++r) {
      if ((items[r].kind == PACE_DIAG_COLUMN_INTEGRAL) != (column == 1)) continue;
      tab.item[m] = items[r];
      tiles += diag_tiles(items[r]);
      if (tiles > 0x7fffffffL) return PACE_ERR_UNSUPPORTED;
      tab.first[++m] = (int)tiles;
    }
  const dim3 grid((unsigned)tab.first[nitems]), block(64 * DG_WAVES);
  if (out_is_double) hipLaunchKernelGGL(k_diag_pack<double>, grid, block, 0, st, g, tab, (double*)out);
  else hipLaunchKernelGGL(k_diag_pack<float>, grid, block, 0, st, g, tab, (float*)out);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
