// Nudging (util/pace/util/nudging.py:44,70): the state relaxed toward a reference that is held or interpolated in time between
// the two ends of a bracket.  Up to PACE_NUDGE_MAX_ITEMS windows of fields per launch.  For every point of an item's window, in
// double on the stored values (the float32 library widens first), with no contraction and no reciprocal, in exactly this order:
//
//   r = ref1 ? r0 + (r1 - r0) * weight : r0
//   t = (r - q) / timescale
//   if tendency:  tendency = (real) t
//   if apply:     field    = (real)(q + t * dt)
//
//   k_nudge  1-D grid, 256 threads = 4 waves, k_ckpt_accumulate's form.  A workgroup takes NG_ROWS * 4 consecutive rows (j, k) of
//            the window of one item, which it finds by table_find (wgmap.h) in the table that travels by value (pack_table.h).  A
//            wave takes a row, lane l the points i = l, l + 64, ...: 512 B contiguous (float32: 256 B) of each of the up to four
//            arrays.  The device-side item holds the four pointers ALREADY at the window's first element -- the four share one
//            storage geometry, so one offset serves them all -- and the window's row extents: 56 B an item, 1.9 KB the table.
//            The three loads of an element are issued before its arithmetic; an element is read and written by the same thread,
//            so in place is safe.  Whether there is a ref1 and a tendency is per item, hence workgroup-uniform; apply is uniform
//            over the launch.
//
// Nothing outside a window is written (not the halo, not level nk, not the row padding), nothing outside the windows' elements is
// read, and with apply == 0 the field is only read.  No atomics, no workspace, no LDS.
#include "common.h"
#include "kernels.h"
#include "pack_table.h"

#define NG_WAVES 4
#ifndef NG_ROWS
#define NG_ROWS 4  // rows a wave walks
#endif

struct NudgeDevItem {
  real* q;  // the four at the window's first element
  const real *r0, *r1;
  real* t;
  double timescale;
  int ni, nj, nrows, pad_;
};
typedef PackTable<NudgeDevItem, PACE_NUDGE_MAX_ITEMS> NudgeTable;

__global__ void __launch_bounds__(64 * NG_WAVES) k_nudge(NudgeTable tab, long sj, long sk, double weight, double dt, int apply) {
  const int b = (int)blockIdx.x;
  const int m = table_find(tab.first, tab.nitems, b);
  const NudgeDevItem& it = tab.item[m];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int r0 = ((b - tab.first[m]) * NG_WAVES + wave) * NG_ROWS;
  const double tau = it.timescale;
  const bool interpolate = it.r1 != nullptr, store_t = it.t != nullptr;
  for (int u = 0; u < NG_ROWS; ++u) {
    const int r = r0 + u;
    if (r >= it.nrows) break;  // (wave-uniform)
    const int k = r / it.nj, j = r - k * it.nj;
    const long row = (long)j * sj + (long)k * sk;
    // (no __restrict__: ref0 and ref1 may be one array, and field is written in place)
    real* q = it.q + row;
    const real* a = it.r0 + row;
    const real* e = interpolate ? it.r1 + row : a;
    real* t = store_t ? it.t + row : nullptr;
    for (int i = lane; i < it.ni; i += 64) {
      const double qv = (double)q[i];
      const double av = (double)a[i];
      double ref = av;
      if (interpolate) {
        const double ev = (double)e[i];
        ref = av + (ev - av) * weight;
      }
      const double tend = (ref - qv) / tau;
      if (store_t) t[i] = (real)tend;
      if (apply) q[i] = (real)(qv + tend * dt);
    }
  }
}

static inline long ng_row_blocks(long rows) { return (rows + NG_WAVES * NG_ROWS - 1) / (NG_WAVES * NG_ROWS); }

int launch_nudge(const Geo& g, const pace_nudge_item_t* items, int nitems, double weight, double dt, int apply, hipStream_t st) {
  NudgeTable tab{};
  static_assert(sizeof(NudgeTable) <= 2048, "the table must stay well inside the 4 KB kernel-argument segment");
  tab.nitems = nitems;
  for (int m = 0; m < nitems; ++m) {
    const pace_nudge_item_t& it = items[m];
    const long origin = IDX3(g, it.i0, it.j0, it.k0);  // (a plane: k0 = 0, nk = 1)
    tab.item[m] = NudgeDevItem{it.field + origin,
                               it.ref0 + origin,
                               it.ref1 ? it.ref1 + origin : nullptr,
                               it.tendency ? it.tendency + origin : nullptr,
                               it.timescale,
                               it.ni,
                               it.nj,
                               it.nj * it.nk,
                               0};
  }
  const int rc = pack_table_fill_first(tab, [](const NudgeDevItem& it) { return ng_row_blocks(it.nrows); });
  if (rc != PACE_OK) return rc;
  hipLaunchKernelGGL(k_nudge, dim3((unsigned)tab.first[nitems]), dim3(64 * NG_WAVES), 0, st, tab, (long)g.sj, g.sk, weight, dt, apply);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
