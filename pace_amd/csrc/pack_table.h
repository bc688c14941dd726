// What the table-driven kernels share (k_diag.hip, k_state.hip, k_restart.hip, k_ckpt.hip, k_gather.hip): a table of items that
// travels by value with its prefix table of per-item workgroup counts, and the dense-side phase of a transposed window tile.
// The maps themselves -- tile constants, tile count, tile of a linear index, table search -- are wgmap.h's.
#pragma once
#include "common.h"
#include "wgmap.h"

// A kernel takes it BY VALUE and indexes it in place (tab.item[m], table_find(tab.first, ...)): it lies in the kernel-argument
// segment and is read by scalar loads.  Taking its address for a function that is not inlined would copy it to scratch.
template <class Item, int MAX>
struct PackTable {
  Item item[MAX];
  int first[MAX + 1];  // first workgroup of each item; first[nitems] = the grid
  int nitems;
};

// first[m + 1] = first[m] + count(item[m]) for the nitems items already in the table
template <class Item, int MAX, class Count>
static inline int pack_table_fill_first(PackTable<Item, MAX>& tab, Count count) {
  long total = 0;
  for (int m = 0; m < tab.nitems; ++m) {
    total += count(tab.item[m]);
    if (total > 0x7fffffffL) return PACE_ERR_UNSUPPORTED;
    tab.first[m + 1] = (int)total;
  }
  return PACE_OK;
}

// The dense side of a wi x ws tile: its points flattened with s fastest over the 256 threads, so that a thread's neighbours
// move runs of up to 32 contiguous dense elements per i (8 points per thread).  `dense` is the tile's first element, `istride`
// the dense elements between i and i + 1, `step` the distance between two elements (k_state_unpack: one species of seven).
// The value is cast before it is staged.
template <class T, class S>
__device__ __forceinline__ void wt_runs_to_lds(T* __restrict__ tile, const S* __restrict__ dense, long istride, long step, int wi,
                                               int ws) {
  for (int f = (int)threadIdx.x; f < wi * ws; f += 64 * WT_WAVES) {
    const int li = f / ws, s = f - li * ws;
    tile[s * WT_PITCH + li] = (T)dense[((long)li * istride + s) * step];
  }
}
template <class T>
__device__ __forceinline__ void wt_lds_to_runs(T* __restrict__ dense, const T* __restrict__ tile, long istride, int wi, int ws) {
  for (int f = (int)threadIdx.x; f < wi * ws; f += 64 * WT_WAVES) {
    const int li = f / ws, s = f - li * ws;
    dense[(long)li * istride + s] = tile[s * WT_PITCH + li];
  }
}
