// The checkpointers of pace.util (util/pace/util/checkpointer/thresholds.py:59-162, validation.py:14-143) on the device: the
// calibration's running minimum / maximum / sum of magnitudes over trials, the thresholds derived from them, and the validation
// of a savepoint's variables against expected values under numpy's assert_allclose rules.  Up to PACE_CKPT_MAX_ITEMS variables
// per launch; a variable is a base pointer, logical extents (ni, nj, nk) in storage order and strides (1, sj, sk) -- no Geo:
// 2-D fields (nk = 1), dense 1-D arrays and the dycore's temporaries are variables too.  Field elements are widened to double
// first (exact); every accumulator, expected value and result is double in both libraries.
//
//   k_ckpt_accumulate          1-D grid, 256 threads = 4 waves.  A workgroup takes CK_ROWS * 4 consecutive rows (j, k) of one
//                              item, which it finds by table_find (wgmap.h) in the table that travels by value (pack_table.h).  A wave
//                              takes a row, lane l the points i = l, l + 64, ...: 512 B contiguous of the field and of each of
//                              the three dense accumulators (row r of them starts at r * ni).  first: plain stores; otherwise
//                              read-modify-write of the thread's own elements -- no atomics, and one accumulator per element
//                              added to in trial order, so asum has numpy's bits.
//   k_ckpt_thresholds_partial  the accumulators are dense, so the elements of an item are flattened over the threads: a workgroup
//                              takes CK_CHUNK = 256 * CK_PER consecutive elements, every load 64 contiguous doubles per wave.
//   k_ckpt_validate_partial    as k_ckpt_accumulate over the rows of the item's WINDOW: wave per row, lanes along i.  The expected
//                              values are addressed by their own three strides (an [x, z, y]-ordered or C-ordered target needs
//                              no transposing copy).  That read is STRIDED wherever the target's fastest axis is not x, which
//                              is the usual case -- an (x, y, z) field against a C-ordered slab: ei = nj * nk, the 64 lanes of
//                              a wave read 64 different lines.  The rows a wave walks are therefore consecutive along the axis
//                              of the smaller expected stride (k for that slab), so that a lane uses its lines whole.
//                              DESIGN.md 4.15 has what it costs.
//   k_ckpt_combine<N>          grid (nitems), one wave folds the item's partials first[m] .. first[m + 1] - 1.
//
// Both reductions are built as pace_state_extrema (k_driver.hip): partials, then a combine; EVERY workgroup writes its partial,
// the order of every fold is fixed by the launch shape; no atomics, no host synchronisation.  Within a workgroup the fold goes
// through LDS (ck_block_reduce_store).  The padding of a row (i >= ni) and, for validation, anything outside the window is
// never read.
#include "common.h"
#include "kernels.h"
#include "pack_table.h"

#define CK_WAVES 4
#define CK_ROWS 16                     // rows a wave walks (accumulate, validate)
#define CK_PER 32                      // elements a thread folds (thresholds)
#define CK_CHUNK (64 * CK_WAVES * CK_PER)

struct CkAccItem {
  const real* f;
  double *mn, *mx, *asum;
  long sj, sk;
  int ni, nj, nrows, pad_;
};
struct CkThrItem {
  const double *mn, *mx, *asum;
  long count;
};
struct CkValItem {
  const real* f;
  const double* expected;
  long sj, sk, ei, ej, ek;
  double rtol, atol;
  int i0, j0, k0, wi, wj, wk;
};
template <class Item>
using CkTable = PackTable<Item, PACE_CKPT_MAX_ITEMS>;

// ---- calibration: the fold of one trial ----------------------------------------------------------------------------------------
// numpy's minimum / maximum (loops_minmax: (a < b || isnan(a)) ? a : b): a NaN on either side gives NaN, and stays
__device__ __forceinline__ double ck_np_min(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double ck_np_max(double a, double b) { return (a > b || a != a) ? a : b; }

__global__ void __launch_bounds__(64 * CK_WAVES) k_ckpt_accumulate(CkTable<CkAccItem> tab, int first) {
  const int b = (int)blockIdx.x;
  const int m = table_find(tab.first, tab.nitems, b);
  const CkAccItem& it = tab.item[m];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int r0 = ((b - tab.first[m]) * CK_WAVES + wave) * CK_ROWS;
  const real* __restrict__ q = it.f;
  for (int u = 0; u < CK_ROWS; ++u) {
    const int r = r0 + u;
    if (r >= it.nrows) break;  // (wave-uniform)
    const int k = r / it.nj, j = r - k * it.nj;
    const real* __restrict__ row = q + (long)j * it.sj + (long)k * it.sk;
    double* __restrict__ mn = it.mn + (long)r * it.ni;
    double* __restrict__ mx = it.mx + (long)r * it.ni;
    double* __restrict__ asum = it.asum + (long)r * it.ni;
    for (int i = lane; i < it.ni; i += 64) {
      const double v = (double)row[i];
      const double a = fabs(v);
      if (first) {  // (uniform over the launch)
        mn[i] = v;
        mx[i] = v;
        asum[i] = a;
      } else {
        const double lo = mn[i], hi = mx[i], sum = asum[i];  // (the four loads first, then the three stores)
        mn[i] = ck_np_min(lo, v);
        mx[i] = ck_np_max(hi, v);
        asum[i] = sum + a;
      }
    }
  }
}

// ---- the folds of the two reductions -------------------------------------------------------------------------------------------
// thresholds: [0] nanmax (NaN = nothing yet), [1] max that keeps a NaN, [2] all zero (1 / 0), [3] a count
struct CkThr {
  double rel, absolute, all_zero, nan_count;
};
__device__ __forceinline__ void ck_fold(CkThr& a, const CkThr& b) {
  a.rel = (b.rel > a.rel || a.rel != a.rel) ? b.rel : a.rel;
  a.absolute = (b.absolute > a.absolute || b.absolute != b.absolute) ? b.absolute : a.absolute;
  a.all_zero = (a.all_zero != 0.0 && b.all_zero != 0.0) ? 1.0 : 0.0;
  a.nan_count += b.nan_count;
}
__device__ __forceinline__ CkThr ck_identity(const CkThr*) { return CkThr{NAN, -INFINITY, 1.0, 0.0}; }
__device__ __forceinline__ void ck_finalise(CkThr&) {}  // (what the combine does to an item's result before it is written)

// validation: two counts, two maxima, the smallest index (+inf = none), a count
struct CkVal {
  double nrel, nabs, max_abs, max_rel, first_index, compared;
};
__device__ __forceinline__ void ck_fold(CkVal& a, const CkVal& b) {
  a.nrel += b.nrel;
  a.nabs += b.nabs;
  a.max_abs = b.max_abs > a.max_abs ? b.max_abs : a.max_abs;
  a.max_rel = b.max_rel > a.max_rel ? b.max_rel : a.max_rel;
  a.first_index = b.first_index < a.first_index ? b.first_index : a.first_index;
  a.compared += b.compared;
}
__device__ __forceinline__ CkVal ck_identity(const CkVal*) { return CkVal{0.0, 0.0, 0.0, 0.0, INFINITY, 0.0}; }
__device__ __forceinline__ void ck_finalise(CkVal& e) {  // no violating element: -1
  if (!(e.first_index < INFINITY)) e.first_index = -1.0;
}

// a result as N doubles (CkThr: 4, CkVal: 6)
template <class R>
struct CkWords {
  static constexpr int N = (int)(sizeof(R) / sizeof(double));
};

// every thread of the NT-thread workgroup must call it; thread 0 writes the workgroup's result to out[0 .. N - 1].  The fold
// goes through LDS in steps of eight -- 256 -> 32 -> 4 -> 1: three barriers -- and not through wave shuffles: a result is up
// to six doubles, six shuffle steps of six words each per wave and launch are more instructions than these few LDS reads, it
// happens once per workgroup beside 64 rows of streaming, and the emulated tier pays per shuffle.  A thread writes back only its
// own entry and reads, beside it, entries no thread of the step writes: one barrier per step.
// FINAL: the result is an item's, not a partial: ck_finalise is applied to it.
template <class R, int NT, bool FINAL = false>
__device__ __forceinline__ void ck_block_reduce_store(R e, double* out) {
  __shared__ R part[NT];
  const int t = (int)threadIdx.x;
  part[t] = e;
  for (int live = NT; live > 1;) {
    const int n = live >= 8 ? live / 8 : 1;  // threads that fold in this step, live / n entries each
    const int per = live / n;
    __syncthreads();
    if (t < n) {
      for (int v = 1; v < per; ++v) ck_fold(e, part[t + n * v]);
      part[t] = e;
    }
    live = n;
  }
  if (t == 0) {
    if (FINAL) ck_finalise(e);
    const double* w = reinterpret_cast<const double*>(&e);
    for (int n = 0; n < CkWords<R>::N; ++n) out[n] = w[n];
  }
}

// ---- calibration: the thresholds -----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64 * CK_WAVES) k_ckpt_thresholds_partial(CkTable<CkThrItem> tab, double n_trials,
                                                                            double* __restrict__ partial) {
  const int b = (int)blockIdx.x;
  const int m = table_find(tab.first, tab.nitems, b);
  const CkThrItem& it = tab.item[m];
  const long e0 = (long)(b - tab.first[m]) * CK_CHUNK;
  CkThr acc = ck_identity((const CkThr*)nullptr);
  for (int u = 0; u < CK_PER; ++u) {
    const long e = e0 + u * (64 * CK_WAVES) + (long)threadIdx.x;
    if (e < it.count) {
      const double spread = it.mx[e] - it.mn[e];
      const double mean_abs = it.asum[e] / n_trials;
      const double quotient = spread / mean_abs;  // 0 / 0 is NaN and is skipped; x / 0 is inf and counts
      ck_fold(acc, CkThr{quotient, spread, mean_abs == 0.0 ? 1.0 : 0.0, spread != spread ? 1.0 : 0.0});
    }
  }
  ck_block_reduce_store<CkThr, 64 * CK_WAVES>(acc, partial + (long)b * 4);
}

// ---- validation ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64 * CK_WAVES) k_ckpt_validate_partial(CkTable<CkValItem> tab, double* __restrict__ partial) {
  const int b = (int)blockIdx.x;
  const int m = table_find(tab.first, tab.nitems, b);
  const CkValItem& it = tab.item[m];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int r0 = ((b - tab.first[m]) * CK_WAVES + wave) * CK_ROWS;
  // the rows of a wave follow one another along whichever of j and k the expected values are closer together in: for a
  // C-ordered slab that is k (ek = 1), and a lane's sixteen rows read two lines of the expected array instead of sixteen
  const bool k_fastest = it.ek < it.ej;
  const int nrows = it.wj * it.wk;
  const bool rel_on = it.rtol == it.rtol, abs_on = it.atol == it.atol;  // a NaN tolerance: that test is skipped
  const real* __restrict__ q = it.f;
  const double* __restrict__ x = it.expected;
  CkVal acc = ck_identity((const CkVal*)nullptr);
  int nrel = 0, nabs = 0, compared = 0;
  for (int u = 0; u < CK_ROWS; ++u) {
    const int r = r0 + u;
    if (r >= nrows) break;  // (wave-uniform)
    const int k = k_fastest ? r % it.wk : r / it.wj, j = k_fastest ? r / it.wk : r - k * it.wj;
    const real* __restrict__ row = q + it.i0 + (long)(it.j0 + j) * it.sj + (long)(it.k0 + k) * it.sk;
    const long x0 = (long)j * it.ej + (long)k * it.ek;
    for (int i = lane; i < it.wi; i += 64) {
      const long index = x0 + (long)i * it.ei;
      const double a = (double)row[i];
      const double d = x[index];
      const bool a_nan = a != a, d_nan = d != d;
      bool bad_rel, bad_abs;
      if (a_nan || d_nan) {
        bad_abs = a_nan != d_nan;
        bad_rel = d != 0.0 && bad_abs;  // (the relative test sees only d != 0; a NaN d is "not zero")
      } else if (fabs(a) == INFINITY || fabs(d) == INFINITY) {
        bad_abs = !(a == d);
        bad_rel = d != 0.0 && bad_abs;
      } else {
        const double err = fabs(a - d);
        bad_abs = !(err <= it.atol);
        bad_rel = d != 0.0 && !(err <= it.rtol * fabs(d));
        acc.max_abs = err > acc.max_abs ? err : acc.max_abs;
        if (d != 0.0) {
          const double rel = err / fabs(d);
          acc.max_rel = rel > acc.max_rel ? rel : acc.max_rel;
        }
      }
      bad_rel = bad_rel && rel_on;
      bad_abs = bad_abs && abs_on;
      nrel += bad_rel;
      nabs += bad_abs;
      compared += 1;
      if ((bad_rel || bad_abs) && (double)index < acc.first_index) acc.first_index = (double)index;
    }
  }
  acc.nrel = (double)nrel;
  acc.nabs = (double)nabs;
  acc.compared = (double)compared;
  ck_block_reduce_store<CkVal, 64 * CK_WAVES>(acc, partial + (long)b * 6);
}

// ---- stage two -----------------------------------------------------------------------------------------------------------------
struct CkFirst {
  int first[PACE_CKPT_MAX_ITEMS + 1];
};
template <class Item>
static inline CkFirst ck_firsts(const CkTable<Item>& tab) {  // the prefix table alone, for the combine
  CkFirst f;
  memcpy(f.first, tab.first, sizeof(f.first));
  return f;
}

template <class R>
__global__ void __launch_bounds__(64) k_ckpt_combine(CkFirst tab, const double* __restrict__ partial, double* __restrict__ out) {
  constexpr int N = CkWords<R>::N;
  const int m = (int)blockIdx.x;
  R e = ck_identity((const R*)nullptr);
  for (int b = tab.first[m] + (int)threadIdx.x; b < tab.first[m + 1]; b += 64) {
    R p;
    double* w = reinterpret_cast<double*>(&p);
    for (int n = 0; n < N; ++n) w[n] = partial[(long)b * N + n];
    ck_fold(e, p);
  }
  ck_block_reduce_store<R, 64, true>(e, out + (long)m * N);
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
static inline long ck_row_blocks(long rows) { return (rows + CK_WAVES * CK_ROWS - 1) / (CK_WAVES * CK_ROWS); }
static inline long ck_chunk_blocks(long count) { return (count + CK_CHUNK - 1) / CK_CHUNK; }

long ckpt_thresholds_blocks(const pace_ckpt_item_t* items, int nitems) {
  long blocks = 0;
  for (int m = 0; m < nitems; ++m) blocks += ck_chunk_blocks((long)items[m].ni * items[m].nj * items[m].nk);
  return blocks;
}
long ckpt_validate_blocks(const pace_ckpt_item_t* items, int nitems) {
  long blocks = 0;
  for (int m = 0; m < nitems; ++m) blocks += ck_row_blocks((long)items[m].wj * items[m].wk);
  return blocks;
}

int launch_ckpt_accumulate(const pace_ckpt_item_t* items, int nitems, int first, hipStream_t st) {
  CkTable<CkAccItem> tab{};
  tab.nitems = nitems;
  for (int m = 0; m < nitems; ++m) {
    const pace_ckpt_item_t& it = items[m];
    tab.item[m] = CkAccItem{it.field, it.mn, it.mx, it.asum, (long)it.sj, (long)it.sk, it.ni, it.nj, it.nj * it.nk, 0};
  }
  const int rc = pack_table_fill_first(tab, [](const CkAccItem& it) { return ck_row_blocks(it.nrows); });
  if (rc != PACE_OK) return rc;
  hipLaunchKernelGGL(k_ckpt_accumulate, dim3((unsigned)tab.first[nitems]), dim3(64 * CK_WAVES), 0, st, tab, first);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}

int launch_ckpt_thresholds(const pace_ckpt_item_t* items, int nitems, int n_trials, void* workspace, double* out, hipStream_t st) {
  CkTable<CkThrItem> tab{};
  tab.nitems = nitems;
  for (int m = 0; m < nitems; ++m) {
    const pace_ckpt_item_t& it = items[m];
    tab.item[m] = CkThrItem{it.mn, it.mx, it.asum, (long)it.ni * it.nj * it.nk};
  }
  const int rc = pack_table_fill_first(tab, [](const CkThrItem& it) { return ck_chunk_blocks(it.count); });
  if (rc != PACE_OK) return rc;
  const CkFirst firsts = ck_firsts(tab);
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(k_ckpt_thresholds_partial, dim3((unsigned)tab.first[nitems]), dim3(64 * CK_WAVES), 0, st, tab, (double)n_trials, partial);
  PACE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_ckpt_combine<CkThr>, dim3((unsigned)nitems), dim3(64), 0, st, firsts, partial, out);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}

int launch_ckpt_validate(const pace_ckpt_item_t* items, int nitems, void* workspace, double* out, hipStream_t st) {
  CkTable<CkValItem> tab{};
  tab.nitems = nitems;
  for (int m = 0; m < nitems; ++m) {
    const pace_ckpt_item_t& it = items[m];
    tab.item[m] = CkValItem{it.field, it.expected, (long)it.sj, (long)it.sk, (long)it.ei, (long)it.ej, (long)it.ek, it.rtol, it.atol,
                            it.i0, it.j0, it.k0, it.wi, it.wj, it.wk};
  }
  const int rc = pack_table_fill_first(tab, [](const CkValItem& it) { return ck_row_blocks((long)it.wj * it.wk); });
  if (rc != PACE_OK) return rc;
  const CkFirst firsts = ck_firsts(tab);
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(k_ckpt_validate_partial, dim3((unsigned)tab.first[nitems]), dim3(64 * CK_WAVES), 0, st, tab, partial);
  PACE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_ckpt_combine<CkVal>, dim3((unsigned)nitems), dim3(64), 0, st, firsts, partial, out);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
