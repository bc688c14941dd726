// The driver's per-step sanity check of the state (driver/pace/driver/safety_checks.py:80-110): the minimum, the maximum and the
// NaN counts of up to PACE_STATE_EXTREMA_MAX_FIELDS fields in one launch pair, so that the host decides about every registered
// variable after ONE transfer of 4 doubles per field.
//
//   k_state_extrema_partial   grid (nblk, nfields), 256 threads = 4 waves.  A row of the window (i contiguous) is read by one
//                             wave, lane l takes i = i0 + l, i0 + l + 64, ...; a wave takes SX_ROWS consecutive rows, a
//                             workgroup 4 * SX_ROWS.  The four numbers are reduced over the 64 lanes by shuffles, over the four
//                             waves through LDS, and thread 0 writes the workgroup's partial: EVERY workgroup writes one (the
//                             identity where it has no row), so the workspace needs no clearing and no stale value is ever read.
//   k_state_extrema_combine   grid (nfields), one wave: lane l folds partials l, l + 64, ..., then the same shuffles.
//
// No atomics: the order of every fold is fixed by the launch shape, and min / max / integer sums do not depend on it anyway.
// The window of a field is the compute domain, origin (3, 3, 0), extent (n, n, nk), or the logical storage (n + 7, n + 7, nk + 1);
// the padding of a row beyond n + 7 is never read.  min / max skip NaNs by the comparisons being false for them; +-inf are
// values.  Counts are kept as 32-bit integers per thread (at most SX_ROWS rows) and as doubles from the partials on (exact:
// a field has fewer than 2^32 elements, geom_check).
#include "common.h"
#include "kernels.h"

#define SX_ROWS 8   // rows a wave walks
#define SX_WAVES 4  // waves of a stage-one workgroup

struct ExtremaFields {
  const real* f[PACE_STATE_EXTREMA_MAX_FIELDS];
  unsigned compute_only;  // bit m: field m is looked at over its compute domain only
};

struct Extrema {
  double mn, mx, nan_window, nan_compute;
};

__device__ __forceinline__ void extrema_fold(Extrema& a, const Extrema& b) {
  a.mn = b.mn < a.mn ? b.mn : a.mn;
  a.mx = b.mx > a.mx ? b.mx : a.mx;
  a.nan_window += b.nan_window;
  a.nan_compute += b.nan_compute;
}

// every lane of the wave must call it; lane 0 ends with the wave's result
__device__ __forceinline__ void extrema_wave_reduce(Extrema& e) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    Extrema o;
    o.mn = __shfl_down(e.mn, (unsigned)d, 64);
    o.mx = __shfl_down(e.mx, (unsigned)d, 64);
    o.nan_window = __shfl_down(e.nan_window, (unsigned)d, 64);
    o.nan_compute = __shfl_down(e.nan_compute, (unsigned)d, 64);
    extrema_fold(e, o);
  }
}

__global__ void __launch_bounds__(64 * SX_WAVES) k_state_extrema_partial(Geo g, ExtremaFields fields, double* __restrict__ partial) {
  const int m = (int)blockIdx.y;
  const bool compute_only = (fields.compute_only >> m) & 1u;
  const real* __restrict__ q = fields.f[m];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  // the window: w points of a row from i0, h rows of a level from j0, nlev levels
  const int i0 = compute_only ? g.is : 0, w = compute_only ? g.n : g.ni;
  const int j0 = compute_only ? g.js : 0, h = compute_only ? g.n : g.nj;
  const int nlev = compute_only ? g.nk : g.nk + 1;
  const long rows = (long)h * nlev;
  const long r0 = ((long)blockIdx.x * SX_WAVES + wave) * SX_ROWS;

  double mn = INFINITY, mx = -INFINITY;
  int nan_window = 0, nan_compute = 0;
  for (int u = 0; u < SX_ROWS; ++u) {
    const long r = r0 + u;
    if (r >= rows) break;  // (wave-uniform)
    const int k = (int)(r / h);
    const int j = j0 + (int)(r - (long)k * h);
    const bool row_in_compute = compute_only || (k < g.nk && j >= g.js && j <= g.je);
    const real* __restrict__ row = q + IDX3(g, 0, j, k);
    for (int i = i0 + lane; i < i0 + w; i += 64) {
      const double v = (double)row[i];
      mn = v < mn ? v : mn;
      mx = v > mx ? v : mx;
      const int is_nan = v != v;
      nan_window += is_nan;
      nan_compute += (row_in_compute && i >= g.is && i <= g.ie) ? is_nan : 0;
    }
  }

  Extrema e{mn, mx, (double)nan_window, (double)nan_compute};
  extrema_wave_reduce(e);
  __shared__ Extrema per_wave[SX_WAVES];
  if (lane == 0) per_wave[wave] = e;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int v = 1; v < SX_WAVES; ++v) extrema_fold(e, per_wave[v]);
    double* out = partial + ((long)m * gridDim.x + blockIdx.x) * 4;
    out[0] = e.mn;
    out[1] = e.mx;
    out[2] = e.nan_window;
    out[3] = e.nan_compute;
  }
}

__global__ void __launch_bounds__(64) k_state_extrema_combine(const double* __restrict__ partial, int nblk, double* __restrict__ out) {
  const int m = (int)blockIdx.x;
  Extrema e{INFINITY, -INFINITY, 0.0, 0.0};
  for (int b = (int)threadIdx.x; b < nblk; b += 64) {
    const double* p = partial + ((long)m * nblk + b) * 4;
    extrema_fold(e, Extrema{p[0], p[1], p[2], p[3]});
  }
  extrema_wave_reduce(e);
  if (threadIdx.x == 0) {
    out[4 * m + 0] = e.mn;
    out[4 * m + 1] = e.mx;
    out[4 * m + 2] = e.nan_window;
    out[4 * m + 3] = e.nan_compute;
  }
}

// workgroups of stage one per field: the rows of the larger window, the whole storage, whatever the fields' flags
static inline int extrema_blocks(const Geo& g) {
  const long rows = (long)g.nj * (g.nk + 1);
  return (int)((rows + SX_WAVES * SX_ROWS - 1) / (SX_WAVES * SX_ROWS));
}

size_t state_extrema_workspace_bytes(const Geo& g) {
  return (size_t)PACE_STATE_EXTREMA_MAX_FIELDS * extrema_blocks(g) * 4 * sizeof(double);
}

int launch_state_extrema(const Geo& g, const real* const* fields, const int* compute_only, int nfields, void* workspace,
                         double* out, hipStream_t st) {
  ExtremaFields f{};
  for (int m = 0; m < nfields; ++m) {
    f.f[m] = fields[m];
    if (compute_only[m]) f.compute_only |= 1u << m;
  }
  const int nblk = extrema_blocks(g);
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(k_state_extrema_partial, dim3((unsigned)nblk, (unsigned)nfields), dim3(64 * SX_WAVES), 0, st, g, f, partial);
  PACE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_state_extrema_combine, dim3((unsigned)nfields), dim3(64), 0, st, partial, nblk, out);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
