// Horizontal tracer advection (Fortran tracer_2d_1l): the stencils of fv3core/pace/fv3core/stencils/tracer_2d_1l.py:19-170
// around FiniteVolumeTransport(hord_tr = 8) (the monotone-PPM instance of the transport kernel, k_fvtp2d.hip).
// All HBM-bound streaming passes, one thread per (i, j, k), i fastest.
#include "common.h"
#include "kernels.h"

// flux_compute (tracer_2d_1l.py:19-77)
__global__ void __launch_bounds__(256)
k_tracer_flux_compute(Geo g, Met m, const real* __restrict__ cx, const real* __restrict__ cy, real* __restrict__ xfx,
                      real* __restrict__ yfx) {
  PLANE_IJK(g);
  const long c = IDX3(g, i, j, k);
  const long c2 = IDX2(g, i, j);
  if (i >= g.is && i <= g.ie + 1 && j >= g.js - 3 && j <= g.je + 3) {
    const double v = cx[c];
    xfx[c] = (v > 0.0) ? v * m.dxa[c2 - 1] * m.dy[c2] * m.sin_sg3[c2 - 1] : v * m.dxa[c2] * m.dy[c2] * m.sin_sg1[c2];
  }
  if (i >= g.is - 3 && i <= g.ie + 3 && j >= g.js && j <= g.je + 1) {
    const double v = cy[c];
    yfx[c] = (v > 0.0) ? v * m.dya[c2 - g.sj] * m.dx[c2] * m.sin_sg4[c2 - g.sj] : v * m.dya[c2] * m.dx[c2] * m.sin_sg2[c2];
  }
}

// divide_fluxes_by_n_substeps (tracer_2d_1l.py:80-106): origin_full, domain_full(add = (1, 1, 0)) = the whole storage plane
__global__ void __launch_bounds__(256)
k_tracer_divide(Geo g, real* __restrict__ a0, real* __restrict__ a1, real* __restrict__ a2, real* __restrict__ a3,
                real* __restrict__ a4, real* __restrict__ a5, double frac) {
  PLANE_IJK(g);
  const long c = IDX3(g, i, j, k);
  a0[c] = a0[c] * frac;
  a1[c] = a1[c] * frac;
  a2[c] = a2[c] * frac;
  a3[c] = a3[c] * frac;
  a4[c] = a4[c] * frac;
  a5[c] = a5[c] * frac;
}

// The bodies of the three compute-domain stencils below, shared by their plain and their per-level (_levels) kernels: one
// text, so the two forms cannot differ in a cast or an association.
__device__ __forceinline__ void apply_mass_flux_cell(const Geo& g, const Met& m, const real* __restrict__ dp1,
                                                     const real* __restrict__ mfx, const real* __restrict__ mfy,
                                                     real* __restrict__ dp2, int i, int j, int k) {
  if (i < g.is || i > g.ie || j < g.js || j > g.je) return;
  const long c = IDX3(g, i, j, k);
  // (the casts: with real = float the whole expression would otherwise be evaluated in float, every operand being a real load)
  dp2[c] = (double)dp1[c] + ((double)mfx[c] - (double)mfx[c + 1] + (double)mfy[c] - (double)mfy[c + g.sj]) * (double)m.rarea[IDX2(g, i, j)];
}
__device__ __forceinline__ void apply_tracer_flux_cell(const Geo& g, const Met& m, real* __restrict__ q,
                                                       const real* __restrict__ dp1, const real* __restrict__ fx,
                                                       const real* __restrict__ fy, const real* __restrict__ dp2, int i, int j,
                                                       int k) {
  if (i < g.is || i > g.ie || j < g.js || j > g.je) return;
  const long c = IDX3(g, i, j, k);
  q[c] = ((double)q[c] * (double)dp1[c] +
          ((double)fx[c] - (double)fx[c + 1] + (double)fy[c] - (double)fy[c + g.sj]) * (double)m.rarea[IDX2(g, i, j)]) / (double)dp2[c];
}
__device__ __forceinline__ void swap_dp_cell(const Geo& g, real* __restrict__ dp1, real* __restrict__ dp2, int i, int j, int k) {
  if (i < g.is || i > g.ie || j < g.js || j > g.je) return;
  const long c = IDX3(g, i, j, k);
  const double t = dp1[c];
  dp1[c] = dp2[c];
  dp2[c] = t;
}

// apply_mass_flux (tracer_2d_1l.py:115-135), compute domain
__global__ void __launch_bounds__(256)
k_apply_mass_flux(Geo g, Met m, const real* __restrict__ dp1, const real* __restrict__ mfx, const real* __restrict__ mfy,
                  real* __restrict__ dp2) {
  PATCH_IJK(g);
  apply_mass_flux_cell(g, m, dp1, mfx, mfy, dp2, i, j, k);
}

// apply_tracer_flux (tracer_2d_1l.py:138-158), compute domain
__global__ void __launch_bounds__(256)
k_apply_tracer_flux(Geo g, Met m, real* __restrict__ q, const real* __restrict__ dp1, const real* __restrict__ fx,
                    const real* __restrict__ fy, const real* __restrict__ dp2) {
  PATCH_IJK(g);
  apply_tracer_flux_cell(g, m, q, dp1, fx, fy, dp2, i, j, k);
}

// swap_dp (tracer_2d_1l.py:166-170), compute domain
__global__ void __launch_bounds__(256) k_swap_dp(Geo g, real* __restrict__ dp1, real* __restrict__ dp2) {
  PLANE_IJK(g);
  swap_dp_cell(g, dp1, dp2, i, j, k);
}

// ---- Courant-number sub-cycling per level (the Fortran tracer_2d_1L: cmax(k) over the globe, level k sub-cycled
// int(1. + cmax(k)) times; include/pace_hip.h has the arithmetic).
//
//   k_tracer_cmax       grid (64-point segments of i, groups of sixteen rows j, levels), 256 threads = 4 waves: a wave takes four
//            rows of the compute domain, a lane a cell of each (its eight field loads in flight together; one row a wave
//            measured 49 us at C192 x 79).  Every per-cell value is >= 0 or a NaN, and the bit patterns of such
//            doubles order like unsigned 64-bit integers with every NaN above infinity -- so the maximum is an integer maximum
//            of patterns: exact, independent of the order, and a NaN wins (fmax would drop it).  Fold over the wave by
//            shuffles, over the four waves through LDS, ONE 64-bit integer atomic maximum per workgroup into cmax[k], which
//            the caller zeroed (0.0 is the pattern 0).  Lanes outside the compute domain load nothing and fold zeros.
//   k_tracer_subcycles  one wave: lane l takes levels l, l + 64, ...; the tiles' maximum by patterns again, then the count.
//   k_tracer_divide_levels, k_*_levels   the stencils above with a block-uniform test of ksplt[k] before any field access.
__device__ __forceinline__ unsigned long long tracer_bits(double v) {
  unsigned long long b;
  memcpy(&b, &v, sizeof(b));
  return b;
}
__device__ __forceinline__ double tracer_from_bits(unsigned long long b) {
  double v;
  memcpy(&v, &b, sizeof(v));
  return v;
}
__device__ __forceinline__ unsigned long long tracer_max_bits(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned long long tracer_wave_max(unsigned long long b) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) b = tracer_max_bits(b, __shfl_down(b, (unsigned)d, 64));
  return b;  // (lane 0 holds the wave's)
}

#define CMAX_WAVES 4
#define CMAX_ROWS 4
__global__ void __launch_bounds__(64 * CMAX_WAVES)
k_tracer_cmax(Geo g, const real* __restrict__ cx, const real* __restrict__ cy, const real* __restrict__ sin_sg5,
              unsigned long long* __restrict__ cmax, int nplain) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int i = g.is + (int)blockIdx.x * 64 + lane;
  const int j0 = g.js + ((int)blockIdx.y * CMAX_WAVES + wave) * CMAX_ROWS;
  const int k = (int)blockIdx.z;
  const bool plain = k < nplain;  // (uniform over the workgroup: the plain levels do not read the plane)
  // the loads of the wave's rows are all issued before the arithmetic
  double x[CMAX_ROWS], y[CMAX_ROWS], sine[CMAX_ROWS];
  bool inside[CMAX_ROWS];
#pragma unroll
  for (int r = 0; r < CMAX_ROWS; ++r) {
    const int j = j0 + r;
    inside[r] = i <= g.ie && j <= g.je;
    x[r] = 0.0, y[r] = 0.0, sine[r] = 1.0;
    if (inside[r]) {
      const long c = IDX3(g, i, j, k);
      x[r] = (double)cx[c];
      y[r] = (double)cy[c];
      if (!plain) sine[r] = (double)sin_sg5[IDX2(g, i, j)];
    }
  }
  unsigned long long b = 0ULL;
#pragma unroll
  for (int r = 0; r < CMAX_ROWS; ++r) {
    // max(|cx|, |cy|) by patterns: fabs clears the sign, so a NaN of either field is the larger pattern
    const double m = tracer_from_bits(tracer_max_bits(tracer_bits(fabs(x[r])), tracer_bits(fabs(y[r]))));
    const double v = plain ? m : (m + 1.0) - sine[r];
    // (a NaN may carry a sign: cleared, so that it orders above infinity.  A value below zero -- a sine above 1 + m, which no
    // grid has -- keeps its sign, is the largest pattern of all and is refused by k_tracer_subcycles)
    const unsigned long long bits = v != v ? tracer_bits(fabs(v)) : tracer_bits(v);
    if (inside[r]) b = tracer_max_bits(b, bits);
  }
  b = tracer_wave_max(b);
  __shared__ unsigned long long per_wave[CMAX_WAVES];
  if (lane == 0) per_wave[wave] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long w = per_wave[0];
    for (int v = 1; v < CMAX_WAVES; ++v) w = tracer_max_bits(w, per_wave[v]);
    if (w != 0ULL) {
#ifdef PACE_EMU
      if (w > cmax[k]) cmax[k] = w;  // (the emulation runs one workgroup at a time)
#else
      atomicMax(cmax + k, w);
#endif
    }
  }
}

struct SubcyclesArgs {
  const unsigned long long* cmax[PACE_TRACER_MAX_TILES];
  int32_t* out;
  int ntiles, nk, max_subcycles, pad_;
};

__global__ void __launch_bounds__(64) k_tracer_subcycles(SubcyclesArgs A) {
  const int lane = (int)threadIdx.x;
  int largest = 0, refused = 0;
  for (int k = lane; k < A.nk; k += 64) {
    unsigned long long b = 0ULL;
    for (int t = 0; t < A.ntiles; ++t) b = tracer_max_bits(b, A.cmax[t][k]);
    // a value below zero has the largest patterns of all: it is refused with the NaNs
    const double s = 1.0 + tracer_from_bits(b);
    int n = 0;
    if ((b >> 63) == 0ULL && s < (double)A.max_subcycles + 1.0) n = (int)s;  // (a NaN and an infinity fail the comparison)
    A.out[2 + k] = n;
    largest = n > largest ? n : largest;
    refused += n == 0 ? 1 : 0;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int other = __shfl_down(largest, (unsigned)d, 64);
    largest = other > largest ? other : largest;
    refused += __shfl_down(refused, (unsigned)d, 64);
  }
  if (lane == 0) {
    A.out[0] = largest;
    A.out[1] = refused;
  }
}

// k_tracer_divide with frac = 1 / ksplt[k]; a level that takes one sub-cycle (or is refused: 0) is neither read nor written
__global__ void __launch_bounds__(256)
k_tracer_divide_levels(Geo g, real* __restrict__ a0, real* __restrict__ a1, real* __restrict__ a2, real* __restrict__ a3,
                       real* __restrict__ a4, real* __restrict__ a5, const int32_t* __restrict__ ksplt) {
  const int n_split = ksplt[blockIdx.y];
  if (n_split <= 1) return;
  PLANE_IJK(g);
  const double frac = 1.0 / n_split;
  const long c = IDX3(g, i, j, k);
  a0[c] = a0[c] * frac;
  a1[c] = a1[c] * frac;
  a2[c] = a2[c] * frac;
  a3[c] = a3[c] * frac;
  a4[c] = a4[c] * frac;
  a5[c] = a5[c] * frac;
}

__global__ void __launch_bounds__(256)
k_apply_mass_flux_levels(Geo g, Met m, const real* __restrict__ dp1, const real* __restrict__ mfx,
                         const real* __restrict__ mfy, real* __restrict__ dp2, const int32_t* __restrict__ ksplt,
                         int min_subcycles) {
  if (ksplt[blockIdx.z] < min_subcycles) return;
  PATCH_IJK(g);
  apply_mass_flux_cell(g, m, dp1, mfx, mfy, dp2, i, j, k);
}

__global__ void __launch_bounds__(256)
k_apply_tracer_flux_levels(Geo g, Met m, real* __restrict__ q, const real* __restrict__ dp1, const real* __restrict__ fx,
                           const real* __restrict__ fy, const real* __restrict__ dp2, const int32_t* __restrict__ ksplt,
                           int min_subcycles) {
  if (ksplt[blockIdx.z] < min_subcycles) return;
  PATCH_IJK(g);
  apply_tracer_flux_cell(g, m, q, dp1, fx, fy, dp2, i, j, k);
}

__global__ void __launch_bounds__(256)
k_swap_dp_levels(Geo g, real* __restrict__ dp1, real* __restrict__ dp2, const int32_t* __restrict__ ksplt, int min_subcycles) {
  if (ksplt[blockIdx.y] < min_subcycles) return;
  PLANE_IJK(g);
  swap_dp_cell(g, dp1, dp2, i, j, k);
}

int launch_tracer_cmax(const Geo& g, const real* cx, const real* cy, const real* sin_sg5, double* cmax, hipStream_t st) {
  const int rows = CMAX_WAVES * CMAX_ROWS;
  const dim3 grid((unsigned)((g.n + 63) / 64), (unsigned)((g.n + rows - 1) / rows), (unsigned)g.nk);
  if (grid.y > 65535u || grid.z > 65535u) return PACE_ERR_UNSUPPORTED;
  // Fortran "k < npz/6" with k counted from 1: the levels 0 .. nk/6 - 2 take the plain form
  hipLaunchKernelGGL(k_tracer_cmax, grid, dim3(64 * CMAX_WAVES), 0, st, g, cx, cy, sin_sg5, (unsigned long long*)cmax, g.nk / 6 - 1);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
int launch_tracer_subcycles(const double* const* cmax, int ntiles, int nk, int max_subcycles, int32_t* out, hipStream_t st) {
  SubcyclesArgs A;
  for (int t = 0; t < PACE_TRACER_MAX_TILES; ++t) A.cmax[t] = t < ntiles ? (const unsigned long long*)cmax[t] : nullptr;
  A.out = out, A.ntiles = ntiles, A.nk = nk, A.max_subcycles = max_subcycles, A.pad_ = 0;
  hipLaunchKernelGGL(k_tracer_subcycles, dim3(1), dim3(64), 0, st, A);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
int launch_tracer_divide_levels(const Geo& g, real* cxd, real* xfx, real* mfxd, real* cyd, real* yfx, real* mfyd,
                                const int32_t* ksplt, hipStream_t st) {
  hipLaunchKernelGGL(k_tracer_divide_levels, plane_grid(g, g.nk), dim3(256), 0, st, g, cxd, xfx, mfxd, cyd, yfx, mfyd, ksplt);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
int launch_apply_mass_flux_levels(const Geo& g, const Met& m, const real* dp1, const real* mfx, const real* mfy, real* dp2,
                                  const int32_t* ksplt, int min_subcycles, hipStream_t st) {
  hipLaunchKernelGGL(k_apply_mass_flux_levels, patch_grid(g, g.nk), PATCH_BLOCK, 0, st, g, m, dp1, mfx, mfy, dp2, ksplt,
                     min_subcycles);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
int launch_apply_tracer_flux_levels(const Geo& g, const Met& m, real* q, const real* dp1, const real* fx, const real* fy,
                                    const real* dp2, const int32_t* ksplt, int min_subcycles, hipStream_t st) {
  hipLaunchKernelGGL(k_apply_tracer_flux_levels, patch_grid(g, g.nk), PATCH_BLOCK, 0, st, g, m, q, dp1, fx, fy, dp2, ksplt,
                     min_subcycles);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
int launch_swap_dp_levels(const Geo& g, real* dp1, real* dp2, const int32_t* ksplt, int min_subcycles, hipStream_t st) {
  hipLaunchKernelGGL(k_swap_dp_levels, plane_grid(g, g.nk), dim3(256), 0, st, g, dp1, dp2, ksplt, min_subcycles);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}

int launch_tracer_flux_compute(const Geo& g, const Met& m, const real* cx, const real* cy, real* xfx, real* yfx,
                               hipStream_t st) {
  hipLaunchKernelGGL(k_tracer_flux_compute, plane_grid(g, g.nk), dim3(256), 0, st, g, m, cx, cy, xfx, yfx);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
int launch_tracer_divide(const Geo& g, real* cxd, real* xfx, real* mfxd, real* cyd, real* yfx, real* mfyd,
                         int n_split, hipStream_t st) {
  hipLaunchKernelGGL(k_tracer_divide, plane_grid(g, g.nk), dim3(256), 0, st, g, cxd, xfx, mfxd, cyd, yfx, mfyd, 1.0 / n_split);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
int launch_apply_mass_flux(const Geo& g, const Met& m, const real* dp1, const real* mfx, const real* mfy, real* dp2,
                           hipStream_t st) {
  hipLaunchKernelGGL(k_apply_mass_flux, patch_grid(g, g.nk), PATCH_BLOCK, 0, st, g, m, dp1, mfx, mfy, dp2);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
int launch_apply_tracer_flux(const Geo& g, const Met& m, real* q, const real* dp1, const real* fx, const real* fy,
                             const real* dp2, hipStream_t st) {
  hipLaunchKernelGGL(k_apply_tracer_flux, patch_grid(g, g.nk), PATCH_BLOCK, 0, st, g, m, q, dp1, fx, fy, dp2);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
int launch_swap_dp(const Geo& g, real* dp1, real* dp2, hipStream_t st) {
  hipLaunchKernelGGL(k_swap_dp, plane_grid(g, g.nk), dim3(256), 0, st, g, dp1, dp2);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
