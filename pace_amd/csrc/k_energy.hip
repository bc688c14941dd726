// The total-energy fixer (consv_te > 0; the Fortran FV3's compute_total_energy and the consv > consv_min block of
// Lagrangian_to_Eulerian, non-hydrostatic, MOIST_CAPPA / USE_COND, nwat = 6; the reference stops at the global sum).
// include/pace_hip.h has the arithmetic, operation by operation; all of it is double on the stored values (the float32 library
// widens first), with no contraction, no reciprocal and no transcendental.
//
//   k_energy_columns<MODE>  1-D grid, 256 threads = 4 waves.  A workgroup takes 64 points of i of four consecutive rows j: a wave
//            takes a row, lane l the point i = 3 + 64 * segment + l (k_held_suarez's form), and walks its column from the bottom
//            level up, ONCE: the geopotential, the energy and (MODE 1) the pkz-weighted mass are running sums in registers, so
//            every field is fetched once (u's row j + 1 and v's column i + 1 are the neighbouring lane's / wave's lines).  A
//            level's loads are all issued before its arithmetic.  MODE 0 stores te0_2d.  MODE 1 forms te_2d = te0_2d - te and
//            zsum1, encodes area * te_2d and area * zsum1 (the doubles in registers, before any narrowing) as 4 + 1 signed 64-bit
//            words each, folds the ten words over the wave by shuffles and over the four waves through LDS -- integer addition:
//            any order gives the same words -- and ten lanes add the workgroup's words to global memory with 64-bit integer
//            vector atomics.  The planes are stored after the fold.  Lanes past the row's end or the last row load and store
//            nothing and fold zeros.
//   k_energy_finalize       one thread: sums the tiles' words in tile order, decodes the two sums exactly (carry propagation in
//            base 2^40, then ONE rounding to nearest-even of the 192-bit magnitude), and writes S_te, S_z, dtmp, e_flux.
//   k_l2e_finish_dtmp       k_l2e_finish's last-step form with dtmp read from the four doubles instead of 0.
//
// Nothing outside the planes' compute windows, the ten words and the four doubles is written; nothing outside the compute domain
// of the (staggered) fields is read.  No floating-point atomics, no workspace, no host synchronisation.
#include "common.h"
#include "kernels.h"
#include "thermo.h"

#define EN_WAVES 4
#define EN_LIMB_BITS 40
#define EN_LIMB_MASK ((1ULL << EN_LIMB_BITS) - 1ULL)

struct EnergyArgs {
  Water6Const q;
  const real *pt, *delp, *delz, *w, *u, *v, *pkz, *phis, *rsin2, *cosa_s, *area;
  real *te0_2d, *te_2d, *zsum1;
  long long* words;
  double r_vir;
  long sk;
  int sj, n, nk, nseg;
};

__device__ __forceinline__ unsigned long long energy_double_bits(double v) {
  unsigned long long b;
  memcpy(&b, &v, sizeof(b));
  return b;
}

// v -> word[0 .. 3] += the four 40-bit limbs of trunc(|v| * 2^40), negated for v < 0; a v that is not finite or not below 2^120
// in magnitude -> word[4] += 1 and nothing else.  The significand is only shifted: exact; bits below 2^-40 are dropped.
__device__ __forceinline__ void energy_encode(double v, long long (&word)[5]) {
  const unsigned long long b = energy_double_bits(v);
  const int field = (int)((b >> 52) & 0x7ffULL);
  if (field >= 1023 + 120) {  // 2^120 and above, infinity, NaN
    word[4] += 1;
    return;
  }
  const unsigned long long frac = b & ((1ULL << 52) - 1ULL);
  const unsigned long long mant = field == 0 ? frac : (frac | (1ULL << 52));  // |v| = mant * 2^(max(field, 1) - 1075)
  const int s = (field == 0 ? 1 : field) - 1075 + EN_LIMB_BITS;                // trunc(|v| * 2^40) = mant shifted by s
  const bool neg = (b >> 63) != 0ULL;
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int sh = s - EN_LIMB_BITS * n;
    unsigned long long limb = 0ULL;
    if (sh >= 0 && sh < EN_LIMB_BITS) limb = (mant << sh) & EN_LIMB_MASK;  // (bits shifted past 2^64 lie above the limb)
    else if (sh < 0 && sh > -53) limb = (mant >> (-sh)) & EN_LIMB_MASK;
    word[n] += neg ? -(long long)limb : (long long)limb;
  }
}

__device__ __forceinline__ void energy_atomic_add(long long* p, long long v) {
#ifdef PACE_EMU
  __atomic_fetch_add(p, v, __ATOMIC_RELAXED);
#else
  atomicAdd((unsigned long long*)p, (unsigned long long)v);  // (two's complement: the wrapping sum is the signed sum)
#endif
}

template <int MODE>
__global__ void __launch_bounds__(64 * EN_WAVES) k_energy_columns(EnergyArgs A) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int b = (int)blockIdx.x;
  const int seg = b % A.nseg, jg = b / A.nseg;
  const int i = seg * 64 + lane, j = jg * EN_WAVES + wave;  // within the compute domain
  const bool active = i < A.n && j < A.n;
  const long c2d = (long)(i + 3) + (long)(j + 3) * A.sj;
  double te = 0.0, zsum = 0.0;
  if (active) {
    // (no __restrict__: nothing forbids the caller's inputs to share an array)
    const double rsin2 = (double)A.rsin2[c2d], cosa = (double)A.cosa_s[c2d];
    double phi_below = (double)A.phis[c2d];
    for (int k = A.nk - 1; k >= 0; --k) {
      const long c = c2d + (long)k * A.sk;
      const double delz = (double)A.delz[c], delp = (double)A.delp[c], pt = (double)A.pt[c], w = (double)A.w[c];
      const double u0 = (double)A.u[c], u1 = (double)A.u[c + A.sj], v0 = (double)A.v[c], v1 = (double)A.v[c + 1];
      const double qv = (double)A.q.qvapor[c];
      const double ql = (double)A.q.qliquid[c] + (double)A.q.qrain[c];
      const double qs = (double)A.q.qice[c] + (double)A.q.qsnow[c] + (double)A.q.qgraupel[c];
      double pkz = 0.0;
      if (MODE == 1) pkz = (double)A.pkz[c];
      const double phi_above = phi_below - phys::GRAV * delz;
      const double ke = (0.5 * rsin2) * ((((u0 * u0 + u1 * u1) + v0 * v0) + v1 * v1) - ((u0 + u1) * (v0 + v1)) * cosa);
      const double gz = ql + qs;
      const double cvm = moist_cvm(qv + gz, qv, ql, qs);
      double e = cvm * pt;
      if (MODE == 1) e = e / ((1.0 + A.r_vir * qv) * (1.0 - gz));
      te = te + delp * (e + 0.5 * (((phi_above + phi_below) + w * w) + ke));
      if (MODE == 1) zsum = zsum + pkz * delp;
      phi_below = phi_above;
    }
  }
  if (MODE == 0) {
    if (active) A.te0_2d[c2d] = (real)te;
    return;
  }
  double te_2d = 0.0;
  long long word_te[5] = {0, 0, 0, 0, 0}, word_z[5] = {0, 0, 0, 0, 0};
  if (active) {
    const double area = (double)A.area[c2d];
    te_2d = (double)A.te0_2d[c2d] - te;
    energy_encode(area * te_2d, word_te);
    energy_encode(area * zsum, word_z);
  }
#pragma unroll
  for (int m = 0; m < 5; ++m) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      word_te[m] += __shfl_down(word_te[m], (unsigned)d, 64);
      word_z[m] += __shfl_down(word_z[m], (unsigned)d, 64);
    }
  }
  __shared__ long long per_wave[EN_WAVES][10];
  if (lane == 0) {
#pragma unroll
    for (int m = 0; m < 5; ++m) {
      per_wave[wave][m] = word_te[m];
      per_wave[wave][5 + m] = word_z[m];
    }
  }
  __syncthreads();
  if (active) {
    A.te_2d[c2d] = (real)te_2d;
    A.zsum1[c2d] = (real)zsum;
  }
  if (threadIdx.x < 10) {
    long long s = 0;
    for (int v = 0; v < EN_WAVES; ++v) s += per_wave[v][threadIdx.x];
    if (s != 0) energy_atomic_add(A.words + threadIdx.x, s);
  }
}

int launch_energy_columns(const Geo& g, int mode, const real* const* water, const real* pt, const real* delp, const real* delz,
                          const real* w, const real* u, const real* v, const real* pkz, const real* phis, const real* rsin2,
                          const real* cosa_s, const real* area, real* te0_2d, real* te_2d, real* zsum1, int64_t* words,
                          double r_vir, hipStream_t st) {
  EnergyArgs A;
  A.q = water6(water);
  A.pt = pt, A.delp = delp, A.delz = delz, A.w = w, A.u = u, A.v = v, A.pkz = pkz, A.phis = phis, A.rsin2 = rsin2;
  A.cosa_s = cosa_s, A.area = area, A.te0_2d = te0_2d, A.te_2d = te_2d, A.zsum1 = zsum1;
  A.words = (long long*)words;
  A.r_vir = r_vir;
  A.sk = g.sk, A.sj = g.sj, A.n = g.n, A.nk = g.nk;
  A.nseg = (g.n + 63) / 64;
  const long blocks = (long)A.nseg * ((g.n + EN_WAVES - 1) / EN_WAVES);
  if (blocks > 0x7fffffffL) return PACE_ERR_UNSUPPORTED;
  if (mode == 0) hipLaunchKernelGGL(k_energy_columns<0>, dim3((unsigned)blocks), dim3(64 * EN_WAVES), 0, st, A);
  else hipLaunchKernelGGL(k_energy_columns<1>, dim3((unsigned)blocks), dim3(64 * EN_WAVES), 0, st, A);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}

struct EnergyFinalizeArgs {
  const long long* words[PACE_ENERGY_MAX_TILES];
  double* out;
  double consv_te, dt_atmos;
  int ntiles, pad_;
};

// word[0 .. 4] (summed over the tiles) -> the sum: M = sum_n word[n] * 2^(40 n) exactly, M * 2^-40 rounded once to nearest-even
__device__ double energy_decode(const long long* word) {
  if (word[4] != 0) {
    const unsigned long long nan_bits = 0x7ff8000000000000ULL;
    double nan;
    memcpy(&nan, &nan_bits, sizeof(nan));
    return nan;
  }
  // carries in base 2^40: limb[n] in [0, 2^40), top the signed rest (|word[n]| < 2^63 - 2^40 and |carry| < 2^24: no overflow)
  long long carry = 0;
  for (int n = 0; n < 4; ++n) carry = (word[n] + carry) >> EN_LIMB_BITS;  // (arithmetic shift: the floor)
  const bool neg = carry < 0;
  unsigned long long limb[4];
  carry = 0;
  for (int n = 0; n < 4; ++n) {
    const long long t = (neg ? -word[n] : word[n]) + carry;
    limb[n] = (unsigned long long)t & EN_LIMB_MASK;
    carry = t >> EN_LIMB_BITS;
  }
  const unsigned long long top = (unsigned long long)carry;  // >= 0 now, < 2^24
  // |M| in three 64-bit words
  unsigned long long x[3];
  x[0] = limb[0] | (limb[1] << 40);
  x[1] = (limb[1] >> 24) | (limb[2] << 16) | (limb[3] << 56);
  x[2] = (limb[3] >> 8) | (top << 32);
  int p = -1;  // the highest set bit
  for (int n = 2; n >= 0 && p < 0; --n)
    if (x[n] != 0ULL) {
      int h = 63;
      while (((x[n] >> h) & 1ULL) == 0ULL) --h;
      p = 64 * n + h;
    }
  if (p < 0) return 0.0;
  unsigned long long mant;
  int shift = 0;
  if (p <= 52) {
    mant = x[0];
  } else {
    shift = p - 52;  // 1 .. 139: mant = |M| >> shift, rounded on the bits below
    const int wq = shift >> 6, wr = shift & 63;
    mant = x[wq] >> wr;
    if (wr != 0 && wq + 1 < 3) mant |= x[wq + 1] << (64 - wr);
    mant &= (1ULL << 53) - 1ULL;
    const int rb = shift - 1;
    const bool round = ((x[rb >> 6] >> (rb & 63)) & 1ULL) != 0ULL;
    bool sticky = false;
    for (int n = 0; n < 3; ++n) {
      if (64 * n >= rb) break;
      const unsigned long long below = rb - 64 * n >= 64 ? ~0ULL : ((1ULL << (rb - 64 * n)) - 1ULL);
      if ((x[n] & below) != 0ULL) sticky = true;
    }
    if (round && (sticky || (mant & 1ULL))) mant += 1ULL;  // (2^53 is a double too)
  }
  // mant * 2^(shift - 40): both factors doubles, the product exact (no subnormal: |M| >= 1 gives at least 2^-40)
  const unsigned long long scale_bits = (unsigned long long)(1023 + shift - EN_LIMB_BITS) << 52;
  double scale;
  memcpy(&scale, &scale_bits, sizeof(scale));
  const double value = (double)mant * scale;
  return neg ? -value : value;
}

__global__ void __launch_bounds__(64) k_energy_finalize(EnergyFinalizeArgs A) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  long long sum[10];
  for (int m = 0; m < 10; ++m) {
    long long s = 0;
    for (int t = 0; t < A.ntiles; ++t) s += A.words[t][m];
    sum[m] = s;
  }
  const double s_te = energy_decode(sum), s_z = energy_decode(sum + 5);
  A.out[0] = s_te;
  A.out[1] = s_z;
  A.out[2] = (A.consv_te * s_te) / (phys::CV_AIR * s_z);
  A.out[3] = (A.consv_te * s_te) / ((((phys::GRAV * A.dt_atmos) * 4.0) * phys::PI) * (phys::RADIUS * phys::RADIUS));
}

int launch_energy_finalize(const int64_t* const* words, int ntiles, double consv_te, double dt_atmos, double* out, hipStream_t st) {
  EnergyFinalizeArgs A;
  for (int t = 0; t < PACE_ENERGY_MAX_TILES; ++t) A.words[t] = t < ntiles ? (const long long*)words[t] : nullptr;
  A.out = out, A.consv_te = consv_te, A.dt_atmos = dt_atmos, A.ntiles = ntiles, A.pad_ = 0;
  hipLaunchKernelGGL(k_energy_finalize, dim3(1), dim3(64), 0, st, A);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}

__global__ void __launch_bounds__(256)
k_l2e_finish_dtmp(Geo g, Water6Const q, real* __restrict__ pe, const real* __restrict__ pe2, real* __restrict__ pt,
                  const real* __restrict__ pkz, double r_vir, const double* __restrict__ result) {
  CELL_IJK(g, 0, 0, 0);
  const int km = g.nk;
  if (k >= 1 && k < km) pe[c] = pe2[c];  // update_ua + copy_from_below, as k_l2e_finish
  // moist_pt_last_step over km + 1 levels (moist_cv.py:73-122) with the dtmp of the finalising launch
  const double dtmp = result[2];
  const double gz = (double)q.qliquid[c] + (double)q.qrain[c] + (double)q.qice[c] + (double)q.qsnow[c] + (double)q.qgraupel[c];
  pt[c] = (pt[c] + dtmp * pkz[c]) / ((1.0 + r_vir * q.qvapor[c]) * (1.0 - gz));
}

int launch_l2e_finish_dtmp(const Geo& g, const real* const* water, real* pe, const real* pe2, real* pt, const real* pkz,
                           double r_vir, const double* result, hipStream_t st) {
  const Water6Const q = water6(water);
  hipLaunchKernelGGL(k_l2e_finish_dtmp, cell_grid(g, 0, 0, g.nk + 1), dim3(64, 4), 0, st, g, q, pe, pe2, pt, pkz, r_vir, result);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
