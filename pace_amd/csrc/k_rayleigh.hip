// Rayleigh_Super (the Fortran fv_dynamics.F90 with rf_fast = .false. and tau > 0, non-hydrostatic, conserve; the reference has
// none): once per dycore step the sponge levels' winds are scaled by f[k] = 1 / (1 + rf[k]) and the kinetic energy lost is added to
// the temperature as heat.  The HOST forms f (include/pace_hip.h: pace_rayleigh_super); here, on the levels k < kmax, in double on
// the stored values (the float32 library widens first), with no contraction and no reciprocal, in exactly this order:
//
//   cells (i, j) of the compute domain (origin (3, 3), extent (n, n)):
//     u1 = 2.0 * (u[i,j] * dx[i,j] + u[i,j+1] * dx[i,j+1]) / (dx[i,j] + dx[i,j+1])            k_c2l<2>'s expressions
//     v1 = 2.0 * (v[i,j] * dy[i,j] + v[i+1,j] * dy[i+1,j]) / (dy[i,j] + dy[i+1,j])
//     ua = a11 * u1 + a12 * v1,  va = a21 * u1 + a22 * v1
//     pt = (real)(pt + ((0.5 * ((ua * ua + va * va) + w * w)) * (1.0 - f[k] * f[k])) * rcv)      conserve only
//     w  = (real)(f[k] * w)
//   u = (real)(f[k] * u) on (n, n + 1) points, v = (real)(f[k] * v) on (n + 1, n) points
//
// The heat of cell (i, j) reads u[i,j+1] and v[i+1,j], which another workgroup scales in place: with conserve there are TWO ordered
// launches, k_rayleigh_heat (pt and w from the old winds) and then k_rayleigh_scale<false> (the winds); without conserve one,
// k_rayleigh_scale<true> (the winds and w).
//
//   both     1-D grid, 256 threads = 4 waves, k_held_suarez's form.  A workgroup takes 64 points of i of four consecutive rows j and
//            RS_LEVELS consecutive levels: a wave takes a row, lane l the point i = 3 + 64 * segment + l -- 512 B contiguous
//            (float32: 256 B) of each array -- and walks the chunk's levels of its column; the heat kernel loads its eight metric
//            values once.  The segment is the fastest index of the grid, then the row group, then the chunk.  The thread of the
//            domain's last row also scales u's row n + 1, the thread of its last column v's column n + 1: no workgroup is launched
//            for the staggered extents.  A level's loads are all issued before its arithmetic.
//            The factors travel in the kernel-argument table (RS_TABLE doubles, fetched by a scalar load with the workgroup's
//            level): no workspace, no upload.  More than RS_TABLE damped levels take a further pair of launches (the levels are
//            independent of each other).
//
// Nothing outside these windows is written on the levels < kmax and nothing at all from level kmax on (not the halo, not level nk,
// not the row padding); u, v, w, pt and the six metric planes are read only on the compute domain plus the staggered row / column.
// No atomics, no workspace, no LDS.
#include "common.h"
#include "kernels.h"

#define RS_WAVES 4
#ifndef RS_LEVELS
#define RS_LEVELS 4  // levels a thread walks
#endif
#define RS_TABLE 128  // factors per launch

struct RsArgs {
  const real *dx, *dy, *a11, *a12, *a21, *a22;
  real *u, *v, *w, *pt;
  double rcv;
  long sk;
  int sj, n, nseg, njg;
  int k0, nlev;  // the launch's levels are k0 .. k0 + nlev - 1; f[m] is level k0 + m's factor
  double f[RS_TABLE];
};

// -> false for a thread outside the compute domain; otherwise its cell's plane index, its first level's offset and its level count
#define RS_THREAD(A)                                                        \
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;     \
  const int b = (int)blockIdx.x;                                            \
  const int nseg = A.nseg, njg = A.njg, n = A.n;                            \
  const int seg = b % nseg, rest = b / nseg;                                \
  const int jg = rest % njg, chunk = rest / njg;                            \
  const int i = seg * 64 + lane, j = jg * RS_WAVES + wave;                  \
  if (i >= n || j >= n) return;                                             \
  const long sj = A.sj, sk = A.sk;                                          \
  const long c2d = (long)(i + 3) + (long)(j + 3) * sj;                      \
  const int m0 = chunk * RS_LEVELS;                                         \
  const int m1 = m0 + RS_LEVELS < A.nlev ? m0 + RS_LEVELS : A.nlev

__global__ void __launch_bounds__(64 * RS_WAVES) k_rayleigh_heat(RsArgs A_) {
  PACE_KERNARG(RsArgs, A, A_);
  RS_THREAD(A);
  // (no __restrict__: the second launch's ordering, not a promise of the caller's, keeps the winds' writes apart from these reads)
  const real* u = A.u;
  const real* v = A.v;
  real* w = A.w;
  real* pt = A.pt;
  const double dx0 = (double)A.dx[c2d], dx1 = (double)A.dx[c2d + sj], dy0 = (double)A.dy[c2d], dy1 = (double)A.dy[c2d + 1];
  const double a11 = (double)A.a11[c2d], a12 = (double)A.a12[c2d], a21 = (double)A.a21[c2d], a22 = (double)A.a22[c2d];
  const double rcv = A.rcv;
  for (int m = m0; m < m1; ++m) {
    const long c = c2d + (long)(A.k0 + m) * sk;
    const double f = A.f[m];
    const double u0 = (double)u[c], u1 = (double)u[c + sj], v0 = (double)v[c], v1 = (double)v[c + 1];
    const double wk = (double)w[c], t = (double)pt[c];
    const double wu0 = u0 * dx0, wu1 = u1 * dx1, wv0 = v0 * dy0, wv1 = v1 * dy1;
    const double ut = 2.0 * (wu0 + wu1) / (dx0 + dx1);
    const double vt = 2.0 * (wv0 + wv1) / (dy0 + dy1);
    const double ua = a11 * ut + a12 * vt;
    const double va = a21 * ut + a22 * vt;
    pt[c] = (real)(t + ((0.5 * ((ua * ua + va * va) + wk * wk)) * (1.0 - f * f)) * rcv);
    w[c] = (real)(f * wk);
  }
}

template <bool W>
__global__ void __launch_bounds__(64 * RS_WAVES) k_rayleigh_scale(RsArgs A_) {
  PACE_KERNARG(RsArgs, A, A_);
  RS_THREAD(A);
  real* u = A.u;
  real* v = A.v;
  real* w = A.w;
  const bool last_i = i == n - 1, last_j = j == n - 1;
  for (int m = m0; m < m1; ++m) {
    const long c = c2d + (long)(A.k0 + m) * sk;
    const double f = A.f[m];
    const double u0 = (double)u[c], v0 = (double)v[c];
    double u1 = 0.0, v1 = 0.0, wk = 0.0;
    if (last_j) u1 = (double)u[c + sj];
    if (last_i) v1 = (double)v[c + 1];
    if (W) wk = (double)w[c];
    u[c] = (real)(f * u0);
    v[c] = (real)(f * v0);
    if (last_j) u[c + sj] = (real)(f * u1);
    if (last_i) v[c + 1] = (real)(f * v1);
    if (W) w[c] = (real)(f * wk);
  }
}

int launch_rayleigh_super(const Geo& g, const Met& met, const real* a11, const real* a12, const real* a21, const real* a22, real* u,
                          real* v, real* w, real* pt, const double* factor, int kmax, double rcv, int conserve, hipStream_t st) {
  RsArgs A;
  A.dx = met.dx, A.dy = met.dy, A.a11 = a11, A.a12 = a12, A.a21 = a21, A.a22 = a22;
  A.u = u, A.v = v, A.w = w, A.pt = pt;
  A.rcv = rcv;
  A.sk = g.sk, A.sj = g.sj, A.n = g.n;
  A.nseg = (g.n + 63) / 64;
  A.njg = (g.n + RS_WAVES - 1) / RS_WAVES;
  // (refused before the first launch: nothing is written on error)
  if ((long)A.nseg * A.njg * ((RS_TABLE + RS_LEVELS - 1) / RS_LEVELS) > 0x7fffffffL) return PACE_ERR_UNSUPPORTED;
  for (int k0 = 0; k0 < kmax; k0 += RS_TABLE) {
    A.k0 = k0;
    A.nlev = kmax - k0 < RS_TABLE ? kmax - k0 : RS_TABLE;
    for (int m = 0; m < RS_TABLE; ++m) A.f[m] = m < A.nlev ? factor[k0 + m] : 1.0;
    const long blocks = (long)A.nseg * A.njg * ((A.nlev + RS_LEVELS - 1) / RS_LEVELS);
    if (conserve) {
      hipLaunchKernelGGL(k_rayleigh_heat, dim3((unsigned)blocks), dim3(64 * RS_WAVES), 0, st, A);
      hipLaunchKernelGGL(k_rayleigh_scale<false>, dim3((unsigned)blocks), dim3(64 * RS_WAVES), 0, st, A);
    } else {
      hipLaunchKernelGGL(k_rayleigh_scale<true>, dim3((unsigned)blocks), dim3(64 * RS_WAVES), 0, st, A);
    }
    PACE_CHECK_LAUNCH();
  }
  return PACE_OK;
}
