// Held-Suarez (1994) forcing, the dry climate benchmark (the Fortran FV3's Held_Suarez_Tend; the reference has none): Newtonian
// relaxation of the temperature toward a zonally symmetric equilibrium and Rayleigh friction of the low-level winds, as tendencies
// for ApplyPhysicsToDycore.  For every cell of the compute domain (origin (3, 3, 0), extent (n, n, nk)), in double on the stored
// values (the float32 library widens first), with no contraction and no reciprocal, in exactly this order:
//
//   ps    = pe[i,j,nk]
//   pm    = 0.5 * (pe[i,j,k] + pe[i,j,k+1])
//   sigma = pm / ps
//   lp    = lean_log(pm / p0)
//   pk    = lean_exp(kappa * lp)
//   x     = ((t0 - delta_t_y * s2) - (delta_theta_z * lp) * c2) * pk
//   teq   = (x < t_strat) ? t_strat : x                       a NaN stays a NaN
//   hx    = (sigma - sigma_b) / (1.0 - sigma_b)               the denominator formed once, on the host
//   h     = (hx < 0.0) ? 0.0 : hx                             a NaN stays a NaN
//   kv    = k_f * h
//   kt    = k_a + ((k_s - k_a) * h) * (c2 * c2)
//   u_dt  = -((kv * ua) / (1.0 + kv * dt))                    likewise v_dt from va
//   pt_dt = -(((kt * (pt - teq)) / (1.0 + kt * dt)) * heating_scale)
//   accumulate: out = (real)((double)out + value), otherwise out = (real)value; teq (if given) is always stored
//
//   k_held_suarez  1-D grid, 256 threads = 4 waves.  A workgroup takes 64 points of i of four consecutive rows j and HS_LEVELS
//            consecutive levels: a wave takes a row, lane l the point i = 3 + 64 * segment + l -- 512 B contiguous (float32: 256 B)
//            of each array, k_nudge's form -- and walks the chunk's levels of its column.  It loads ps, s2 and c2 once and carries
//            pe[k + 1] into the next level, so pe is fetched (HS_LEVELS + 1) / HS_LEVELS times, not twice.  The segment is the
//            fastest index of the grid, then the row group, then the chunk: workgroups next to each other in dispatch order read
//            next to each other in memory.  A level's loads are all issued before its arithmetic.  Whether the tendencies are
//            accumulated and teq stored is uniform over the launch.
//
// Nothing outside the compute domain's nk levels is written (not the halo, not level nk, not the row padding), nothing outside the
// compute domain is read (pe on nk + 1 levels there).  No atomics, no workspace, no LDS.
#include "common.h"
#include "kernels.h"
#include "lean_math.h"

#define HS_WAVES 4
#ifndef HS_LEVELS
#define HS_LEVELS 8  // levels a thread walks
#endif

struct HsArgs {
  const real *pe, *ua, *va, *pt, *s2, *c2;
  real *u_dt, *v_dt, *pt_dt, *teq;
  double dt, p0, kappa, sigma_b, one_minus_sigma_b, k_f, k_a, k_s_minus_k_a, delta_t_y, delta_theta_z, t0, t_strat, heating_scale;
  long sk;
  int sj, n, nk, nseg, njg, accumulate;
};

__global__ void __launch_bounds__(64 * HS_WAVES) k_held_suarez(HsArgs A) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int b = (int)blockIdx.x;
  const int seg = b % A.nseg, rest = b / A.nseg;
  const int jg = rest % A.njg, chunk = rest / A.njg;
  const int i = seg * 64 + lane, j = jg * HS_WAVES + wave;  // within the compute domain
  if (i >= A.n || j >= A.n) return;
  const long c2d = (long)(i + 3) + (long)(j + 3) * A.sj;
  const int k0 = chunk * HS_LEVELS;
  const int k1 = k0 + HS_LEVELS < A.nk ? k0 + HS_LEVELS : A.nk;
  // (no __restrict__: nothing forbids the caller's inputs to share an array)
  const double ps = (double)A.pe[c2d + (long)A.nk * A.sk];
  const double s2 = (double)A.s2[c2d], cc = (double)A.c2[c2d];
  const double c4 = cc * cc;
  const bool accumulate = A.accumulate != 0, store_teq = A.teq != nullptr;
  double pe_lo = (double)A.pe[c2d + (long)k0 * A.sk];
  for (int k = k0; k < k1; ++k) {
    const long c = c2d + (long)k * A.sk;
    const double pe_hi = (double)A.pe[c + A.sk];
    const double ua = (double)A.ua[c], va = (double)A.va[c], pt = (double)A.pt[c];
    double u_old = 0.0, v_old = 0.0, t_old = 0.0;
    if (accumulate) {
      u_old = (double)A.u_dt[c];
      v_old = (double)A.v_dt[c];
      t_old = (double)A.pt_dt[c];
    }
    const double pm = 0.5 * (pe_lo + pe_hi);
    const double sigma = pm / ps;
    const double lp = lean_log(pm / A.p0);
    const double pk = lean_exp(A.kappa * lp);
    const double x = ((A.t0 - A.delta_t_y * s2) - (A.delta_theta_z * lp) * cc) * pk;
    const double teq = (x < A.t_strat) ? A.t_strat : x;
    const double hx = (sigma - A.sigma_b) / A.one_minus_sigma_b;
    const double h = (hx < 0.0) ? 0.0 : hx;
    const double kv = A.k_f * h;
    const double kt = A.k_a + (A.k_s_minus_k_a * h) * c4;
    const double dv = 1.0 + kv * A.dt;
    const double u_dt = -((kv * ua) / dv);
    const double v_dt = -((kv * va) / dv);
    const double pt_dt = -(((kt * (pt - teq)) / (1.0 + kt * A.dt)) * A.heating_scale);
    if (accumulate) {
      A.u_dt[c] = (real)(u_old + u_dt);
      A.v_dt[c] = (real)(v_old + v_dt);
      A.pt_dt[c] = (real)(t_old + pt_dt);
    } else {
      A.u_dt[c] = (real)u_dt;
      A.v_dt[c] = (real)v_dt;
      A.pt_dt[c] = (real)pt_dt;
    }
    if (store_teq) A.teq[c] = (real)teq;
    pe_lo = pe_hi;
  }
}

int launch_held_suarez(const Geo& g, const pace_held_suarez_config_t& cfg, const real* pe, const real* ua, const real* va,
                       const real* pt, const real* sin2lat, const real* cos2lat, real* u_dt, real* v_dt, real* pt_dt, real* teq,
                       hipStream_t st) {
  HsArgs A;
  A.pe = pe, A.ua = ua, A.va = va, A.pt = pt, A.s2 = sin2lat, A.c2 = cos2lat;
  A.u_dt = u_dt, A.v_dt = v_dt, A.pt_dt = pt_dt, A.teq = teq;
  A.dt = cfg.dt, A.p0 = cfg.p0, A.kappa = cfg.kappa, A.sigma_b = cfg.sigma_b;
  A.one_minus_sigma_b = 1.0 - cfg.sigma_b;  // (formed once, in double)
  A.k_f = cfg.k_f, A.k_a = cfg.k_a, A.k_s_minus_k_a = cfg.k_s - cfg.k_a;
  A.delta_t_y = cfg.delta_t_y, A.delta_theta_z = cfg.delta_theta_z, A.t0 = cfg.t0, A.t_strat = cfg.t_strat;
  A.heating_scale = cfg.heating_scale;
  A.sk = g.sk, A.sj = g.sj, A.n = g.n, A.nk = g.nk;
  A.nseg = (g.n + 63) / 64;
  A.njg = (g.n + HS_WAVES - 1) / HS_WAVES;
  A.accumulate = cfg.accumulate;
  const long blocks = (long)A.nseg * A.njg * ((g.nk + HS_LEVELS - 1) / HS_LEVELS);
  if (blocks > 0x7fffffffL) return PACE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_held_suarez, dim3((unsigned)blocks), dim3(64 * HS_WAVES), 0, st, A);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
