// DryConvectiveAdjustment (fv3core/pace/fv3core/stencils/fv_subgridz.py:68-964, the Fortran fv_subgrid_z): the dry convective
// adjustment a driver with fv_sg_adj > 0 runs on the dycore state once per physics step, non-hydrostatic branch.  Local to a
// column, levels 0 ... k_sponge - 1, no transcendental.  The reference runs five stencils over 18 full-size temporaries --
// init (:68-128), three m_loop sweeps with ratio 0.25, 0.5, 0.999 (:230-659), finalize (:667-732) -- and reads pe[isc, jsc, 0]
// on the host in between (:867).  Here: ONE launch, one thread per column (lanes along i), ONE bottom-up pass, no scratch field.
//
// Why one pass is the same arithmetic: a sweep at level k writes level k only; it reads level k - 1, which that sweep has not
// touched yet, and the flux h0 and the flag ri < ri_ref that the same sweep left at level k + 1.  So level k is final for sweep
// s once sweep s has done it, and sweep s + 1 can take level k + 1 right after.  The pass keeps a window of four levels in
// registers: a - 1 (just loaded = init), a (sweep 0 works here), a + 1 (sweep 1), a + 2 (sweep 2, then finalize and store).
// Every input is read once (a level keeps what came in until its finalize), every output written once.  qcon is not kept:
// the reference computes it at the start of a sweep and refreshes it in the take-up branch, which are the only two places
// where the condensates of a level change before its Richardson number is formed, so it always equals the sum over the
// level's current condensates.
// Arithmetic is fp64 in both builds, in the reference's order of operations (no division folded into a reciprocal; x ** 2 and
// (1 - r) ** 2.0 as products).
#include "common.h"
#include "kernels.h"
#include "thermo.h"

// fv_subgridz.py:33-41
#define SGZ_G2 (0.5 * phys::GRAV)
#define SGZ_T1_MIN 160.0
#define SGZ_T2_MIN 165.0
#define SGZ_USTAR2 1.0e-4
#define SGZ_RI_MAX 1.0
#define SGZ_RI_MIN 0.25

// the twelve mixed quantities: the nine tracers in the order of the C ABI (qvapor, qliquid, qrain, qice, qsnow, qgraupel,
// qo3mr, qsgs_tke, qcld), then u0, v0, w0
#define SGZ_NQ 12
enum { SGZ_QV = 0, SGZ_QL, SGZ_QR, SGZ_QI, SGZ_QS, SGZ_QG, SGZ_U = 9, SGZ_V = 10, SGZ_W = 11 };

struct SgzFields {
  real* q[SGZ_NQ];  // inout
  real* pt;         // inout
  real *u_dt, *v_dt;  // out
  const real *delp, *delz, *pkz, *peln, *pe;
};

struct SgzLevel {
  double q[SGZ_NQ];
  double q_in[SGZ_NQ], ta;  // the fields as they came in, for finalize
  double te, t0, se, gz;  // total_energy, t0, static_energy, gz
  double delp, pkz;
  double ri_ref;  // of this level against the one above, capped and scaled by the level's factor (:187-193, :435, :511, :587)
};

// the inputs of one level as loaded: the loads of level a - 2 are issued before the arithmetic of levels a ... a + 2 and are
// first read one trip later, so that their latency is not waited for (one wave per SIMD: nothing else would hide it)
struct SgzRaw {
  double q[SGZ_NQ];
  double pt, delp, pkz, delz, peln;
};

// what a sweep leaves at the level it has just done, for the level above to take up
struct SgzFlux {
  double h[SGZ_NQ + 1];  // h0_* of the twelve quantities and h0_total_energy
  bool mixed;            // ri < ri_ref
};

// tvol (:63-65)
__device__ __forceinline__ double sgz_tvol(const SgzLevel& L) {
  return L.gz + 0.5 * (L.q[SGZ_U] * L.q[SGZ_U] + L.q[SGZ_V] * L.q[SGZ_V] + L.q[SGZ_W] * L.q[SGZ_W]);
}
// standard_cm (:44-60)
__device__ __forceinline__ void sgz_cm(const SgzLevel& L, double& cpm, double& cvm) {
  const double qv = L.q[SGZ_QV];
  const double q_liq = L.q[SGZ_QL] + L.q[SGZ_QR];
  const double q_sol = L.q[SGZ_QI] + L.q[SGZ_QS] + L.q[SGZ_QG];
  cpm = (1.0 - (qv + q_liq + q_sol)) * phys::CP_AIR + qv * phys::CP_VAP + q_liq * phys::C_LIQ + q_sol * phys::C_ICE;
  cvm = (1.0 - (qv + q_liq + q_sol)) * phys::CV_AIR + qv * phys::CV_VAP + q_liq * phys::C_LIQ + q_sol * phys::C_ICE;
}
// adjust_cvm (:136-163)
__device__ __forceinline__ void sgz_adjust_cvm(SgzLevel& L) {
  double cpm, cvm;
  sgz_cm(L, cpm, cvm);
  const double tv = sgz_tvol(L);
  L.t0 = (L.te - tv) / cvm;
  L.se = cpm * L.t0 + tv;
}
// qcon_func (:131-133)
__device__ __forceinline__ double sgz_qcon(const SgzLevel& L) {
  return L.q[SGZ_QL] + L.q[SGZ_QI] + L.q[SGZ_QS] + L.q[SGZ_QR] + L.q[SGZ_QG];
}

__device__ __forceinline__ void sgz_fetch(const SgzFields& f, long c, SgzRaw& R) {
#pragma unroll
  for (int n = 0; n < SGZ_NQ; ++n) R.q[n] = f.q[n][c];
  R.pt = f.pt[c];
  R.delp = f.delp[c];
  R.pkz = f.pkz[c];
  R.delz = f.delz[c];
  R.peln = f.peln[c];
}

// init (:68-128) of level k from its loaded inputs; gzh: the height of the interface below it, counted from interface
// k_sponge; peln_below: peln of that interface
__device__ __forceinline__ void sgz_init(const SgzRaw& R, int k, double& gzh, double& peln_below, SgzLevel& L) {
#pragma unroll
  for (int n = 0; n < SGZ_NQ; ++n) L.q[n] = L.q_in[n] = R.q[n];
  L.t0 = L.ta = R.pt;
  L.delp = R.delp;
  L.pkz = R.pkz;
  double cpm, cvm;
  sgz_cm(L, cpm, cvm);
  L.gz = gzh - SGZ_G2 * R.delz;
  const double tmp = sgz_tvol(L);
  L.se = cpm * L.t0 + tmp;
  L.te = cvm * L.t0 + tmp;
  gzh = gzh - phys::GRAV * R.delz;
  // ri_ref of compute_richardson_number (:187-193): it depends on delp and peln alone, so once per level
  const double d = 400.0e2 - L.delp / (peln_below - R.peln);
  peln_below = R.peln;
  double ri_ref = SGZ_RI_MIN + (SGZ_RI_MAX - SGZ_RI_MIN) * (d > 0 ? d : 0) / 200.0e2;
  if (SGZ_RI_MAX < ri_ref) ri_ref = SGZ_RI_MAX;
  if (k == 3) ri_ref = ri_ref * 1.5;
  if (k == 2) ri_ref = ri_ref * 2.0;
  if (k == 1) ri_ref = ri_ref * 4.0;
  L.ri_ref = ri_ref;
}

// one level of one m_loop sweep (:274-659).  L: level k; A: level k - 1 as the previous sweep left it (not read at k = 0);
// fx: in, what this sweep left at level k + 1 (not read at the bottom level); out, what it leaves at level k
__device__ __forceinline__ void sgz_step(SgzLevel& L, const SgzLevel& A, SgzFlux& fx, bool bottom, bool top, double ratio,
                                         double xvir, double t_max, double t_min) {
  if (!bottom) {
    if (fx.mixed) {  // kh_adjust_up (:225-227)
#pragma unroll
      for (int n = 0; n < SGZ_NQ; ++n) L.q[n] = L.q[n] + fx.h[n] / L.delp;
      L.te = L.te + fx.h[SGZ_NQ] / L.delp;
    }
    sgz_adjust_cvm(L);
  }
  fx.mixed = false;
  if (top) return;
  // compute_richardson_number (:166-193)
  const double tv1 = A.t0 * (1.0 + xvir * A.q[SGZ_QV] - sgz_qcon(A));
  const double tv2 = L.t0 * (1.0 + xvir * L.q[SGZ_QV] - sgz_qcon(L));
  const double pt1 = tv1 / A.pkz;
  const double pt2 = tv2 / L.pkz;
  const double du = A.q[SGZ_U] - L.q[SGZ_U], dv = A.q[SGZ_V] - L.q[SGZ_V];
  double ri = (A.gz - L.gz) * (pt1 - pt2) / (0.5 * (pt1 + pt2) * (du * du + dv * dv + SGZ_USTAR2));
  if (tv1 > t_max && tv1 > tv2) {
    ri = 0;
  } else if (tv2 < t_min) {
    ri = ri < 0.1 ? ri : 0.1;
  }
  const bool mixed = ri < L.ri_ref;
  if (mixed) {
    // compute_mass_flux (:196-210)
    double max_ri_ratio = ri / L.ri_ref;
    if (max_ri_ratio < 0.0) max_ri_ratio = 0.0;
    const double mc = ratio * A.delp * L.delp / (A.delp + L.delp) * ((1.0 - max_ri_ratio) * (1.0 - max_ri_ratio));
    // kh_adjust_down, kh_adjust_energy_down (:213-222)
#pragma unroll
    for (int n = 0; n < SGZ_NQ; ++n) {
      const double h0 = mc * (L.q[n] - A.q[n]);
      L.q[n] = L.q[n] - h0 / L.delp;
      fx.h[n] = h0;
    }
    const double h0 = mc * (L.se - A.se);
    L.te = L.te - h0 / L.delp;
    fx.h[SGZ_NQ] = h0;
    fx.mixed = true;
  }
  // (an unmixed level above the bottom was adjusted right before from the same values)
  if (mixed || bottom) sgz_adjust_cvm(L);
}

// finalize (:667-732) of a level: its outputs, held for one trip (the stores are issued at the top of the next trip, next to
// the loads, so that the wait for the loads is not also a wait for stores just issued)
struct SgzOut {
  double q[SGZ_NQ];
  double pt, u_dt, v_dt;
};
__device__ __forceinline__ void sgz_finalize(const SgzLevel& L, double fra, double rdt, SgzOut& O) {
  O.pt = L.t0;
#pragma unroll
  for (int n = 0; n < SGZ_NQ; ++n) O.q[n] = L.q[n];
  if (fra < 1.0) {  // readjust_by_frac (:662-664)
    O.pt = L.ta + (L.t0 - L.ta) * fra;
#pragma unroll
    for (int n = 0; n < SGZ_NQ; ++n) O.q[n] = L.q_in[n] + (L.q[n] - L.q_in[n]) * fra;
  }
  O.u_dt = rdt * (O.q[SGZ_U] - L.q_in[SGZ_U]);
  O.v_dt = rdt * (O.q[SGZ_V] - L.q_in[SGZ_V]);
}
__device__ __forceinline__ void sgz_store(const SgzFields& f, long c, const SgzOut& O) {
  f.u_dt[c] = O.u_dt;
  f.v_dt[c] = O.v_dt;
  f.pt[c] = O.pt;
#pragma unroll
  for (int n = 0; n < SGZ_NQ; ++n) f.q[n][c] = O.q[n];
}

// One wave per workgroup: at C192 the 36 864 columns are 576 waves for 1024 SIMDs, so occupancy is no constraint and the
// window may take the registers it needs; what bounds the kernel is the chain of fp64 divisions per level.
__global__ void __launch_bounds__(64)
k_dry_convective_adjust(Geo g, SgzFields f, int ks, double xvir, double t_max, double fv_sg_adj, double timestep) {
  const int i = g.is + blockIdx.x * 64 + threadIdx.x;
  const int j = g.js + blockIdx.y;
  if (i > g.ie || j > g.je) return;
  const long c2 = IDX2(g, i, j);
  // the reference's host-side read of state.pe[isc, jsc, 0] (:867)
  const double t_min = (double)f.pe[IDX2(g, g.is, g.js)] < 2.0 ? SGZ_T1_MIN : SGZ_T2_MIN;
  const double fra = timestep / fv_sg_adj;
  const double rdt = 1.0 / timestep;

  SgzLevel W0, W1, W2, W3;  // levels a - 1, a, a + 1, a + 2
  SgzFlux F0, F1, F2;       // what sweep 0, 1, 2 left at the level below the one it does next
  F0.mixed = F1.mixed = F2.mixed = false;
  SgzRaw R;
  double gzh = 0.0;
  double peln_below = f.peln[c2 + (long)ks * g.sk];
  sgz_fetch(f, c2 + (long)(ks - 1) * g.sk, R);
  sgz_init(R, ks - 1, gzh, peln_below, W1);
  sgz_fetch(f, c2 + (long)(ks - 2) * g.sk, R);
  W2 = W1;  // (placeholders: not read before the window has moved them out)
  W3 = W1;
  W0 = W1;
  SgzOut O;  // the outputs of level a + 3, finalized in the trip before
  for (int a = ks - 1; a >= -2; --a) {
    if (a >= 1) sgz_init(R, a - 1, gzh, peln_below, W0);
    if (a >= 2) sgz_fetch(f, c2 + (long)(a - 2) * g.sk, R);
    if (a + 3 <= ks - 1) sgz_store(f, c2 + (long)(a + 3) * g.sk, O);
    if (a >= 0) sgz_step(W1, W0, F0, a == ks - 1, a == 0, 0.25, xvir, t_max, t_min);
    if (a + 1 >= 0 && a + 1 <= ks - 1) sgz_step(W2, W1, F1, a + 1 == ks - 1, a + 1 == 0, 0.5, xvir, t_max, t_min);
    if (a + 2 <= ks - 1) {
      sgz_step(W3, W2, F2, a + 2 == ks - 1, a + 2 == 0, 0.999, xvir, t_max, t_min);
      sgz_finalize(W3, fra, rdt, O);
    }
    W3 = W2;
    W2 = W1;
    W1 = W0;
  }
  sgz_store(f, c2, O);
}

int launch_dry_convective_adjust(const Geo& g, real* const* tracers, real* pt, real* ua, real* va, real* w, real* u_dt,
                                 real* v_dt, const real* delp, const real* delz, const real* pkz, const real* peln,
                                 const real* pe, int k_sponge, double xvir, double t_max, double fv_sg_adj, double timestep,
                                 hipStream_t st) {
  SgzFields f;
  for (int n = 0; n < 9; ++n) f.q[n] = tracers[n];
  f.q[SGZ_U] = ua;
  f.q[SGZ_V] = va;
  f.q[SGZ_W] = w;
  f.pt = pt;
  f.u_dt = u_dt;
  f.v_dt = v_dt;
  f.delp = delp;
  f.delz = delz;
  f.pkz = pkz;
  f.peln = peln;
  f.pe = pe;
  hipLaunchKernelGGL(k_dry_convective_adjust, dim3((unsigned)((g.n + 63) / 64), (unsigned)g.n), dim3(64), 0, st, g, f,
                     k_sponge, xvir, t_max, fv_sg_adj, timestep);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
