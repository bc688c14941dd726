// The stencils of LagrangianToEulerian around the vertical remaps (fv3core/pace/fv3core/stencils/remapping.py:42-283,
// moist_cv.py:16-172), for the modes the reference implements (non-hydrostatic, kord_tm < 0); the saturation adjustment,
// between the remaps and k_l2e_finish, is k_satadj.hip.  All of them are local in (i, j) and -- once ps = pe[km] is read -- in k, so each is ONE thread-per-cell
// launch: [k][j][i] storage, lanes along i, 64 x 4 patches.
//   k_l2e_prepare    init_pe + moist_cv_pt_pressure + pn2_pk_delp (3 stencils, 15 computations)
//   k_l2e_post       undo_delz_adjust_and_copy_peln + moist_pkz
//   k_l2e_pressures  pressures_mapu / pressures_mapv (the bottom-pressure broadcast fields never exist)
//   k_l2e_finish     update_ua + copy_from_below, then moist_pt_last_step or the division by pkz
#include "common.h"
#include "kernels.h"
#include "thermo.h"

// moist_cv_nwat6_fn + moist_cvm + set_cappa (moist_cv.py:16-46)
__device__ __forceinline__ void moist_cv(const Water6Const& q, long c, double r_vir, double& gz, double& cappa) {
  // (the casts: with real = float the condensate sums would otherwise be formed in float)
  const double qv = q.qvapor[c];
  const double ql = (double)q.qliquid[c] + (double)q.qrain[c];
  const double qs = (double)q.qice[c] + (double)q.qsnow[c] + (double)q.qgraupel[c];
  gz = ql + qs;
  cappa = moist_cappa(moist_cvm(qv + gz, qv, ql, qs), 1.0 + r_vir * qv);
}

__global__ void __launch_bounds__(256)
k_l2e_prepare(Geo g, Water6Const q, real* __restrict__ q_con, real* __restrict__ pt, real* __restrict__ cappa,
              real* __restrict__ delp, real* __restrict__ delz, const real* __restrict__ pe, real* __restrict__ pe1,
              real* __restrict__ pe2, const real* __restrict__ ak, const real* __restrict__ bk, real* __restrict__ dp2,
              real* __restrict__ ps, real* __restrict__ pn2, const real* __restrict__ peln, real* __restrict__ pk,
              double ptop, double akap, double r_vir) {
  CELL_IJK(g, 0, 1, 0);
  const int km = g.nk;
  // init_pe over the compute domain + the extra row je+1 (remapping.py:42-56)
  pe1[c] = pe[c];
  if (k == 0) pe2[c] = ptop;
  if (k == km) pe2[c] = pe[c];
  if (j > g.je) return;
  const double psv = pe[c2 + (long)km * g.sk];
  if (k == km) {
    ps[c2] = psv;
    pn2[c] = peln[c];
    return;
  }
  // moist_pt_func + delz_adjust (remapping.py:133-154)
  double gz, cp;
  moist_cv(q, c, r_vir, gz, cp);
  q_con[c] = gz;
  cappa[c] = cp;
  const double p = pt[c], dpo = delp[c], dzo = delz[c];
  pt[c] = p * exp(cp / (1.0 - cp) * log(phys::RDG * dpo / dzo * p));
  delz[c] = -dzo / dpo;
  // pressure_updates + pn2_pk_delp (remapping.py:155-193)
  const double e0 = (k == 0) ? ptop : ak[k] + bk[k] * psv;
  const double e1 = (k + 1 == km) ? psv : ak[k + 1] + bk[k + 1] * psv;
  if (k > 0) pe2[c] = e0;
  const double d = e1 - e0;
  dp2[c] = d;
  delp[c] = d;
  const double lp = log(e0);
  pn2[c] = lp;
  pk[c] = exp(akap * lp);
}

__global__ void __launch_bounds__(256)
k_l2e_post(Geo g, Water6Const q, real* __restrict__ q_con, real* __restrict__ pkz, const real* __restrict__ pt,
           real* __restrict__ cappa, const real* __restrict__ delp, real* __restrict__ delz, real* __restrict__ peln,
           real* __restrict__ pe0, const real* __restrict__ pn2, double r_vir) {
  CELL_IJK(g, 0, 0, 0);
  const int km = g.nk;
  pe0[c] = peln[c];
  peln[c] = pn2[c];
  if (k == km) return;
  const double dz = -(double)delz[c] * (double)delp[c];  // (in double: pkz below is formed from it, not from what delz stores)
  delz[c] = dz;
  double gz, cp;
  moist_cv(q, c, r_vir, gz, cp);
  q_con[c] = gz;
  cappa[c] = cp;
  pkz[c] = moist_pkz(cp, delp[c], dz, pt[c]);
}

// dir 0: pressures_mapu (neighbour to the south, window + 1 row); dir 1: pressures_mapv (neighbour to the west, + 1 column)
template <int DIR>
__global__ void __launch_bounds__(256)
k_l2e_pressures(Geo g, const real* __restrict__ pe, const real* __restrict__ pe1, const real* __restrict__ ak,
                const real* __restrict__ bk, real* __restrict__ pe0, real* __restrict__ pe3) {
  CELL_IJK(g, DIR == 1 ? 1 : 0, DIR == 0 ? 1 : 0, 0);
  const int km = g.nk;
  const long nb = DIR == 0 ? -(long)g.sj : -1L;
  const long cb = c2 + (long)km * g.sk;
  if (DIR == 0) {
    pe0[c] = (k == 0) ? pe[c] : 0.5 * ((double)pe[c + nb] + (double)pe1[c]);  // (the casts: the pair sums in double)
    const double bkh = 0.5 * bk[k];
    pe3[c] = ak[k] + bkh * ((double)pe[cb + nb] + (double)pe[cb]);
  } else {
    if (k == 0) {
      pe3[c] = ak[0];
      pe0[c] = pe[c];
    } else {
      const double bkh = 0.5 * bk[k];
      pe0[c] = 0.5 * ((double)pe[c + nb] + (double)pe[c]);
      pe3[c] = ak[k] + bkh * ((double)pe[cb + nb] + (double)pe[cb]);
    }
  }
}

__global__ void __launch_bounds__(256)
k_l2e_finish(Geo g, Water6Const q, real* __restrict__ pe, const real* __restrict__ pe2, real* __restrict__ pt,
             const real* __restrict__ pkz, double r_vir, int last_step) {
  CELL_IJK(g, 0, 0, 0);
  const int km = g.nk;
  if (k >= 1 && k < km) pe[c] = pe2[c];  // update_ua + copy_from_below: pe becomes the Eulerian interfaces
  if (last_step) {
    // moist_pt_last_step over km + 1 levels with dtmp = 0 (moist_cv.py:73-122, remapping.py:680-692)
    const double gz = (double)q.qliquid[c] + (double)q.qrain[c] + (double)q.qice[c] + (double)q.qsnow[c] + (double)q.qgraupel[c];
    pt[c] = (pt[c] + 0.0 * pkz[c]) / ((1.0 + r_vir * q.qvapor[c]) * (1.0 - gz));
  } else if (k < km) {
    pt[c] = pt[c] / pkz[c];
  }
}

int launch_l2e_prepare(const Geo& g, const real* const* water, real* q_con, real* pt, real* cappa, real* delp,
                       real* delz, const real* pe, real* pe1, real* pe2, const real* ak, const real* bk, real* dp2,
                       real* ps, real* pn2, const real* peln, real* pk, double ptop, double akap, double r_vir,
                       hipStream_t st) {
  const Water6Const q = water6(water);
  hipLaunchKernelGGL(k_l2e_prepare, cell_grid(g, 0, 1, g.nk + 1), dim3(64, 4), 0, st, g, q, q_con, pt, cappa, delp, delz, pe, pe1,
                     pe2, ak, bk, dp2, ps, pn2, peln, pk, ptop, akap, r_vir);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}

int launch_l2e_post(const Geo& g, const real* const* water, real* q_con, real* pkz, const real* pt, real* cappa,
                    const real* delp, real* delz, real* peln, real* pe0, const real* pn2, double r_vir, hipStream_t st) {
  const Water6Const q = water6(water);
  hipLaunchKernelGGL(k_l2e_post, cell_grid(g, 0, 0, g.nk + 1), dim3(64, 4), 0, st, g, q, q_con, pkz, pt, cappa, delp, delz, peln,
                     pe0, pn2, r_vir);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}

int launch_l2e_pressures(const Geo& g, int dir, const real* pe, const real* pe1, const real* ak, const real* bk,
                         real* pe0, real* pe3, hipStream_t st) {
  if (dir == 0) hipLaunchKernelGGL(k_l2e_pressures<0>, cell_grid(g, 0, 1, g.nk + 1), dim3(64, 4), 0, st, g, pe, pe1, ak, bk, pe0, pe3);
  else hipLaunchKernelGGL(k_l2e_pressures<1>, cell_grid(g, 1, 0, g.nk + 1), dim3(64, 4), 0, st, g, pe, pe1, ak, bk, pe0, pe3);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}

int launch_l2e_finish(const Geo& g, const real* const* water, real* pe, const real* pe2, real* pt, const real* pkz,
                      double r_vir, int last_step, hipStream_t st) {
  const Water6Const q = water6(water);
  hipLaunchKernelGGL(k_l2e_finish, cell_grid(g, 0, 0, g.nk + 1), dim3(64, 4), 0, st, g, q, pe, pe2, pt, pkz, r_vir, last_step);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
