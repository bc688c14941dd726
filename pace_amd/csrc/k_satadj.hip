// SatAdjust3d (fv3core/pace/fv3core/stencils/saturation_adjustment.py:561-1108): the fast saturation adjustment of the GFDL
// microphysics that LagrangianToEulerian runs after the remaps, non-hydrostatic branch.  Pointwise in (i, j, k):
//   k_sat_adjust_tables  the four saturation tables satadjust reads (table2, des2, tablew, desw) for indices -1 ... 2620,
//                        once per SatAdjust3d object, from the reference's on-the-fly forms (:46-160)
//   k_sat_adjust         satadjust (:561-944) over origin (isc, jsc, kmp), domain (nx, ny, nz - kmp): one thread per
//                        point, lanes along i, 64 x 4 patches; the wqs1 / wqs2 functions interpolate from the tables
//                        as the Fortran does with qs_table instead of evaluating 14-27 exp / log pairs per point
// Arithmetic is fp64 in both builds, in the reference's order of operations (no division folded into a reciprocal).
#include "common.h"
#include "kernels.h"
#include "thermo.h"

// saturation_adjustment.py:27-33
#define SA_DELT 0.1
#define SA_QS_LENGTH 2621
// table records: index -1 ... QS_LENGTH - 1, four doubles each (include/pace_hip.h PACE_SAT_ADJUST_TABLE_DOUBLES)
#define SA_FIRST (-1)
#define SA_RECORDS (SA_QS_LENGTH + 1)

// ---- the tables, as the reference evaluates them on the fly (:36-160) ----------------------------------------------------
__device__ __forceinline__ double sa_q_table_oneline(double dhc, double lhc, double tem) {
  return phys::E00 * exp((dhc * log(tem / phys::TICE) + (tem - phys::TICE) / (tem * phys::TICE) * lhc) / phys::RVGAS);
}
__device__ __forceinline__ double sa_vapor(double tem) { return sa_q_table_oneline(phys::DC_VAP, phys::LV0, tem); }
__device__ __forceinline__ double sa_ice(double tem) { return sa_q_table_oneline(phys::D2ICE, phys::LI2, tem); }
__device__ __forceinline__ double sa_tem_lower(double i) { return phys::T_SAT_MIN + SA_DELT * i; }
__device__ __forceinline__ double sa_tem_upper(double i) { return 253.16 + SA_DELT * i; }

// qs_table2_fn (:84-121), with its blend of the ice and water tables at i = 1599 and 1600
__device__ double sa_table2(int i) {
  double tem0 = sa_tem_lower(i);
  double table2 = i < 1600 ? sa_ice(tem0) : sa_vapor(tem0);
  if (i == 1599) {
    double table = sa_ice(tem0);
    tem0 = sa_tem_upper(i - 1400);
    table = (0.05 * (phys::TICE - tem0)) * table + (0.05 * (tem0 - 253.16)) * sa_vapor(tem0);
    const double m1 = sa_ice(sa_tem_lower(1598));
    const double p1 = sa_vapor(sa_tem_lower(1600));
    table2 = 0.25 * (m1 + 2.0 * table + p1);
  }
  if (i == 1600) {
    const double table = sa_vapor(sa_tem_upper(i - 1400));
    const double m1 = sa_ice(sa_tem_lower(1599));
    const double p1 = sa_vapor(sa_tem_lower(1601));
    table2 = 0.25 * (m1 + 2.0 * table + p1);
  }
  return table2;
}
__device__ __forceinline__ double sa_tablew(int i) { return sa_vapor(sa_tem_lower(i)); }

// des2_table / desw_table (:133-160); des_end (:124-130) ends BOTH on table2(i - 1)
__device__ __forceinline__ double sa_des(double t, double t_p1, int i) {
  double des = fmax(0.0, t_p1 - t);
  if (i == SA_QS_LENGTH - 1) des = fmax(0.0, t - sa_table2(i - 1));
  return des;
}

__global__ void __launch_bounds__(256) k_sat_adjust_tables(double* __restrict__ tables) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= SA_RECORDS) return;
  const int i = r + SA_FIRST;
  const double t2 = sa_table2(i), tw = sa_tablew(i);
  double* rec = tables + 4 * r;
  rec[0] = t2;
  rec[1] = sa_des(t2, sa_table2(i + 1), i);
  rec[2] = tw;
  rec[3] = sa_des(tw, sa_tablew(i + 1), i);
}

// ---- satadjust -------------------------------------------------------------------------------------------------------------
struct SatTab {
  double t, d;  // table2 / des2 (ice phase, T = 0) or tablew / desw (water, T = 2)
};
template <int T>
__device__ __forceinline__ SatTab sa_rec(const double* __restrict__ tab, int it) {
  const double* p = tab + 4 * (it - SA_FIRST) + T;
  return SatTab{p[0], p[1]};
}

__device__ __forceinline__ double sa_dim(double a, double b) { return a - b > 0 ? a - b : 0; }

// ap1_for_wqs2 (:502-505); the index is clamped to the tables (it only matters for a non-finite temperature)
__device__ __forceinline__ double sa_ap1(double ta) {
  const double ap1 = 10.0 * sa_dim(ta, phys::T_SAT_MIN) + 1.0;
  return fmin(ap1, (double)SA_QS_LENGTH) - 1;
}
__device__ __forceinline__ int sa_idx(double f) {
  const int i = (int)f;
  return i < SA_FIRST ? SA_FIRST : (i > SA_QS_LENGTH - 1 ? SA_QS_LENGTH - 1 : i);
}

// wqs2_fn_2 / wqs2_fn_w (:535-555) through wqsat_and_dqdt (:526-532)
template <int T>
__device__ __forceinline__ void sa_wqs2(const double* __restrict__ tab, double ta, double den, double& wqsat, double& dqdt) {
  const double ap1 = sa_ap1(ta);
  const double it = floor(ap1), it2 = floor(ap1 - 0.5);
  const SatTab a = sa_rec<T>(tab, sa_idx(it));
  const double d2 = sa_rec<T>(tab, sa_idx(it2)).d, d2p1 = sa_rec<T>(tab, sa_idx(it2 + 1)).d;
  const double es = a.t + (ap1 - it) * a.d;
  const double denom = phys::RVGAS * ta * den;
  wqsat = es / denom;
  dqdt = 10.0 * (d2 + (ap1 - it2) * (d2p1 - d2));
  dqdt = dqdt / denom;
}

// wqs1_fn_w / wqs1_fn_2 (:558-567) through wqsat_wsq1 (:530-532)
template <int T>
__device__ __forceinline__ double sa_wqs1(const double* __restrict__ tab, double it, double ap1, double ta, double den) {
  const SatTab a = sa_rec<T>(tab, sa_idx(it));
  const double es = a.t + (ap1 - it) * a.d;
  return es / (phys::RVGAS * ta * den);
}

__device__ __forceinline__ double sa_cvm(double mc_air, double qv, double c_vap, double q_liq, double q_sol) {
  return mc_air + qv * c_vap + q_liq * phys::C_LIQ + q_sol * phys::C_ICE;
}

__global__ void __launch_bounds__(256)
k_sat_adjust(Geo g, Water6 q, real* __restrict__ qa_out, real* __restrict__ te0_out, real* __restrict__ ptf,
             real* __restrict__ q_con_out, real* __restrict__ pkz_out, real* __restrict__ cappa_out, const real* __restrict__ dpf,
             const real* __restrict__ delzf, const real* __restrict__ areaf, const real* __restrict__ hsf,
             const double* __restrict__ tab, pace_sat_adjust_params_t p, int kmp, int last_step, int consv_te) {
  CELL_IJK(g, 0, 0, kmp);

  double qv = q.qvapor[c], ql = q.qliquid[c], qi = q.qice[c], qr = q.qrain[c], qs = q.qsnow[c], qg = q.qgraupel[c];
  const double dp = dpf[c], delz = delzf[c];
  const double c_air = p.c_air, c_vap = p.c_vap;

  double q_liq = ql + qr;
  double q_sol = qi + qs + qg;
  double qpz = q_liq + q_sol;
  double pt1 = ptf[c] / ((1.0 + p.zvir * qv) * (1.0 - qpz));
  const double t0 = pt1;
  qpz = qpz + qv;
  const double den = -dp / (phys::GRAV * delz);
  const double mc_air = (1.0 - qpz) * c_air;
  double cvm = sa_cvm(mc_air, qv, c_vap, q_liq, q_sol);
  double lhi = phys::LI00 + phys::DC_ICE * pt1;
  double icp2 = lhi / cvm;
  double lhl, lcp2;
  double te0 = 0.0;
  if (consv_te) te0 = -cvm * t0;
  // fix negative cloud ice with snow
  if (qi < 0.0) {
    qs = qs + qi;
    qi = 0.0;
  }
  // melt_cloud_ice (:183-197)
  if ((qi > 1.0e-8) && (pt1 > phys::TICE)) {
    const double factmp = p.fac_imlt * (pt1 - phys::TICE) / icp2;
    double sink = qi < factmp ? qi : factmp;
    qi = qi - sink;
    ql = ql + sink;
    q_liq = q_liq + sink;
    q_sol = q_sol - sink;
    cvm = sa_cvm(mc_air, qv, c_vap, q_liq, q_sol);
    sink = -sink;
    pt1 = pt1 + sink * lhi / cvm;
  }
  lhi = phys::LI00 + phys::DC_ICE * pt1;
  icp2 = lhi / cvm;
  // fix_negative_snow (:200-209)
  if (qs < 0.0) {
    qg = qg + qs;
    qs = 0.0;
  } else if (qg < 0.0) {
    const double tmp = fmin(-qg, fmax(qs, 0.0));
    qg = qg + tmp;
    qs = qs - tmp;
  }
  // fix_negative_cloud_water (:213-223)
  if (ql < 0.0) {
    const double tmp = fmin(-ql, fmax(qr, 0.0));
    ql = ql + tmp;
    qr = qr - tmp;
  } else if (qr < 0.0) {
    const double tmp = fmin(-qr, fmax(ql, 0.0));
    ql = ql - tmp;
    qr = qr + tmp;
  }
  // complete_freezing (:227-238)
  {
    const double dtmp = phys::TICE - 48.0 - pt1;
    if (ql > 0.0 && dtmp > 0.0) {
      const double sink = fmin(ql, dtmp / icp2);
      ql = ql - sink;
      qi = qi + sink;
      q_liq = q_liq - sink;
      q_sol = q_sol + sink;
      cvm = sa_cvm(mc_air, qv, c_vap, q_liq, q_sol);
      pt1 = pt1 + sink * lhi / cvm;
    }
  }
  double wqsat, dq2dt;
  sa_wqs2<2>(tab, pt1, den, wqsat, dq2dt);
  lhl = p.lv00 + p.d0_vap * pt1;
  lcp2 = lhl / cvm;
  lhi = phys::LI00 + phys::DC_ICE * pt1;
  icp2 = lhi / cvm;
  double tcp3 = lcp2 + icp2 * fmin(1.0, sa_dim(phys::TICE, pt1) / 48.0);
  double dq0 = (qv - wqsat) / (1.0 + tcp3 * dq2dt);
  double src;
  if (dq0 > 0) {  // whole grid - box saturated
    src = fmin(p.sat_adj0 * dq0, fmax(p.ql_gen - ql, p.fac_v2l * dq0));
  } else {  // ql_evaporation (:482-486)
    const double factor = -fmin(1.0, p.fac_l2v * 10.0 * (1.0 - qv / wqsat));
    src = -fmin(ql, factor * dq0);
  }
  // wqsat_correct (:489-495)
  qv = qv - src;
  ql = ql + src;
  q_liq = q_liq + src;
  cvm = sa_cvm(mc_air, qv, c_vap, q_liq, q_sol);
  pt1 = pt1 + src * lhl / cvm;
  lhl = p.lv00 + p.d0_vap * pt1;
  lcp2 = lhl / cvm;
  lhi = phys::LI00 + phys::DC_ICE * pt1;
  icp2 = lhi / cvm;
  tcp3 = lcp2 + icp2 * fmin(1.0, sa_dim(phys::TICE, pt1) / 48.0);
  if (last_step) {
    sa_wqs2<2>(tab, pt1, den, wqsat, dq2dt);
    dq0 = (qv - wqsat) / (1.0 + tcp3 * dq2dt);
    if (dq0 > 0) {
      src = dq0;
    } else {
      const double factor = -fmin(1.0, p.fac_l2v * 10.0 * (1.0 - qv / wqsat));
      src = -fmin(ql, factor * dq0);
    }
    qv = qv - src;
    ql = ql + src;
    q_liq = q_liq + src;
    cvm = sa_cvm(mc_air, qv, c_vap, q_liq, q_sol);
    pt1 = pt1 + src * lhl / cvm;
    lhl = p.lv00 + p.d0_vap * pt1;
    lcp2 = lhl / cvm;
    lhi = phys::LI00 + phys::DC_ICE * pt1;
    icp2 = lhi / cvm;
  }
  // homogenous_freezing (:241-253)
  {
    const double dtmp = phys::T_WFR - pt1;
    if (ql > 0.0 && dtmp > 0.0) {
      double sink = fmin(ql, dtmp / icp2);
      sink = fmin(sink, ql * dtmp * 0.125);
      ql = ql - sink;
      qi = qi + sink;
      q_liq = q_liq - sink;
      q_sol = q_sol + sink;
      cvm = sa_cvm(mc_air, qv, c_vap, q_liq, q_sol);
      pt1 = pt1 + sink * lhi / cvm;
    }
  }
  lhi = phys::LI00 + phys::DC_ICE * pt1;
  icp2 = lhi / cvm;
  // heterogeneous_freezing, the Bigg mechanism (:257-272)
  {
    const double exptc = exp(0.66 * (phys::TICE0 - pt1));
    const double tc = phys::TICE0 - pt1;
    if (ql > 0.0 && tc > 0.0) {
      double sink = 3.3333e-10 * p.mdt * (exptc - 1.0) * den * (ql * ql);
      sink = fmin(ql, sink);
      sink = fmin(sink, tc / icp2);
      ql = ql - sink;
      qi = qi + sink;
      q_liq = q_liq - sink;
      q_sol = q_sol + sink;
      cvm = sa_cvm(mc_air, qv, c_vap, q_liq, q_sol);
      pt1 = pt1 + sink * lhi / cvm;
    }
  }
  lhi = phys::LI00 + phys::DC_ICE * pt1;
  icp2 = lhi / cvm;
  // make_graupel (:275-290)
  {
    const double dtmp = (phys::TICE - 0.1) - pt1;
    if (qr > 1e-7 && dtmp > 0.0) {
      const double rainfac = (dtmp * 0.025) * (dtmp * 0.025);
      const double tmp = 1.0 < rainfac ? qr : rainfac * qr;
      const double sink = fmin(tmp, p.fac_r2g * dtmp / icp2);
      qr = qr - sink;
      qg = qg + sink;
      q_liq = q_liq - sink;
      q_sol = q_sol + sink;
      cvm = sa_cvm(mc_air, qv, c_vap, q_liq, q_sol);
      pt1 = pt1 + sink * lhi / cvm;
    }
  }
  lhi = phys::LI00 + phys::DC_ICE * pt1;
  icp2 = lhi / cvm;
  // melt_snow (:293-314)
  {
    const double dtmp = pt1 - (phys::TICE + 0.1);
    const double dimqs = sa_dim(p.qs_mlt, ql);
    if (qs > 1e-7 && dtmp > 0.0) {
      const double snowfac = (dtmp * 0.1) * (dtmp * 0.1);
      double tmp = 1.0 < snowfac ? qs : snowfac * qs;
      const double sink = fmin(tmp, p.fac_smlt * dtmp / icp2);
      tmp = fmin(sink, dimqs);
      qs = qs - sink;
      ql = ql + tmp;
      qr = qr + sink - tmp;
      q_liq = q_liq + sink;
      q_sol = q_sol - sink;
      cvm = sa_cvm(mc_air, qv, c_vap, q_liq, q_sol);
      pt1 = pt1 - sink * lhi / cvm;
    }
  }
  // autoconversion_cloud_to_rain (:317-322)
  if (ql > p.ql0_max) {
    const double sink = p.fac_l2r * (ql - p.ql0_max);
    qr = qr + sink;
    ql = ql - sink;
  }
  double iqs2, dqsdt;
  sa_wqs2<0>(tab, pt1, den, iqs2, dqsdt);
  const double expsubl = exp(0.875 * log(qi * den));
  lhl = p.lv00 + p.d0_vap * pt1;
  lcp2 = lhl / cvm;
  lhi = phys::LI00 + phys::DC_ICE * pt1;
  icp2 = lhi / cvm;
  const double tcp2 = lcp2 + icp2;
  const double adj_fac = last_step ? 1.0 : p.sat_adj0;
  // sublimation (:325-394)
  {
    double src = 0.0;
    if (pt1 < p.t_sub) {
      src = sa_dim(qv, 1e-6);
    } else if (pt1 < phys::TICE0) {
      const double dq = qv - iqs2;
      const double sink = adj_fac * dq / (1.0 + tcp2 * dqsdt);
      double pidep;
      if (qi > 1.0e-8) {
        pidep = p.sdt * dq * 349138.78 * expsubl /
                (iqs2 * den * phys::LAT2 / (0.0243 * phys::RVGAS * (pt1 * pt1)) + 4.42478e4);
      } else {
        pidep = 0.0;
      }
      if (dq > 0.0) {
        const double tmp = phys::TICE - pt1;
        const double qi_crt = p.qi_lim < 0.1 * tmp ? p.qi_gen * p.qi_lim / den : p.qi_gen * 0.1 * tmp / den;
        const double maxtmp = qi_crt - qi > pidep ? qi_crt - qi : pidep;
        src = sink < maxtmp ? sink : maxtmp;
        src = src < tmp / tcp2 ? src : tmp / tcp2;
      } else {
        const double dimtmp = sa_dim(pt1, p.t_sub);
        pidep = 1.0 < (dimtmp * 0.2) ? pidep : pidep * dimtmp * 0.2;
        src = pidep > sink ? pidep : sink;
        src = src > -qi ? src : -qi;
      }
    }
    qv = qv - src;
    qi = qi + src;
    q_sol = q_sol + src;
    cvm = sa_cvm(mc_air, qv, c_vap, q_liq, q_sol);
    const double lh = lhl + lhi;
    pt1 = pt1 + src * lh / cvm;
  }
  // virtual temperature updated
  const double q_con = q_liq + q_sol;
  double tmp = 1.0 + p.zvir * qv;
  const double pt = pt1 * tmp * (1.0 - q_con);
  tmp *= phys::RDGAS;
  const double cappa = tmp / (tmp + cvm);
  // fix negative graupel with available cloud ice
  if (qg < 0) {
    const double mintmp = fmin(-qg, fmax(0.0, qi));
    qg = qg + mintmp;
    qi = qi - mintmp;
  }
  // autoconversion from cloud ice to snow
  const double qim = p.qi0_max / den;
  if (qi > qim) {
    const double sink = p.fac_i2s * (qi - qim);
    qi = qi - sink;
    qs = qs + sink;
  }
  if (consv_te) te0_out[c] = dp * (te0 + cvm * pt1);
  if (p.do_qa && last_step) {
    cvm = mc_air + (qv + q_liq + q_sol) * c_vap;
    lhl = p.lv00 + p.d0_vap * pt1;
    lcp2 = lhl / cvm;
    lhi = phys::LI00 + phys::DC_ICE * pt1;
    icp2 = lhi / cvm;
    // combine water species
    if (p.rad_snow) q_sol = p.rad_graupel ? qi + qs + qg : qi + qs;
    else q_sol = qi;
    q_liq = p.rad_rain ? ql + qr : ql;
    const double q_cond = q_sol + q_liq;
    // the "liquid - frozen water temperature" (tin) for the saturated specific humidity
    const double tin = p.tintqs ? pt1 : pt1 - (lcp2 * q_cond + icp2 * q_sol);
    const double ap1 = sa_ap1(tin), it = floor(ap1);
    const double wqs1 = sa_wqs1<2>(tab, it, ap1, tin, den);
    const double iqs1 = sa_wqs1<0>(tab, it, ap1, tin, den);
    double qstar;
    if (tin < phys::T_WFR) {
      qstar = iqs1;
    } else if (tin >= phys::TICE) {
      qstar = wqs1;
    } else {
      const double rqi = q_cond > 1e-6 ? q_sol / q_cond : (phys::TICE - tin) / (phys::TICE - phys::T_WFR);
      qstar = rqi * iqs1 + (1.0 - rqi) * wqs1;
    }
    // higher than 10 m is "land", with more subgrid variability; "scale-aware": 100 km as the base
    const double mindw = fmin(1.0, fabs((double)hsf[c2]) / (10.0 * phys::GRAV));
    const double dw = p.dw_ocean + (p.dw_land - p.dw_ocean) * mindw;
    const double dbl_sqrt_area = dw * sqrt(sqrt((double)areaf[c2]) / 100.0e3);
    const double hvar = fmin(0.2, fmax(0.01, dbl_sqrt_area));
    // partial cloudiness by a subgrid linear pdf
    const double rh = qpz / qstar;
    double qa;
    if (rh > 0.75 && qpz > 1.0e-8) {
      const double dq = hvar * qpz;
      const double q_plus = qpz + dq;
      const double q_minus = qpz - dq;
      if (p.icloud_f == 2) {
        if (qpz > qstar) {
          qa = 1.0;
        } else if ((qstar < q_plus) && (q_cond > 1.0e-8)) {
          const double r = (q_plus - qstar) / dq;
          qa = fmin(1.0, r * r);
        } else {
          qa = 0.0;
        }
      } else if (qstar < q_minus) {
        qa = 1.0;
      } else {
        if (qstar < q_plus) {
          qa = p.icloud_f == 0 ? (q_plus - qstar) / (dq + dq) : (q_plus - qstar) / (2.0 * dq * (1.0 - q_cond));
        } else {
          qa = 0.0;
        }
        if (q_cond > 1.0e-8) qa = fmax(p.cld_min, qa);  // minimum cloudiness where there is substantial condensate
        qa = fmin(1.0, qa);
      }
    } else {
      qa = 0.0;
    }
    qa_out[c] = qa;
  }
  q.qvapor[c] = qv;
  q.qliquid[c] = ql;
  q.qrain[c] = qr;
  q.qsnow[c] = qs;
  q.qice[c] = qi;
  q.qgraupel[c] = qg;
  ptf[c] = pt;
  q_con_out[c] = q_con;
  cappa_out[c] = cappa;
  // compute_pkz_func (moist_cv.py:125-127)
  pkz_out[c] = moist_pkz(cappa, dp, delz, pt);
}

int launch_sat_adjust_tables(double* tables, hipStream_t st) {
  hipLaunchKernelGGL(k_sat_adjust_tables, dim3((SA_RECORDS + 255) / 256), dim3(256), 0, st, tables);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}

int launch_sat_adjust(const Geo& g, real* const* water, real* qcld, real* te, real* pt, real* q_con, real* pkz, real* cappa,
                      const real* delp, const real* delz, const real* area, const real* hs, const double* tables,
                      const pace_sat_adjust_params_t& p, int kmp, int last_step, int consv_te, hipStream_t st) {
  hipLaunchKernelGGL(k_sat_adjust, cell_grid(g, 0, 0, g.nk - kmp), dim3(64, 4), 0, st, g, water6(water), qcld, te, pt,
                     q_con, pkz, cappa, delp, delz, area, hs, tables, p, kmp, last_step, consv_te);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
