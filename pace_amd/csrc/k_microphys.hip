// Microphysics (physics/pace/physics/stencils/microphysics.py:26-1827, physics/pace/physics/functions/microphysics_funcs.py): the
// GFDL cloud microphysics, the one package of the reference's Physics.  The reference runs fields_init, then ntimes x
// (warm_rain(first half), sedimentation, warm_rain(second half), icloud), then fields_update, as five stencils over 45 full 3-D
// work fields.  Here: ONE launch, one thread per column (lanes along i), the work state of a column in the workspace buffer as
// MP_NW arrays [array][level][column] (columns compact, so every access is coalesced along i), per-column scalars in registers.
// Levels are walked in the reference's order wherever it has a FORWARD / BACKWARD computation; computations the reference
// spreads over several PARALLEL blocks are fused into the sweep that has their operands:
//
//   init        forward   fields_init (:100-303): dry mixing ratios, fix_negative with the borrowing of vapour from below
//   per sub-step
//     prepare   backward  warm_rain's is_first block (:359-372), ze (:411-421) as the layer depth dz = ze[k] - ze[k + 1], rain's no_fall
//     fall      forward   warm_rain first half (:407-671): fall speed, revap_racc, the implicit fall with sedi_w, revap_racc
//     autoconv  forward   :682-756, the slope of cloud water from the levels above and below as they are before this sweep
//     melt      forward   sedimentation (:790-866): fall speeds, stop_k, melting of cloud ice; no_fall of ice, snow, graupel, rain
//     fall      forward   the implicit falls of ice, snow, graupel (:893-1418) and warm_rain's second half, level by level: a
//                         level's fall reads the level above of the same species only
//     autoconv  forward
//     icloud    forward   :1542-1716, pimlt / pihom one level ahead so that the slope of cloud ice sees both neighbours after it
//   update      forward   fields_update (:1766-1827): the momentum transport, the ten tendencies (accumulated), mm/day
//
// no_fall (:380-405) is, after its FORWARD and BACKWARD pass, one flag per column: no level holds more than QRMIN.
// Only the NamelistDefaults switches are implemented (pace_amd/physics/stencils/microphysics.py refuses every other value):
// use_ppm, do_sedi_heat, prog_ccn, de_ice, const_v* off, irain_f 0; do_sedi_w, sedi_transport, fix_negative, do_qa, fast_sat_adj,
// z_slope_liq, z_slope_ice on; p_nonhydro False as the reference hard-codes it.  With do_qa the cloud fraction block of
// subgrid_z_proc is not run and qa_dt is set to zero.
// Arithmetic is fp64 in the reference's order of operations, divisions kept; x ** 2 is a product, any other power is pow().
// The factors setupm / _set_timestep compute come in by value (pace_microphysics_config_t).
#include "common.h"
#include "kernels.h"
#include "thermo.h"

// microphysics_funcs.py:7-42
namespace mp {
constexpr double VCONS = 6.6280504;
constexpr double VCONG = 87.2382675;
constexpr double NORMS = 942477796.076938;
constexpr double NORMG = 5026548245.74367;
constexpr double VCONR = 2503.23638966667;
constexpr double NORMR = 25132741228.7183;
constexpr double THR = 1.0e-8;
constexpr double THI = 1.0e-8;
constexpr double THG = 1.0e-8;
constexpr double THS = 1.0e-8;
constexpr double AA = -4.14122e-5;
constexpr double BB = -0.00538922;
constexpr double CC = -0.0516344;
constexpr double DD_FS = 0.00216078;
constexpr double EE = 1.9714;
constexpr double VR_MIN = 1.0e-3;
constexpr double VF_MIN = 1.0e-5;
constexpr double P_MIN = 100.0;
constexpr double DT_FR = 8.0;
constexpr double SFCRHO = 1.2;
constexpr double RHOR = 1.0e3;
constexpr double QCMIN = 1.0e-12;
constexpr double QRMIN = 1.0e-8;
constexpr double QVMIN = 1.0e-20;
}  // namespace mp

typedef pace_microphysics_config_t MpCfg;

// Branch counters of tools/make_golden_microphysics.py (make emu-mpcov): the emulation runs one thread at a time, so plain
// increments do; the counters live behind the work arrays.  In every other build MP_COV is nothing.
#if defined(PACE_MP_COVERAGE) && defined(PACE_EMU)
enum { COV_rain_falls = 0, COV_rain_no_fall, COV_ice_falls, COV_ice_no_fall, COV_snow_falls, COV_snow_no_fall, COV_graupel_falls,
       COV_graupel_no_fall, COV_sedi_ice_melt, COV_rain_evaporation, COV_rain_accretion, COV_autoconv_land, COV_autoconv_ocean,
       COV_icloud_ice_melt, COV_icloud_water_freeze, COV_psaci, COV_psacw, COV_pracs, COV_psmlt, COV_pgmlt, COV_pgfr, COV_pgacs,
       COV_instant_evaporation, COV_condensation, COV_ice_deposition, COV_ice_sublimation, COV_snow_sublimation,
       COV_graupel_sublimation, COV_graupel_deposition, COV_fix_negative, COV_N };
static long long* mp_cov = nullptr;
#define MP_COV(name) (++mp_cov[COV_##name])
#define MP_COV_WORDS COV_N
#else
#define MP_COV(name) ((void)0)
#define MP_COV_WORDS 0
#endif

enum { MP_QV = 0, MP_QL, MP_QR, MP_QI, MP_QS, MP_QG, MP_TZ, MP_DP1, MP_DEN, MP_DENFAC, MP_DZ, MP_VTR, MP_VTI, MP_VTS, MP_VTG,
       MP_M1, MP_NW };

struct MpFields {
  const real *pt, *qv, *ql, *qr, *qi, *qs, *qg, *ua, *va, *delp, *dz, *land, *area;
  real* w;
  real *qv_dt, *ql_dt, *qr_dt, *qi_dt, *qs_dt, *qg_dt, *qa_dt, *udt, *vdt, *pt_dt;
  real *rain, *snow, *ice, *graupel;
};

// the species and the temperature of one point
struct MpPt {
  double qv, ql, qr, qi, qs, qg, tz;
};

// a column of the workspace
struct MpCol {
  double* p;
  long nc, na;  // stride of a level, of an array
  __device__ __forceinline__ double& operator()(int a, int k) const { return p[a * na + k * nc]; }
};

__device__ __forceinline__ double mp_min(double a, double b) { return a < b ? a : b; }
__device__ __forceinline__ double mp_max(double a, double b) { return a > b ? a : b; }
__device__ __forceinline__ double mp_dim(double x, double y) {
  const double d = x - y;
  return d > 0.0 ? d : 0.0;
}
__device__ __forceinline__ double mp_cvm(const MpCfg& c, double qv, double q_liq, double q_sol) {
  return c.c_air + qv * c.c_vap + q_liq * phys::C_LIQ + q_sol * phys::C_ICE;
}
__device__ __forceinline__ MpPt mp_load(const MpCol& W, int k) {
  return MpPt{W(MP_QV, k), W(MP_QL, k), W(MP_QR, k), W(MP_QI, k), W(MP_QS, k), W(MP_QG, k), W(MP_TZ, k)};
}
__device__ __forceinline__ void mp_store(const MpCol& W, int k, const MpPt& P) {
  W(MP_QV, k) = P.qv;
  W(MP_QL, k) = P.ql;
  W(MP_QR, k) = P.qr;
  W(MP_QI, k) = P.qi;
  W(MP_QS, k) = P.qs;
  W(MP_QG, k) = P.qg;
  W(MP_TZ, k) = P.tz;
}

// wqs1, wqs2, iqs1, iqs2 (microphysics_funcs.py:53-162)
__device__ __forceinline__ double mp_wqs1(double ta, double den) {
  return (phys::E00 *
          exp((phys::DC_VAP * log(ta / phys::TICE) + phys::LV0 * (ta - phys::TICE) / (ta * phys::TICE)) / phys::RVGAS)) /
         (phys::RVGAS * ta * den);
}
__device__ __forceinline__ double mp_wqs2(double ta, double den, double& dqdt) {
  const double tmp = mp_wqs1(ta, den);
  dqdt = tmp * (phys::DC_VAP + phys::LV0 / ta) / (phys::RVGAS * ta);
  return tmp;
}
__device__ __forceinline__ double mp_iqs1(double ta, double den) {
  if (ta < phys::TICE) {
    if (ta >= phys::T_SAT_MIN)
      return (phys::E00 *
              exp((phys::D2ICE * log(ta / phys::TICE) + phys::LI2 * (ta - phys::TICE) / (ta * phys::TICE)) / phys::RVGAS)) /
             (phys::RVGAS * ta * den);
    return (phys::E00 * exp((phys::D2ICE * log(1.0 - 160.0 / phys::TICE) - phys::LI2 * 160.0 / (phys::T_SAT_MIN * phys::TICE)) /
                            phys::RVGAS)) /
           (phys::RVGAS * phys::T_SAT_MIN * den);
  }
  if (ta <= phys::TICE + 102.0) return mp_wqs1(ta, den);
  return mp_wqs1(phys::TICE + 102.0, den);
}
__device__ __forceinline__ double mp_iqs2(double ta, double den, double& dqdt) {
  const double tmp = mp_iqs1(ta, den);
  if (ta < phys::TICE) {
    if (ta >= phys::T_SAT_MIN)
      dqdt = tmp * (phys::D2ICE + phys::LI2 / ta) / (phys::RVGAS * ta);
    else
      dqdt = tmp * (phys::D2ICE + phys::LI2 / phys::T_SAT_MIN) / (phys::RVGAS * phys::T_SAT_MIN);
  } else {
    if (ta <= phys::TICE + 102.0)
      dqdt = tmp * (phys::DC_VAP + phys::LV0 / ta) / (phys::RVGAS * ta);
    else
      dqdt = tmp * (phys::DC_VAP + phys::LV0 / (phys::TICE + 102.0)) / (phys::RVGAS * (phys::TICE + 102.0));
  }
  return tmp;
}

// acr3d (:165-179)
__device__ __forceinline__ double mp_acr3d(double v1, double v2, double q1, double q2, double c, double cac_ik, double cac_i1k,
                                           double cac_i2k, double rho) {
  const double t1 = sqrt(q1 * rho);
  const double s1 = sqrt(q2 * rho);
  const double s2 = sqrt(s1);
  return c * fabs(v1 - v2) * q1 * s2 * (cac_ik * t1 + cac_i1k * sqrt(t1) * s2 + cac_i2k * s1);
}
// smlt, gmlt (:182-199)
__device__ __forceinline__ double mp_smlt(double tc, double dqs, double qsrho, double psacw, double psacr, const double* c,
                                          double rho, double rhofac) {
  return (c[0] * tc / rho - c[1] * dqs) * (c[2] * sqrt(qsrho) + c[3] * pow(qsrho, 0.65625) * sqrt(rhofac)) +
         c[4] * tc * (psacw + psacr);
}
__device__ __forceinline__ double mp_gmlt(double tc, double dqs, double qgrho, double pgacw, double pgacr, const double* c,
                                          double rho) {
  return (c[0] * tc / rho - c[1] * dqs) * (c[2] * sqrt(qgrho) + c[3] * pow(qgrho, 0.6875) / pow(rho, 0.25)) +
         c[4] * tc * (pgacw + pgacr);
}

// revap_racc (:202-291)
__device__ __forceinline__ void mp_revap_racc(const MpCfg& c, double dt, double h_var, double den, double denfac, MpPt& P) {
  if (P.tz > c.t_wfr && P.qr > mp::QRMIN) {
    const double lhl = c.lv00 + c.d0_vap * P.tz;
    double q_liq = P.ql + P.qr;
    const double q_sol = P.qi + P.qs + P.qg;
    double cvm = mp_cvm(c, P.qv, q_liq, q_sol);
    const double lcpk = lhl / cvm;
    const double tin = P.tz - lcpk * P.ql;
    const double qpz = P.qv + P.ql;
    double dqsdt;
    const double qsat = mp_wqs2(tin, den, dqsdt);
    double dqh = mp_max(P.ql, h_var * mp_max(qpz, mp::QCMIN));
    dqh = mp_min(dqh, 0.2 * qpz);
    const double dqv = qsat - P.qv;
    const double q_minus = qpz - dqh;
    const double q_plus = qpz + dqh;
    if (dqv > mp::QVMIN && qsat > q_minus) {
      double dq;
      if (qsat > q_plus)
        dq = qsat - qpz;
      else
        dq = 0.25 * ((q_minus - qsat) * (q_minus - qsat)) / dqh;
      const double qden = P.qr * den;
      const double t2 = tin * tin;
      double evap = c.crevp[0] * t2 * dq * (c.crevp[1] * sqrt(qden) + c.crevp[2] * exp(0.725 * log(qden))) /
                    (c.crevp[3] * t2 + c.crevp[4] * qsat * den);
      evap = mp_min(P.qr, mp_min(dt * evap, dqv / (1.0 + lcpk * dqsdt)));
      P.qr = P.qr - evap;
      P.qv = P.qv + evap;
      q_liq = q_liq - evap;
      cvm = mp_cvm(c, P.qv, q_liq, q_sol);
      P.tz = P.tz - evap * lhl / cvm;
      if (evap > 0.0) MP_COV(rain_evaporation);
    }
    if (P.qr > mp::QRMIN && P.ql > 1.0e-6 && qsat < q_minus) {
      MP_COV(rain_accretion);
      double sink = dt * denfac * c.cracw * exp(0.95 * log(P.qr * den));
      sink = sink / (1.0 + sink) * P.ql;
      P.ql = P.ql - sink;
      P.qr = P.qr + sink;
    }
  }
}

// fall_speed (:294-379), const_vi / const_vs / const_vg off
__device__ __forceinline__ void mp_fall_speed(const MpCfg& c, const MpPt& P, double den, double& vtg, double& vti, double& vts) {
  const double rhof = sqrt(mp_min(10.0, mp::SFCRHO / den));
  const double vi0 = 0.01 * c.vi_fac;
  if (P.qi < mp::THI) {
    vti = mp::VF_MIN;
  } else {
    const double tc = P.tz - c.tice;
    vti = (3.0 + log(P.qi * den) / c.log_10) * (tc * (mp::AA * tc + mp::BB) + mp::CC) + mp::DD_FS * tc + mp::EE;
    vti = vi0 * exp(c.log_10 * vti) * 0.8;
    vti = mp_min(c.vi_max, mp_max(mp::VF_MIN, vti));
  }
  if (P.qs < mp::THS) {
    vts = mp::VF_MIN;
  } else {
    vts = c.vs_fac * mp::VCONS * rhof * exp(0.0625 * log(P.qs * den / mp::NORMS));
    vts = mp_min(c.vs_max, mp_max(mp::VF_MIN, vts));
  }
  if (P.qg < mp::THG) {
    vtg = mp::VF_MIN;
  } else {
    vtg = c.vg_fac * mp::VCONG * rhof * sqrt(sqrt(sqrt(P.qg * den / mp::NORMG)));
    vtg = mp_min(c.vg_max, mp_max(mp::VF_MIN, vtg));
  }
}

// compute_rain_fspeed (:382-416), const_vr off
__device__ __forceinline__ double mp_rain_fspeed(const MpCfg& c, bool fall, double qr, double den) {
  if (!fall) return mp::VF_MIN;
  const double qden = qr * den;
  if (qr < mp::THR) return mp::VR_MIN;
  const double v = c.vr_fac * mp::VCONR * sqrt(mp_min(10.0, mp::SFCRHO / den)) * exp(0.2 * log(qden / mp::NORMR));
  return mp_min(c.vr_max, mp_max(mp::VR_MIN, v));
}

// the implicit fall of one species, level by level (warm_rain :510-592, sedimentation :967-1061 and its two repeats): what a
// level takes over from the level above
struct MpFall {
  double qm, dd, m1, vt;
};
// q: the species' mixing ratio at this level (updated); dm: the level's mass before the fall (sedi_w); returns the level's m1
__device__ __forceinline__ double mp_fall_level(MpFall& F, bool top, double dt, double vt, double dz, double dp1, double dm,
                                                double& q, double& w) {
  const double dd = dt * vt;
  const double qmass = q * dp1;
  const double qm = top ? qmass / (dz + dd) : (qmass + F.dd * F.qm) / (dz + dd);
  const double qmd = qm * dz;
  const double m1 = top ? qmass - qmd : F.m1 + qmass - qmd;
  q = qmd / dp1;
  if (top)
    w = (dm * w + m1 * vt) / (dm - m1);
  else
    w = (dm * w - F.m1 * F.vt + m1 * vt) / (dm + F.m1 - m1);
  F.qm = qm;
  F.dd = dd;
  F.m1 = m1;
  F.vt = vt;
  return m1;
}
__device__ __forceinline__ double mp_mass(double dp1, const MpPt& P) {
  return dp1 * (1.0 + P.qv + P.ql + P.qr + P.qi + P.qs + P.qg);
}

// the slope limiter of z_slope_liq / z_slope_ice (:682-717, :1596-1631): qa, q, qb the levels k - 1, k, k + 1
__device__ __forceinline__ double mp_slope(bool edge, double qa, double q, double qb) {
  if (edge) return 0.0;
  const double dq = 0.5 * (q - qa);
  const double dqb = 0.5 * (qb - q);
  double dl = 0.5 * mp_min(fabs(dq + dqb), 0.5 * q);
  if (dq * dqb <= 0.0) {
    if (dq > 0.0)
      dl = mp_min(dl, mp_min(dq, -dqb));
    else
      dl = 0.0;
  }
  return dl;
}

// autoconv_subgrid_var (:449-482), use_ccn
__device__ __forceinline__ void mp_autoconv(const MpCfg& c, double ccn, double c_praut, double den, double dl, double land,
                                            MpPt& P) {
  const double qc0 = c.fac_rc * ccn;
  if (P.tz > c.t_wfr + mp::DT_FR) {
    dl = mp_min(mp_max(1.0e-6, dl), 0.5 * P.ql);
    const double qc = qc0;
    const double dq = 0.5 * (P.ql + dl - qc);
    if (dq > 0.0) {
      const double sink = mp_min(1.0, dq / dl) * c.dt_rain * c_praut * den * exp(c.so3 * log(P.ql));
      P.ql = P.ql - sink;
      P.qr = P.qr + sink;
      if (land > 0.5)
        MP_COV(autoconv_land);
      else
        MP_COV(autoconv_ocean);
    }
  }
}

// subgrid_z_proc (:485-941), do_qa and fast_sat_adj on
__device__ __forceinline__ void mp_subgrid_z_proc(const MpCfg& c, double rh_adj, double rh_rain, double den, double denfac,
                                                  double p1, MpPt& P) {
  double lhl = c.lv00 + c.d0_vap * P.tz;
  double lhi = phys::LI00 + phys::DC_ICE * P.tz;
  double q_liq = P.ql + P.qr;
  double q_sol = P.qi + P.qs + P.qg;
  double cvm = mp_cvm(c, P.qv, q_liq, q_sol);
  double lcpk = lhl / cvm;
  double icpk = lhi / cvm;
  double tcpk = lcpk + icpk;
  double tcp3 = lcpk + icpk * mp_min(1.0, mp_dim(c.tice, P.tz) / (c.tice - c.t_wfr));
  if (!(p1 >= mp::P_MIN)) return;
  if (P.tz < phys::T_MIN) {
    const double sink = mp_dim(1.0e-7, P.qv);
    P.qv = P.qv - sink;
    P.qi = P.qi + sink;
    q_sol = q_sol + sink;
    cvm = mp_cvm(c, P.qv, q_liq, q_sol);
    P.tz = P.tz + sink * (lhl + lhi) / cvm;
    return;
  }
  lhl = c.lv00 + c.d0_vap * P.tz;
  lhi = phys::LI00 + phys::DC_ICE * P.tz;
  lcpk = lhl / cvm;
  icpk = lhi / cvm;
  tcpk = lcpk + icpk;
  tcp3 = lcpk + icpk * mp_min(1.0, mp_dim(c.tice, P.tz) / (c.tice - c.t_wfr));
  // instant evaporation / sublimation of all clouds if rh < rh_adj
  const double qpz = P.qv + P.ql + P.qi;
  const double tin = P.tz - (lhl * (P.ql + P.qi) + lhi * P.qi) /
                                (c.c_air + qpz * c.c_vap + P.qr * phys::C_LIQ + (P.qs + P.qg) * phys::C_ICE);
  if (tin > c.t_sub + 6.0) {
    const double rh = qpz / mp_iqs1(tin, den);
    if (rh < rh_adj) {
      if (P.ql > 0.0) MP_COV(instant_evaporation);
      P.tz = tin;
      P.qv = qpz;
      P.ql = 0.0;
      P.qi = 0.0;
      return;
    }
  }
  // cloud water <--> vapor adjustment
  double dwsdt;
  const double qsw = mp_wqs2(P.tz, den, dwsdt);
  const double dq0 = qsw - P.qv;
  double evap;
  if (dq0 > 0.0) {
    const double factor = mp_min(1.0, c.fac_l2v * (10.0 * dq0 / qsw));
    evap = mp_min(P.ql, factor * dq0 / (1.0 + tcp3 * dwsdt));
  } else {
    evap = dq0 / (1.0 + tcp3 * dwsdt);
    if (evap < 0.0) MP_COV(condensation);
  }
  P.qv = P.qv + evap;
  P.ql = P.ql - evap;
  q_liq = q_liq - evap;
  cvm = mp_cvm(c, P.qv, q_liq, q_sol);
  P.tz = P.tz - evap * lhl / cvm;
  lhi = phys::LI00 + phys::DC_ICE * P.tz;
  icpk = lhi / cvm;
  // complete freezing below t_wfr
  const double dtmp = c.t_wfr - P.tz;
  if (dtmp > 0.0 && P.ql > mp::QCMIN) {
    const double sink = mp_min(P.ql, mp_min(P.ql * dtmp * 0.125, dtmp / icpk));
    P.ql = P.ql - sink;
    P.qi = P.qi + sink;
    q_liq = q_liq - sink;
    q_sol = q_sol + sink;
    cvm = mp_cvm(c, P.qv, q_liq, q_sol);
    P.tz = P.tz + sink * lhi / cvm;
  }
  lhi = phys::LI00 + phys::DC_ICE * P.tz;
  icpk = lhi / cvm;
  const double dt_pisub = 0.5 * c.dts;  // fast_sat_adj: no Bigg mechanism here
  lhl = c.lv00 + c.d0_vap * P.tz;
  lhi = phys::LI00 + phys::DC_ICE * P.tz;
  lcpk = lhl / cvm;
  icpk = lhi / cvm;
  tcpk = lcpk + icpk;
  // sublimation / deposition of ice
  if (P.tz < c.tice) {
    double dqsdt;
    const double qsi = mp_iqs2(P.tz, den, dqsdt);
    const double dq = P.qv - qsi;
    double sink = dq / (1.0 + tcpk * dqsdt);
    double pidep;
    if (P.qi > mp::QRMIN)
      pidep = dt_pisub * dq * 349138.78 * exp(0.875 * log(P.qi * den)) /
              (qsi * den * phys::LAT2 / (0.0243 * phys::RVGAS * (P.tz * P.tz)) + 4.42478e4);
    else
      pidep = 0.0;
    if (dq > 0.0) {
      const double tmp = c.tice - P.tz;
      const double qi_crt = c.qi_gen * mp_min(c.qi_lim, 0.1 * tmp) / den;
      sink = mp_min(sink, mp_min(mp_max(qi_crt - P.qi, pidep), tmp / tcpk));
    } else {
      pidep = pidep * mp_min(1.0, mp_dim(P.tz, c.t_sub) * 0.2);
      sink = mp_max(pidep, mp_max(sink, -P.qi));
    }
    P.qv = P.qv - sink;
    P.qi = P.qi + sink;
    q_sol = q_sol + sink;
    cvm = mp_cvm(c, P.qv, q_liq, q_sol);
    P.tz = P.tz + sink * (lhl + lhi) / cvm;
    if (sink > 0.0) MP_COV(ice_deposition);
    if (sink < 0.0) MP_COV(ice_sublimation);
  }
  lhl = c.lv00 + c.d0_vap * P.tz;
  lhi = phys::LI00 + phys::DC_ICE * P.tz;
  lcpk = lhl / cvm;
  icpk = lhi / cvm;
  tcpk = lcpk + icpk;
  // sublimation / deposition of snow
  if (P.qs > mp::QRMIN) {
    double dqsdt;
    const double qsi = mp_iqs2(P.tz, den, dqsdt);
    const double qden = P.qs * den;
    const double tmp = exp(0.65625 * log(qden));
    const double tsq = P.tz * P.tz;
    const double dq = (qsi - P.qv) / (1.0 + tcpk * dqsdt);
    double pssub = c.cssub[0] * tsq * (c.cssub[1] * sqrt(qden) + c.cssub[2] * tmp * sqrt(denfac)) /
                   (c.cssub[3] * tsq + c.cssub[4] * qsi * den);
    pssub = (qsi - P.qv) * c.dts * pssub;
    if (pssub > 0.0) {
      pssub = mp_min(pssub * mp_min(1.0, mp_dim(P.tz, c.t_sub) * 0.2), P.qs);
    } else {
      if (P.tz > c.tice)
        pssub = 0.0;
      else
        pssub = mp_max(pssub, mp_max(dq, (P.tz - c.tice) / tcpk));
    }
    if (pssub > 0.0) MP_COV(snow_sublimation);
    P.qs = P.qs - pssub;
    P.qv = P.qv + pssub;
    q_sol = q_sol - pssub;
    cvm = mp_cvm(c, P.qv, q_liq, q_sol);
    P.tz = P.tz - pssub * (lhl + lhi) / cvm;
  }
  lhl = c.lv00 + c.d0_vap * P.tz;
  lhi = phys::LI00 + phys::DC_ICE * P.tz;
  lcpk = lhl / cvm;
  icpk = lhi / cvm;
  tcpk = lcpk + icpk;
  // graupel sublimation / deposition
  if (P.qg > mp::QRMIN) {
    double dqsdt;
    const double qsi = mp_iqs2(P.tz, den, dqsdt);
    const double dq = (P.qv - qsi) / (1.0 + tcpk * dqsdt);
    double pgsub = (P.qv / qsi - 1.0) * P.qg;
    if (pgsub > 0.0) {
      if (P.tz > c.tice)
        pgsub = 0.0;
      else
        pgsub = mp_min(mp_min(c.fac_v2g * pgsub, 0.2 * dq), mp_min(P.ql + P.qr, (c.tice - P.tz) / tcpk));
    } else {
      pgsub = mp_max(c.fac_g2v * pgsub, dq) * mp_min(1.0, mp_dim(P.tz, c.t_sub) * 0.1);
    }
    if (pgsub > 0.0) MP_COV(graupel_deposition);
    if (pgsub < 0.0) MP_COV(graupel_sublimation);
    P.qg = P.qg + pgsub;
    P.qv = P.qv - pgsub;
    q_sol = q_sol + pgsub;
    cvm = mp_cvm(c, P.qv, q_liq, q_sol);
    P.tz = P.tz + pgsub * (lhl + lhi) / cvm;
  }
  lhl = c.lv00 + c.d0_vap * P.tz;
  lcpk = lhl / cvm;
  // minimum evaporation of rain in dry environmental air
  if (P.qr > mp::QCMIN) {
    double dqsdt;
    const double qsw2 = mp_wqs2(P.tz, den, dqsdt);
    const double sink = mp_min(P.qr, mp_dim(rh_rain * qsw2, P.qv) / (1.0 + lcpk * dqsdt));
    P.qv = P.qv + sink;
    P.qr = P.qr - sink;
    q_liq = q_liq - sink;
    cvm = mp_cvm(c, P.qv, q_liq, q_sol);
    P.tz = P.tz - sink * lhl / cvm;
  }
}

// the head of icloud (:1542-1593): pimlt / pihom; q_liq, q_sol, cvm go on to icloud_main
struct MpIce {
  MpPt P;
  double q_liq, q_sol, cvm;
};
__device__ __forceinline__ MpIce mp_icloud_head(const MpCfg& c, const MpPt& in, double den) {
  MpIce I;
  I.P = in;
  MpPt& P = I.P;
  const double lhi = phys::LI00 + phys::DC_ICE * P.tz;
  I.q_liq = P.ql + P.qr;
  I.q_sol = P.qi + P.qs + P.qg;
  I.cvm = mp_cvm(c, P.qv, I.q_liq, I.q_sol);
  const double icpk = lhi / I.cvm;
  if (P.tz > c.tice && P.qi > mp::QCMIN) {
    MP_COV(icloud_ice_melt);
    const double melt = mp_min(P.qi, c.fac_imlt * (P.tz - c.tice) / icpk);
    const double tmp = mp_min(melt, mp_dim(c.ql_mlt, P.ql));
    P.ql = P.ql + tmp;
    P.qr = P.qr + melt - tmp;
    P.qi = P.qi - melt;
    I.q_liq = I.q_liq + melt;
    I.q_sol = I.q_sol - melt;
    I.cvm = mp_cvm(c, P.qv, I.q_liq, I.q_sol);
    P.tz = P.tz - melt * lhi / I.cvm;
  } else if (P.tz < c.t_wfr && P.ql > mp::QCMIN) {
    MP_COV(icloud_water_freeze);
    const double dtmp = c.t_wfr - P.tz;
    const double factor = mp_min(1.0, dtmp / mp::DT_FR);
    const double sink = mp_min(P.ql * factor, dtmp / icpk);
    const double qi_crt = c.qi_gen * mp_min(c.qi_lim, 0.1 * (c.tice - P.tz)) / den;
    const double tmp = mp_min(sink, mp_dim(qi_crt, P.qi));
    P.ql = P.ql - sink;
    P.qs = P.qs + sink - tmp;
    P.qi = P.qi + tmp;
    I.q_liq = I.q_liq - sink;
    I.q_sol = I.q_sol + sink;
    I.cvm = mp_cvm(c, P.qv, I.q_liq, I.q_sol);
    P.tz = P.tz + sink * lhi / I.cvm;
  }
  return I;
}

// icloud_main (:944-1384), const_vi off
__device__ __forceinline__ void mp_icloud_main(const MpCfg& c, double rh_adj, double rh_rain, double den, double denfac,
                                               double vtg, double vtr, double vts, double p1, double di, MpIce& I) {
  MpPt& P = I.P;
  double q_liq = I.q_liq, q_sol = I.q_sol, cvm = I.cvm;
  double lhi = phys::LI00 + phys::DC_ICE * P.tz;
  double icpk = lhi / cvm;
  if (p1 >= mp::P_MIN) {
    double pgacr = 0.0, pgacw = 0.0;
    double tc = P.tz - c.tice;
    if (tc >= 0.0) {
      // melting of snow
      const double dqs0 = c.ces0 / p1 - P.qv;
      if (P.qs > mp::QCMIN) {
        double psacw, psacr, pracs;
        if (P.ql > mp::QRMIN) {
          const double factor = denfac * c.csacw * exp(0.8125 * log(P.qs * den));
          psacw = factor / (1.0 + c.dts * factor) * P.ql;
        } else {
          psacw = 0.0;
        }
        if (P.qr > mp::QRMIN) {
          psacr = mp_min(mp_acr3d(vts, vtr, P.qr, P.qs, c.csacr, c.acco[0][1], c.acco[1][1], c.acco[2][1], den), P.qr * c.rdts);
          pracs = mp_acr3d(vtr, vts, P.qs, P.qr, c.cracs, c.acco[0][0], c.acco[1][0], c.acco[2][0], den);
        } else {
          psacr = 0.0;
          pracs = 0.0;
        }
        const double psmlt = mp_max(0.0, mp_smlt(tc, dqs0, P.qs * den, psacw, psacr, c.csmlt, den, denfac));
        if (psacw != 0.0) MP_COV(psacw);
        if (pracs != 0.0) MP_COV(pracs);
        if (psmlt != 0.0) MP_COV(psmlt);
        const double sink = mp_min(P.qs, mp_min(c.dts * (psmlt + pracs), tc / icpk));
        P.qs = P.qs - sink;
        const double tmp = mp_min(sink, mp_dim(c.qs_mlt, P.ql));
        P.ql = P.ql + tmp;
        P.qr = P.qr + sink - tmp;
        q_liq = q_liq + sink;
        q_sol = q_sol - sink;
        cvm = mp_cvm(c, P.qv, q_liq, q_sol);
        P.tz = P.tz - sink * lhi / cvm;
        tc = P.tz - c.tice;
      }
      lhi = phys::LI00 + phys::DC_ICE * P.tz;
      icpk = lhi / cvm;
      // melting of graupel
      if (P.qg > mp::QCMIN && tc > 0.0) {
        if (P.qr > mp::QRMIN)
          pgacr = mp_min(mp_acr3d(vtg, vtr, P.qr, P.qg, c.cgacr, c.acco[0][2], c.acco[1][2], c.acco[2][2], den), c.rdts * P.qr);
        const double qden = P.qg * den;
        if (P.ql > mp::QRMIN) {
          const double factor = c.cgacw * qden / sqrt(den * sqrt(sqrt(qden)));
          pgacw = factor / (1.0 + c.dts * factor) * P.ql;
        }
        double pgmlt = c.dts * mp_gmlt(tc, dqs0, qden, pgacw, pgacr, c.cgmlt, den);
        pgmlt = mp_min(mp_max(0.0, pgmlt), mp_min(P.qg, tc / icpk));
        if (pgmlt != 0.0) MP_COV(pgmlt);
        P.qg = P.qg - pgmlt;
        P.qr = P.qr + pgmlt;
        q_liq = q_liq + pgmlt;
        q_sol = q_sol - pgmlt;
        cvm = mp_cvm(c, P.qv, q_liq, q_sol);
        P.tz = P.tz - pgmlt * lhi / cvm;
      }
    } else {
      // cloud ice: psaci, psaut, pgaci
      if (P.qi > 3.0e-7) {
        double psaci, psaut;
        if (P.qs > 1.0e-7) {
          const double factor = c.dts * denfac * c.csaci * exp(0.05 * tc + 0.8125 * log(P.qs * den));
          psaci = factor / (1.0 + factor) * P.qi;
        } else {
          psaci = 0.0;
        }
        const double qim = c.qi0_crt / den;
        const double tmp = c.fac_i2s * exp(0.025 * tc);
        di = mp_max(di, mp::QRMIN);
        const double q_plus = P.qi + di;
        if (q_plus > (qim + mp::QRMIN)) {
          double dq;
          if (qim > (P.qi - di))
            dq = (0.25 * ((q_plus - qim) * (q_plus - qim))) / di;
          else
            dq = P.qi - qim;
          psaut = tmp * dq;
        } else {
          psaut = 0.0;
        }
        if (psaci != 0.0) MP_COV(psaci);
        const double sink = mp_min(0.75 * P.qi, psaci + psaut);
        P.qi = P.qi - sink;
        P.qs = P.qs + sink;
        if (P.qg > 1.0e-6) {
          const double factor = c.dts * c.cgaci * sqrt(den) * P.qg;
          const double pgaci = factor / (1.0 + factor) * P.qi;
          P.qi = P.qi - pgaci;
          P.qg = P.qg + pgaci;
        }
      }
      // cold rain: rain to snow and graupel
      tc = P.tz - c.tice;
      if (P.qr > 1e-7 && tc < 0.0) {
        double psacr;
        if (P.qs > 1.0e-7)
          psacr = c.dts * mp_acr3d(vts, vtr, P.qr, P.qs, c.csacr, c.acco[0][1], c.acco[1][1], c.acco[2][1], den);
        else
          psacr = 0.0;
        double pgfr = c.dts * c.cgfr[0] / den * (exp(-c.cgfr[1] * tc) - 1.0) * exp(1.75 * log(P.qr * den));
        double sink = psacr + pgfr;
        const double factor = mp_min(sink, mp_min(P.qr, -tc / icpk)) / mp_max(sink, mp::QRMIN);
        psacr = factor * psacr;
        pgfr = factor * pgfr;
        if (pgfr != 0.0) MP_COV(pgfr);
        sink = psacr + pgfr;
        P.qr = P.qr - sink;
        P.qs = P.qs + psacr;
        P.qg = P.qg + pgfr;
        q_liq = q_liq - sink;
        q_sol = q_sol + sink;
        cvm = mp_cvm(c, P.qv, q_liq, q_sol);
        P.tz = P.tz + sink * lhi / cvm;
      }
      lhi = phys::LI00 + phys::DC_ICE * P.tz;
      icpk = lhi / cvm;
      // graupel production: accretion and autoconversion of snow
      if (P.qs > 1.0e-7) {
        double sink;
        if (P.qg > mp::QRMIN)
          sink = c.dts * mp_acr3d(vtg, vts, P.qs, P.qg, c.cgacs, c.acco[0][3], c.acco[1][3], c.acco[2][3], den);
        else
          sink = 0.0;
        if (sink != 0.0) MP_COV(pgacs);
        const double qsm = c.qs0_crt / den;
        if (P.qs > qsm) {
          const double factor = c.dts * 1.0e-3 * exp(0.09 * (P.tz - c.tice));
          sink = sink + factor / (1.0 + factor) * (P.qs - qsm);
        }
        sink = mp_min(P.qs, sink);
        P.qs = P.qs - sink;
        P.qg = P.qg + sink;
      }
      if (P.qg > 1.0e-7 && P.tz < c.tice0) {
        if (P.ql > 1.0e-6) {
          const double qden = P.qg * den;
          const double factor = c.dts * c.cgacw * qden / sqrt(den * sqrt(sqrt(qden)));
          pgacw = factor / (1.0 + factor) * P.ql;
        } else {
          pgacw = 0.0;
        }
        if (P.qr > 1.0e-6)
          pgacr = mp_min(c.dts * mp_acr3d(vtg, vtr, P.qr, P.qg, c.cgacr, c.acco[0][2], c.acco[1][2], c.acco[2][2], den), P.qr);
        else
          pgacr = 0.0;
        double sink = pgacr + pgacw;
        const double factor = mp_min(sink, mp_dim(c.tice, P.tz) / icpk) / mp_max(sink, mp::QRMIN);
        pgacr = factor * pgacr;
        pgacw = factor * pgacw;
        sink = pgacr + pgacw;
        P.qg = P.qg + sink;
        P.qr = P.qr - pgacr;
        P.ql = P.ql - pgacw;
        q_liq = q_liq - sink;
        q_sol = q_sol + sink;
        cvm = mp_cvm(c, P.qv, q_liq, q_sol);
        P.tz = P.tz + sink * lhi / cvm;
      }
    }
  }
  mp_subgrid_z_proc(c, rh_adj, rh_rain, den, denfac, p1, P);
}

// the per-column scalars every sweep may need
struct MpColumn {
  double h_var, rh_adj, rh_rain, ccn, c_praut, land;
  double rain, snow, ice, graupel;
};

// warm_rain's autoconversion with subgrid variability (:682-756): the slope reads cloud water as this sweep finds it
__device__ __forceinline__ void mp_autoconv_sweep(const MpCfg& c, const MpCol& W, int nk, const MpColumn& S) {
  double ql_above = 0.0;
  for (int k = 0; k < nk; ++k) {
    MpPt P = mp_load(W, k);
    const bool edge = k == 0 || k == nk - 1;
    const double ql_below = edge ? 0.0 : W(MP_QL, k + 1);
    double dl = mp_slope(edge, ql_above, P.ql, ql_below);
    dl = mp_max(dl, mp_max(mp::QVMIN, S.h_var * P.ql));
    ql_above = P.ql;
    mp_autoconv(c, S.ccn, S.c_praut, W(MP_DEN, k), dl, S.land, P);
    W(MP_QL, k) = P.ql;
    W(MP_QR, k) = P.qr;
  }
}

// the falls of one half of a sub-step.  first: warm_rain(is_first = True); otherwise the three falls of sedimentation followed,
// at each level, by warm_rain(is_first = False)
__device__ __forceinline__ void mp_fall_sweep(const MpCfg& c, const MpCol& W, real* wfld, long sk, int nk, bool first, bool fall_r,
                                              bool fall_i, bool fall_s, bool fall_g, MpColumn& S) {
  MpFall Fr{0, 0, 0, 0}, Fi{0, 0, 0, 0}, Fs{0, 0, 0, 0}, Fg{0, 0, 0, 0};
  const double dt5 = 0.5 * c.dt_rain;
  double r1 = 0.0, i1 = 0.0, s1 = 0.0, g1 = 0.0;
  fall_i = fall_i && c.vi_fac >= 1.0e-5;
  if (fall_r)
    MP_COV(rain_falls);
  else
    MP_COV(rain_no_fall);
  if (!first) {
    if (fall_i)
      MP_COV(ice_falls);
    else
      MP_COV(ice_no_fall);
    if (fall_s)
      MP_COV(snow_falls);
    else
      MP_COV(snow_no_fall);
    if (fall_g)
      MP_COV(graupel_falls);
    else
      MP_COV(graupel_no_fall);
  }
  for (int k = 0; k < nk; ++k) {
    MpPt P = mp_load(W, k);
    const double dp1 = W(MP_DP1, k), dz = W(MP_DZ, k), den = W(MP_DEN, k), denfac = W(MP_DENFAC, k);
    double w = (double)wfld[k * sk];
    const bool top = k == 0;
    double m1_sol = 0.0;
    if (!first) {
      if (fall_i) {
        const double dm = mp_mass(dp1, P);
        i1 = mp_fall_level(Fi, top, c.dts, W(MP_VTI, k), dz, dp1, dm, P.qi, w);
        m1_sol = i1;
      }
      if (fall_s) {
        const double dm = mp_mass(dp1, P);
        s1 = mp_fall_level(Fs, top, c.dts, W(MP_VTS, k), dz, dp1, dm, P.qs, w);
        m1_sol = m1_sol + s1;
      }
      if (fall_g) {
        const double dm = mp_mass(dp1, P);
        g1 = mp_fall_level(Fg, top, c.dts, W(MP_VTG, k), dz, dp1, dm, P.qg, w);
        m1_sol = m1_sol + g1;
      }
    }
    const double vtr = mp_rain_fspeed(c, fall_r, P.qr, den);
    W(MP_VTR, k) = vtr;
    double m1_rain = 0.0;
    if (fall_r) {
      mp_revap_racc(c, dt5, S.h_var, den, denfac, P);
      const double dm = mp_mass(dp1, P);
      m1_rain = r1 = mp_fall_level(Fr, top, c.dt_rain, vtr, dz, dp1, dm, P.qr, w);
      mp_revap_racc(c, dt5, S.h_var, den, denfac, P);
    }
    mp_store(W, k, P);
    wfld[k * sk] = (real)w;
    if (first)
      W(MP_M1, k) = W(MP_M1, k) + m1_rain;
    else
      W(MP_M1, k) = W(MP_M1, k) + m1_rain + m1_sol;
  }
  // (the value at the bottom level is what reached the ground)
  S.rain = S.rain + r1;
  if (!first) {
    S.snow = S.snow + s1;
    S.graupel = S.graupel + g1;
    S.ice = S.ice + i1;
  }
}

__global__ void __launch_bounds__(64) k_microphysics(Geo g, MpFields f, MpCfg c, double* ws) {
  const int i = g.is + blockIdx.x * 64 + threadIdx.x;
  const int j = g.js + blockIdx.y;
  if (i > g.ie || j > g.je) return;
  const long c2 = IDX2(g, i, j);
  const int nk = g.nk;
  const long sk = g.sk;
  MpCol W;
  W.nc = (long)g.n * g.n;
  W.na = W.nc * nk;
  W.p = ws + (long)(j - g.js) * g.n + (i - g.is);

  MpColumn S;
  S.rain = S.snow = S.ice = S.graupel = 0.0;
  const double land = (double)f.land[c2];
  S.land = land;
  {  // horizontal subgrid variability (:197-208)
    const double s_leng = sqrt(sqrt((double)f.area[c2] * 1.0e-10));
    const double t_land = c.dw_land * s_leng;
    const double t_ocean = c.dw_ocean * s_leng;
    double h_var = t_land * land + t_ocean * (1.0 - land);
    h_var = mp_min(0.2, mp_max(0.01, h_var));
    S.h_var = h_var;
    S.rh_adj = 1.0 - h_var - c.rh_inc;
    S.rh_rain = mp_max(0.35, S.rh_adj - c.rh_inr);
  }

  // ---- fields_init (:100-303) ----
  {
    double qv_above = 0.0, dp1_above = 0.0;  // vapour of the level above before it is set to zero
    for (int k = 0; k < nk; ++k) {
      const long q = c2 + k * sk;
      MpPt P{(double)f.qv[q], (double)f.ql[q], (double)f.qr[q], (double)f.qi[q], (double)f.qs[q], (double)f.qg[q], (double)f.pt[q]};
      const double dp0 = (double)f.delp[q];
      const double dp1 = dp0 * (1.0 - P.qv);
      const double omq = dp0 / dp1;
      P.qv = P.qv * omq;
      P.ql = P.ql * omq;
      P.qr = P.qr * omq;
      P.qi = P.qi * omq;
      P.qs = P.qs * omq;
      P.qg = P.qg * omq;
      if (k == nk - 1) {  // ccn = ccn_surface * (den / den_surface), the bottom value for the whole column (:178-195)
        const double den0 = -dp1 / (phys::GRAV * (double)f.dz[q]);
        const double p1 = den0 * phys::RDGAS * P.tz;
        double ccn = (c.ccn_l * land + c.ccn_o * (1.0 - land)) * 1.0e6;
        ccn = ccn * phys::RDGAS * P.tz / p1;
        S.ccn = ccn;
        S.c_praut = c.cpaut * pow(ccn * mp::RHOR, -1.0 / 3.0);
      }
      // fix_negative (:211-257)
      const double cvm = mp_cvm(c, P.qv, P.qr + P.ql, P.qi + P.qs + P.qg);
      const double lcpk = (c.lv00 + c.d0_vap * P.tz) / cvm;
      const double icpk = (phys::LI00 + phys::DC_ICE * P.tz) / cvm;
      if (P.qi < 0.0 || P.qs < 0.0 || P.qg < 0.0 || P.qr < 0.0 || P.ql < 0.0 || P.qv < 0.0) MP_COV(fix_negative);
      if (P.qi < 0.0) {
        P.qs = P.qs + P.qi;
        P.qi = 0.0;
      }
      if (P.qs < 0.0) {
        P.qg = P.qg + P.qs;
        P.qs = 0.0;
      }
      if (P.qg < 0.0) {
        P.qr = P.qr + P.qg;
        P.tz = P.tz - P.qg * icpk;
        P.qg = 0.0;
      }
      if (P.qr < 0.0) {
        P.ql = P.ql + P.qr;
        P.qr = 0.0;
      }
      if (P.ql < 0.0) {
        P.qv = P.qv + P.ql;
        P.tz = P.tz - P.ql * lcpk;
        P.ql = 0.0;
      }
      // vapour borrows from below (:259-268): level k takes up the deficit of level k - 1, which is then set to zero
      if (k > 0) {
        if (qv_above < 0.0) {
          P.qv = P.qv + qv_above * dp1_above / dp1;
          W(MP_QV, k - 1) = 0.0;
        }
      }
      qv_above = P.qv;
      dp1_above = dp1;
      mp_store(W, k, P);
      W(MP_DP1, k) = dp1;
      W(MP_M1, k) = 0.0;
    }
    if (nk >= 2) {  // the bottom layer borrows from the one above (:271-303)
      const double qa = W(MP_QV, nk - 2), qb = W(MP_QV, nk - 1);
      const double da = W(MP_DP1, nk - 2), db = W(MP_DP1, nk - 1);
      if (qb < 0.0 && qa > 0.0) {
        const double dq = mp_min(-qb * db, qa * da);
        W(MP_QV, nk - 2) = qa - dq / da;
        W(MP_QV, nk - 1) = qb + dq / db;
      }
    }
  }

  for (int n = 0; n < c.ntimes; ++n) {
    bool fall_r = false, fall_i = false, fall_s = false, fall_g = false;
    {  // ---- warm_rain, is_first (:359-372, :411-421, :498-508), p_nonhydro False ----
      double ze = c.zs;
      for (int k = nk - 1; k >= 0; --k) {
        const long q = c2 + k * sk;
        const double dz0 = (double)f.dz[q], t0 = (double)f.pt[q];
        const double den0 = -W(MP_DP1, k) / (phys::GRAV * dz0);
        const double dz1 = dz0 * W(MP_TZ, k) / t0;
        const double den = den0 * dz0 / dz1;
        W(MP_DEN, k) = den;
        W(MP_DENFAC, k) = sqrt(mp::SFCRHO / den);
        const double ze_k = ze - dz1;
        W(MP_DZ, k) = ze_k - ze;
        ze = ze_k;
        fall_r = fall_r || W(MP_QR, k) > mp::QRMIN;
      }
    }
    mp_fall_sweep(c, W, f.w + c2, sk, nk, true, fall_r, false, false, false, S);
    mp_autoconv_sweep(c, W, nk, S);
    {  // ---- sedimentation (:790-866): fall speeds, melting of cloud ice before the fall ----
      bool stop = false;
      fall_r = false;
      for (int k = 0; k < nk; ++k) {
        MpPt P = mp_load(W, k);
        double vtg, vti, vts;
        mp_fall_speed(c, P, W(MP_DEN, k), vtg, vti, vts);
        W(MP_VTG, k) = vtg;
        W(MP_VTI, k) = vti;
        W(MP_VTS, k) = vts;
        const double lhi = phys::LI00 + phys::DC_ICE * P.tz;
        double q_liq = P.ql + P.qr;
        double q_sol = P.qi + P.qs + P.qg;
        double cvm = mp_cvm(c, P.qv, q_liq, q_sol);
        const double icpk = lhi / cvm;
        stop = stop || P.tz > c.tice || k == nk - 1;
        if (stop) {
          const double tc = P.tz - c.tice;
          if (P.qi > mp::QCMIN && tc > 0.0) {
            MP_COV(sedi_ice_melt);
            const double sink = mp_min(P.qi, c.fac_imlt * tc / icpk);
            const double tmp = mp_min(sink, mp_dim(c.ql_mlt, P.ql));
            P.ql = P.ql + tmp;
            P.qr = P.qr + sink - tmp;
            P.qi = P.qi - sink;
            q_liq = q_liq + sink;
            q_sol = q_sol - sink;
            cvm = mp_cvm(c, P.qv, q_liq, q_sol);
            P.tz = P.tz - sink * lhi / cvm;
            mp_store(W, k, P);
          }
        }
        fall_r = fall_r || P.qr > mp::QRMIN;
        fall_i = fall_i || P.qi > mp::QRMIN;
        fall_s = fall_s || P.qs > mp::QRMIN;
        fall_g = fall_g || P.qg > mp::QRMIN;
      }
    }
    mp_fall_sweep(c, W, f.w + c2, sk, nk, false, fall_r, fall_i, fall_s, fall_g, S);
    mp_autoconv_sweep(c, W, nk, S);
    {  // ---- icloud (:1542-1716) ----
      MpIce cur = mp_icloud_head(c, mp_load(W, 0), W(MP_DEN, 0));
      MpIce nxt = cur;
      double qi_above = 0.0;
      for (int k = 0; k < nk; ++k) {
        if (k + 1 < nk) nxt = mp_icloud_head(c, mp_load(W, k + 1), W(MP_DEN, k + 1));
        const bool edge = k == 0 || k == nk - 1;
        double di = mp_slope(edge, qi_above, cur.P.qi, nxt.P.qi);
        di = mp_max(di, mp_max(mp::QVMIN, S.h_var * cur.P.qi));
        qi_above = cur.P.qi;
        const long q = c2 + k * sk;
        const double den0 = -W(MP_DP1, k) / (phys::GRAV * (double)f.dz[q]);
        const double p1 = den0 * phys::RDGAS * (double)f.pt[q];
        mp_icloud_main(c, S.rh_adj, S.rh_rain, W(MP_DEN, k), W(MP_DENFAC, k), W(MP_VTG, k), W(MP_VTR, k), W(MP_VTS, k), p1, di,
                       cur);
        mp_store(W, k, cur.P);
        cur = nxt;
      }
    }
  }

  // ---- fields_update (:1766-1827) ----
  {
    const double convt = 86400.0 * c.rdt * phys::RGRAV;
    const real rain = (real)(S.rain * convt), snow = (real)(S.snow * convt), ice = (real)(S.ice * convt),
               graupel = (real)(S.graupel * convt);
    double u1 = 0.0, v1 = 0.0, m1_above = 0.0;
    for (int k = 0; k < nk; ++k) {
      const long q = c2 + k * sk;
      const double dp0 = (double)f.delp[q];
      const double u0 = (double)f.ua[q], v0 = (double)f.va[q];
      if (k == 0) {
        u1 = u0;
        v1 = v0;
      } else {
        u1 = (dp0 * u0 + m1_above * u1) / (dp0 + m1_above);
        v1 = (dp0 * v0 + m1_above * v1) / (dp0 + m1_above);
        f.udt[q] = (real)((double)f.udt[q] + (u1 - u0) * c.rdt);
        f.vdt[q] = (real)((double)f.vdt[q] + (v1 - v0) * c.rdt);
      }
      m1_above = W(MP_M1, k);
      // the values fields_init kept: the dry mixing ratios before fix_negative
      const double qv_in = (double)f.qv[q];
      const double dp1 = W(MP_DP1, k);
      const double omq0 = dp0 / dp1;
      const MpPt P = mp_load(W, k);
      const double omq = dp1 / dp0;
      f.qv_dt[q] = (real)((double)f.qv_dt[q] + c.rdt * (P.qv - qv_in * omq0) * omq);
      f.ql_dt[q] = (real)((double)f.ql_dt[q] + c.rdt * (P.ql - (double)f.ql[q] * omq0) * omq);
      f.qr_dt[q] = (real)((double)f.qr_dt[q] + c.rdt * (P.qr - (double)f.qr[q] * omq0) * omq);
      f.qi_dt[q] = (real)((double)f.qi_dt[q] + c.rdt * (P.qi - (double)f.qi[q] * omq0) * omq);
      f.qs_dt[q] = (real)((double)f.qs_dt[q] + c.rdt * (P.qs - (double)f.qs[q] * omq0) * omq);
      f.qg_dt[q] = (real)((double)f.qg_dt[q] + c.rdt * (P.qg - (double)f.qg[q] * omq0) * omq);
      const double cvm = mp_cvm(c, P.qv, P.qr + P.ql, P.qi + P.qs + P.qg);
      f.pt_dt[q] = (real)((double)f.pt_dt[q] + c.rdt * (P.tz - (double)f.pt[q]) * cvm / phys::CP_AIR);
      f.qa_dt[q] = (real)0.0;  // do_qa
      f.rain[q] = rain;
      f.snow[q] = snow;
      f.ice[q] = ice;
      f.graupel[q] = graupel;
    }
  }
}

long microphysics_workspace_bytes(const Geo& g) {
  return ((long)MP_NW * g.n * g.n * g.nk + MP_COV_WORDS) * (long)sizeof(double);
}

int launch_microphysics(const Geo& g, void* workspace, const real* const* in, real* wmp, real* const* tend, real* const* precip,
                        const pace_microphysics_config_t& cfg, hipStream_t st) {
  MpFields f;
  f.pt = in[0];
  f.qv = in[1];
  f.ql = in[2];
  f.qr = in[3];
  f.qi = in[4];
  f.qs = in[5];
  f.qg = in[6];
  f.ua = in[7];
  f.va = in[8];
  f.delp = in[9];
  f.dz = in[10];
  f.land = in[11];
  f.area = in[12];
  f.w = wmp;
  f.qv_dt = tend[0];
  f.ql_dt = tend[1];
  f.qr_dt = tend[2];
  f.qi_dt = tend[3];
  f.qs_dt = tend[4];
  f.qg_dt = tend[5];
  f.qa_dt = tend[6];
  f.udt = tend[7];
  f.vdt = tend[8];
  f.pt_dt = tend[9];
  f.rain = precip[0];
  f.snow = precip[1];
  f.ice = precip[2];
  f.graupel = precip[3];
#if defined(PACE_MP_COVERAGE) && defined(PACE_EMU)
  mp_cov = (long long*)workspace + (long)MP_NW * g.n * g.n * g.nk;
#endif
  hipLaunchKernelGGL(k_microphysics, dim3((unsigned)((g.n + 63) / 64), (unsigned)g.n), dim3(64), 0, st, g, f, cfg,
                     (double*)workspace);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
