// Physical constants and the moist thermodynamics shared by the device code.
//
// The constants are the reference's util/pace/util/constants.py:36-97 (GFS_PHYS branch), under the names they have there and in
// pace_amd/util/constants.py.  Derived constants are the same expression, operand for operand, as on the Python side, so the
// folded double is the same; all are double in both the fp64 and the float32-storage build.  One definition per line in plain
// arithmetic: tests/test_capi_and_host.py evaluates them in order and compares with pace_amd/util/constants.py.
#pragma once
#include "common.h"

namespace phys {
constexpr double RADIUS = 6.3712e6;
constexpr double PI = 3.1415926535897931;
constexpr double GRAV = 9.80665;
constexpr double RGRAV = 1.0 / GRAV;
constexpr double RDGAS = 287.05;
constexpr double RVGAS = 461.50;
constexpr double CP_AIR = 1004.6;
constexpr double KAPPA = RDGAS / CP_AIR;
constexpr double DZ_MIN = 2.0;
constexpr double CV_AIR = CP_AIR - RDGAS;
constexpr double RDG = -RDGAS / GRAV;
constexpr double ZVIR = RVGAS / RDGAS - 1;
constexpr double CV_VAP = 3.0 * RVGAS;
constexpr double C_ICE = 1972.0;
constexpr double C_LIQ = 4.1855e3;
constexpr double HLV = 2.5e6;
constexpr double HLF = 3.3358e5;
constexpr double CP_VAP = 4.0 * RVGAS;
constexpr double TICE = 273.16;
constexpr double DC_ICE = C_LIQ - C_ICE;
constexpr double DC_VAP = CP_VAP - C_LIQ;
constexpr double D2ICE = DC_VAP + DC_ICE;
constexpr double LV0 = HLV - DC_VAP * TICE;
constexpr double LI00 = HLF - DC_ICE * TICE;
constexpr double LI2 = LV0 + LI00;
constexpr double E00 = 611.21;
constexpr double T_WFR = TICE - 40.0;
constexpr double TICE0 = TICE - 0.01;
constexpr double T_MIN = 178.0;
constexpr double T_SAT_MIN = TICE - 160.0;
constexpr double LAT2 = (HLV + HLF) * (HLV + HLF);
}  // namespace phys

// The six water species of nwat = 6, in the order of the C ABI's `water` arrays
template <class T>
struct Water6T {
  T *qvapor, *qliquid, *qrain, *qsnow, *qice, *qgraupel;
};
typedef Water6T<real> Water6;             // kernels that adjust the species
typedef Water6T<const real> Water6Const;  // kernels that only read them
template <class T>
static inline Water6T<T> water6(T* const* w) {
  return Water6T<T>{w[0], w[1], w[2], w[3], w[4], w[5]};
}

// moist_cvm (moist_cv.py:16-35; neg_adj3.py's cpm): the heat capacity of moist air at constant volume.  q_all = qv + the
// condensate, summed by the caller in its reference's order; ql / qs = the liquid / solid sums.
__device__ __forceinline__ double moist_cvm(double q_all, double qv, double ql, double qs) {
  return (1.0 - q_all) * phys::CV_AIR + qv * phys::CV_VAP + ql * phys::C_LIQ + qs * phys::C_ICE;
}
// set_cappa (moist_cv.py:38-46); virt = 1 + zvir * qv, the virtual-temperature term
__device__ __forceinline__ double moist_cappa(double cvm, double virt) {
  return phys::RDGAS / (phys::RDGAS + cvm / virt);
}
// compute_pkz_func (moist_cv.py:125-127)
__device__ __forceinline__ double moist_pkz(double cappa, double delp, double delz, double pt) {
  return exp(cappa * log(phys::RDG * delp / delz * pt));
}
