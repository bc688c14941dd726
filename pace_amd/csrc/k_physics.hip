// The Physics shell around the microphysics and the coupling of its result back to the dycore state:
// physics/pace/physics/stencils/physics.py:33-201, get_prs_fv3.py, get_phi_fv3.py and the dycore_only = False halves of
// stencils/pace/stencils/update_atmos_state.py:40-145.  Four streaming kernels, none with a scratch field:
//
//   k_copy_dycore_to_physics       copy_dycore_to_physics: sixteen fields, origin (3, 3, 0), domain (n + 1, n + 1, nk)
//   k_physics_prepare              atmos_phys_driver_statein, get_prs_fv3, get_phi_fv3 and (do_microphysics) prepare_microphysics:
//                                  one thread per column, one sweep down and one sweep up
//   k_physics_update_state         update_physics_state_with_tendencies: ten x + x_dt * dt
//   k_physics_tendencies_to_dycore prepare_tendencies_and_update_tracers
//
// Arithmetic is fp64 in the reference's order of operations with its divisions kept; float64 storage only (the C entry points
// refuse the float32 build).  None of the four contains a transcendental: the reference's prsik (log, exp) is scratch that is
// never read after the call and is not computed.
#include "common.h"
#include "kernels.h"
#include "thermo.h"

#define PHY_KC 4      // levels of a column sweep whose loads are issued together (cf. UPD_KC, k_updphys.hip)
#define PHY_KCHUNK 8  // levels a thread of the three pointwise kernels walks (cf. DWIND_KCHUNK)
// thread of a pointwise kernel -> column i, j of the compute domain widened by D at its high end, levels k0 .. k1 - 1
#define PHY_POINT(g, D)                                      \
  const int i = (g).is + blockIdx.x * 64 + threadIdx.x;      \
  const int j = (g).js + blockIdx.y;                         \
  if (i > (g).ie + (D) || j > (g).je + (D)) return;          \
  const int k0 = blockIdx.z * PHY_KCHUNK;                    \
  const int k1 = k0 + PHY_KCHUNK < (g).nk ? k0 + PHY_KCHUNK : (g).nk

// ---- copy_dycore_to_physics (update_atmos_state.py:95-145): interface dims with interval(0, -1) ---------------------------------
struct PhysCopyFields {
  const real* in[PACE_PHYSICS_COPY_FIELDS];
  real* out[PACE_PHYSICS_COPY_FIELDS];
};

__global__ void __launch_bounds__(64) k_copy_dycore_to_physics(Geo g, PhysCopyFields f) {
  PHY_POINT(g, 1);
  for (int k = k0; k < k1; ++k) {
    const long a = IDX3(g, i, j, k);
    real v[PACE_PHYSICS_COPY_FIELDS];
#pragma unroll
    for (int m = 0; m < PACE_PHYSICS_COPY_FIELDS; ++m) v[m] = f.in[m][a];
#pragma unroll
    for (int m = 0; m < PACE_PHYSICS_COPY_FIELDS; ++m) f.out[m][a] = v[m];
  }
}

// ---- Physics.__call__ before the microphysics (physics.py:280-333), origin (3, 3, 0), domain (n, n, nk) ---------------------------
// The statein's statements need the interface pressure from above (prsi, the running sum of the dry delp) and the first
// interface geopotential from below (phii[k] = phii[k + 1] - delz * GRAV), so a column is swept twice:
//
//   down  q * delp (seven tracers), the dry delp dm = delp - ql - qr - qi - qs - qg, prsi, q / dm (eight tracers), delprsi.
//         dm is left in delp, which is what the reference's delp holds between its second and its last statement.
//   up    the first phii in a register; delp = dm * rTv / (phii[k] - phii[k + 1]) with its two clamps; del_gz (divided by
//         T (1 + ZVIR q), then multiplied by it: two roundings, not an identity) in a register; the second phii, phil;
//         prepare_microphysics' dz and wmp (wmp with the delp just stored: the pressure) and the ten zeroed tendencies.
//
// Nothing outside the compute domain is written and level nk of the layer fields is neither read nor written (the reference
// sweeps get_prs_fv3 / get_phi_fv3 over the halo and multiplies its zero padding by zero); prsi and phii get level nk.
struct PhysPrepareFields {
  real* q[8];  // qvapor, qliquid, qrain, qice, qsnow, qgraupel, qo3mr (times moist, over dry delp), qsgs_tke (over dry delp)
  const real *pt, *delz, *omga;
  real *delp, *prsi, *phii, *phil, *delprsi, *dz, *wmp;
  real* tend[PACE_MICROPHYSICS_TENDENCIES];
};

__global__ void __launch_bounds__(64) k_physics_prepare(Geo g, PhysPrepareFields f, double ptop, int do_microphysics) {
  const int i = g.is + blockIdx.x * 64 + threadIdx.x;
  const int j = g.js + blockIdx.y;
  if (i > g.ie || j > g.je) return;
  const long c = IDX2(g, i, j);
  {
    double prsi = ptop;
    f.prsi[c] = (real)prsi;
    for (int k0 = 0; k0 < g.nk; k0 += PHY_KC) {
      double q[PHY_KC][8], dp[PHY_KC];
#pragma unroll
      for (int u = 0; u < PHY_KC; ++u) {  // the chunk's loads, all issued before its arithmetic
        const int k = k0 + u < g.nk ? k0 + u : g.nk - 1;
        const long a = c + (long)k * g.sk;
#pragma unroll
        for (int m = 0; m < 8; ++m) q[u][m] = f.q[m][a];
        dp[u] = f.delp[a];
      }
#pragma unroll
      for (int u = 0; u < PHY_KC; ++u) {
        const int k = k0 + u;
        if (k >= g.nk) break;
        const long a = c + (long)k * g.sk;
#pragma unroll
        for (int m = 0; m < 7; ++m) q[u][m] = q[u][m] * dp[u];
        const double dm = dp[u] - q[u][1] - q[u][2] - q[u][3] - q[u][4] - q[u][5];  // nwat == 6
        const double below = prsi + dm;
#pragma unroll
        for (int m = 0; m < 8; ++m) f.q[m][a] = (real)(q[u][m] / dm);
        f.delp[a] = (real)dm;
        f.prsi[a + g.sk] = (real)below;
        f.delprsi[a] = (real)(below - prsi);
        prsi = below;
      }
    }
  }
  double phii0 = 0.0;  // the first phii (from delz) at level k + 1
  double phii = 0.0;   // the second one (get_phi_fv3)
  f.phii[c + (long)g.nk * g.sk] = (real)0.0;
  for (int k0 = g.nk - 1; k0 >= 0; k0 -= PHY_KC) {
    double qv[PHY_KC], pt[PHY_KC], dz[PHY_KC], dm[PHY_KC], om[PHY_KC], pi[PHY_KC + 1];
    pi[0] = f.prsi[c + (long)(k0 + 1) * g.sk];
#pragma unroll
    for (int u = 0; u < PHY_KC; ++u) {
      const int k = k0 - u >= 0 ? k0 - u : 0;
      const long a = c + (long)k * g.sk;
      qv[u] = f.q[0][a];
      pt[u] = f.pt[a];
      dz[u] = f.delz[a];
      dm[u] = f.delp[a];
      pi[u + 1] = f.prsi[a];
      om[u] = do_microphysics ? (double)f.omga[a] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < PHY_KC; ++u) {
      const int k = k0 - u;
      if (k < 0) break;
      const long a = c + (long)k * g.sk;
      const double above = phii0 - dz[u] * phys::GRAV;
      const double dphi = above - phii0;
      phii0 = above;
      const double q_rad = qv[u] > 1.0e-10 ? qv[u] : 1.0e-10;
      const double rtv = phys::RDGAS * pt[u] * (1.0 + phys::ZVIR * q_rad);
      double p = dm[u] * rtv / dphi;
      const double hi = pi[u] - 0.01 * dm[u], lo = pi[u + 1] + 0.01 * dm[u];
      p = p < hi ? p : hi;
      p = p > lo ? p : lo;
      f.delp[a] = (real)p;
      const double q_pos = qv[u] > 0.0 ? qv[u] : 0.0;
      double del_gz = dphi / (pt[u] * (1.0 + phys::ZVIR * q_pos));
      del_gz = del_gz * pt[u] * (1.0 + phys::ZVIR * q_pos);
      f.phil[a] = (real)(0.5 * (phii + phii + del_gz));
      const double up = phii + del_gz;
      f.phii[a] = (real)up;
      if (do_microphysics) {
        f.dz[a] = (real)((phii - up) * phys::RGRAV);
        f.wmp[a] = (real)(-om[u] * (1.0 + phys::ZVIR * qv[u]) * pt[u] / p * (phys::RDGAS * phys::RGRAV));
#pragma unroll
        for (int m = 0; m < PACE_MICROPHYSICS_TENDENCIES; ++m) f.tend[m][a] = (real)0.0;
      }
      phii = up;
    }
  }
}

// ---- update_physics_state_with_tendencies (physics.py:158-201), origin (3, 3, 0), domain (n, n, nk) -------------------------------
struct PhysUpdateFields {
  const real* x[PACE_PHYSICS_UPDATED_FIELDS];
  const real* x_dt[PACE_PHYSICS_UPDATED_FIELDS];
  real* out[PACE_PHYSICS_UPDATED_FIELDS];
};

__global__ void __launch_bounds__(64) k_physics_update_state(Geo g, PhysUpdateFields f, double dt) {
  PHY_POINT(g, 0);
  for (int k = k0; k < k1; ++k) {
    const long a = IDX3(g, i, j, k);
    double x[PACE_PHYSICS_UPDATED_FIELDS], x_dt[PACE_PHYSICS_UPDATED_FIELDS];
#pragma unroll
    for (int m = 0; m < PACE_PHYSICS_UPDATED_FIELDS; ++m) {
      x[m] = f.x[m][a];
      x_dt[m] = f.x_dt[m][a];
    }
#pragma unroll
    for (int m = 0; m < PACE_PHYSICS_UPDATED_FIELDS; ++m) f.out[m][a] = (real)(x[m] + x_dt[m] * dt);
  }
}

// ---- prepare_tendencies_and_update_tracers (update_atmos_state.py:40-92), origin (3, 3, 0), domain (n, n, nk) ---------------------
// The sums run qvapor, qliquid, qrain, qsnow, qice, qgraupel, left to right, as the reference writes them.
struct PhysCouplingFields {
  real* tend[3];      // u_dt, v_dt, pt_dt: accumulated into
  const real* t1[9];  // physics_updated_ua, _va, _pt, then the six updated species in the sums' order
  const real* t0[3];  // the physics state's ua, va, pt
  real* q[6];         // the dycore's six species in the sums' order
  const real* prsi;
  real* delp;
};

__global__ void __launch_bounds__(64) k_physics_tendencies_to_dycore(Geo g, PhysCouplingFields f, double rdt) {
  PHY_POINT(g, 0);
  double pe = f.prsi[IDX3(g, i, j, k0)];
  for (int k = k0; k < k1; ++k) {
    const long a = IDX3(g, i, j, k);
    double tend[3], t1[9], t0[3], q[6];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      tend[m] = f.tend[m][a];
      t0[m] = f.t0[m][a];
    }
#pragma unroll
    for (int m = 0; m < 9; ++m) t1[m] = f.t1[m][a];
#pragma unroll
    for (int m = 0; m < 6; ++m) q[m] = f.q[m][a];
    const double below = f.prsi[a + g.sk], delp = f.delp[a];
#pragma unroll
    for (int m = 0; m < 3; ++m) f.tend[m][a] = (real)(tend[m] + (t1[m] - t0[m]) * rdt);
    const double dp = below - pe;
    pe = below;
    double qwat[6];
#pragma unroll
    for (int m = 0; m < 6; ++m) qwat[m] = dp * t1[3 + m];
    const double qt = qwat[0] + qwat[1] + qwat[2] + qwat[3] + qwat[4] + qwat[5];
    const double q_sum = q[0] + q[1] + q[2] + q[3] + q[4] + q[5];
    const double q0 = delp * (1.0 - q_sum) + qt;
    f.delp[a] = (real)q0;
#pragma unroll
    for (int m = 0; m < 6; ++m) f.q[m][a] = (real)(qwat[m] / q0);
  }
}

static inline dim3 pointwise_grid(const Geo& g, int extra) {
  return dim3((unsigned)((g.n + extra + 63) / 64), (unsigned)(g.n + extra), (unsigned)((g.nk + PHY_KCHUNK - 1) / PHY_KCHUNK));
}

int launch_copy_dycore_to_physics(const Geo& g, const real* const* in, real* const* out, hipStream_t st) {
  PhysCopyFields f;
  for (int m = 0; m < PACE_PHYSICS_COPY_FIELDS; ++m) {
    f.in[m] = in[m];
    f.out[m] = out[m];
  }
  hipLaunchKernelGGL(k_copy_dycore_to_physics, pointwise_grid(g, 1), dim3(64), 0, st, g, f);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}

int launch_physics_prepare(const Geo& g, real* const* tracers, const real* pt, const real* delz, real* delp, const real* omga,
                           real* prsi, real* phii, real* phil, real* delprsi, real* dz, real* wmp, real* const* tendencies,
                           double ptop, int do_microphysics, hipStream_t st) {
  PhysPrepareFields f;
  for (int m = 0; m < 8; ++m) f.q[m] = tracers[m];
  f.pt = pt;
  f.delz = delz;
  f.omga = omga;
  f.delp = delp;
  f.prsi = prsi;
  f.phii = phii;
  f.phil = phil;
  f.delprsi = delprsi;
  f.dz = dz;
  f.wmp = wmp;
  for (int m = 0; m < PACE_MICROPHYSICS_TENDENCIES; ++m) f.tend[m] = do_microphysics ? tendencies[m] : nullptr;
  hipLaunchKernelGGL(k_physics_prepare, dim3((unsigned)((g.n + 63) / 64), (unsigned)g.n), dim3(64), 0, st, g, f, ptop,
                     do_microphysics);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}

int launch_physics_update_state(const Geo& g, const real* const* x, const real* const* x_dt, real* const* out, double dt,
                                hipStream_t st) {
  PhysUpdateFields f;
  for (int m = 0; m < PACE_PHYSICS_UPDATED_FIELDS; ++m) {
    f.x[m] = x[m];
    f.x_dt[m] = x_dt[m];
    f.out[m] = out[m];
  }
  hipLaunchKernelGGL(k_physics_update_state, pointwise_grid(g, 0), dim3(64), 0, st, g, f, dt);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}

int launch_physics_tendencies_to_dycore(const Geo& g, real* const* tendencies, const real* const* updated,
                                        const real* const* before, real* const* tracers, const real* prsi, real* delp,
                                        double rdt, hipStream_t st) {
  PhysCouplingFields f;
  for (int m = 0; m < 3; ++m) {
    f.tend[m] = tendencies[m];
    f.t0[m] = before[m];
  }
  for (int m = 0; m < 9; ++m) f.t1[m] = updated[m];
  for (int m = 0; m < 6; ++m) f.q[m] = tracers[m];
  f.prsi = prsi;
  f.delp = delp;
  hipLaunchKernelGGL(k_physics_tendencies_to_dycore, pointwise_grid(g, 0), dim3(64), 0, st, g, f, rdt);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
