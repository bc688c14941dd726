// The end of a dycore-only time step: UpdateAtmosphereState / ApplyPhysicsToDycore (the Fortran atmosphere_state_update /
// fv_update_phys) -- stencils/pace/stencils/update_atmos_state.py:19-37, fv_update_phys.py:30-74, update_dwind_phys.py:446-653.
// Three streaming kernels, none with a scratch field:
//
//   k_fill_gfs_delp           fill_gfs_delp: one thread per column of the FULL domain (halo included), two sweeps
//   k_phys_thermo_pressure    moist_cv + update_pressure_and_surface_winds: one thread per column, one sweep down
//   k_update_dwinds_phys      AGrid2DGridPhysics.__call__: one thread per (i, j), levels in a loop, the metric terms in registers
//   k_zero_tendencies         its set_winds_zero, as a launch of its own AFTER the winds (no thread zeroes what another reads)
//
// Arithmetic is fp64 in both builds, in the reference's order of operations with its divisions kept.
#include "common.h"
#include "kernels.h"
#include "thermo.h"

// ---- fill_gfs_delp (update_atmos_state.py:19-37) over origin (0, 0, 0), domain (n + 6, n + 6, nk + 1) -----------------------
// With K = nk + 1 levels the four intervals are (0, K - 2) backward, (1, K - 1) twice and (0, K - 1): level K - 1 = nk is
// neither read nor written.  The BACKWARD sweep at level k reads level k + 1 as the sweep left it, so the value is carried in a
// register.  The PARALLEL clamp and the two FORWARD computations are one sweep down: the borrowing statement at level k reads
// level k - 1 after the clamp and the borrowing but BEFORE the last computation zeroes it, so that value is carried too and
// level k - 1 is stored when level k is done.  A level is stored only if its bits changed (-0.0 that becomes +0.0 is stored).
// q_min is taken in the storage type: in the float32 build the comparisons and the clamp use float(q_min), as arithmetic on
// float32 fields would, so a clamped level is not below the threshold of the next call, and every value a level of q takes
// between two statements of the reference is the fp64 result rounded once to the storage type.
// Both sweeps take UPD_KC levels at a time: the chunk's loads are issued together, before its arithmetic and its stores (one
// wave per SIMD at C192, so nothing else would hide a level's load latency: cf. k_subgridz.hip).
#define UPD_KC 4

__device__ __forceinline__ bool same_bits(double a, double b) {
  long long x, y;
  memcpy(&x, &a, sizeof x);
  memcpy(&y, &b, sizeof y);
  return x == y;
}

__global__ void __launch_bounds__(64) k_fill_gfs_delp(Geo g, const real* __restrict__ delp, real* __restrict__ q, double q_min_) {
  const double q_min = (double)(real)q_min_;
  const int i = blockIdx.x * 64 + threadIdx.x;
  const int j = blockIdx.y;
  if (i > g.n + 5 || j > g.n + 5) return;
  const long c = IDX2(g, i, j);
  const int kb = g.nk - 1;  // the lowest level touched (the C entry point refuses nk < 2)
  {
    double q1 = q[c + (long)kb * g.sk], dp1 = delp[c + (long)kb * g.sk];
    for (int k0 = kb - 1; k0 >= 0; k0 -= UPD_KC) {
      double qc[UPD_KC], dc[UPD_KC];
#pragma unroll
      for (int u = 0; u < UPD_KC; ++u) {
        const int k = k0 - u;
        qc[u] = k >= 0 ? (double)q[c + (long)k * g.sk] : 0.0;
        dc[u] = k >= 0 ? (double)delp[c + (long)k * g.sk] : 1.0;
      }
#pragma unroll
      for (int u = 0; u < UPD_KC; ++u) {
        const int k = k0 - u;
        if (k < 0) break;
        double q0 = qc[u];
        if (q1 < q_min) {
          q0 = q0 + (q1 - q_min) * dp1 / dc[u];
          q[c + (long)k * g.sk] = (real)q0;
          q0 = (double)(real)q0;  // what the next level reads is what was stored
        }
        q1 = q0;
        dp1 = dc[u];
      }
    }
  }
  double qp = q[c], dpp = delp[c];  // level k - 1 after the clamp and the borrowing
  double stored = qp;               // ... and as it is in memory
  for (int k0 = 1; k0 <= kb; k0 += UPD_KC) {
    double qc[UPD_KC], dc[UPD_KC];
#pragma unroll
    for (int u = 0; u < UPD_KC; ++u) {
      const int k = k0 + u;
      qc[u] = k <= kb ? (double)q[c + (long)k * g.sk] : 0.0;
      dc[u] = k <= kb ? (double)delp[c + (long)k * g.sk] : 1.0;
    }
#pragma unroll
    for (int u = 0; u < UPD_KC; ++u) {
      const int k = k0 + u;
      if (k > kb) break;
      double qk = qc[u];
      if (qk < q_min) qk = q_min;
      if (qp < 0.0) qk = qk + qp * dpp / dc[u];
      const double out = qp < 0.0 ? 0.0 : qp;
      if (!same_bits(out, stored)) q[c + (long)(k - 1) * g.sk] = (real)out;
      // (in the float32 build the borrowing of the next level reads the stored, rounded value, as two stencils would)
      qp = (double)(real)qk;
      stored = qc[u];
      dpp = dc[u];
    }
  }
  {
    const double out = qp < 0.0 ? 0.0 : qp;
    if (!same_bits(out, stored)) q[c + (long)kb * g.sk] = (real)out;
  }
}

// ---- moist_cv + update_pressure_and_surface_winds (fv_update_phys.py:30-74), origin (3, 3, 0), domain (n, n, nk + 1) ---------
struct PhysColumnFields {
  const real *qvapor, *qliquid, *qrain, *qsnow, *qice, *qgraupel;
  real *pt, *t_dt;
  real *pe, *peln, *pk;
  const real *delp, *ua, *va;
  real *ps, *u_srf, *v_srf;
};

__global__ void __launch_bounds__(64) k_phys_thermo_pressure(Geo g, PhysColumnFields f, double dt) {
  const int i = g.is + blockIdx.x * 64 + threadIdx.x;
  const int j = g.js + blockIdx.y;
  if (i > g.ie || j > g.je) return;
  const long c = IDX2(g, i, j);
  double pe = f.pe[c];  // level 0 stays as it is
  for (int k0 = 0; k0 <= g.nk; k0 += UPD_KC) {
    double qv[UPD_KC], ql[UPD_KC], qs[UPD_KC], pt[UPD_KC], td[UPD_KC], dp[UPD_KC];
#pragma unroll
    for (int u = 0; u < UPD_KC; ++u) {  // the chunk's loads, all issued before its arithmetic
      const int k = k0 + u < g.nk ? k0 + u : g.nk;
      const long a = c + (long)k * g.sk;
      qv[u] = f.qvapor[a];
      ql[u] = (double)f.qliquid[a] + (double)f.qrain[a];
      qs[u] = (double)f.qice[a] + (double)f.qsnow[a] + (double)f.qgraupel[a];
      pt[u] = f.pt[a];
      td[u] = f.t_dt[a];
      dp[u] = k >= 1 ? (double)f.delp[a - g.sk] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < UPD_KC; ++u) {
      const int k = k0 + u;
      if (k > g.nk) break;
      const long a = c + (long)k * g.sk;
      const double gz = ql[u] + qs[u];
      const double cvm = moist_cvm(qv[u] + gz, qv[u], ql[u], qs[u]);
      f.pt[a] = (real)(pt[u] + td[u] * dt * phys::CP_AIR / cvm);
      f.t_dt[a] = (real)0.0;
      if (k >= 1) {
        pe = pe + dp[u];
        const double peln = log(pe);
        f.pe[a] = (real)pe;
        f.peln[a] = (real)peln;
        f.pk[a] = (real)exp(phys::KAPPA * peln);
      }
      if (k == g.nk - 1) {
        f.u_srf[c] = f.ua[a];
        f.v_srf[c] = f.va[a];
      }
    }
  }
  f.ps[c] = (real)pe;
}

// ---- AGrid2DGridPhysics.__call__ (update_dwind_phys.py:446-653) ---------------------------------------------------------------
// v3 = u_dt * vlon + v_dt * vlat (three components); ue = v3[j - 1] + v3, ve = v3[i - 1] + v3; on the four tile edges
// ue (rows js and je + 1) and ve (columns is and ie + 1) are blended with a neighbour along the edge -- the one at + 1 up to
// the tile's midpoint (storage index n / 2 + 2, the reference's _im2 = _jm2), the one at - 1 beyond it -- and every blend reads
// UNBLENDED values: the reference computes both halves into ut / vt before it copies either back.  The reference's tests
// `global_is <= im2` / `global_ie > im2` (south, west, east) and `global_is < im2` / `global_ie >= im2` (north) only decide
// whether a SUBTILE holds a half of the edge; the halves themselves are the same on all four edges, and with one subtile per
// tile (the only layout of this library) both tests of either form hold for every n >= 4.
// So u(i, j) is a function of v3 at (i, j - 1), (i, j) and, on rows js and je + 1, (i +- 1, j - 1), (i +- 1, j); v likewise.
// One thread per (i, j) of origin (3, 3), domain (n + 1, n + 1): it updates u(i, j) if i <= ie and v(i, j) if j <= je, keeps
// the unit vectors of its up to five points in registers and walks the levels of its chunk.
struct DwindFields {
  real *u, *v;
  const real *u_dt, *v_dt;
  const real *vlon[3], *vlat[3], *es1[3], *ew2[3];
  const real *edge_vect_w, *edge_vect_e, *edge_vect_s, *edge_vect_n;
};

struct DwindPoint {  // the unit vectors of one A-grid point and its offset from the thread's own column
  double vlon[3], vlat[3];
  long off;
};

__device__ __forceinline__ void dwind_point(const Geo& g, const DwindFields& f, int i, int j, long c, DwindPoint& p) {
  const long a = IDX2(g, i, j);
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    p.vlon[m] = f.vlon[m][a];
    p.vlat[m] = f.vlat[m][a];
  }
  p.off = a - c;
}

__device__ __forceinline__ void dwind_v3(const DwindFields& f, const DwindPoint& p, long a, double* v3) {
  const double ud = f.u_dt[a + p.off], vd = f.v_dt[a + p.off];
#pragma unroll
  for (int m = 0; m < 3; ++m) v3[m] = ud * p.vlon[m] + vd * p.vlat[m];
}

#define DWIND_KCHUNK 8

__global__ void __launch_bounds__(64) k_update_dwinds_phys(Geo g, DwindFields f, double dt5) {
  const int i = g.is + blockIdx.x * 64 + threadIdx.x;
  const int j = g.js + blockIdx.y;
  if (i > g.ie + 1 || j > g.je + 1) return;
  const bool do_u = i <= g.ie, do_v = j <= g.je;
  const int mid = g.n / 2 + 2;  // _im2 = _jm2 = int((npx - 1) / 2) + 2
  const long c = IDX2(g, i, j);
  // u: the south (j == js) and north (j == je + 1) edges blend ue along i; v: the west and east edges blend ve along j
  const bool u_edge = do_u && (j == g.js || j == g.je + 1);
  const bool v_edge = do_v && (i == g.is || i == g.ie + 1);
  const int du = i <= mid ? 1 : -1, dv = j <= mid ? 1 : -1;
  double eu = 0.0, ev = 0.0;
  if (u_edge) eu = j == g.js ? f.edge_vect_s[i] : f.edge_vect_n[i];
  if (v_edge) ev = i == g.is ? f.edge_vect_w[j] : f.edge_vect_e[j];
  DwindPoint P, PS, PW, PUa, PUb, PVa, PVb;  // (i, j), (i, j - 1), (i - 1, j); the neighbour pairs of the two blends
  dwind_point(g, f, i, j, c, P);
  dwind_point(g, f, i, j - 1, c, PS);
  dwind_point(g, f, i - 1, j, c, PW);
  PUa = PUb = PVa = PVb = P;
  if (u_edge) {
    dwind_point(g, f, i + du, j - 1, c, PUa);
    dwind_point(g, f, i + du, j, c, PUb);
  }
  if (v_edge) {
    dwind_point(g, f, i - 1, j + dv, c, PVa);
    dwind_point(g, f, i, j + dv, c, PVb);
  }
  double es1[3], ew2[3];
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    es1[m] = do_u ? (double)f.es1[m][c] : 0.0;
    ew2[m] = do_v ? (double)f.ew2[m][c] : 0.0;
  }
  const int k0 = blockIdx.z * DWIND_KCHUNK;
  const int k1 = k0 + DWIND_KCHUNK < g.nk ? k0 + DWIND_KCHUNK : g.nk;
  for (int k = k0; k < k1; ++k) {
    const long a = c + (long)k * g.sk;
    double v3[3], s[3], w[3];
    dwind_v3(f, P, a, v3);
    if (do_u) {
      dwind_v3(f, PS, a, s);
      double ue[3];
#pragma unroll
      for (int m = 0; m < 3; ++m) ue[m] = s[m] + v3[m];
      if (u_edge) {
        double na[3], nb[3];
        dwind_v3(f, PUa, a, na);
        dwind_v3(f, PUb, a, nb);
#pragma unroll
        for (int m = 0; m < 3; ++m) ue[m] = eu * (na[m] + nb[m]) + (1.0 - eu) * ue[m];
      }
      f.u[a] = (real)((double)f.u[a] + dt5 * (ue[0] * es1[0] + ue[1] * es1[1] + ue[2] * es1[2]));
    }
    if (do_v) {
      dwind_v3(f, PW, a, w);
      double ve[3];
#pragma unroll
      for (int m = 0; m < 3; ++m) ve[m] = w[m] + v3[m];
      if (v_edge) {
        double na[3], nb[3];
        dwind_v3(f, PVa, a, na);
        dwind_v3(f, PVb, a, nb);
#pragma unroll
        for (int m = 0; m < 3; ++m) ve[m] = ev * (na[m] + nb[m]) + (1.0 - ev) * ve[m];
      }
      f.v[a] = (real)((double)f.v[a] + dt5 * (ve[0] * ew2[0] + ve[1] * ew2[1] + ve[2] * ew2[2]));
    }
  }
}

// set_winds_zero (update_dwind_phys.py:11-17): origin (2, 2, 0), domain (n + 2, n + 2, nk); a thread walks the levels of its
// chunk (one workgroup per row segment and LEVEL was 61 000 workgroups of two stores per thread at C192: dispatch-bound)
__global__ void __launch_bounds__(64) k_zero_tendencies(Geo g, real* __restrict__ u_dt, real* __restrict__ v_dt) {
  const int i = g.is - 1 + blockIdx.x * 64 + threadIdx.x;
  const int j = g.js - 1 + blockIdx.y;
  if (i > g.ie + 1 || j > g.je + 1) return;
  const int k0 = blockIdx.z * DWIND_KCHUNK;
  const int k1 = k0 + DWIND_KCHUNK < g.nk ? k0 + DWIND_KCHUNK : g.nk;
  for (int k = k0; k < k1; ++k) {
    const long a = IDX3(g, i, j, k);
    u_dt[a] = (real)0.0;
    v_dt[a] = (real)0.0;
  }
}

int launch_fill_gfs_delp(const Geo& g, const real* delp, real* q, double q_min, hipStream_t st) {
  const int m = g.n + 6;
  hipLaunchKernelGGL(k_fill_gfs_delp, dim3((unsigned)((m + 63) / 64), (unsigned)m), dim3(64), 0, st, g, delp, q, q_min);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}

int launch_phys_thermo_pressure(const Geo& g, const real* const* water, real* pt, real* t_dt, real* pe, const real* delp,
                                real* peln, real* pk, const real* ua, const real* va, real* ps, real* u_srf, real* v_srf,
                                double dt, hipStream_t st) {
  PhysColumnFields f;
  f.qvapor = water[0];
  f.qliquid = water[1];
  f.qrain = water[2];
  f.qsnow = water[3];
  f.qice = water[4];
  f.qgraupel = water[5];
  f.pt = pt;
  f.t_dt = t_dt;
  f.pe = pe;
  f.peln = peln;
  f.pk = pk;
  f.delp = delp;
  f.ua = ua;
  f.va = va;
  f.ps = ps;
  f.u_srf = u_srf;
  f.v_srf = v_srf;
  hipLaunchKernelGGL(k_phys_thermo_pressure, dim3((unsigned)((g.n + 63) / 64), (unsigned)g.n), dim3(64), 0, st, g, f, dt);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}

int launch_update_dwinds_phys(const Geo& g, real* u, real* v, real* u_dt, real* v_dt, const real* const* vlon,
                              const real* const* vlat, const real* const* es1, const real* const* ew2, const real* edge_vect_w,
                              const real* edge_vect_e, const real* edge_vect_s, const real* edge_vect_n, double dt5,
                              hipStream_t st) {
  DwindFields f;
  f.u = u;
  f.v = v;
  f.u_dt = u_dt;
  f.v_dt = v_dt;
  for (int m = 0; m < 3; ++m) {
    f.vlon[m] = vlon[m];
    f.vlat[m] = vlat[m];
    f.es1[m] = es1[m];
    f.ew2[m] = ew2[m];
  }
  f.edge_vect_w = edge_vect_w;
  f.edge_vect_e = edge_vect_e;
  f.edge_vect_s = edge_vect_s;
  f.edge_vect_n = edge_vect_n;
  const unsigned bx = (unsigned)((g.n + 1 + 63) / 64), bx0 = (unsigned)((g.n + 2 + 63) / 64);
  hipLaunchKernelGGL(k_update_dwinds_phys, dim3(bx, (unsigned)(g.n + 1), (unsigned)((g.nk + DWIND_KCHUNK - 1) / DWIND_KCHUNK)),
                     dim3(64), 0, st, g, f, dt5);
  PACE_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_zero_tendencies, dim3(bx0, (unsigned)(g.n + 2), (unsigned)((g.nk + DWIND_KCHUNK - 1) / DWIND_KCHUNK)),
                     dim3(64), 0, st, g, u_dt, v_dt);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
