// Host-side launch functions (one per reference class on the hot path).
#pragma once
#include "common.h"
#include "wgmap.h"

// d_sw's separate wind outputs get the halo of the inputs (k_dsw.hip k_copy_wind_halo): a copy the frame workgroups of the one-launch
// form take along (their stage A waits for a round trip anyway); `done` tells the caller whether this launch took it
struct FxWindHalo {
  const real *u, *v;
  real *u_out, *v_out;
  bool done;
};
int launch_fxadv(const Geo& g, const Met& m, const real* uc, const real* vc, real* crx, real* cry,
                 real* xfx, real* yfx, real* ut, real* vt, double dt, real* cx_acc, real* cy_acc,
                 hipStream_t st, int part = 0, int contra_out = 0, FxWindHalo* wind_halo = nullptr);
// the frame of the plane outside the faces d_sw's winds are written on, point p of its level (k_copy_wind_halo's enumeration)
__device__ __forceinline__ void wind_halo_copy_point(const Geo& g, int p, int k, const real* __restrict__ u, const real* __restrict__ v,
                                                     real* __restrict__ u_out, real* __restrict__ v_out) {
  const int nsouth = g.js, nnorth = g.nj - 1 - g.je, nmid = g.je - g.js + 1, nwest = g.is, neast = g.ni - 1 - g.ie;
  const int rows = (nsouth + nnorth) * g.ni;
  int i, j;
  if (p < rows) {
    const int r = p / g.ni;
    i = p - r * g.ni, j = r < nsouth ? r : g.je + 1 + (r - nsouth);
  } else {
    p -= rows;
    const int w = nwest + neast, r = p / w, c = p - r * w;
    if (r >= nmid) return;
    j = g.js + r, i = c < nwest ? c : g.ie + 1 + (c - nwest);
  }
  const long ch = IDX3(g, i, j, k);
  const bool in_i = i >= g.is && i <= g.ie, in_j = j >= g.js && j <= g.je;
  if (!(in_i && (in_j || j == g.je + 1))) u_out[ch] = u[ch];
  if (!((in_i || i == g.ie + 1) && in_j)) v_out[ch] = v[ch];
}
__host__ __device__ __forceinline__ int wind_halo_points(const Geo& g) {
  return (g.js + g.nj - 1 - g.je) * g.ni + (g.je - g.js + 1) * (g.is + g.ni - 1 - g.ie);
}
int launch_fvtp2d(const Geo& g, const Met& m, const real* q, const real* crx, const real* cry,
                  const real* xfx, const real* yfx, real* fx, real* fy, const real* xmf,
                  const real* ymf, int hord, int nlev, hipStream_t st);
// Optional fused del-n damping of the same scalar (FiniteVolumeTransport calls DelnFlux on q right after the transport,
// fvtp2d.py:338-345; d_sw also needs DelnFluxNoSG(w) next to the transport of w).  DMODE -1: none; 0: damping fluxes
// written to fx2o / fy2o; 1: added to fx / fy; 2: added mass-weighted (delnflux.py:318-328).
struct FvDamp {
  const real* damp_k;
  const real* nord_k;
  const real* mass;
  real* fx2o;
  real* fy2o;
  int nmax, mass_given;
  // epilogue (EPI > 0): qout = q * amass + flux_increment(fx, fy) (apply_fluxes, d_sw.py:122-145) is written instead of
  // the fluxes; EPI == 2 additionally turns the damping fluxes into dw / heat_s / diss_est (heat_diss, d_sw.py:63-103)
  real* qout;
  const real* amass;
  real* dw;
  real* heat_s;
  real* diss_est;
  const real* damp_w_k;
  const real* ke_bg_k;
  double dt;
  // optional accumulators of the final fluxes (EPI == 0): the mass-flux half of flux_capacitor, mfx += fx, mfy += fy
  real* accx;
  real* accy;
  // optional 2-D field added to q AFTER the fused damping has read it: the transported scalar is q + add2d while the damped
  // one is q (d_sw: absolute vorticity = relative vorticity + fC_agrid, d_sw.py:389-402, damping acts on the relative one)
  const real* add2d;
  // optional (EPI == 0): instead of storing the fluxes, finish u_and_v_from_ke (d_sw.py:406-477) with them -- the transported
  // scalar is then the absolute vorticity: u = u * dx + ke - ke[i+1] + fy, v = v * dy + ke - ke[j+1] - fx, each on the face the
  // flux lives on, by the workgroup that owns the face
  real* u_upd;
  real* v_upd;
  const real* ke;
  // optional: where the results of that go instead of u_upd / v_upd themselves (launch_d_sw: a workspace copy, so that the kernel
  // that follows -- heating + final wind update in one -- reads the intermediate winds of its neighbours race-free)
  real* u_out;
  real* v_out;
};

int launch_transport(const Geo& g, const Met& m, const real* q, const real* crx, const real* cry, const real* xfx,
                     const real* yfx, real* fx, real* fy, const real* xmf, const real* ymf, int hord, int nlev,
                     int dmode, int epi, const FvDamp& dp, hipStream_t st);
int launch_transport_scalars3(const Geo& g, const Met& m, const real* w, const real* q_con, const real* pt, const real* crx,
                              const real* cry, const real* xfx, const real* yfx, const real* xmf, const real* ymf, int nlev,
                              const FvDamp& dpw, const FvDamp& dpq, const FvDamp& dpt, hipStream_t st);
// k_fvt.hip: the lean transport kernel of the production tilings (every tile edge on a workgroup-tile boundary); same contract
// as launch_transport with the unit fluxes resolved (xu = xmf or xfx); PACE_ERR_UNSUPPORTED for the calls it does not cover
int launch_transport_lean(const Geo& g, const Met& m, const real* q, const real* crx, const real* cry, const real* xfx,
                          const real* yfx, real* fx, real* fy, const real* xu, const real* yu, int hord, int nlev, int dmode,
                          int epi, const FvDamp& dp, hipStream_t st);

// the winds of d_sw as the fifth pass of the scalar-phase kernel (fvt_core.h): the vorticity transport (u_and_v_from_ke), the
// vorticity damping, the dissipative heating and the final winds.  u_out / v_out: buffers of their own; copy_halo: they also get
// the halo u / v have (the caller swaps the buffers).
struct DswWinds {
  const real *rel_vort, *u, *v, *ke, *vort_b;
  real *u_out, *v_out, *heat_source;
  int do_skeb, copy_halo;
  int ke_plus_vort;  // `ke` is the plain kinetic energy: the kernel adds the damped vorticity to it (divergence_damping.py:161-185)
  double d_con;
};
// The device column block of d_sw: one array of nk + 1 per slot, uploaded by dsw_prepare, read by the launchers of k_dsw.hip and k_fvt.hip
enum DswColumn {
  DSWC_NORD_V, DSWC_NORD_W, DSWC_NORD_T, DSWC_DAMP_VT, DSWC_DAMP_W, DSWC_DAMP_T, DSWC_D2_DIVG, DSWC_D_CON, DSWC_KE_BG, DSWC_FAC_VT, DSWC_FAC_T,
  DSWC_FAC_VT_C, DSWC_FAC_W_C, DSWC_COUNT
};
static inline const real* dsw_column(const real* kc, const Geo& g, DswColumn slot) { return kc + (long)slot * (g.nk + 1); }
// the damping orders the fused scalar kernel takes (fvt_core.h): nmax_* = the column's highest nord_v / nord_w / nord_t
static inline bool dsw_fused_takes_orders(int nmax_v, int nmax_w, int nmax_t) { return nmax_v <= 2 && nmax_w <= 2 && nmax_t <= 2; }
// the field arguments of the d_sw entry points (include/pace_hip.h pace_d_sw; its unused zh is not among them)
struct DswFields {
  real *delpc, *delp, *pt, *u, *v, *w, *uc, *vc;
  const real *ua, *va;
  real *divgd, *mfx, *mfy, *cx, *cy, *crx, *cry, *xfx, *yfx, *q_con, *heat_source, *diss_est;
  double dt;
};
// (f: delp, pt, w, q_con, the Courant numbers and area fluxes, mfx, mfy, diss_est and dt are read from it)
int launch_dsw_scalars_lean(const Geo& g, const Met& m, const DswFields& f, real* const* outs, real* dw, real* heat_s, const real* kc, int hord,
                            int nmax_v, int nmax_w, int nmax_t, hipStream_t st, const DswWinds* winds = nullptr);
// whether launch_transport_lean takes this geometry with this order (fp64 build, tiling, row alignment)
bool transport_lean_covers(const Geo& g, int hord);

// The metric fields the transport kernels read (kernel arguments live in SGPRs: the full pace_metrics_t is 43 pointers, and the
// register allocator answered with ~300 SGPR spills -- v_readlane / v_writelane traffic on the vector pipe)
struct FvMet {
  const real *area, *rarea, *dxa, *dya, *dx, *dy, *del6_u, *del6_v;
};
static inline FvMet fv_met(const Met& m) { return FvMet{m.area, m.rarea, m.dxa, m.dya, m.dx, m.dy, m.del6_u, m.del6_v}; }

// Workgroup -> (tile, level) of the transport kernels: the map of wgmap.h (a level belongs to one XCD) at this workgroup's place
// in its launch; the emulation takes the same map
__device__ __forceinline__ FvTile fv_tile_of_workgroup() {
  const int gx = gridDim.x, gy = gridDim.y, nlev = gridDim.z;
  return fv_tile_of_linear(blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z), gx, gy, nlev);
}
int launch_delnflux(const Geo& g, const Met& m, int mode, const real* q, real* fx, real* fy,
                    const real* mass, const real* damp_k, const real* nord_k, int nmax, int mass_given,
                    int nlev, hipStream_t st);
int launch_a2b_ord4(const Geo& g, const Met& m, real* qin, real* qout, int k0, int k1, int replace, hipStream_t st);
// the same with the input tile staged in LDS (qout must not alias qin)
int launch_a2b_ord4_tiled(const Geo& g, const Met& m, const real* qin, real* qout, int k0, int k1, hipStream_t st);
// up to four fields (each with its own level range) in one pair of launches
int launch_a2b_ord4_batch(const Geo& g, const Met& m, const real* const* qin, real* const* qout, const int* k0, const int* k1,
                          int nfields, hipStream_t st);
int64_t dsw_workspace_bytes(const Geo& g);
// whether launch_d_sw can write the four transported scalars to separate buffers (pace_dsw_config_t::delp_out ...); where it can, a
// whole-d_sw call runs the winds as the fifth pass of the same kernel, and they can have buffers of their own too (u_out, v_out)
bool dsw_pingpong_supported(const Geo& g, const pace_dsw_config_t* cfg);
// what launch_d_sw accepts with this column namelist (pace_d_sw_outputs_supported): 0, or 3 = the scalars' outputs and the winds'
int dsw_outputs_supported(const Geo& g, const pace_column_t* col, const pace_dsw_config_t* cfg);
int dsw_prepare(const Geo& g, const pace_column_t* col, void* ws, hipStream_t st);
int launch_d_sw(const Geo& g, const Met& m, const pace_column_t* col, const pace_dsw_config_t* cfg, void* ws, int phases,
                const DswFields& f, hipStream_t st);
int64_t riem3_workspace_bytes(const Geo& g);
int launch_riem_solver3(const Geo& g, void* ws, int last_call, double dt, const real* cappa, double ptop,
                        const real* zs, const real* wsd, real* delz, const real* q_con, const real* delp,
                        const real* pt, real* zh, real* pe, real* ppe, real* pk3, real* pk, real* peln,
                        real* w, double p_fac, hipStream_t st);
// k_ppm.hip: XPiecewiseParabolic / YPiecewiseParabolic on a window (axis 0 = x, 1 = y)
int launch_ppm1d(const Geo& g, const Met& m, int axis, int iord, const real* q, const real* c, real* out, int i0, int j0,
                 int k0, int ni, int nj, int nk, hipStream_t st);
// k_dsw.hip: DivergenceDamping.__call__
int launch_divergence_damping(const Geo& g, const Met& m, const real* u, const real* v, const real* va, real* vort_b,
                              const real* ua, real* divg_d, real* vc, real* uc, real* delpc, real* ke,
                              const real* rel_vort_agrid, double dt, const real* d2_bg_dev, int kstart, int nonzero_nord,
                              double dddmp, double d4_bg, real* da, real* db, hipStream_t st, bool skip_dead = false,
                              bool ke_by_consumer = false, const int* ddh_tab = nullptr);
// k_riem3f.hip: both column solvers as one k-cooperative kernel (16 lanes per column), no workspace
bool riem_column_supported(const Geo& g);
int launch_riem_solver3_column(const Geo& g, int last_call, double dt, const real* cappa, double ptop, const real* zs,
                               const real* wsd, real* delz, const real* q_con, const real* delp, const real* pt,
                               real* zh, real* pe, real* ppe, real* pk3, real* pk, real* peln, real* w,
                               double p_fac, hipStream_t st);
int launch_riem_solver_c_column(const Geo& g, double dt2, const real* cappa, double ptop, const real* hs, const real* ws3,
                                const real* ptc, const real* q_con, const real* delpc, real* gz, real* pef,
                                const real* w3, double p_fac, hipStream_t st);
// k_sim1.hip: Sim1Solver as a class of its own (not the hot path)
int64_t sim1_workspace_bytes(const Geo& g);
int launch_sim1_solver(const Geo& g, void* ws, int n_halo, double dt, double p_fac, const real* gamma, const real* cp3,
                       real* pe, const real* delta_mass, const real* pm, const real* pem, real* w, real* dz,
                       const real* pt, const real* ws2d, hipStream_t st);
// k_csw.hip
int64_t csw_workspace_bytes(const Geo& g);
int launch_d2a2c_vect(const Geo& g, const Met& m, void* ws, real* uc, real* vc, const real* u, const real* v,
                      real* ua, real* va, real* utc, real* vtc, hipStream_t st);
int launch_c_sw(const Geo& g, const Met& m, void* ws, real* delpc, real* ptc, real* delp, real* pt,
                const real* u, const real* v, real* w, real* uc, real* vc, real* ua, real* va,
                real* ut, real* vt, real* divgd, real* omga, double dt2, int nord, hipStream_t st, int part = 0);
// k_riem3.hip (C-grid solver)
int64_t riemc_workspace_bytes(const Geo& g);
int launch_riem_solver_c(const Geo& g, void* ws, double dt2, const real* cappa, double ptop, const real* hs,
                         const real* ws3, const real* ptc, const real* q_con, const real* delpc, real* gz,
                         real* pef, const real* w3, double p_fac, hipStream_t st);
// k_acoustic.hip
int64_t updatedzc_workspace_bytes(const Geo& g);
int launch_updatedzc(const Geo& g, const Met& m, void* ws_, const real* dp_ref, const real* zs, const real* ut,
                     const real* vt, real* gz, real* ws, double dt, hipStream_t st);
int64_t updatedzd_workspace_bytes(const Geo& g);
int launch_updatedzd(const Geo& g, const Met& m, void* ws_, const pace_updatedzd_k_t* kc, const real* zs, real* zh,
                     const real* crx, const real* cry, const real* xfx, const real* yfx, real* wsd, double dt,
                     int hord_tm, hipStream_t st);
int launch_gz_from_surface(const Geo& g, const real* zs, const real* delz, real* gz, hipStream_t st);
int launch_scale_copy(const Geo& g, const real* src, real* dst, double factor, int scale, int halo, int nlev,
                      hipStream_t st);
int launch_p_grad_c(const Geo& g, const Met& m, real* uc, real* vc, const real* delpc, const real* pkc,
                    const real* gz, double dt2, hipStream_t st);
int64_t nh_p_grad_workspace_bytes(const Geo& g);
int launch_nh_p_grad(const Geo& g, const Met& m, void* ws_, real* u, real* v, real* pp, real* gz, real* pk3,
                     real* delp, double dt, double ptop, double akap, hipStream_t st);
int launch_edge_pe(const Geo& g, real* pe, const real* delp, double ptop, hipStream_t st);
int launch_pk3_halo(const Geo& g, real* pk3, const real* delp, double ptop, double akap, hipStream_t st);
int launch_ray_fast(const Geo& g, real* u, real* v, real* w, const double* dp, const double* pfull, double dt,
                    double ptop, double rf_cutoff, double tau, int hydrostatic, hipStream_t st);
int64_t del2cubed_workspace_bytes(const Geo& g);
int launch_del2cubed(const Geo& g, const Met& m, void* ws_, real* qdel, double cd, int nmax, hipStream_t st);
int launch_diffusive_heating(const Geo& g, const real* delp, const real* delz, const real* cappa,
                             const real* heat_source, real* pt, double delt_time_factor, int nlev, hipStream_t st);
// k_halo.hip
int launch_halo_copy(const Geo& g, const pace_halo_desc_t* descs, int ndesc, int unpack, hipStream_t st);
int launch_halo_cube(const Geo& g, const pace_halo_xfer_t* table_on_device, int n, hipStream_t st);
// k_tracer.hip
int launch_tracer_flux_compute(const Geo& g, const Met& m, const real* cx, const real* cy, real* xfx, real* yfx,
                               hipStream_t st);
int launch_tracer_divide(const Geo& g, real* cxd, real* xfx, real* mfxd, real* cyd, real* yfx, real* mfyd,
                         int n_split, hipStream_t st);
int launch_apply_mass_flux(const Geo& g, const Met& m, const real* dp1, const real* mfx, const real* mfy, real* dp2,
                           hipStream_t st);
int launch_apply_tracer_flux(const Geo& g, const Met& m, real* q, const real* dp1, const real* fx, const real* fy,
                             const real* dp2, hipStream_t st);
int launch_tracer_cmax(const Geo& g, const real* cx, const real* cy, const real* sin_sg5, double* cmax, hipStream_t st);
int launch_tracer_subcycles(const double* const* cmax, int ntiles, int nk, int max_subcycles, int32_t* out, hipStream_t st);
int launch_tracer_divide_levels(const Geo& g, real* cxd, real* xfx, real* mfxd, real* cyd, real* yfx, real* mfyd,
                                const int32_t* ksplt, hipStream_t st);
int launch_apply_mass_flux_levels(const Geo& g, const Met& m, const real* dp1, const real* mfx, const real* mfy, real* dp2,
                                  const int32_t* ksplt, int min_subcycles, hipStream_t st);
int launch_apply_tracer_flux_levels(const Geo& g, const Met& m, real* q, const real* dp1, const real* fx, const real* fy,
                                    const real* dp2, const int32_t* ksplt, int min_subcycles, hipStream_t st);
int launch_swap_dp_levels(const Geo& g, real* dp1, real* dp2, const int32_t* ksplt, int min_subcycles, hipStream_t st);
int64_t map_single_workspace_bytes(const Geo& g, int nq);
int launch_map_fields(const Geo& g, void* ws, real* const* q, int nq, const real* pe1, const real* pe2, const real* qs,
                      double qmin, int kord, int iv, int xstag, int ystag, hipStream_t st);
int launch_fillz(const Geo& g, real* const* q, int nq, const real* dp, hipStream_t st);
int launch_l2e_prepare(const Geo& g, const real* const* water, real* q_con, real* pt, real* cappa, real* delp,
                       real* delz, const real* pe, real* pe1, real* pe2, const real* ak, const real* bk, real* dp2,
                       real* ps, real* pn2, const real* peln, real* pk, double ptop, double akap, double r_vir,
                       hipStream_t st);
int launch_l2e_post(const Geo& g, const real* const* water, real* q_con, real* pkz, const real* pt, real* cappa,
                    const real* delp, real* delz, real* peln, real* pe0, const real* pn2, double r_vir, hipStream_t st);
int launch_l2e_pressures(const Geo& g, int dir, const real* pe, const real* pe1, const real* ak, const real* bk,
                         real* pe0, real* pe3, hipStream_t st);
int launch_l2e_finish(const Geo& g, const real* const* water, real* pe, const real* pe2, real* pt, const real* pkz,
                      double r_vir, int last_step, hipStream_t st);
// k_satadj.hip
int launch_sat_adjust_tables(double* tables, hipStream_t st);
int launch_sat_adjust(const Geo& g, real* const* water, real* qcld, real* te, real* pt, real* q_con, real* pkz, real* cappa,
                      const real* delp, const real* delz, const real* area, const real* hs, const double* tables,
                      const pace_sat_adjust_params_t& p, int kmp, int last_step, int consv_te, hipStream_t st);

// k_subgridz.hip
int launch_dry_convective_adjust(const Geo& g, real* const* tracers, real* pt, real* ua, real* va, real* w, real* u_dt,
                                 real* v_dt, const real* delp, const real* delz, const real* pkz, const real* peln,
                                 const real* pe, int k_sponge, double xvir, double t_max, double fv_sg_adj, double timestep,
                                 hipStream_t st);
// k_updphys.hip
int launch_fill_gfs_delp(const Geo& g, const real* delp, real* q, double q_min, hipStream_t st);
int launch_phys_thermo_pressure(const Geo& g, const real* const* water, real* pt, real* t_dt, real* pe, const real* delp,
                                real* peln, real* pk, const real* ua, const real* va, real* ps, real* u_srf, real* v_srf,
                                double dt, hipStream_t st);
int launch_update_dwinds_phys(const Geo& g, real* u, real* v, real* u_dt, real* v_dt, const real* const* vlon,
                              const real* const* vlat, const real* const* es1, const real* const* ew2, const real* edge_vect_w,
                              const real* edge_vect_e, const real* edge_vect_s, const real* edge_vect_n, double dt5,
                              hipStream_t st);
// k_microphys.hip
long microphysics_workspace_bytes(const Geo& g);
int launch_microphysics(const Geo& g, void* workspace, const real* const* in, real* wmp, real* const* tend, real* const* precip,
                        const pace_microphysics_config_t& cfg, hipStream_t st);
// k_physics.hip
int launch_copy_dycore_to_physics(const Geo& g, const real* const* in, real* const* out, hipStream_t st);
int launch_physics_prepare(const Geo& g, real* const* tracers, const real* pt, const real* delz, real* delp, const real* omga,
                           real* prsi, real* phii, real* phil, real* delprsi, real* dz, real* wmp, real* const* tendencies,
                           double ptop, int do_microphysics, hipStream_t st);
int launch_physics_update_state(const Geo& g, const real* const* x, const real* const* x_dt, real* const* out, double dt,
                                hipStream_t st);
int launch_physics_tendencies_to_dycore(const Geo& g, real* const* tendencies, const real* const* updated,
                                        const real* const* before, real* const* tracers, const real* prsi, real* delp,
                                        double rdt, hipStream_t st);
// k_driver.hip
size_t state_extrema_workspace_bytes(const Geo& g);
int launch_state_extrema(const Geo& g, const real* const* fields, const int* compute_only, int nfields, void* workspace,
                         double* out, hipStream_t st);
// k_diag.hip
int launch_diag_pack(const Geo& g, const pace_diag_item_t* items, int nitems, int out_is_double, void* out, hipStream_t st);
// k_plev.hip
int launch_plev_diag(const Geo& g, const real* peln, const double* log_p, int nlevels, const pace_plev_item_t* items, int nitems,
                     int i0, int j0, int ni, int nj, int out_is_double, void* out, hipStream_t st);
// k_gather.hip
int launch_cube_xfer(const Geo& g, const pace_cube_item_t* table_on_device, int n, int dense_is_double, void* dense, int scatter,
                     hipStream_t st);
// k_regrid.hip
int launch_cube_regrid(const Geo& g, const pace_regrid_point_t* points_on_device, int npoints,
                       const pace_regrid_item_t* items_on_device, int n, int dense_is_double, void* dense, hipStream_t st);
// k_state.hip
int launch_state_unpack(const Geo& g, const pace_unpack_item_t* items, int nitems, const double* in, hipStream_t st);
// k_restart.hip
size_t restart_pack_workspace_bytes(const pace_restart_item_t* items, int nitems);
int launch_restart_pack(const Geo& g, const pace_restart_item_t* items, int nitems, int out_type, void* out, uint64_t* sums,
                        void* workspace, hipStream_t st);
int launch_pe_peln_from_delp(const Geo& g, const real* delp, double ptop, real* pe, real* peln, hipStream_t st);
// k_ckpt.hip
long ckpt_thresholds_blocks(const pace_ckpt_item_t* items, int nitems);
long ckpt_validate_blocks(const pace_ckpt_item_t* items, int nitems);
int launch_ckpt_accumulate(const pace_ckpt_item_t* items, int nitems, int first, hipStream_t st);
int launch_ckpt_thresholds(const pace_ckpt_item_t* items, int nitems, int n_trials, void* workspace, double* out, hipStream_t st);
int launch_ckpt_validate(const pace_ckpt_item_t* items, int nitems, void* workspace, double* out, hipStream_t st);
// k_nudge.hip
int launch_nudge(const Geo& g, const pace_nudge_item_t* items, int nitems, double weight, double dt, int apply, hipStream_t st);
// k_heldsuarez.hip
int launch_held_suarez(const Geo& g, const pace_held_suarez_config_t& cfg, const real* pe, const real* ua, const real* va,
                       const real* pt, const real* sin2lat, const real* cos2lat, real* u_dt, real* v_dt, real* pt_dt, real* teq,
                       hipStream_t st);
// k_rayleigh.hip
int launch_rayleigh_super(const Geo& g, const Met& met, const real* a11, const real* a12, const real* a21, const real* a22, real* u,
                          real* v, real* w, real* pt, const double* factor, int kmax, double rcv, int conserve, hipStream_t st);
// k_energy.hip
int launch_energy_columns(const Geo& g, int mode, const real* const* water, const real* pt, const real* delp, const real* delz,
                          const real* w, const real* u, const real* v, const real* pkz, const real* phis, const real* rsin2,
                          const real* cosa_s, const real* area, real* te0_2d, real* te_2d, real* zsum1, int64_t* words,
                          double r_vir, hipStream_t st);
int launch_energy_finalize(const int64_t* const* words, int ntiles, double consv_te, double dt_atmos, double* out, hipStream_t st);
int launch_l2e_finish_dtmp(const Geo& g, const real* const* water, real* pe, const real* pe2, real* pt, const real* pkz,
                           double r_vir, const double* result, hipStream_t st);
// k_dycore.hip
int launch_fv_setup_pt(const Geo& g, real* const* water, real* q_con, real* pkz, real* pt, real* cappa,
                       const real* delp, const real* delz, real* dp1, hipStream_t st);
int launch_omega_from_w(const Geo& g, const real* delp, const real* delz, const real* w, real* omga, hipStream_t st);
int launch_neg_adj3(const Geo& g, real* const* water, real* qcld, real* pt, const real* delp, hipStream_t st);
int launch_c2l(const Geo& g, const Met& m, int order, const real* u, const real* v, const real* a11, const real* a12,
               const real* a21, const real* a22, real* ua, real* va, hipStream_t st);
// k_stencils.hip: per-stencil device implementations (pace_stencil)
int launch_stencil(const Geo& g, const Met& m, int id, void* const* fields, int nfields, const double* scalars, int nscalars,
                   const int* origin, const int* domain, hipStream_t st);
int launch_swap_dp(const Geo& g, real* dp1, real* dp2, hipStream_t st);
int launch_zero_data(const Geo& g, real* mfxd, real* mfyd, real* cxd, real* cyd, real* heat_source, real* diss_estd,
                     int first_timestep, hipStream_t st);
int launch_interface_pressure(const Geo& g, const real* delp, real* pem, double ptop, hipStream_t st);
