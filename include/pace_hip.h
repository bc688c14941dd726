/* pace_hip.h -- C ABI of libpace_hip.so: MI355X (gfx950) kernels for the FV3 acoustic substep.
 *
 * This is the drop-in boundary: each entry point replaces what the reference executes *under*
 * one of its Python classes (a chain of GT4Py FrozenStencil launches, dsl/pace/dsl/stencil.py:395-434).
 * Plain pointers and sizes only; no allocation, no global state, re-entrant per stream.  All
 * `pace_real_t*` arguments are DEVICE pointers unless stated otherwise.  Every function returns
 * PACE_OK (0) or a negative PACE_ERR_* code; nothing is written on error.
 *
 * Field layout: 3-D fields are [k][j][i], i fastest, logical shape (N+7, N+7, nz+1) with origin
 * (3,3,0) exactly as the reference allocates them (util/pace/util/initialization/sizer.py:132-155);
 * row stride `sj` (>= N+7) and level stride `sk` (>= sj*(N+7)) are given in pace_geom_t.  2-D metric
 * fields share the row stride.  K-fields are dense arrays of nk (or nk+1) doubles.
 */
#ifndef PACE_HIP_H
#define PACE_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Storage type of every DEVICE field, metric and K-array: double in libpace_hip.so, float in libpace_hip_f32.so (the same
 * sources compiled with -DPACE_REAL_FLOAT; dsl/pace/dsl/typing.py:24 -- the reference's PACE_FLOAT_PRECISION switch).  Strides
 * in pace_geom_t count elements of this type.  Scalars passed by value, HOST arrays and the arithmetic inside the kernels stay
 * double in both builds.  pace_real_bytes() tells which build a library is. */
#ifdef PACE_REAL_FLOAT
typedef float pace_real_t;
#else
typedef double pace_real_t;
#endif

#define PACE_OK 0
#define PACE_ERR_ARG (-1)
#define PACE_ERR_LAUNCH (-2)
#define PACE_ERR_UNSUPPORTED (-3)

typedef struct {
  int32_t n;   /* cells per tile edge (C<n>) */
  int32_t nk;  /* number of layers nz */
  int32_t sj;  /* row stride in doubles */
  int32_t pad_;
  int64_t sk;  /* level stride in doubles */
} pace_geom_t;

/* Read-only grid metrics, i.e. pace.util.grid.GridData / DampingCoefficients
 * (util/pace/util/grid/helper.py:21-45,306-530).  2-D device arrays with row stride sj. */
typedef struct {
  const pace_real_t *area, *rarea, *rarea_c;
  const pace_real_t *dx, *dy, *dxa, *dya, *dxc, *dyc;
  const pace_real_t *rdx, *rdy, *rdxa, *rdya, *rdxc, *rdyc;
  const pace_real_t *cosa, *rsina, *cosa_u, *cosa_v, *cosa_s;
  const pace_real_t *sina_u, *sina_v, *rsin_u, *rsin_v, *rsin2;
  const pace_real_t *sin_sg1, *sin_sg2, *sin_sg3, *sin_sg4;
  const pace_real_t *cos_sg1, *cos_sg2, *cos_sg3, *cos_sg4;
  const pace_real_t *del6_u, *del6_v, *divg_u, *divg_v;
  const pace_real_t *fC, *fC_agrid;
  const pace_real_t *edge_w, *edge_e; /* length nj, indexed by j */
  const pace_real_t *edge_s, *edge_n; /* length ni, indexed by i */
  /* a2b_ord4 corner extrapolation weights x1/(x2-x1) (a2b_ord4.py:43-56) for the corner
   * points sw(is,js), nw-stencil(ie+1,js), ne(ie+1,je+1), se-stencil(is,je+1), three diagonals
   * each, precomputed on the host from lon/lat (HOST values, copied by value). */
  double a2b_corner_w[4][3];
  double da_min, da_min_c;
} pace_metrics_t;

/* Column namelist (d_sw.get_column_namelist, fv3core/pace/fv3core/stencils/d_sw.py:633-683)
 * expanded to one value per level; HOST arrays of length nk. */
typedef struct {
  const double *nord, *nord_v, *nord_w, *nord_t;
  const double *damp_vt, *damp_w, *damp_t;
  const double *d2_divg, *d_con, *ke_bg;
  /* calc_damp (delnflux.py:21-38) = (damp_c * da)^(nord+1), evaluated by the host exactly where the
   * reference evaluates it: fac_vt = (damp_vt, da_min, nord_v), fac_t = (damp_t, da_min, nord_t) in
   * DelnFlux.__init__ (delnflux.py:1001-1003); fac_vt_c = (damp_vt, da_min_c, nord_v),
   * fac_w_c = (damp_w, da_min_c, nord_w) in d_sw.py:924-933. */
  const double *fac_vt, *fac_t, *fac_vt_c, *fac_w_c;
} pace_column_t;

/* flags of pace_dsw_config_t */
#define PACE_DSW_SKIP_DEAD_OUTPUTS 1 /* delpc, divgd, uc, vc are not brought to the state the reference leaves them in: they are
                                      * work fields of DivergenceDamping (divergence_damping.py:561-600) that c_sw recomputes before
                                      * anything reads them again (d_sw.py:1032-1033, dyn_core.py:720-852).  Their contents are
                                      * unspecified after the call, and so are the 3 x 3 corner blocks of the halo of delp, pt, w,
                                      * q_con (which the next halo update overwrites); every other value of every other argument
                                      * is unaffected, bit for bit.  This is what the acoustic loop asks for.
                                      * The default (0) is the reference's FULL contract: every argument over the whole storage as
                                      * TranslateD_SW compares it (translate_d_sw.py:36-65) -- the halo of divgd / uc / vc in the
                                      * state the damping's in-place passes and corner fills leave it (divergence_damping.py:579-600),
                                      * delpc's halo untouched, the corner blocks of the four scalars as FiniteVolumeTransport's
                                      * in-place corner copies leave them (fvtp2d.py:262-345). */

typedef struct {
  /* sizeof(pace_dsw_config_t) of the header the caller was built with: a mismatch is refused (PACE_ERR_ARG) instead of
   * reading fields the caller never set.  Zero-initialise the struct, then fill it. */
  int32_t struct_bytes;
  int32_t flags; /* PACE_DSW_* */
  int32_t hord_dp, hord_tm, hord_vt, hord_mt;
  int32_t nord;
  int32_t do_skeb;
  double dddmp, d4_bg, d_con;
  /* Optional separate outputs of the four scalars d_sw transports (all four or none; NULL = the reference's in-place update).
   * d_sw.py:148-201,331-350 overwrite delp, pt, w, q_con cell by cell while the transport of the neighbouring cells still reads
   * them -- the reference gets away with it through full-field temporaries; here one kernel does transport and update, so the
   * new values need a buffer of their own.  With outputs given (distinct from the inputs, same layout, 16-byte aligned) the
   * compute domain AND the halo of each input are written there and the inputs are left as they were: the caller swaps the
   * buffers (pace_amd: Quantity.swap_storage).  Without them the library writes to its workspace and copies back.
   * Only where pace_d_sw_pingpong_supported() says so; otherwise PACE_ERR_UNSUPPORTED. */
  pace_real_t *delp_out, *pt_out, *w_out, *q_con_out;
  /* Optional separate outputs of the D-grid winds, both or none, only together with the four above and only in calls that run
   * the whole of d_sw (pace_d_sw, pace_d_sw_overlapped, pace_d_sw_phases with 2, 4 and 8 set): u and v are then left as they were
   * and the updated winds (d_sw.py:406-477,582-608) are written to u_out / v_out, halo included -- the caller swaps the buffers.
   * The winds are updated by the kernel that transports the scalars, tile by tile, and a tile reads the old wind on the face its
   * neighbour writes.  Without them that kernel writes to the workspace and the winds are copied back. */
  pace_real_t *u_out, *v_out;
} pace_dsw_config_t;

/* ---- FiniteVolumeFluxPrep.__call__ (fv3core/pace/fv3core/stencils/fxadv.py:565-661) ---- */
int pace_fxadv(const pace_geom_t* geom, const pace_metrics_t* met, const pace_real_t* uc, const pace_real_t* vc,
               pace_real_t* crx, pace_real_t* cry, pace_real_t* x_area_flux, pace_real_t* y_area_flux,
               pace_real_t* uc_contra, pace_real_t* vc_contra, double dt, void* stream);

/* ---- XPiecewiseParabolic / YPiecewiseParabolic.__call__ (fv3core/pace/fv3core/stencils/xppm.py:290-355, yppm.py:290-355):
 * mean value of q_in advected through the x- (axis 0) or y- (axis 1) interfaces of the window origin (i0, j0, k0), domain
 * (ni, nj, nk) -- the origin / domain the reference class is constructed with.  iord in {5, 6, 8} (the sign is ignored, as
 * `mord = abs(iord)`).  Corner halos of q_in are the caller's business, as in the reference. */
int pace_ppm(const pace_geom_t* geom, const pace_metrics_t* met, int axis, int iord, const pace_real_t* q_in,
             const pace_real_t* c, pace_real_t* q_mean_advected, int i0, int j0, int k0, int ni, int nj, int nk,
             void* stream);

/* ---- DivergenceDamping.__call__ (fv3core/pace/fv3core/stencils/divergence_damping.py:482-632).  workspace: two fields
 * (pace_divergence_damping_workspace_bytes).  nord_col: HOST array of nk values (the class's nord_col K-field; the column is
 * split at its first positive entry, divergence_damping.py:307-331); d2_bg: DEVICE array of nk values.  In place, as the
 * reference: divg_d, uc, vc are work fields and end as the last iteration leaves them, delpc and damped_rel_vort_bgrid are
 * outputs, ke += damping. */
int64_t pace_divergence_damping_workspace_bytes(const pace_geom_t* geom);
int pace_divergence_damping(const pace_geom_t* geom, const pace_metrics_t* met, void* workspace, const pace_real_t* u,
                            const pace_real_t* v, const pace_real_t* va, pace_real_t* damped_rel_vort_bgrid,
                            const pace_real_t* ua, pace_real_t* divg_d, pace_real_t* vc, pace_real_t* uc,
                            pace_real_t* delpc, pace_real_t* ke, const pace_real_t* rel_vort_agrid, double dt,
                            const double* nord_col_host, const pace_real_t* d2_bg_dev, double dddmp, double d4_bg,
                            int nord, void* stream);

/* ---- FiniteVolumeTransport.__call__ without damping (fvtp2d.py:262-345).  x/y_mass_flux may be
 * NULL (area fluxes are used as unit fluxes).  hord in {5, 6, 8}.  nlev = number of levels
 * processed (nk, or nk+1 for interface fields).  q's corner halos are NOT rewritten: corner reads
 * go through the copy_corners index map, which yields identical fluxes. */
int pace_fvtp2d(const pace_geom_t* geom, const pace_metrics_t* met, const pace_real_t* q, const pace_real_t* crx,
                const pace_real_t* cry, const pace_real_t* x_area_flux, const pace_real_t* y_area_flux,
                pace_real_t* q_x_flux, pace_real_t* q_y_flux, const pace_real_t* x_mass_flux,
                const pace_real_t* y_mass_flux, int hord, int nlev, void* stream);

/* ---- The fused form d_sw uses for q_con and pt (d_sw.py:1075-1117): FiniteVolumeTransport with mass fluxes AND its
 * DelnFlux(mass = delp) (fvtp2d.py:262-345), followed by apply_fluxes (d_sw.py:122-145):
 *   qout = q * delp + flux_increment(q_x_flux, q_y_flux) * rarea      on the compute domain,
 * in ONE kernel; the flux fields never reach memory.  damp_k / nord_k as for pace_delnflux.  qout must not alias q. */
int pace_fvtp2d_update(const pace_geom_t* geom, const pace_metrics_t* met, const pace_real_t* q,
                       const pace_real_t* crx, const pace_real_t* cry, const pace_real_t* x_area_flux,
                       const pace_real_t* y_area_flux, const pace_real_t* x_mass_flux, const pace_real_t* y_mass_flux,
                       const pace_real_t* delp, const pace_real_t* damp_k, const pace_real_t* nord_k, int nmax,
                       pace_real_t* qout, int hord, int nlev, void* stream);

/* ---- DelnFluxNoSG.__call__ (delnflux.py:1050-1261): damping fluxes fx2, fy2 of q.
 * nord_k, damp_k: DEVICE arrays, one entry per level (see DESIGN.md for how the reference's
 * nord0..nord3 externals map to per-level values).  If mass_given != 0, d2 starts from q
 * (copy_stencil_interval) instead of damp*q.  nmax = max(nord_k). */
int pace_delnflux_nosg(const pace_geom_t* geom, const pace_metrics_t* met, const pace_real_t* q, pace_real_t* fx2,
                       pace_real_t* fy2, const pace_real_t* damp_k, const pace_real_t* nord_k, int nmax,
                       int mass_given, int nlev, void* stream);

/* ---- DelnFlux.__call__ (delnflux.py:945-1047): fx, fy += damping flux (mass-weighted if
 * mass != NULL).  damp_k = (damp_c*da_min)^(nord+1) per level (calc_damp, delnflux.py:21-38). */
int pace_delnflux(const pace_geom_t* geom, const pace_metrics_t* met, const pace_real_t* q, pace_real_t* fx,
                  pace_real_t* fy, const pace_real_t* mass, const pace_real_t* damp_k, const pace_real_t* nord_k,
                  int nmax, int nlev, void* stream);

/* ---- AGrid2BGridFourthOrder.__call__ (a2b_ord4.py:668-761) on levels [k0, k1). ---- */
int pace_a2b_ord4(const pace_geom_t* geom, const pace_metrics_t* met, pace_real_t* qin, pace_real_t* qout, int k0,
                  int k1, int replace, void* stream);

/* ---- DGridShallowWaterLagrangianDynamics.__call__ (d_sw.py:935-1237).
 * workspace: DEVICE scratch of pace_d_sw_workspace_bytes() bytes, owned by the caller for the
 * object's lifetime (the reference allocates its temporaries in __init__, d_sw.py:765-784);
 * it also carries uc_contra / vc_contra between calls.  col holds HOST arrays. */
int64_t pace_d_sw_workspace_bytes(const pace_geom_t* geom);
/* 1 if pace_d_sw* accept separate outputs (pace_dsw_config_t::delp_out ...) for this geometry and these orders, else 0. */
int pace_d_sw_pingpong_supported(const pace_geom_t* geom, const pace_dsw_config_t* cfg);
/* 1 if whole-d_sw calls also accept separate outputs of the winds (pace_dsw_config_t::u_out, v_out) -- the library then updates
 * the winds in the kernel that transports the scalars, and pace_d_sw_overlapped has nothing left for its side stream --, else 0.
 * (The damping orders nord_v, nord_w, nord_t of the column namelist must be <= 2, as get_column_namelist makes them,
 * d_sw.py:633-683; otherwise the call returns PACE_ERR_UNSUPPORTED.) */
int pace_d_sw_wind_outputs_supported(const pace_geom_t* geom, const pace_dsw_config_t* cfg);
/* The two queries above AND the condition on the column namelist in one call (what pace_d_sw* really accepts for this object):
 * 0 = no separate outputs, 1 = the four scalars', 3 = the scalars' and the winds' (this library answers 0 or 3: the kernel that
 * gives the scalars outputs of their own takes the winds too).  col: the HOST arrays given to pace_d_sw_prepare
 * (get_column_namelist, d_sw.py:633-683). */
int pace_d_sw_outputs_supported(const pace_geom_t* geom, const pace_column_t* col, const pace_dsw_config_t* cfg);
/* Once per object, after zero-filling the workspace: uploads the column namelist (synchronises). */
int pace_d_sw_prepare(const pace_geom_t* geom, const pace_column_t* col, void* workspace, void* stream);
int pace_d_sw(const pace_geom_t* geom, const pace_metrics_t* met, const pace_column_t* col,
              const pace_dsw_config_t* cfg, void* workspace, pace_real_t* delpc, pace_real_t* delp, pace_real_t* pt,
              pace_real_t* u, pace_real_t* v, pace_real_t* w, pace_real_t* uc, pace_real_t* vc, const pace_real_t* ua,
              const pace_real_t* va, pace_real_t* divgd, pace_real_t* mfx, pace_real_t* mfy, pace_real_t* cx,
              pace_real_t* cy, pace_real_t* crx, pace_real_t* cry, pace_real_t* xfx, pace_real_t* yfx,
              pace_real_t* q_con, const pace_real_t* zh, pace_real_t* heat_source, pace_real_t* diss_est, double dt,
              void* stream);

/* The two halves of pace_d_sw, same arguments.  pace_d_sw_transport: flux preparation and the transport of delp, w,
 * q_con, pt (d_sw.py:935-1117) -- everything updatedzd / riem_solver3 read.  pace_d_sw_winds: the rest
 * (d_sw.py:1119-1237); it reads only what the first half left behind, so it may be launched on a second stream
 * and run concurrently with the vertical solver.  pace_d_sw == transport followed by winds on one stream. */
int pace_d_sw_transport(const pace_geom_t* geom, const pace_metrics_t* met, const pace_column_t* col,
                        const pace_dsw_config_t* cfg, void* workspace, pace_real_t* delpc, pace_real_t* delp,
                        pace_real_t* pt, pace_real_t* u, pace_real_t* v, pace_real_t* w, pace_real_t* uc,
                        pace_real_t* vc, const pace_real_t* ua, const pace_real_t* va, pace_real_t* divgd,
                        pace_real_t* mfx, pace_real_t* mfy, pace_real_t* cx, pace_real_t* cy, pace_real_t* crx,
                        pace_real_t* cry, pace_real_t* xfx, pace_real_t* yfx, pace_real_t* q_con,
                        const pace_real_t* zh, pace_real_t* heat_source, pace_real_t* diss_est, double dt,
                        void* stream);
int pace_d_sw_winds(const pace_geom_t* geom, const pace_metrics_t* met, const pace_column_t* col,
                    const pace_dsw_config_t* cfg, void* workspace, pace_real_t* delpc, pace_real_t* delp,
                    pace_real_t* pt, pace_real_t* u, pace_real_t* v, pace_real_t* w, pace_real_t* uc, pace_real_t* vc,
                    const pace_real_t* ua, const pace_real_t* va, pace_real_t* divgd, pace_real_t* mfx,
                    pace_real_t* mfy, pace_real_t* cx, pace_real_t* cy, pace_real_t* crx, pace_real_t* cry,
                    pace_real_t* xfx, pace_real_t* yfx, pace_real_t* q_con, const pace_real_t* zh,
                    pace_real_t* heat_source, pace_real_t* diss_est, double dt, void* stream);

/* Finer split for callers that overlap on two streams (same arguments after `phases`).  Bit mask: 1 = flux preparation
 * (fxadv), 2 = transport of delp, w, q_con, pt, 4 = winds A (kinetic energy ... vorticity damping fluxes), 8 = winds B
 * (dissipative heating, final u/v update).  2 and 4 depend only on 1 and use disjoint workspace fields; 8 needs 2 and
 * 4.  pace_d_sw_transport == phases 3, pace_d_sw_winds == phases 12, pace_d_sw == 15.  Instead of 1: 16 = the part of the flux
 * preparation that reads no halo value of uc / vc (the box [is+2, ie-1] x [js+2, je-1]) -- it may run while the uc / vc halo
 * exchange is in flight (dyn_core.py:817-820) --, 32 = the rest of it, after the exchange.  Instead of 4: 64 = kinetic energy and
 * relative vorticity (they need only the flux preparation), 128 = the rest of winds A.
 * Where pace_d_sw_wind_outputs_supported() and the call runs 2, 4 and 8 together, the library orders the work differently: kinetic
 * energy, vorticity and divergence damping first, then ONE kernel that transports the scalars and the vorticity, updates the
 * winds and forms the dissipative heating.  256 (alone; a measurement aid): only that kernel, on the kinetic energy /
 * vorticities a previous call left in the workspace. */
int pace_d_sw_phases(int phases, const pace_geom_t* geom, const pace_metrics_t* met, const pace_column_t* col,
                     const pace_dsw_config_t* cfg, void* workspace, pace_real_t* delpc, pace_real_t* delp,
                     pace_real_t* pt, pace_real_t* u, pace_real_t* v, pace_real_t* w, pace_real_t* uc,
                     pace_real_t* vc, const pace_real_t* ua, const pace_real_t* va, pace_real_t* divgd,
                     pace_real_t* mfx, pace_real_t* mfy, pace_real_t* cx, pace_real_t* cy, pace_real_t* crx,
                     pace_real_t* cry, pace_real_t* xfx, pace_real_t* yfx, pace_real_t* q_con, const pace_real_t* zh,
                     pace_real_t* heat_source, pace_real_t* diss_est, double dt, void* stream);

/* The same four phases in ONE call, the wind half on `side_stream` (prep: 1 = the whole flux preparation, 32 = its frame after
 * phases 16): flux preparation and scalars on `stream`, winds A on the side stream after the preparation, winds B there after the
 * scalars.  The three events are the caller's (hipEvent_t; e.g. torch.cuda.Event.cuda_event); ev_done is recorded on the side
 * stream at the end -- the caller's stream must wait for it before u, v, uc, vc, heat_source, diss_est, delpc or divgd are used. */
int pace_d_sw_overlapped(int prep, const pace_geom_t* geom, const pace_metrics_t* met, const pace_column_t* col,
                     const pace_dsw_config_t* cfg, void* workspace, pace_real_t* delpc, pace_real_t* delp,
                     pace_real_t* pt, pace_real_t* u, pace_real_t* v, pace_real_t* w, pace_real_t* uc,
                     pace_real_t* vc, const pace_real_t* ua, const pace_real_t* va, pace_real_t* divgd,
                     pace_real_t* mfx, pace_real_t* mfy, pace_real_t* cx, pace_real_t* cy, pace_real_t* crx,
                     pace_real_t* cry, pace_real_t* xfx, pace_real_t* yfx, pace_real_t* q_con, const pace_real_t* zh,
                     pace_real_t* heat_source, pace_real_t* diss_est, double dt, void* stream,
                         void* side_stream, void* ev_prep, void* ev_scalars, void* ev_done);

/* ---- NonhydrostaticVerticalSolver.__call__ (riem_solver3.py:208-321), compute domain.
 * zs, ws: 2-D.  workspace: pace_riem_solver3_workspace_bytes() bytes of DEVICE scratch. */
int64_t pace_riem_solver3_workspace_bytes(const pace_geom_t* geom);
int pace_riem_solver3(const pace_geom_t* geom, void* workspace, int last_call, double dt, const pace_real_t* cappa,
                      double ptop, const pace_real_t* zs, const pace_real_t* ws, pace_real_t* delz,
                      const pace_real_t* q_con, const pace_real_t* delp, const pace_real_t* pt, pace_real_t* zh,
                      pace_real_t* pe, pace_real_t* ppe, pace_real_t* pk3, pace_real_t* pk, pace_real_t* peln,
                      pace_real_t* w, double p_fac, void* stream);

/* ---- CGridShallowWaterDynamics.__call__ (fv3core/pace/fv3core/stencils/c_sw.py:599-766), including
 * DGrid2AGrid2CGridVectors (d2a2c_vect.py:529-655).  delpc / ptc are the class attributes the reference
 * exposes (c_sw.py:497-502, read by dyn_core.py:795-800).  workspace: pace_c_sw_workspace_bytes().
 * delp, pt, w are inputs -- except the two cells next to each corner of the tile's halo, which end as the reference's in-place
 * corner fills of the C-grid transport leave them (c_sw.py:483-600; TranslateC_SW compares the three over the whole storage). */
int64_t pace_c_sw_workspace_bytes(const pace_geom_t* geom);
int pace_c_sw(const pace_geom_t* geom, const pace_metrics_t* met, void* workspace, pace_real_t* delpc,
              pace_real_t* ptc, pace_real_t* delp, pace_real_t* pt, const pace_real_t* u,
              const pace_real_t* v, pace_real_t* w, pace_real_t* uc, pace_real_t* vc, pace_real_t* ua,
              pace_real_t* va, pace_real_t* ut, pace_real_t* vt, pace_real_t* divgd, pace_real_t* omga, double dt2,
              int nord, void* stream);
/* The same in two parts around the u / v halo exchange in front of c_sw (dyn_core.py:744-745; an extension for overlapping
 * that exchange with compute): part 1 = the points of its first pass that read no halo value of u / v (the box
 * [is+1, ie-1] x [js+1, je-1]); part 2 = everything else, after the exchange; part 0 = pace_c_sw.  Same arguments. */
int pace_c_sw_part(int part, const pace_geom_t* geom, const pace_metrics_t* met, void* workspace, pace_real_t* delpc,
                   pace_real_t* ptc, pace_real_t* delp, pace_real_t* pt, const pace_real_t* u,
                   const pace_real_t* v, pace_real_t* w, pace_real_t* uc, pace_real_t* vc, pace_real_t* ua,
                   pace_real_t* va, pace_real_t* ut, pace_real_t* vt, pace_real_t* divgd, pace_real_t* omga,
                   double dt2, int nord, void* stream);
/* ---- DGrid2AGrid2CGridVectors.__call__ alone (d2a2c_vect.py:529-655), dord4 = True; same workspace. */
int pace_d2a2c_vect(const pace_geom_t* geom, const pace_metrics_t* met, void* workspace, pace_real_t* uc,
                    pace_real_t* vc, const pace_real_t* u, const pace_real_t* v, pace_real_t* ua, pace_real_t* va,
                    pace_real_t* utc, pace_real_t* vtc, void* stream);

/* ---- Sim1Solver.__call__ (sim1_solver.py:144-219) as a class of its own: the semi-implicit vertical solver on the compute
 * domain widened by n_halo (the reference builds it with n_halo = 0 for riem_solver3 and 1 for riem_solver_c).  gamma, cp3,
 * delta_mass, pm, pem, potential_temperature in; pe out (nk + 1 interfaces); w, dz inout; ws 2-D.  workspace:
 * pace_sim1_solver_workspace_bytes.  Inside pace_riem_solver3 / pace_riem_solver_c the same arithmetic runs fused. */
int64_t pace_sim1_solver_workspace_bytes(const pace_geom_t* geom);
int pace_sim1_solver(const pace_geom_t* geom, void* workspace, int n_halo, double dt, double p_fac,
                     const pace_real_t* gamma, const pace_real_t* cp3, pace_real_t* pe, const pace_real_t* delta_mass,
                     const pace_real_t* pm, const pace_real_t* pem, pace_real_t* w, pace_real_t* dz,
                     const pace_real_t* potential_temperature, const pace_real_t* ws, void* stream);

/* ---- NonhydrostaticVerticalSolverCGrid.__call__ (riem_solver_c.py:160-250), compute domain +- 1. */
int64_t pace_riem_solver_c_workspace_bytes(const pace_geom_t* geom);
int pace_riem_solver_c(const pace_geom_t* geom, void* workspace, double dt2, const pace_real_t* cappa, double ptop,
                       const pace_real_t* hs, const pace_real_t* ws, const pace_real_t* ptc, const pace_real_t* q_con,
                       const pace_real_t* delpc, pace_real_t* gz, pace_real_t* pef, const pace_real_t* w3,
                       double p_fac, void* stream);

/* ---- UpdateGeopotentialHeightOnCGrid.__call__ (updatedzc.py:172-207).  dp_ref: DEVICE K-array (nk). */
int64_t pace_updatedzc_workspace_bytes(const pace_geom_t* geom);
int pace_updatedzc(const pace_geom_t* geom, const pace_metrics_t* met, void* workspace, const pace_real_t* dp_ref,
                   const pace_real_t* zs, const pace_real_t* ut, const pace_real_t* vt, pace_real_t* gz,
                   pace_real_t* ws, double dt, void* stream);

/* ---- UpdateHeightOnDGrid.__call__ (updatedzd.py:281-356).  K-dependent constants: gk/beta/gamma from
 * cubic_spline_interpolation_constants (updatedzd.py:129-154) as DEVICE arrays of nk, the four scalars the
 * interpolation stencil derives from them (:180-192), and the DelnFluxNoSG column arguments on nk+1 levels
 * (damp = column_namelist["damp_vt"], nord = nord_v expanded per level), DEVICE arrays. */
typedef struct {
  const pace_real_t *gk, *beta, *gamma;
  double xt1_top, a_bot, xt1_bot, xt2_bot;
  const pace_real_t *damp, *nord;
  int32_t nmax, pad_;
} pace_updatedzd_k_t;
int64_t pace_updatedzd_workspace_bytes(const pace_geom_t* geom);
int pace_updatedzd(const pace_geom_t* geom, const pace_metrics_t* met, void* workspace, const pace_updatedzd_k_t* kc,
                   const pace_real_t* surface_height, pace_real_t* height, const pace_real_t* courant_number_x,
                   const pace_real_t* courant_number_y, const pace_real_t* x_area_flux,
                   const pace_real_t* y_area_flux, pace_real_t* ws, double dt, int hord_tm, void* stream);

/* ---- dyn_core.py stencils: gz_from_surface_height_and_thicknesses (:83-96, compute domain),
 * compute_geopotential (:115-117, halo 2, nk+1 levels), basic.copy_defn as used at dyn_core.py:773-781
 * (full domain, nk+1 levels), p_grad_c_stencil (:120-171, hydrostatic = False). */
int pace_zero_data(const pace_geom_t* geom, pace_real_t* mfxd, pace_real_t* mfyd, pace_real_t* cxd, pace_real_t* cyd,
                   pace_real_t* heat_source, pace_real_t* diss_estd, int first_timestep, void* stream);  /* dyn_core.py:51-80 */
int pace_interface_pressure_from_toa_pressure_and_thickness(const pace_geom_t* geom, const pace_real_t* delp,
                                                            pace_real_t* pem, double ptop, void* stream);  /* :99-112 */
int pace_gz_from_surface_height_and_thicknesses(const pace_geom_t* geom, const pace_real_t* zs,
                                                const pace_real_t* delz, pace_real_t* gz, void* stream);
int pace_compute_geopotential(const pace_geom_t* geom, const pace_real_t* zh, pace_real_t* gz, void* stream);
int pace_copy(const pace_geom_t* geom, const pace_real_t* src, pace_real_t* dst, void* stream);
int pace_p_grad_c(const pace_geom_t* geom, const pace_metrics_t* met, pace_real_t* uc, pace_real_t* vc,
                  const pace_real_t* delpc, const pace_real_t* pkc, const pace_real_t* gz, double dt2, void* stream);

/* ---- NonHydrostaticPressureGradient.__call__ (nh_p_grad.py:187-255). */
int64_t pace_nh_p_grad_workspace_bytes(const pace_geom_t* geom);
int pace_nh_p_grad(const pace_geom_t* geom, const pace_metrics_t* met, void* workspace, pace_real_t* u,
                   pace_real_t* v, pace_real_t* pp, pace_real_t* gz, pace_real_t* pk3, pace_real_t* delp, double dt,
                   double ptop, double akap, void* stream);

/* ---- pe_halo.edge_pe (pe_halo.py:6-34) and PK3Halo.__call__ (pk3_halo.py:55-69). */
int pace_edge_pe(const pace_geom_t* geom, pace_real_t* pe, const pace_real_t* delp, double ptop, void* stream);
int pace_pk3_halo(const pace_geom_t* geom, pace_real_t* pk3, const pace_real_t* delp, double ptop, double akap,
                  void* stream);

/* ---- RayleighDamping.__call__ (ray_fast.py:186-206).  dp, pfull: HOST K-arrays (nk). */
int pace_ray_fast(const pace_geom_t* geom, pace_real_t* u, pace_real_t* v, pace_real_t* w, const double* dp,
                  const double* pfull, double dt, double ptop, double rf_cutoff, double tau, int hydrostatic,
                  void* stream);

/* ---- HyperdiffusionDamping.__call__ (del2cubed.py:168-194) and apply_diffusive_heating
 * (temperature_adjust.py:8-43, first nlev levels of the compute domain). */
int64_t pace_del2cubed_workspace_bytes(const pace_geom_t* geom);
int pace_del2cubed(const pace_geom_t* geom, const pace_metrics_t* met, void* workspace, pace_real_t* qdel, double cd,
                   int nmax, void* stream);
int pace_apply_diffusive_heating(const pace_geom_t* geom, const pace_real_t* delp, const pace_real_t* delz,
                                 const pace_real_t* cappa, const pace_real_t* heat_source, pace_real_t* pt,
                                 double delt_time_factor, int nlev, void* stream);

/* ---- TracerAdvection (Fortran tracer_2d_1l): the stencils around FiniteVolumeTransport(hord = 8) in
 * fv3core/pace/fv3core/stencils/tracer_2d_1l.py -- flux_compute (:19-77), divide_fluxes_by_n_substeps (:80-106),
 * apply_mass_flux (:115-135), apply_tracer_flux (:138-158), swap_dp (:166-170).  The transport itself is pace_fvtp2d
 * with hord = 8 (monotone PPM, xppm.py:76-145,185-287). */
int pace_tracer_flux_compute(const pace_geom_t* geom, const pace_metrics_t* met, const pace_real_t* cx,
                             const pace_real_t* cy, pace_real_t* xfx, pace_real_t* yfx, void* stream);
int pace_tracer_divide_fluxes(const pace_geom_t* geom, pace_real_t* cxd, pace_real_t* xfx, pace_real_t* mfxd,
                              pace_real_t* cyd, pace_real_t* yfx, pace_real_t* mfyd, int n_split, void* stream);
int pace_apply_mass_flux(const pace_geom_t* geom, const pace_metrics_t* met, const pace_real_t* dp1,
                         const pace_real_t* x_mass_flux, const pace_real_t* y_mass_flux, pace_real_t* dp2,
                         void* stream);
int pace_apply_tracer_flux(const pace_geom_t* geom, const pace_metrics_t* met, pace_real_t* q, const pace_real_t* dp1,
                           const pace_real_t* fx, const pace_real_t* fy, const pace_real_t* dp2, void* stream);
int pace_swap_dp(const pace_geom_t* geom, pace_real_t* dp1, pace_real_t* dp2, void* stream);

/* ---- Courant-number sub-cycling per level (the Fortran tracer_2d_1L: mp_reduce_max(cmax, npz), level k sub-cycled
 * int(1. + cmax(k)) times; the reference fixes cmax = 2.0 and keeps the two cmax stencils, tracer_2d_1l.py:103-112, and their
 * call site, :312-339, commented out).  Both storage types; every operation is double on the stored values (the float32 library
 * widens first; exact).  Nothing here is sensitive to FMA contraction: fabs, comparisons, one add, one subtract, one reciprocal.
 *
 * pace_tracer_cmax: ONE launch per tile.  cx, cy share the storage geometry of geom, sin_sg5 is a plane of the same row stride,
 * cmax is nk doubles on the device, which the caller zeroes before the launch.  For every level k = 0 .. nk - 1, cmax[k] becomes
 * the maximum of its old value and, over the cells i = 3 .. n + 2, j = 3 .. n + 2 of the compute domain ONLY -- not column n + 3
 * of cx, not row n + 3 of cy, no halo --, of
 *   m                             for k < nk / 6 - 1     (integer division: the Fortran's "k < npz/6", k counted from 1)
 *   (m + 1.0) - sin_sg5[i,j]      otherwise,             m = max(|cx[i,j,k]|, |cy[i,j,k]|)
 * (the reference's commented draft takes one more plain level; this is the Fortran's split).  Every value is >= 0, so the
 * maximum is taken on the bit patterns as unsigned 64-bit integers -- a fold over the workgroup, then one integer atomic maximum
 * per workgroup and level: exact, bitwise the same for every order and launch shape.  A NaN (its sign cleared) orders above
 * infinity: a NaN of cx, cy or sin_sg5 in the window reaches cmax[k].  No workspace.  Nothing outside cmax[0 .. nk - 1] is
 * written; nothing outside the two fields' and the plane's compute windows is read.
 * PACE_ERR_ARG: a NULL argument, cmax the same array as an input.
 *
 * pace_tracer_subcycles: ONE launch for any number of tiles (1 .. PACE_TRACER_MAX_TILES).  cmax_tables: HOST array of ntiles
 * device pointers, each to a tile's nk doubles; out: nk + 2 int32 on the device.
 *   out[2 + k] = (int)(1.0 + c),  c = the maximum over the tiles of cmax[k], the sum and the truncation in double exactly so
 *                (c = nextafter(1, 0) gives 2: the sum rounds to 2.0);
 *                0 if c is a NaN, infinite, below zero, or the result would exceed max_subcycles
 *   out[0]     = the largest entry,   out[1] = the number of levels set to 0
 * PACE_ERR_ARG: NULL cmax_tables, entry or out, ntiles out of range, nk outside 1 .. PACE_TRACER_MAX_LEVELS, max_subcycles
 * outside 1 .. PACE_TRACER_MAX_SUBCYCLES, out the same array as a table.
 *
 * pace_tracer_divide_fluxes_levels: pace_tracer_divide_fluxes with frac = 1.0 / ksplt[k] read per level from the device (ksplt:
 * nk int32), over the same planes -- the whole storage plane of the levels 0 .. nk - 1.  A level with ksplt[k] == 1 (or a refused
 * one, 0) is neither read nor written.
 *
 * pace_apply_mass_flux_levels, pace_apply_tracer_flux_levels, pace_swap_dp_levels: the three compute-domain stencils above -- the
 * same expressions, casts included -- on the levels with ksplt[k] >= min_subcycles only; the test is uniform over a workgroup
 * and precedes every field access.
 * PACE_ERR_ARG of the four: a NULL argument, min_subcycles < 1, ksplt or an input the same array as an output, dp1 == dp2 of
 * the swap.
 *
 * The transport has no such form: a level's transport depends on that level alone and levels are the slowest storage axis, so a
 * run of consecutive levels k0 .. k0 + nlev - 1 is pace_fvtp2d with every field pointer advanced by k0 * sk elements. */
#define PACE_TRACER_MAX_TILES 64
#define PACE_TRACER_MAX_LEVELS 4096
#define PACE_TRACER_MAX_SUBCYCLES 1024
int pace_tracer_cmax(const pace_geom_t* geom, const pace_real_t* cx, const pace_real_t* cy, const pace_real_t* sin_sg5,
                     double* cmax, void* stream);
int pace_tracer_subcycles(const double* const* cmax_tables, int ntiles, int nk, int max_subcycles, int32_t* out, void* stream);
int pace_tracer_divide_fluxes_levels(const pace_geom_t* geom, pace_real_t* cxd, pace_real_t* xfx, pace_real_t* mfxd,
                                     pace_real_t* cyd, pace_real_t* yfx, pace_real_t* mfyd, const int32_t* ksplt, void* stream);
int pace_apply_mass_flux_levels(const pace_geom_t* geom, const pace_metrics_t* met, const pace_real_t* dp1,
                                const pace_real_t* x_mass_flux, const pace_real_t* y_mass_flux, pace_real_t* dp2,
                                const int32_t* ksplt, int min_subcycles, void* stream);
int pace_apply_tracer_flux_levels(const pace_geom_t* geom, const pace_metrics_t* met, pace_real_t* q, const pace_real_t* dp1,
                                  const pace_real_t* fx, const pace_real_t* fy, const pace_real_t* dp2, const int32_t* ksplt,
                                  int min_subcycles, void* stream);
int pace_swap_dp_levels(const pace_geom_t* geom, pace_real_t* dp1, pace_real_t* dp2, const int32_t* ksplt, int min_subcycles,
                        void* stream);

/* ---- MapSingle (Fortran map_single / map1_ppm / map_scalar): fv3core/pace/fv3core/stencils/map_single.py:96-200 with
 * RemapProfile (cs_profile), remap_profile.py:566-681.  q1 is remapped in place from the nk layers bounded by the
 * interface values pe1 to those bounded by pe2 (both nk + 1 levels; pressure or log-pressure -- remapping.py:587-627).
 * kord: 9 or 10 (sign ignored, as the reference takes abs); iv: the reference's `mode` (-2 vertical velocity -- needs the
 * bottom value qs, a 2-D field --, -1 winds, 0 positive-definite tracers, 1 others, 2 as remap_profile.py:387-395).
 * xstag / ystag: the field is staggered in x / y and owns one more column / row (`dims` of the reference's constructor).
 * workspace: pace_map_single_workspace_bytes() of device memory (5 fields; the reference keeps 14). */
int64_t pace_map_single_workspace_bytes(const pace_geom_t* geom);
int pace_map_single(const pace_geom_t* geom, void* workspace, pace_real_t* q1, const pace_real_t* pe1,
                    const pace_real_t* pe2, const pace_real_t* qs, double qmin, int kord, int iv, int xstag,
                    int ystag, void* stream);

/* MapNTracer (Fortran mapn_tracer): fv3core/pace/fv3core/stencils/mapn_tracer.py:13-82 -- nq (<= 16) tracers that share
 * pe1 / pe2 are remapped (iv = 0, one kord) by ONE three-launch sequence instead of nq MapSingle calls.  tracers is a
 * HOST array of nq device pointers.  workspace: pace_mapn_tracer_workspace_bytes(geom, nq). */
int64_t pace_mapn_tracer_workspace_bytes(const pace_geom_t* geom, int nq);
int pace_mapn_tracer(const pace_geom_t* geom, void* workspace, pace_real_t* const* tracers, int nq,
                     const pace_real_t* pe1, const pace_real_t* pe2, int kord, void* stream);

/* FillNegativeTracerValues (Fortran fillz): fv3core/pace/fv3core/stencils/fillz.py:120-163 -- negative tracer masses
 * borrow from the layers above / below, then the column is rescaled; all nq tracers in one launch.  tracers: HOST array
 * of nq device pointers; dp2: layer thicknesses. */
int pace_fillz(const pace_geom_t* geom, pace_real_t* const* tracers, int nq, const pace_real_t* dp2, void* stream);

/* ---- LagrangianToEulerian: the stencils around the remaps (fv3core/pace/fv3core/stencils/remapping.py:286-695 calls them
 * in this order; pace_amd/fv3core/stencils/remapping.py is the host sequence).  Non-hydrostatic, kord_tm < 0; the saturation
 * adjustment is pace_sat_adjust below.  water: HOST array of the six device pointers qvapor, qliquid, qrain, qsnow, qice, qgraupel; ak / bk: device
 * arrays of nk + 1 hybrid coefficients; ps: 2-D field.
 *   pace_l2e_prepare   = init_pe (:42-56) + moist_cv_pt_pressure (:85-171) + pn2_pk_delp (:174-193)
 *   pace_l2e_post      = undo_delz_adjust_and_copy_peln (:59-80) + moist_cv.moist_pkz (moist_cv.py:130-172)
 *   pace_l2e_pressures = pressures_mapu (dir 0, :196-227) / pressures_mapv (dir 1, :230-254)
 *   pace_l2e_finish    = update_ua + copy_from_below (:257-283), then moist_pt_last_step (moist_cv.py:84-122, last_step
 *                        != 0) or adjust_divide_stencil (pt / pkz) */
int pace_l2e_prepare(const pace_geom_t* geom, const pace_real_t* const* water, pace_real_t* q_con, pace_real_t* pt,
                     pace_real_t* cappa, pace_real_t* delp, pace_real_t* delz, const pace_real_t* pe,
                     pace_real_t* pe1, pace_real_t* pe2, const pace_real_t* ak, const pace_real_t* bk,
                     pace_real_t* dp2, pace_real_t* ps, pace_real_t* pn2, const pace_real_t* peln, pace_real_t* pk,
                     double ptop, double akap, double r_vir, void* stream);
int pace_l2e_post(const pace_geom_t* geom, const pace_real_t* const* water, pace_real_t* q_con, pace_real_t* pkz,
                  const pace_real_t* pt, pace_real_t* cappa, const pace_real_t* delp, pace_real_t* delz,
                  pace_real_t* peln, pace_real_t* pe0, const pace_real_t* pn2, double r_vir, void* stream);
int pace_l2e_pressures(const pace_geom_t* geom, int dir, const pace_real_t* pe, const pace_real_t* pe1,
                       const pace_real_t* ak, const pace_real_t* bk, pace_real_t* pe0, pace_real_t* pe3,
                       void* stream);
int pace_l2e_finish(const pace_geom_t* geom, const pace_real_t* const* water, pace_real_t* pe, const pace_real_t* pe2,
                    pace_real_t* pt, const pace_real_t* pkz, double r_vir, int last_step, void* stream);

/* ---- The total-energy fixer (consv_te > 0; the Fortran FV3's compute_total_energy and the consv > consv_min block of
 * Lagrangian_to_Eulerian: non-hydrostatic, MOIST_CAPPA / USE_COND, nwat = 6.  The reference carries te_2d / te0_2d and dtmp
 * and stops at the global sum).  Both storage types; every operation is double on the stored values (the float32 library
 * widens first; exact), without FMA, without a reciprocal, without a transcendental.
 *
 * pace_energy_columns: ONE launch.  water: HOST array of the six device pointers qvapor, qliquid, qrain, qsnow, qice, qgraupel;
 * pt, delp, delz, w, u, v, pkz share the storage geometry of geom; phis, rsin2, cosa_s, area, te0_2d, te_2d, zsum1 are planes of
 * the same row stride.  For every column (i, j) of the compute domain -- origin (3, 3), extent (n, n) -- one pass from the bottom
 * level up, k = nk - 1 ... 0, in this order:
 *   phi_below = phis[i,j]                         before the first level
 *   phi_above = phi_below - GRAV * delz[k]
 *   ke   = (0.5 * rsin2) * ((((u0 * u0 + u1 * u1) + v0 * v0) + v1 * v1) - ((u0 + u1) * (v0 + v1)) * cosa_s)
 *              u0 = u[i,j,k], u1 = u[i,j+1,k], v0 = v[i,j,k], v1 = v[i+1,j,k]: the D-grid winds around the cell
 *   ql   = qliquid + qrain;  qs = (qice + qsnow) + qgraupel;  gz = ql + qs              moist_cv.py's nwat-6 order
 *   cvm  = (1 - (qvapor + gz)) * CV_AIR + qvapor * CV_VAP + ql * C_LIQ + qs * C_ICE     csrc/thermo.h moist_cvm
 *   e    = cvm * pt                                                     mode 0: pt holds the temperature
 *   e    = (cvm * pt) / ((1 + r_vir * qvapor) * (1 - gz))               mode 1: pt as between pace_l2e_post and pace_l2e_finish
 *   te   = te + delp[k] * (e + 0.5 * (((phi_above + phi_below) + w[k] * w[k]) + ke))      te = 0 before the first level
 *   zsum = zsum + pkz[k] * delp[k]                                      mode 1 only; zsum = 0 before the first level
 *   phi_below = phi_above
 * (the Fortran sums from the top down; the bottom-up pass reads delz once and differs in rounding only).
 *   mode 0 stores te0_2d[i,j] = (pace_real_t)te; pkz, area, te_2d, zsum1, words are not used and may be NULL.
 *   mode 1 reads te0_2d, forms te_2d = (double)te0_2d[i,j] - te, stores te_2d[i,j] = (pace_real_t)te_2d and zsum1[i,j] =
 *          (pace_real_t)zsum, and ADDS area * te_2d into words[0 .. 4] and area * zsum into words[5 .. 9] -- the products of the
 *          doubles in registers, before the narrowing.  The caller zeroes `words` (PACE_ENERGY_WORDS int64 on the device) before
 *          the first launch of a sum.
 * Reproducible accumulator: a sum is five signed 64-bit words.  A finite v with |v| < 2^120 adds the four 40-bit limbs
 * l_n = (trunc(|v| * 2^40) >> 40 n) & (2^40 - 1) to word[n], n = 0 .. 3, negated for v < 0 (the significand is only shifted:
 * exact; bits below 2^-40 are dropped toward zero); any other v (NaN, infinity, |v| >= 2^120) adds 1 to word[4] and nothing
 * else.  The additions are integer additions (a fold over the workgroup, then 64-bit integer atomics; no floating-point atomics):
 * the words do not depend on the order, the launch shape or the partition into tiles.  23 bits of headroom: fewer than 2^23
 * addends per sum over all the tiles that are finalised together.
 * Nothing outside the planes' compute windows and the ten words is written; nothing outside the compute domain of the fields is
 * read (u on n + 1 rows, v on n + 1 columns).
 * PACE_ERR_ARG: a NULL geom, water entry or array the mode uses, a mode other than 0 / 1, an output that is an input or another
 * output.
 *
 * pace_energy_finalize: ONE launch for any number of tiles (1 .. PACE_ENERGY_MAX_TILES).  words: HOST array of ntiles device
 * pointers, in tile order, each to a tile's ten words; out: four doubles on the device.  The words are summed over the tiles, then
 * each sum is decoded: M = sum_n word[n] * 2^(40 n) as an exact integer, the value M * 2^-40 rounded ONCE to the nearest double
 * (ties to even), NaN if word[4] != 0.
 *   out[0] = S_te  the sum of area * te_2d        out[1] = S_z  the sum of area * zsum1
 *   out[2] = dtmp   = (consv_te * S_te) / (CV_AIR * S_z)
 *   out[3] = e_flux = (consv_te * S_te) / ((((GRAV * dt_atmos) * 4) * PI) * (RADIUS * RADIUS))      W / m^2
 * PACE_ERR_ARG: NULL words, entry or out, ntiles out of range, a consv_te that is not finite, a dt_atmos that is not finite and
 * positive.
 *
 * pace_l2e_finish_dtmp: pace_l2e_finish's last-step form with the temperature increment of the fixer,
 *   pt = (pt + dtmp * pkz) / ((1 + r_vir * qvapor) * (1 - gz)),   gz = (((qliquid + qrain) + qice) + qsnow) + qgraupel,
 * dtmp = energy_result[2] read on the device (the host never needs it); pe as pace_l2e_finish. */
#define PACE_ENERGY_WORDS 10
#define PACE_ENERGY_MAX_TILES 64
int pace_energy_columns(const pace_geom_t* geom, int mode, const pace_real_t* const* water, const pace_real_t* pt,
                        const pace_real_t* delp, const pace_real_t* delz, const pace_real_t* w, const pace_real_t* u,
                        const pace_real_t* v, const pace_real_t* pkz, const pace_real_t* phis, const pace_real_t* rsin2,
                        const pace_real_t* cosa_s, const pace_real_t* area, pace_real_t* te0_2d, pace_real_t* te_2d,
                        pace_real_t* zsum1, int64_t* words, double r_vir, void* stream);
int pace_energy_finalize(const int64_t* const* words, int ntiles, double consv_te, double dt_atmos, double* out, void* stream);
int pace_l2e_finish_dtmp(const pace_geom_t* geom, const pace_real_t* const* water, pace_real_t* pe, const pace_real_t* pe2,
                         pace_real_t* pt, const pace_real_t* pkz, double r_vir, const double* energy_result, void* stream);

/* ---- SatAdjust3d (fv3core/pace/fv3core/stencils/saturation_adjustment.py:947-1108): the fast saturation adjustment that
 * LagrangianToEulerian runs between the remap of v and moist_pt_last_step / the division by pkz (remapping.py:627-672).
 *   pace_sat_adjust_tables  fills `tables` (a DEVICE buffer of PACE_SAT_ADJUST_TABLE_DOUBLES doubles, in both builds) with the
 *                           saturation tables satadjust reads -- table2, des2, tablew, desw (compute_q_tables, :540-558; the
 *                           reference evaluates each entry on the fly, :46-160) -- for indices -1 ... 2620, one record of four
 *                           doubles per index.  Once per SatAdjust3d object.
 *   pace_sat_adjust         the satadjust stencil (:561-944), non-hydrostatic, over origin (3, 3, kmp), domain (n, n, nk - kmp)
 *                           (:953-976); nothing else is written.  water: HOST array of the six device pointers qvapor, qliquid,
 *                           qrain, qsnow, qice, qgraupel (inout); qcld (out, only where do_qa && last_step); te (out, only where
 *                           consv_te: the reference's fast_mp_consv); pt (inout); q_con, pkz, cappa (out); delp, delz (in);
 *                           area (the float64 cell area, area_64), hs: 2-D fields; params: the externals and the factors
 *                           SatAdjust3d.__call__ computes on the host (:1038-1069).  hydrostatic != 0 is PACE_ERR_UNSUPPORTED. */
#define PACE_SAT_ADJUST_TABLE_DOUBLES (4 * 2622)
typedef struct {
  /* externals (:957-975) */
  int32_t hydrostatic, rad_snow, rad_rain, rad_graupel, tintqs, icloud_f;
  int32_t do_qa; /* hard-coded True by the reference's __call__ (:1071) */
  int32_t pad_;
  double sat_adj0, ql_gen, qs_mlt, ql0_max, t_sub, qi_gen, qi_lim, qi0_max, dw_ocean, dw_land, cld_min;
  /* the scalar arguments of satadjust (:577-594) */
  double sdt, zvir, fac_i2s, c_air, c_vap, mdt, fac_r2g, fac_smlt, fac_l2r, fac_imlt, d0_vap, lv00, fac_v2l, fac_l2v;
} pace_sat_adjust_params_t;
int pace_sat_adjust_tables(double* tables, void* stream);
int pace_sat_adjust(const pace_geom_t* geom, pace_real_t* const* water, pace_real_t* qcld, pace_real_t* te, pace_real_t* pt,
                    pace_real_t* q_con, pace_real_t* pkz, pace_real_t* cappa, const pace_real_t* delp, const pace_real_t* delz,
                    const pace_real_t* area, const pace_real_t* hs, const double* tables, const pace_sat_adjust_params_t* params,
                    int kmp, int last_step, int consv_te, void* stream);

/* ---- DryConvectiveAdjustment (fv3core/pace/fv3core/stencils/fv_subgridz.py:740-964, the Fortran fv_subgrid_z): the dry
 * convective adjustment a driver with fv_sg_adj > 0 applies to the dycore state once per physics step, non-hydrostatic.  One
 * launch, no host synchronisation: init, the three m_loop sweeps and finalize over origin (3, 3, 0), domain (n, n, k_sponge);
 * nothing else is written.  tracers: HOST array of the nine device pointers qvapor, qliquid, qrain, qice, qsnow, qgraupel,
 * qo3mr, qsgs_tke, qcld (inout); pt, ua, va, w (inout); u_dt, v_dt (out: overwritten, not accumulated); delp, delz, pkz (in);
 * peln, pe (in, interface fields; of pe only element (3, 3, 0) is read, on the device, to choose t_min as :867 does on the
 * host).  3 <= k_sponge <= nk; nwat == 0 sets xvir = 0, any other value ZVIR; fv_sg_adj and timestep in seconds, both > 0. */
int pace_dry_convective_adjust(const pace_geom_t* geom, pace_real_t* const* tracers, pace_real_t* pt, pace_real_t* ua,
                               pace_real_t* va, pace_real_t* w, pace_real_t* u_dt, pace_real_t* v_dt, const pace_real_t* delp,
                               const pace_real_t* delz, const pace_real_t* pkz, const pace_real_t* peln, const pace_real_t* pe,
                               int k_sponge, int nwat, double fv_sg_adj, double timestep, void* stream);

/* ---- The end of a dycore-only step: UpdateAtmosphereState / ApplyPhysicsToDycore (stencils/pace/stencils/
 * update_atmos_state.py:19-37, fv_update_phys.py:30-74, update_dwind_phys.py:446-653; the Fortran fv_update_phys and
 * update_dwinds_phys).  fp64 arithmetic in the reference's order; no scratch field.
 *   pace_fill_gfs_delp         fill_gfs_delp(delp, q, q_min) over the FULL domain, halo included: origin (0, 0, 0), domain
 *                              (n + 6, n + 6, nk + 1); levels 0 .. nk - 1 of q may change, level nk is not touched; nk >= 2.
 *                              q_min is used in the storage type (float(q_min) in the float32 build)
 *   pace_phys_thermo_pressure  moist_cv and update_pressure_and_surface_winds in one launch over origin (3, 3, 0), domain
 *                              (n, n, nk + 1).  water: HOST array of the six device pointers qvapor, qliquid, qrain, qsnow, qice,
 *                              qgraupel (in).  pt += t_dt * dt * CP_AIR / cvm and t_dt = 0 on nk + 1 levels; pe[k] = pe[k - 1] +
 *                              delp[k - 1], peln = log(pe), pk = exp(KAPPA * peln) for k >= 1 (level 0 of the three is kept);
 *                              ps = pe[nk]; u_srf, v_srf = ua, va at level nk - 1 (2-D fields)
 *   pace_update_dwinds_phys    AGrid2DGridPhysics.__call__: u += dt5 * (ue . es1) on origin (3, 3, 0), domain (n, n + 1, nk),
 *                              v += dt5 * (ve . ew2) on (n + 1, n, nk), with the four tile-edge blends; then u_dt = v_dt = 0
 *                              on origin (2, 2, 0), domain (n + 2, n + 2, nk) (a second launch on the same stream).  The
 *                              one-point halo of u_dt, v_dt must be up to date.  vlon, vlat, es1, ew2: HOST arrays of the three
 *                              device pointers of their Cartesian components (2-D fields); edge_vect_*: 1-D device arrays of
 *                              n + 7 entries indexed like the fields.  n even, n >= 4. */
int pace_fill_gfs_delp(const pace_geom_t* geom, const pace_real_t* delp, pace_real_t* q, double q_min, void* stream);
int pace_phys_thermo_pressure(const pace_geom_t* geom, const pace_real_t* const* water, pace_real_t* pt, pace_real_t* t_dt,
                              pace_real_t* pe, const pace_real_t* delp, pace_real_t* peln, pace_real_t* pk, const pace_real_t* ua,
                              const pace_real_t* va, pace_real_t* ps, pace_real_t* u_srf, pace_real_t* v_srf, double dt,
                              void* stream);
int pace_update_dwinds_phys(const pace_geom_t* geom, pace_real_t* u, pace_real_t* v, pace_real_t* u_dt, pace_real_t* v_dt,
                            const pace_real_t* const* vlon, const pace_real_t* const* vlat, const pace_real_t* const* es1,
                            const pace_real_t* const* ew2, const pace_real_t* edge_vect_w, const pace_real_t* edge_vect_e,
                            const pace_real_t* edge_vect_s, const pace_real_t* edge_vect_n, double dt5, void* stream);

/* ---- Microphysics (physics/pace/physics/stencils/microphysics.py:1897-2533): the GFDL cloud microphysics, non-hydrostatic,
 * NamelistDefaults switches.  One launch over origin (3, 3, 0), domain (n, n, nk), no host synchronisation: fields_init, ntimes x
 * (warm_rain, sedimentation, warm_rain, icloud), fields_update.  float64 storage only (PACE_ERR_UNSUPPORTED otherwise).
 *   workspace      pace_microphysics_workspace_bytes(geom) bytes of device memory: the work state of the columns
 *   cfg            namelist values and the factors the reference's setupm / _set_timestep compute on the host, by value; a
 *                  struct_bytes other than sizeof(pace_microphysics_config_t) is PACE_ERR_ARG
 *   in             HOST array of PACE_MICROPHYSICS_INPUTS device pointers: pt, qvapor, qliquid, qrain, qice, qsnow, qgraupel, ua,
 *                  va, delprsi, delz (3-D), land, area (2-D); read only
 *   wmp            vertical velocity (inout: the sedimentation transports it)
 *   tendencies     HOST array of PACE_MICROPHYSICS_TENDENCIES device pointers: qv_dt, ql_dt, qr_dt, qi_dt, qs_dt, qg_dt, qa_dt, udt,
 *                  vdt, pt_dt; ACCUMULATED into (udt, vdt from level 1 on), except qa_dt, which is set to zero (do_qa)
 *   precipitation  HOST array of four device pointers: rain, snow, ice, graupel (out, mm/day, the column's value on every level) */
#define PACE_MICROPHYSICS_INPUTS 13
#define PACE_MICROPHYSICS_TENDENCIES 10
typedef struct {
  int32_t struct_bytes; /* sizeof(pace_microphysics_config_t) */
  int32_t ntimes;       /* sub-steps */
  double timestep, rdt, dts, rdts, dt_rain;
  double c_air, c_vap, d0_vap, lv00, cpaut, fac_rc, so3, zs, log_10, tice, tice0, t_wfr, t_sub;
  double ccn_l, ccn_o, dw_land, dw_ocean, rh_inc, rh_inr;
  double vr_fac, vr_max, vi_fac, vi_max, vs_fac, vs_max, vg_fac, vg_max;
  double ql_mlt, qs_mlt, qi0_crt, qs0_crt, qi_gen, qi_lim;
  double cracs, csacr, cgacr, cgacs;
  double acco[3][4];
  double csacw, csaci, cgacw, cgaci, cracw;
  double cssub[5], crevp[5], cgfr[2], csmlt[5], cgmlt[5];
  double ces0, fac_i2s, fac_g2v, fac_v2g, fac_imlt, fac_l2v;
} pace_microphysics_config_t;
int64_t pace_microphysics_workspace_bytes(const pace_geom_t* geom);
int pace_microphysics(const pace_geom_t* geom, void* workspace, const pace_microphysics_config_t* cfg,
                      const pace_real_t* const* in, pace_real_t* wmp, pace_real_t* const* tendencies,
                      pace_real_t* const* precipitation, void* stream);

/* ---- The Physics shell and the physics-to-dycore coupling (physics/pace/physics/stencils/physics.py:33-201, get_prs_fv3.py,
 * get_phi_fv3.py; stencils/pace/stencils/update_atmos_state.py:40-145).  One launch each, no host synchronisation, no
 * allocation, no scratch field; fp64 arithmetic in the reference's order, no transcendental.  float64 storage only
 * (PACE_ERR_UNSUPPORTED otherwise).  Every table is a HOST array of device pointers.
 *   pace_copy_dycore_to_physics        copy_dycore_to_physics over origin (3, 3, 0), domain (n + 1, n + 1, nk): out[m] = in[m]
 *                                      for PACE_PHYSICS_COPY_FIELDS fields (the reference's order: qvapor, qliquid, qrain, qsnow,
 *                                      qice, qgraupel, qo3mr, qsgs_tke, qcld, pt, delp, delz, ua, va, w, omga)
 *   pace_physics_prepare               what Physics.__call__ does before the microphysics, over origin (3, 3, 0), domain
 *                                      (n, n, nk): atmos_phys_driver_statein (nwat 6), get_prs_fv3, get_phi_fv3 and, with
 *                                      do_microphysics != 0, prepare_microphysics.  tracers: qvapor, qliquid, qrain, qice, qsnow,
 *                                      qgraupel, qo3mr (times the moist delp, over the dry one), qsgs_tke (over the dry one).
 *                                      delp (inout) becomes the clamped mid-layer pressure; prsi and phii (out) get nk + 1 levels,
 *                                      phil and delprsi nk.  do_microphysics: dz, wmp (out) and the PACE_MICROPHYSICS_TENDENCIES
 *                                      tendencies (set to zero); otherwise omga, dz, wmp and tendencies are not used and may be
 *                                      NULL.  Nothing outside the compute domain is written (the reference runs get_prs_fv3 and
 *                                      get_phi_fv3 over the halo too), level nk of the layer fields is neither read nor written,
 *                                      and the reference's prsik is not computed.
 *   pace_physics_update_state          update_physics_state_with_tendencies: out[m] = x[m] + x_dt[m] * dt for
 *                                      PACE_PHYSICS_UPDATED_FIELDS fields over origin (3, 3, 0), domain (n, n, nk)
 *   pace_physics_tendencies_to_dycore  prepare_tendencies_and_update_tracers over origin (3, 3, 0), domain (n, n, nk).
 *                                      tendencies: u_dt, v_dt, pt_dt, ACCUMULATED into (+= (updated - before) * rdt); updated:
 *                                      physics_updated_ua, _va, _pt, _specific_humidity, _qliquid, _qrain, _qsnow, _qice,
 *                                      _qgraupel (nine); before: the physics state's ua, va, pt; tracers: the dycore's qvapor,
 *                                      qliquid, qrain, qsnow, qice, qgraupel (inout); prsi: nk + 1 levels; delp (inout): the dycore's */
#define PACE_PHYSICS_COPY_FIELDS 16
#define PACE_PHYSICS_UPDATED_FIELDS 10
int pace_copy_dycore_to_physics(const pace_geom_t* geom, const pace_real_t* const* in, pace_real_t* const* out, void* stream);
int pace_physics_prepare(const pace_geom_t* geom, pace_real_t* const* tracers, const pace_real_t* pt, const pace_real_t* delz,
                         pace_real_t* delp, const pace_real_t* omga, pace_real_t* prsi, pace_real_t* phii, pace_real_t* phil,
                         pace_real_t* delprsi, pace_real_t* dz, pace_real_t* wmp, pace_real_t* const* tendencies, double ptop,
                         int do_microphysics, void* stream);
int pace_physics_update_state(const pace_geom_t* geom, const pace_real_t* const* x, const pace_real_t* const* x_dt,
                              pace_real_t* const* out, double dt, void* stream);
int pace_physics_tendencies_to_dycore(const pace_geom_t* geom, pace_real_t* const* tendencies, const pace_real_t* const* updated,
                                      const pace_real_t* const* before, pace_real_t* const* tracers, const pace_real_t* prsi,
                                      pace_real_t* delp, double rdt, void* stream);

/* ---- The driver's check of the state (driver/pace/driver/safety_checks.py:80-110): the extrema and the NaN counts of up to
 * PACE_STATE_EXTREMA_MAX_FIELDS fields in one launch pair, both storage types, no host synchronisation, no atomics (the result
 * does not depend on the order workgroups run in).  fields: HOST array of nfields device pointers; compute_only: HOST array of
 * nfields flags.  The window of field m is its compute domain, origin (3, 3, 0), extent (n, n, nk), where compute_only[m] != 0,
 * and otherwise the logical storage (n + 7, n + 7, nk + 1); the padding of a row beyond n + 7 is never read.  out: DEVICE
 * array of 4 * nfields doubles, per field
 *   [0] the minimum of the values in the window that are no NaN (+inf if there is none), [1] their maximum (-inf),
 *   [2] the number of NaNs in the window, [3] the number of NaNs in the compute domain
 * (+-inf are values).  workspace: at least pace_state_extrema_workspace_bytes(geom) bytes of device memory, whatever nfields is;
 * it holds nothing between calls and need not be cleared.  nfields < 1 or > PACE_STATE_EXTREMA_MAX_FIELDS: PACE_ERR_ARG. */
#define PACE_STATE_EXTREMA_MAX_FIELDS 16
int64_t pace_state_extrema_workspace_bytes(const pace_geom_t* geom);
int pace_state_extrema(const pace_geom_t* geom, const pace_real_t* const* fields, const int* compute_only, int nfields,
                       void* workspace, double* out, void* stream);

/* ---- The driver's diagnostics (driver/pace/driver/diagnostics.py:144-253): up to PACE_DIAG_MAX_ITEMS items gathered from the
 * fields, transposed to the files' axis order, narrowed and written to one packed device buffer by ONE launch, both storage
 * types, no atomics, no workspace, no host synchronisation.  items: HOST array of nitems items; out: DEVICE array of float32, or
 * of float64 where out_is_double != 0.  Fields are stored x-fastest; an item's output is (x, y, z) in C order, z fastest:
 *   PACE_DIAG_WINDOW3D         out[out_offset + (i * nj + j) * nk + k] = field(i0 + i, j0 + j, k0 + k)
 *   PACE_DIAG_PLANE            out[out_offset + i * nj + j] = field(i0 + i, j0 + j); field points at element (0, 0) of a 2-D
 *                              field or of ONE level of a 3-D one (the caller adds level * sk); k0 = 0, nk = 1
 *   PACE_DIAG_COLUMN_INTEGRAL  out[out_offset + i * nj + j] = RGRAV * sum over k = k0 .. k0 + nk - 1 of field * weight, summed
 *                              in double in ascending k with one accumulator, product then add
 * The narrowing is a plain cast (round to nearest even, overflow to +-inf).  Nothing outside an item's window is read and
 * nothing outside its ni * nj * nk (ni * nj) output elements is written.  PACE_ERR_ARG: nitems < 1 or > PACE_DIAG_MAX_ITEMS, an
 * unknown kind, a window that is empty or outside the storage (n + 7, n + 7, nk + 1), a negative out_offset, a
 * COLUMN_INTEGRAL without weight. */
#define PACE_DIAG_MAX_ITEMS 32
enum { PACE_DIAG_WINDOW3D = 0, PACE_DIAG_PLANE = 1, PACE_DIAG_COLUMN_INTEGRAL = 2 };
typedef struct {
  const pace_real_t* field;  /* element (0,0,0) of the storage, or of the level's plane for a PLANE item */
  const pace_real_t* weight; /* COLUMN_INTEGRAL: delp; otherwise NULL */
  int32_t kind;              /* PACE_DIAG_WINDOW3D | PACE_DIAG_PLANE | PACE_DIAG_COLUMN_INTEGRAL */
  int32_t i0, j0, k0;        /* origin of the window in the storage */
  int32_t ni, nj, nk;        /* extent (nk = 1 for PLANE) */
  int64_t out_offset;        /* in output elements */
} pace_diag_item_t;
int pace_diag_pack(const pace_geom_t* geom, const pace_diag_item_t* items, int nitems, int out_is_double, void* out,
                   void* stream);

/* ---- Pressure-level diagnostics (`p_select`; this project's extension, the reference stops at z_select): up to
 * PACE_PLEV_MAX_ITEMS planes -- layer fields and the geometric height on up to PACE_PLEV_MAX_LEVELS pressure surfaces --
 * interpolated linearly in log p and written to one packed device buffer by ONE launch, both storage types, no atomics, no
 * workspace, no host synchronisation.  peln: the state's log interface pressures, nk + 1 levels of ln(Pa); log_p: HOST array of
 * nlevels natural logs of the target pressures (the kernel has no transcendental); items: HOST array of nitems items; one
 * horizontal window (i0, j0, ni, nj) serves all items; out: DEVICE array of float32, or of float64 where out_is_double != 0;
 * an item's output is out[out_offset + i * nj + j], (x, y) in C order like a PACE_DIAG_PLANE.  All arithmetic is in double on
 * the stored values (the float32 library widens first), without FMA, in exactly this order, with lp = log_p[level], nz = nk:
 *   PACE_PLEV_LAYER   a cell-centre (x, y, z) field f; pm[k] = 0.5 * (peln[k] + peln[k + 1]);
 *                       kb = the largest k in 1 .. nz - 2 with pm[k] <= lp, 0 if there is none
 *                       if   not (lp > pm[0]):   f[0]
 *                       elif lp >= pm[nz - 1]:   f[nz - 1]                                (clamped: no extrapolation)
 *                       else: t = (lp - pm[kb]) / (pm[kb + 1] - pm[kb]);  f[kb] + (f[kb + 1] - f[kb]) * t
 *   PACE_PLEV_HEIGHT  geometric height [m] from field = delz and surface = phis:
 *                       zi[nz] = phis * RGRAV;  zi[k] = zi[k + 1] - delz[k], k = nz - 1 .. 0
 *                       kb = the largest k in 1 .. nz - 1 with peln[k] <= lp, 0 if there is none
 *                       t = (lp - peln[kb]) / (peln[kb + 1] - peln[kb]);  zi[kb] + (zi[kb + 1] - zi[kb]) * t
 *                     (extrapolated with the top layer's slope above the model top, with the lowest layer's below the ground)
 * The definitions are total: every comparison with a NaN is false, and a non-monotone or NaN column yields a value by these
 * rules.  Nothing outside the window's columns is read and nothing outside an item's ni * nj output elements is written.
 * PACE_ERR_ARG: nlevels < 1 or > PACE_PLEV_MAX_LEVELS, nitems < 1 or > PACE_PLEV_MAX_ITEMS, an unknown kind, a level outside
 * 0 .. nlevels - 1, an item without field, a HEIGHT item without surface, geom->nk < 2, a window that is empty or outside the
 * storage (n + 7, n + 7), a negative out_offset. */
#define PACE_PLEV_MAX_ITEMS 32
#define PACE_PLEV_MAX_LEVELS 8
enum { PACE_PLEV_LAYER = 0, PACE_PLEV_HEIGHT = 1 };
typedef struct {
  const pace_real_t* field;   /* LAYER: the 3-D field; HEIGHT: delz */
  const pace_real_t* surface; /* HEIGHT: phis (2-D); LAYER: NULL */
  int32_t kind;               /* PACE_PLEV_LAYER | PACE_PLEV_HEIGHT */
  int32_t level;              /* index into log_p[] */
  int64_t out_offset;         /* in output elements */
} pace_plev_item_t;
int pace_plev_diag(const pace_geom_t* geom, const pace_real_t* peln, const double* log_p, int nlevels,
                   const pace_plev_item_t* items, int nitems, int i0, int j0, int ni, int nj, int out_is_double, void* out,
                   void* stream);

/* ---- A host model's arrays into the state (fv3core/pace/fv3core/initialization/geos_wrapper.py:207-270): the inverse of
 * pace_diag_pack.  Up to PACE_UNPACK_MAX_ITEMS windows of fields are filled from one packed device buffer by ONE launch, both
 * storage types, no atomics, no workspace, no host synchronisation.  items: HOST array of nitems items; in: DEVICE array of
 * float64 in both libraries (the float32 library narrows with a plain cast: round to nearest even, overflow to +-inf).
 *   field(i0 + i, j0 + j, k0 + k) = (pace_real_t) in[in_offset + e * in_step]
 *   PACE_ORDER_ZFAST  e = (i * nj + j) * nk + k   a C-ordered array; with in_step = 7 one species of a C-ordered (x, y, z, 7) one
 *   PACE_ORDER_XFAST  e = i + ni * (j + nj * k)   Fortran order, which is the device's own
 * and for a PACE_DIAG_PLANE item the same expressions with nk = 1, k = 0; its field points at element (0, 0) of a 2-D field or
 * of ONE level of a 3-D one.  Nothing outside an item's window is written (not the halo, not other levels, not the row padding)
 * and nothing outside its ni * nj * nk source elements is read.  Two items whose windows overlap on one field: undefined.
 * PACE_ERR_ARG: nitems < 1 or > PACE_UNPACK_MAX_ITEMS, a kind other than WINDOW3D and PLANE, an unknown order, a window that is
 * empty or outside the storage (n + 7, n + 7, nk + 1), a negative in_offset, in_step < 1, a field that is NULL. */
#define PACE_UNPACK_MAX_ITEMS 32
enum { PACE_ORDER_ZFAST = 0, PACE_ORDER_XFAST = 1 };
typedef struct {
  pace_real_t* field;      /* element (0,0,0) of the storage (2-D field for PLANE) */
  int32_t kind;            /* PACE_DIAG_WINDOW3D | PACE_DIAG_PLANE */
  int32_t order;           /* layout of the item's source elements */
  int32_t i0, j0, k0, ni, nj, nk;   /* destination window in the storage; nk = 1, k0 = 0 for PLANE */
  int32_t in_step;         /* >= 1: distance in elements between consecutive source elements along the fastest axis */
  int64_t in_offset;       /* in source elements */
} pace_unpack_item_t;
int pace_state_unpack(const pace_geom_t* geom, const pace_unpack_item_t* items, int nitems, const double* in, void* stream);

/* ---- The state into the data sections of Fortran FV3 restart files (NetCDF-3: dense, big-endian), with FMS's per-variable sums:
 * the inverse of pace_state_unpack's XFAST items.  Up to PACE_RESTART_MAX_ITEMS windows of fields are gathered by ONE launch into
 * one device BYTE buffer, both storage types, no atomics, no host synchronisation.  items: HOST array of nitems items.
 *   output element e = i + ni * (j + nj * k) of an item = field(i0 + i, j0 + j, k0 + k), x fastest: the file's (z, y, x) C order,
 *   which is the storage's own; the row padding is dropped.  The value is widened to double (exact), for PACE_RESTART_BE_F32 then
 *   narrowed by a plain cast (round to nearest even, overflow to +-inf), and written BIG-endian at out + out_offset + e * size.
 *   sums[m] = the wrapping (mod 2^64) sum over item m's elements of the bit pattern of the value as written, before the swap:
 *   64 bits for BE_F64, the 32 bits zero-extended for BE_F32.  Per-workgroup partials, then a combine: integer addition commutes,
 *   so the result does not depend on the order workgroups run in.
 * float64 library -> BE_F64 moves bits: -0.0, denormals, +-inf and NaN payloads arrive unchanged.  out == NULL: sums only;
 * sums == NULL: pack only.  Nothing outside a window is read; nothing outside an item's ni * nj * nk elements is written.
 * workspace: at least pace_restart_pack_workspace_bytes(geom, items, nitems) bytes of device memory (0 for arguments that
 * pace_restart_pack refuses); it holds nothing between calls, need not be cleared and may be NULL where sums is.
 * PACE_ERR_ARG: nitems < 1 or > PACE_RESTART_MAX_ITEMS, a kind other than WINDOW3D and PLANE, an unknown out_type, a window that
 * is empty or outside the storage (n + 7, n + 7, nk + 1), a NULL field, an out_offset that is negative or no multiple of the
 * output element's size, out and sums both NULL, sums without workspace. */
#define PACE_RESTART_MAX_ITEMS 32
enum { PACE_RESTART_BE_F64 = 0, PACE_RESTART_BE_F32 = 1 };
typedef struct {
  const pace_real_t* field;   /* element (0,0,0) of the storage; for PLANE: of a 2-D field or of ONE level's plane */
  int32_t kind;               /* PACE_DIAG_WINDOW3D | PACE_DIAG_PLANE */
  int32_t i0, j0, k0, ni, nj, nk;   /* window in the storage; PLANE: k0 = 0, nk = 1 */
  int64_t out_offset;         /* BYTES into out; a multiple of the output element's size */
} pace_restart_item_t;
int64_t pace_restart_pack_workspace_bytes(const pace_geom_t* geom, const pace_restart_item_t* items, int nitems);
int pace_restart_pack(const pace_geom_t* geom, const pace_restart_item_t* items, int nitems, int out_type, void* out,
                      uint64_t* sums, void* workspace, void* stream);

/* ---- The interface pressures of a state read from a Fortran restart, which holds delp only
 * (driver/pace/driver/initialization.py:422-442), ONE launch:
 *   pe(i, j, k) = ptop + sum over l < k of delp(i, j, l),  peln = log(pe),  k = 0 .. nk
 * on every column of the WHOLE storage (n + 7) x (n + 7), halo and stagger row included (the reference writes .data, not the
 * view); the row padding is neither read nor written.  The sum is one double accumulator in ascending k (the order of a
 * sequential numpy cumsum), the logarithm is taken of that double, and both results are narrowed on the store only (float32
 * library).  No atomics, no workspace, no host synchronisation.  PACE_ERR_ARG: a NULL pointer, nk < 1. */
int pace_pe_peln_from_delp(const pace_geom_t* geom, const pace_real_t* delp, double ptop, pace_real_t* pe, pace_real_t* peln,
                           void* stream);

/* ---- The checkpointers (util/pace/util/checkpointer/thresholds.py:59-162, validation.py:14-143): calibration and validation
 * of up to PACE_CKPT_MAX_ITEMS variables per call, both storage types, no atomics, no host synchronisation.  items: HOST array.
 * A variable is its base pointer, its logical extents (ni, nj, nk) in storage order and its strides (1, sj, sk) in elements --
 * no pace_geom_t: 2-D fields (nk = 1), dense 1-D arrays (nj = nk = 1) and temporaries are variables too.  Elements are widened
 * to double first; accumulators, expected values and results are double in both libraries.  The padding of a row (i >= ni) is
 * never read.
 *   pace_ckpt_accumulate  ONE launch.  mn, mx, asum: dense DEVICE arrays of ni * nj * nk doubles, x fastest.  first != 0:
 *                         mn = mx = v, asum = |v| (they need no initialisation); otherwise mn = minimum(mn, v), mx =
 *                         maximum(mx, v), asum = asum + |v| with numpy's NaN propagation; one accumulator per element, added
 *                         to in call order.
 *   pace_ckpt_thresholds  partials, then a combine.  out: DEVICE array of 4 * nitems doubles, per item
 *                           [0] the maximum of (mx - mn) / (asum / n_trials) over the quotients that are no NaN (numpy's nanmax:
 *                               0 / 0 is skipped, x / 0 is inf and counts), NaN if every quotient is a NaN
 *                           [1] the maximum of mx - mn, NaN if one of them is (numpy's max)
 *                           [2] 1.0 if asum / n_trials == 0 everywhere, else 0.0
 *                           [3] the number of elements whose mx - mn is a NaN
 *   pace_ckpt_validate    partials, then a combine.  The window (i0, j0, k0, wi, wj, wk) of the storage against expected, a
 *                         DEVICE array of doubles whose element for window point (i, j, k) is expected[i * ei + j * ej + k * ek].
 *                         With output a and expected d, numpy.testing.assert_allclose's rules: the relative test where d != 0
 *                         with bound rtol * |d|, the absolute test everywhere with bound atol; a NaN rtol / atol skips that test;
 *                         both NaN match, one NaN violates; if either is infinite they match only if a == d; otherwise a
 *                         violation iff !(|a - d| <= bound).  out: DEVICE array of 6 * nitems doubles, per item
 *                           [0] violations of the relative test, [1] of the absolute test,
 *                           [2] the largest |a - d| over finite pairs, [3] the largest |a - d| / |d| over finite pairs with d != 0,
 *                           [4] the smallest expected-array offset i * ei + j * ej + k * ek of a violating element (its flat
 *                               index in a dense expected array), -1 if there is none, [5] the number of elements compared.
 *                         Nothing outside the window is read.
 * workspace: at least pace_ckpt_*_workspace_bytes(items, nitems) bytes of device memory (0: invalid items); it holds nothing
 * between calls and need not be cleared.  PACE_ERR_ARG: nitems < 1 or > PACE_CKPT_MAX_ITEMS, a NULL pointer the call uses, an
 * extent < 1, sj < ni, sk < sj * (nj - 1) + ni, n_trials < 1, a window that is empty or outside the extents, a negative expected
 * stride.  PACE_ERR_UNSUPPORTED: a variable of 2^31 elements or more. */
#define PACE_CKPT_MAX_ITEMS 32
typedef struct {
  const pace_real_t* field; /* element (0, 0, 0) of the storage */
  int32_t ni, nj, nk;       /* logical extents in storage order, x fastest */
  int32_t pad_;
  int64_t sj, sk;           /* strides in elements; the stride along i is 1 */
  double* mn;               /* accumulate (written), thresholds (read): dense, ni * nj * nk */
  double* mx;
  double* asum;
  int32_t i0, j0, k0;       /* validate: origin of the window in the storage */
  int32_t wi, wj, wk;       /* ... and its extent */
  const double* expected;   /* validate: the expected values */
  int64_t ei, ej, ek;       /* ... and their element strides along the storage axes i, j, k */
  double rtol, atol;        /* validate: NaN skips the test */
} pace_ckpt_item_t;
int pace_ckpt_accumulate(const pace_ckpt_item_t* items, int nitems, int first, void* stream);
int64_t pace_ckpt_thresholds_workspace_bytes(const pace_ckpt_item_t* items, int nitems);
int pace_ckpt_thresholds(const pace_ckpt_item_t* items, int nitems, int n_trials, void* workspace, double* out, void* stream);
int64_t pace_ckpt_validate_workspace_bytes(const pace_ckpt_item_t* items, int nitems);
int pace_ckpt_validate(const pace_ckpt_item_t* items, int nitems, void* workspace, double* out, void* stream);

/* ---- Nudging (util/pace/util/nudging.py:44,70): the state relaxed toward reference fields.  Up to PACE_NUDGE_MAX_ITEMS windows
 * of fields by ONE launch, both storage types, no atomics, no workspace, no host synchronisation.  items: HOST array of nitems
 * items.  field, ref0, ref1 and tendency of an item share the storage geometry of geom.  For every point of an item's window, in
 * double on the stored values (the float32 library widens first; exact), without FMA and without a reciprocal, in this order:
 *   r = ref1 ? r0 + (r1 - r0) * weight : r0      the reference, held (ref1 == NULL) or interpolated within its bracket
 *   t = (r - q) / timescale                      the nudging tendency
 *   if tendency:    tendency = (pace_real_t) t
 *   if apply != 0:  field    = (pace_real_t)(q + t * dt)
 * In the float64 library with ref1 == NULL that is the reference's expression bit for bit.  The narrowing is a plain cast (round to
 * nearest even, overflow to +-inf).  For a PACE_DIAG_PLANE item k0 = 0 and nk = 1, and each pointer is element (0, 0) of a 2-D field
 * or of ONE level.  Nothing outside the windows is written (not the halo, not level nk, not the row padding), nothing outside the
 * windows' elements is read, and with apply == 0 the field is only read.  ref0 and ref1 may be one array; tendency may be ref0 or
 * ref1 (an element is read and written by one thread).  Two items whose windows overlap on one written array: undefined.
 * PACE_ERR_ARG: nitems < 1 or > PACE_NUDGE_MAX_ITEMS, a kind other than WINDOW3D and PLANE, a window that is empty or outside the
 * storage (n + 7, n + 7, nk + 1), a NULL field or ref0, tendency == NULL with apply == 0 (nothing to do), a timescale that is not
 * finite and > 0, a weight outside [0, 1] or NaN, a dt that is not finite, a field whose pointer equals ref0, ref1 or tendency. */
#define PACE_NUDGE_MAX_ITEMS 32
typedef struct {
  pace_real_t* field;            /* the state's field, element (0,0,0) of its storage; read, and written when apply != 0 */
  const pace_real_t* ref0;       /* reference at the bracket's start, same storage geometry */
  const pace_real_t* ref1;       /* reference at the bracket's end, or NULL: no interpolation */
  pace_real_t* tendency;         /* out, same geometry, or NULL */
  int32_t kind;                  /* PACE_DIAG_WINDOW3D | PACE_DIAG_PLANE */
  int32_t i0, j0, k0, ni, nj, nk;   /* window in the storage; PLANE: k0 = 0, nk = 1 */
  double timescale;              /* seconds */
} pace_nudge_item_t;
int pace_nudge(const pace_geom_t* geom, const pace_nudge_item_t* items, int nitems, double weight, double dt, int apply,
               void* stream);

/* ---- Held-Suarez (1994) forcing (the Fortran FV3's Held_Suarez_Tend; the reference has none): Newtonian relaxation of the
 * temperature toward a zonally symmetric equilibrium and Rayleigh friction of the low-level winds, as the tendencies that
 * pace_update_dwinds_phys and pace_phys_thermo_pressure apply.  ONE launch, both storage types, no atomics, no workspace, no host synchronisation.  pe, ua,
 * va, pt, u_dt, v_dt, pt_dt and teq share the storage geometry of geom; sin2lat and cos2lat are 2-D planes of the same row
 * stride holding sin(lat)^2 and cos(lat)^2 of the cell centres.  For every cell of the compute domain -- origin (3, 3, 0), extent
 * (n, n, nk) -- in double on the stored values (the float32 library widens first; exact), without FMA and without a reciprocal, in
 * this order, with lean_log / lean_exp of csrc/lean_math.h (<= 0.55 ulp):
 *   ps    = pe[i,j,nk]
 *   pm    = 0.5 * (pe[i,j,k] + pe[i,j,k+1])
 *   sigma = pm / ps
 *   lp    = lean_log(pm / p0)
 *   pk    = lean_exp(kappa * lp)
 *   x     = ((t0 - delta_t_y * s2) - (delta_theta_z * lp) * c2) * pk
 *   teq   = (x < t_strat) ? t_strat : x                       a NaN stays a NaN
 *   hx    = (sigma - sigma_b) / (1.0 - sigma_b)               the denominator formed once, in double
 *   h     = (hx < 0.0) ? 0.0 : hx                             a NaN stays a NaN
 *   kv    = k_f * h
 *   kt    = k_a + ((k_s - k_a) * h) * (c2 * c2)
 *   u_dt  = -((kv * ua) / (1.0 + kv * dt))                    likewise v_dt from va
 *   pt_dt = -(((kt * (pt - teq)) / (1.0 + kt * dt)) * heating_scale)
 *   accumulate: out = (pace_real_t)((double)out + value); otherwise out = (pace_real_t)value; teq (if given) is always stored
 * 1 / (1 + k dt) is backward Euler: applied over dt, friction and relaxation are contractions for every dt; dt = 0 gives the
 * plain Held-Suarez rates.  The narrowing is a plain cast.  Nothing outside the compute domain's nk levels is written (not the
 * halo, not level nk, not the row padding); nothing outside the compute domain is read (pe on nk + 1 levels there); the inputs
 * are only read.
 * PACE_ERR_ARG: a NULL geom or cfg or any NULL array but teq, struct_bytes != sizeof(pace_held_suarez_config_t), a dt that is
 * negative or not finite, sigma_b outside [0, 1), p0 <= 0, a rate (k_f, k_a, k_s) that is negative or not finite, accumulate other
 * than 0 / 1, an output pointer equal to an input pointer or to another output. */
typedef struct {
  int32_t struct_bytes;   /* sizeof(pace_held_suarez_config_t) */
  int32_t accumulate;     /* 0: the three tendencies are stored; 1: added to what the arrays hold */
  double dt;              /* seconds, >= 0: the implicit factor */
  double p0, kappa, sigma_b, k_f, k_a, k_s;         /* 1e5 Pa, RDGAS / CP_AIR, 0.7, 1/86400, 1/(40*86400), 1/(4*86400)  [1/s] */
  double delta_t_y, delta_theta_z, t0, t_strat;     /* 60 K, 10 K, 315 K, 200 K */
  double heating_scale;   /* multiplies pt_dt: CV_AIR / CP_AIR where the tendency is applied as a constant-pressure heating */
} pace_held_suarez_config_t;
int pace_held_suarez(const pace_geom_t* geom, const pace_held_suarez_config_t* cfg, const pace_real_t* pe,
                     const pace_real_t* ua, const pace_real_t* va, const pace_real_t* pt, const pace_real_t* sin2lat,
                     const pace_real_t* cos2lat, pace_real_t* u_dt, pace_real_t* v_dt, pace_real_t* pt_dt, pace_real_t* teq,
                     void* stream);

/* ---- DynamicalCore (fv3core/pace/fv3core/stencils/fv_dynamics.py:92-624): the stencils it runs itself.  water: HOST
 * array of the six device pointers qvapor, qliquid, qrain, qsnow, qice, qgraupel.
 *   pace_fv_setup_pt  = moist_cv.fv_setup (moist_cv.py:175-234, moist_phys, nwat 6) + pt_to_potential_density_pt
 *                       (fv_dynamics.py:41-54): compute_preamble's two stencils in one pass
 *   pace_omega_from_w = fv_dynamics.py:57-67
 *   pace_neg_adj3     = AdjustNegativeTracerMixingRatio.__call__ (fv3core/pace/fv3core/stencils/neg_adj3.py:377-420),
 *                       non-hydrostatic: fix_neg_water, fillq(qgraupel), fillq(qrain), fix_water_vapor_down, fix_neg_cloud
 *   pace_c2l_ord      = CubedToLatLon's stencil (stencils/pace/stencils/c2l_ord.py:15-112), order 2 or 4 (order 4 expects
 *                       the halos of u, v updated); a11..a22: 2-D metric fields */
int pace_fv_setup_pt(const pace_geom_t* geom, pace_real_t* const* water, pace_real_t* q_con, pace_real_t* pkz,
                     pace_real_t* pt, pace_real_t* cappa, const pace_real_t* delp, const pace_real_t* delz,
                     pace_real_t* dp1, void* stream);
int pace_omega_from_w(const pace_geom_t* geom, const pace_real_t* delp, const pace_real_t* delz, const pace_real_t* w,
                      pace_real_t* omga, void* stream);
int pace_neg_adj3(const pace_geom_t* geom, pace_real_t* const* water, pace_real_t* qcld, pace_real_t* pt,
                  const pace_real_t* delp, void* stream);
int pace_c2l_ord(const pace_geom_t* geom, const pace_metrics_t* met, int order, const pace_real_t* u,
                 const pace_real_t* v, const pace_real_t* a11, const pace_real_t* a12, const pace_real_t* a21,
                 const pace_real_t* a22, pace_real_t* ua, pace_real_t* va, void* stream);

/* ---- Rayleigh_Super (the Fortran fv_dynamics.F90, rf_fast = .false., tau > 0; the reference has none): once per dycore step the
 * sponge levels' u, v and w are scaled by a per-level factor and, with conserve, the kinetic energy lost is added to pt as heat.
 * Non-hydrostatic.  met (dx, dy) and a11 .. a22 are what pace_c2l_ord takes; u, v, w, pt share the storage geometry of geom; pt is
 * the temperature.  factor: HOST array of nk doubles, each in (0, 1]: f[k] = 1 / (1 + rf[k]) on the leading damped levels, exactly
 * 1.0 from the first undamped level on; kmax = the number of leading levels with f[k] < 1.  On the levels k < kmax, in double on the
 * stored values (the float32 library widens first), without FMA and without a reciprocal, every input read before it is written:
 *   cells (i, j) of the compute domain -- origin (3, 3), extent (n, n):
 *     u1 = 2.0 * (u[i,j] * dx[i,j] + u[i,j+1] * dx[i,j+1]) / (dx[i,j] + dx[i,j+1])
 *     v1 = 2.0 * (v[i,j] * dy[i,j] + v[i+1,j] * dy[i+1,j]) / (dy[i,j] + dy[i+1,j])
 *     ua = a11 * u1 + a12 * v1,  va = a21 * u1 + a22 * v1                             (pace_c2l_ord, order 2, bit for bit)
 *     conserve:  pt[i,j,k] = (pace_real_t)(pt + ((0.5 * ((ua * ua + va * va) + w * w)) * (1.0 - f[k] * f[k])) * rcv)
 *     w[i,j,k] = (pace_real_t)(f[k] * w)
 *   u[i,j,k] = (pace_real_t)(f[k] * u) on (n, n + 1) points,  v[i,j,k] = (pace_real_t)(f[k] * v) on (n + 1, n) points
 * conserve = 1: TWO ordered launches (heat and w from the old winds; then the winds); conserve = 0: one; kmax = 0: none.  No
 * atomics, no workspace, no host synchronisation.  Nothing else is written (not the halo, not level nk, not the row padding,
 * no level >= kmax); u, v, w, pt and the six metric planes are read only on the compute domain plus the staggered row / column.
 * PACE_ERR_ARG, with nothing written: a NULL argument, conserve other than 0 / 1, with conserve an rcv that is not finite, a
 * factor that is NaN, <= 0 or > 1, a damped level after an undamped one, any two of u, v, w, pt the same array. */
int pace_rayleigh_super(const pace_geom_t* geom, const pace_metrics_t* met, const pace_real_t* a11, const pace_real_t* a12,
                        const pace_real_t* a21, const pace_real_t* a22, pace_real_t* u, pace_real_t* v, pace_real_t* w,
                        pace_real_t* pt, const double* factor, double rcv, int conserve, void* stream);

/* Per-stencil device implementations behind FrozenStencil (dsl/pace/dsl/stencil.py:395-434) for gtscript definitions that the
 * reference's Translate tests launch as stencils of their own: `id` selects the definition, `fields` are its field arguments in
 * the definition's order (2-D metric arguments come from `met`, K-fields are device arrays of nk + 1 entries), `scalars` its
 * float arguments, origin / domain the launch window (region statements write only inside it).
 *   PACE_ST_FLUX_CAPACITOR  d_sw.py:33-60     fields cx, cy, xflux, yflux, crx_adv, cry_adv, fx, fy
 *   PACE_ST_HEAT_DISS       d_sw.py:63-103    fields fx2, fy2, w, heat_source, diss_est, dw, damp_w (K), ke_bg (K); scalars dt
 *   PACE_ST_APPLY_FLUXES    d_sw.py:122-145   fields q, delp, gx, gy
 *   PACE_ST_UBKE / _VBKE    translate_d_sw.py:67-81 / 118-133 (d_sw.py interpolate_uc_vc_to_cell_corners)
 *                                             fields uc, vc, ut (vt), ub (vb); scalars dt5
 *   PACE_ST_COPY_CORNERS_X / _Y         corners.py:307-425   fields q_in, q_out
 *   PACE_ST_FILL_CORNERS_BGRID_X / _Y   corners.py:592-712   fields q_in, q_out
 *   PACE_ST_FILL_CORNERS_DGRID          corners.py:987-1151  fields x_in, x_out, y_in, y_out; scalars mysign
 *   PACE_ST_FILL_CORNERS_2CELLS_X / _Y  corners.py:170-177   fields q_out, q_in
 *   PACE_ST_XTP_U / _YTP_V   translate_xtp_u.py:13-23 / translate_ytp_v.py (xtp_u.py:9-91, ytp_v.py:9-91)
 *                            fields c (contravariant corner wind x dt), u (v), flux; scalars iord (5, 6 or 7)
 *   PACE_ST_MOIST_PT_LAST_STEP  moist_cv.py:84-118 (nwat = 6)  fields qvapor, qliquid, qrain, qsnow, qice, qgraupel, gz, pt, pkz;
 *                            scalars dtmp, r_vir
 *   PACE_ST_MOIST_PKZ        moist_cv.py:130-172 (nwat = 6; translate_moistcvpluspkz_2d.py:19)  fields qvapor, qliquid, qrain, qsnow,
 *                            qice, qgraupel, q_con, gz, cvm, pkz, pt, cappa, delp, delz; scalar r_vir
 *   PACE_ST_MOIST_PT         moist_cv.py:48-70 moist_pt_func as the stencil translate_moistcvpluspt_2d.py:9-50 builds  fields qvapor,
 *                            qliquid, qrain, qsnow, qice, qgraupel, q_con, pt, cappa, delp, delz; scalar r_vir */
enum {
  PACE_ST_FLUX_CAPACITOR = 1,
  PACE_ST_HEAT_DISS = 2,
  PACE_ST_APPLY_FLUXES = 3,
  PACE_ST_UBKE = 4,
  PACE_ST_VBKE = 5,
  PACE_ST_COPY_CORNERS_X = 6,
  PACE_ST_COPY_CORNERS_Y = 7,
  PACE_ST_FILL_CORNERS_BGRID_X = 8,
  PACE_ST_FILL_CORNERS_BGRID_Y = 9,
  PACE_ST_FILL_CORNERS_DGRID = 10,
  PACE_ST_FILL_CORNERS_2CELLS_X = 11,
  PACE_ST_FILL_CORNERS_2CELLS_Y = 12,
  PACE_ST_XTP_U = 13,
  PACE_ST_YTP_V = 14,
  PACE_ST_MOIST_PT_LAST_STEP = 15,
  PACE_ST_MOIST_PKZ = 16,
  PACE_ST_MOIST_PT = 17
};
int pace_stencil(const pace_geom_t* geom, const pace_metrics_t* met, int id, void* const* fields, int nfields, const double* scalars,
                 int nscalars, const int* origin, const int* domain, void* stream);


/* ---- Halo exchange pack / unpack: what HaloDataTransformer.async_pack / async_unpack do
 * (util/pace/util/halo_data_transformer.py:387-461 CPU, :560-921 GPU kernels), with the rotation
 * (rotate.py:4-50) and boundary slicing (_boundary_utils.py:58-95) folded into an affine index map.
 * Strip element (a, b, k), 0 <= a < na, 0 <= b < nb, 0 <= k < nk, lives at message offset (k*nb + b)*na + a
 * and at field index (i0 + a*di_a + b*di_b, j0 + a*dj_a + b*dj_b, k).  pack: buf = sign * field;
 * unpack: field = buf.  descs is a HOST array; field / buf are DEVICE pointers. */
typedef struct {
  pace_real_t* field;
  pace_real_t* buf;
  int32_t i0, j0, di_a, dj_a, di_b, dj_b;
  int32_t na, nb, nk, pad_;
  double sign;
} pace_halo_desc_t;
int pace_halo_pack(const pace_geom_t* geom, const pace_halo_desc_t* descs, int ndesc, void* stream);
int pace_halo_unpack(const pace_geom_t* geom, const pace_halo_desc_t* descs, int ndesc, void* stream);

/* ---- Halo update of tiles that share a device, without a message: one launch moves every strip of every field of every tile.
 * Entry t writes, for 0 <= a < na, 0 <= b < nb, 0 <= k < nk,
 *   dst[(ri0 + a, rj0 + b, k)] = sign * src[(i0 + a*di_a + b*di_b, j0 + a*dj_a + b*dj_b, k)]
 * -- the destination half is the receiver's strip of pace_halo_unpack, the source half the sender's strip of pace_halo_pack
 * (rotation, vector component swap and sign folded into the map).  All fields share `geom`.  dst / src are DEVICE pointers and
 * so is `table`: it holds hundreds of entries (6 tiles x 4 edges x fields), which the kernel reads in place, one per workgroup
 * row.  PACE_HALO_XFER_B_FAST: consecutive lanes walk b, not a (the host sets it where the longer unit-stride run lies along b).
 * The entries cannot be checked here: whoever builds the table guarantees that every strip lies inside its field's storage and
 * that no destination overlaps a source.  n == 0: nothing to do. */
#define PACE_HALO_XFER_B_FAST 1
typedef struct {
  pace_real_t* dst;
  const pace_real_t* src;
  int32_t ri0, rj0, na, nb, nk, flags;
  int32_t i0, j0, di_a, dj_a, di_b, dj_b;
  double sign;
} pace_halo_xfer_t;
int pace_halo_cube(const pace_geom_t* geom, const pace_halo_xfer_t* table_on_device, int n, void* stream);

/* ---- Gather and scatter across the cube (util/pace/util/communicator.py:111-329): windows of any number of fields of any of the
 * six tiles' storages of one geometry, moved between the fields and ONE dense device buffer by ONE launch, both storage types,
 * no atomics, no workspace, no host synchronisation.  The dense side of an item is (x, y, z) in C order, z fastest, at
 * dense + offset (the axis order of the reference's arrays and of pace_diag_pack); dense_type names its element type.
 *   pace_cube_gather    dense[offset + (i * nj + j) * nk + k] = (dense type) field(i0 + i, j0 + j, k0 + k)
 *   pace_cube_scatter   field(i0 + i, j0 + j, k0 + k) = (pace_real_t) dense[offset + (i * nj + j) * nk + k]
 * and for a PACE_DIAG_PLANE item the same with k0 = 0, nk = 1; its field points at element (0, 0) of a 2-D field or of ONE level
 * of a 3-D one.  The conversion is a plain cast (round to nearest even, overflow to +-inf); where the types agree (the float64
 * library with PACE_DENSE_F64, the float32 library with PACE_DENSE_F32) bits move unchanged: -0.0, NaN payloads, denormals.
 * Nothing outside a window is read or written on the field side, nothing outside an item's ni * nj * nk elements on the dense side.
 * table_on_device is DEVICE memory, read in place: n items, and right behind them int32_t first[n + 1], the prefix sums of the
 * items' tile counts (first[0] = 0, first[n] = all tiles), where an item has
 *   ceil(ni / 64) * ceil(nk / 32) * nj tiles (WINDOW3D),   ceil(ni / 64) * ceil(nj / 32) tiles (PLANE).
 * The entry point refuses only what it can see -- n < 1 or n > PACE_CUBE_MAX_ITEMS, an unknown dense_type, a NULL pointer
 * (PACE_ERR_ARG).  The entries cannot be checked here: whoever builds the table guarantees that every window is non-empty and
 * inside the storage (n + 7, n + 7, nk + 1), that no field is NULL, no offset negative, that the prefix table is the one above and
 * first[n] < 2^31, and for scatter that no two items overlap on one field (pace_amd/util/gather.py check_cube_items). */
#define PACE_CUBE_MAX_ITEMS 4096
enum { PACE_DENSE_F64 = 0, PACE_DENSE_F32 = 1 };
typedef struct {            /* one window of one field of one tile */
  void*   field;            /* element (0,0,0) of the storage (2-D field or one level's plane for a PLANE item) */
  int32_t kind;             /* PACE_DIAG_WINDOW3D | PACE_DIAG_PLANE */
  int32_t i0, j0, k0, ni, nj, nk;
  int64_t offset;           /* in elements of the dense buffer */
} pace_cube_item_t;
int pace_cube_gather(const pace_geom_t* geom, const pace_cube_item_t* table_on_device, int n, int dense_type, void* dense,
                     void* stream);
int pace_cube_scatter(const pace_geom_t* geom, const pace_cube_item_t* table_on_device, int n, int dense_type, const void* dense,
                      void* stream);

/* ---- Regridding the cube to a list of points (lat-lon diagnostics; no counterpart in the reference): piecewise-linear
 * interpolation of cell-centre fields of the six tiles' storages of one geometry to `npoints` target points, any number of
 * variables by ONE launch into ONE dense device buffer, both storage types, no atomics, no workspace, no host synchronisation.
 * A point names three source cells (tile, i, j) -- storage indices, the halo origin added -- and three float64 weights
 * (pace_amd/util/latlon.py builds them from the spherical Delaunay triangulation of the cell centres).  An item is one variable
 * given as its six tiles' pointers: PACE_DIAG_WINDOW3D with the levels k0 .. k0 + nk - 1, or PACE_DIAG_PLANE (nk is read as 1,
 * k0 as 0) whose pointers are at element (0, 0) of a 2-D field or of ONE level of a 3-D one.  With f_m(k) the stored value of
 * source m at level k, widened to double first in the float32 library,
 *   dense[offset + p * nk + k] = (dense type)((w0 * f_0(k0 + k) + w1 * f_1(k0 + k)) + w2 * f_2(k0 + k))
 * in double, in exactly this order, products then adds, without FMA; the cast is plain (round to nearest even, overflow to
 * +-inf).  NaN and inf propagate by ordinary arithmetic: 0 * NaN and 0 * inf are NaN.  Only the three named elements per point
 * and level are read, nothing is written outside an item's npoints * nk dense elements, and the storages are not written.
 * points_on_device and items_on_device are DEVICE memory, read in place: npoints points; n items, and right behind them
 * int32_t first[n + 1], the prefix sums of the items' tile counts (first[0] = 0, first[n] = all tiles), where an item has
 *   ceil(npoints / 64) * ceil(nk / 32) tiles (WINDOW3D),   ceil(npoints / 64) tiles (PLANE).
 * The entry point refuses only what it can see -- npoints < 1, n < 1 or n > PACE_REGRID_MAX_ITEMS (a variable is one item for
 * all six tiles, where pace_cube_gather's table has six), an unknown dense_type, a NULL pointer (PACE_ERR_ARG).  The entries
 * cannot be checked here: whoever builds the tables guarantees that every tile is 0 .. 5, every source inside the storage
 * (n + 7, n + 7; the host check asks for the compute domain), every weight finite, every kind one of the two, every level range inside nk + 1 levels, no field NULL, no
 * offset negative, the prefix table the one above and first[n] < 2^31 (pace_amd/util/latlon.py check_regrid_table,
 * check_regrid_items). */
#define PACE_REGRID_MAX_ITEMS 1024
typedef struct {            /* one target point: 64 bytes */
  int32_t tile[3];          /* the three sources: tile 0 .. 5, */
  int32_t i[3];             /* ... x and */
  int32_t j[3];             /* ... y index in the storage */
  int32_t pad_;
  double  w[3];             /* their weights */
} pace_regrid_point_t;
typedef struct {            /* one variable */
  void*   field[6];         /* element (0,0,0) of each tile's storage (2-D field or one level's plane for a PLANE item) */
  int32_t kind;             /* PACE_DIAG_WINDOW3D | PACE_DIAG_PLANE */
  int32_t k0, nk, pad_;
  int64_t offset;           /* in elements of the dense buffer */
} pace_regrid_item_t;
int pace_cube_regrid(const pace_geom_t* geom, const pace_regrid_point_t* points_on_device, int npoints,
                     const pace_regrid_item_t* items_on_device, int n, int dense_type, void* dense, void* stream);

const char* pace_version(void);
/* sizeof(pace_real_t) of this build: 8 (libpace_hip.so) or 4 (libpace_hip_f32.so). */
int pace_real_bytes(void);
/* Text of the last HIP error this library saw on the calling thread ("" if none). */
const char* pace_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
