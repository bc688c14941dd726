// extern "C" entry points of libpace_hip.so (declared in include/pace_hip.h).  Argument checking and
// struct unpacking only; kernels live in k_*.hip.
#include "common.h"
#include "kernels.h"
#include "thermo.h"

#include <cstdio>

thread_local char g_pace_err[256] = "";
int g_pace_sync_launches = pace_env_on("PACE_SYNC_LAUNCHES");
void pace_set_err(const char* where, hipError_t e) {
  snprintf(g_pace_err, sizeof(g_pace_err), "%s: %s", where, hipGetErrorString(e));
}

// Entry prologue: argument check, then drop any stale "last error" another library (e.g. the caching
// allocator's event queries) left on this thread, so PACE_CHECK_LAUNCH only reports our own launches.
// The geometry is validated on every entry: the kernels address fields with 32-bit byte offsets from a uniform base
// (k_fvtp2d.hip), so a field must stay below 4 GB, and the strides must cover the (N+7) x (N+7) x (nk+1) storage.
static inline int geom_check(const pace_geom_t* g) {
  if (g == nullptr) return PACE_ERR_ARG;
  if (g->n < 1 || g->nk < 1) return PACE_ERR_ARG;
  if (g->sj < g->n + 7 || g->sk < (int64_t)g->sj * (g->n + 7)) return PACE_ERR_ARG;
  if ((int64_t)(g->nk + 1) * g->sk * (int64_t)sizeof(real) >= ((int64_t)1 << 32)) return PACE_ERR_UNSUPPORTED;
  return PACE_OK;
}

#define NEED(p)                              \
  if (!(p)) return PACE_ERR_ARG;             \
  {                                          \
    const int geom_rc_ = geom_check(geom);   \
    if (geom_rc_ != PACE_OK) return geom_rc_; \
  }                                          \
  (void)hipGetLastError()

static inline hipStream_t S(void* s) { return (hipStream_t)s; }

// PACE_LEGACY_COLUMN_SOLVERS=1 selects the round-1 thread-per-column kernels of k_riem3.hip (kept for more than 128 layers and
// for A/B measurements, and the form that walks a column's levels IN THE REFERENCE'S ORDER: the whole acoustic loop then agrees with
// the oracle to w 6e-9 / diss_estd 1e-7 where the scans' re-association gives 4e-7 / 2e-6 -- tests/helpers.py ACOUSTIC_TOL).
static bool legacy_column_solvers() {
  return pace_env_on("PACE_LEGACY_COLUMN_SOLVERS");  // (read at every call: tests switch between the two forms within one process)
}

// The window of an item of the pack kernels (pace_diag_item_t, pace_unpack_item_t, pace_restart_item_t name these fields alike):
// a 3-D window or a plane (`columns`: or a column integral) of a field that is there, inside the storage's (n + 7)^2 points and
// nk + 1 levels; a plane is given by its field pointer alone: k0 = 0, nk = 1.
template <class Item>
static bool window_ok(const pace_geom_t* geom, const Item& it, bool columns = false) {
  const int ni = geom->n + 7, nlev = geom->nk + 1;
  if (it.kind != PACE_DIAG_WINDOW3D && it.kind != PACE_DIAG_PLANE && !(columns && it.kind == PACE_DIAG_COLUMN_INTEGRAL)) return false;
  if (!it.field) return false;
  if (it.i0 < 0 || it.ni < 1 || it.ni > ni - it.i0 || it.j0 < 0 || it.nj < 1 || it.nj > ni - it.j0) return false;
  return it.kind == PACE_DIAG_PLANE ? (it.k0 == 0 && it.nk == 1) : (it.k0 >= 0 && it.nk >= 1 && it.nk <= nlev - it.k0);
}

extern "C" {

const char* pace_last_error(void) { return g_pace_err; }

int pace_real_bytes(void) { return (int)sizeof(real); }

const char* pace_version(void) {
#ifdef PACE_EMU
  return "pace_amd 0.1 (CPU emulation build -- test infrastructure only)";
#else
  return "pace_amd 0.1 (gfx950)";
#endif
}

int pace_fxadv(const pace_geom_t* geom, const pace_metrics_t* met, const real* uc, const real* vc, real* crx,
               real* cry, real* xfx, real* yfx, real* ut, real* vt, double dt, void* stream) {
  NEED(geom && met && uc && vc && crx && cry && xfx && yfx && ut && vt);
  return launch_fxadv(make_geo(geom), *met, uc, vc, crx, cry, xfx, yfx, ut, vt, dt, nullptr, nullptr, S(stream), 0, 1);
}

int pace_fvtp2d(const pace_geom_t* geom, const pace_metrics_t* met, const real* q, const real* crx,
                const real* cry, const real* xfx, const real* yfx, real* fx, real* fy, const real* xmf,
                const real* ymf, int hord, int nlev, void* stream) {
  NEED(geom && met && q && crx && cry && xfx && yfx && fx && fy);
  if ((xmf == nullptr) != (ymf == nullptr)) return PACE_ERR_ARG;
  if (nlev < 1 || nlev > geom->nk + 1) return PACE_ERR_ARG;
  return launch_fvtp2d(make_geo(geom), *met, q, crx, cry, xfx, yfx, fx, fy, xmf, ymf, hord, nlev, S(stream));
}

int pace_fvtp2d_update(const pace_geom_t* geom, const pace_metrics_t* met, const real* q, const real* crx,
                       const real* cry, const real* x_area_flux, const real* y_area_flux,
                       const real* x_mass_flux, const real* y_mass_flux, const real* delp, const real* damp_k,
                       const real* nord_k, int nmax, real* qout, int hord, int nlev, void* stream) {
  NEED(geom && met && q && crx && cry && x_area_flux && y_area_flux && x_mass_flux && y_mass_flux && delp && damp_k && nord_k && qout);
  if (nlev < 1 || nlev > geom->nk + 1 || qout == q) return PACE_ERR_ARG;
  FvDamp dp{};
  dp.damp_k = damp_k; dp.nord_k = nord_k; dp.nmax = nmax; dp.mass_given = 1; dp.mass = delp;
  dp.qout = qout; dp.amass = delp;
  return launch_transport(make_geo(geom), *met, q, crx, cry, x_area_flux, y_area_flux, nullptr, nullptr, x_mass_flux, y_mass_flux,
                          hord, nlev, 2, 1, dp, S(stream));
}

int pace_delnflux_nosg(const pace_geom_t* geom, const pace_metrics_t* met, const real* q, real* fx2, real* fy2,
                       const real* damp_k, const real* nord_k, int nmax, int mass_given, int nlev, void* stream) {
  NEED(geom && met && q && fx2 && fy2 && damp_k && nord_k);
  if (nlev < 1 || nlev > geom->nk + 1) return PACE_ERR_ARG;
  return launch_delnflux(make_geo(geom), *met, 0, q, fx2, fy2, nullptr, damp_k, nord_k, nmax, mass_given, nlev, S(stream));
}

int pace_delnflux(const pace_geom_t* geom, const pace_metrics_t* met, const real* q, real* fx, real* fy,
                  const real* mass, const real* damp_k, const real* nord_k, int nmax, int nlev, void* stream) {
  NEED(geom && met && q && fx && fy && damp_k && nord_k);
  if (nlev < 1 || nlev > geom->nk + 1) return PACE_ERR_ARG;
  return launch_delnflux(make_geo(geom), *met, mass ? 2 : 1, q, fx, fy, mass, damp_k, nord_k, nmax, mass ? 1 : 0, nlev,
                         S(stream));
}

int pace_a2b_ord4(const pace_geom_t* geom, const pace_metrics_t* met, real* qin, real* qout, int k0, int k1,
                  int replace, void* stream) {
  NEED(geom && met && qin && qout);
  if (k0 < 0 || k1 <= k0 || k1 > geom->nk + 1) return PACE_ERR_ARG;
  return launch_a2b_ord4(make_geo(geom), *met, qin, qout, k0, k1, replace, S(stream));
}

int pace_ppm(const pace_geom_t* geom, const pace_metrics_t* met, int axis, int iord, const real* q_in, const real* c,
             real* q_mean_advected, int i0, int j0, int k0, int ni, int nj, int nk, void* stream) {
  NEED(geom && met && q_in && c && q_mean_advected);
  if (axis < 0 || axis > 1 || ni < 1 || nj < 1 || nk < 1 || k0 < 0 || k0 + nk > geom->nk + 1) return PACE_ERR_ARG;
  // the window must leave the three cells an interface needs on either side inside the storage
  const int lo_i = axis == 0 ? 3 : 0, lo_j = axis == 1 ? 3 : 0;
  if (i0 < lo_i || j0 < lo_j || i0 + ni > geom->n + 7 - (axis == 0 ? 2 : 0) || j0 + nj > geom->n + 7 - (axis == 1 ? 2 : 0))
    return PACE_ERR_ARG;
  return launch_ppm1d(make_geo(geom), *met, axis, iord, q_in, c, q_mean_advected, i0, j0, k0, ni, nj, nk, S(stream));
}

int64_t pace_divergence_damping_workspace_bytes(const pace_geom_t* geom) {
  return geom ? (int64_t)2 * geom->sk * (geom->nk + 1) * (int64_t)sizeof(real) : 0;
}

int pace_divergence_damping(const pace_geom_t* geom, const pace_metrics_t* met, void* workspace, const real* u, const real* v,
                            const real* va, real* damped_rel_vort_bgrid, const real* ua, real* divg_d, real* vc,
                            real* uc, real* delpc, real* ke, const real* rel_vort_agrid, double dt,
                            const double* nord_col_host, const real* d2_bg_dev, double dddmp, double d4_bg, int nord,
                            void* stream) {
  NEED(geom && met && workspace && u && v && va && damped_rel_vort_bgrid && ua && divg_d && vc && uc && delpc && ke);
  NEED(rel_vort_agrid && nord_col_host && d2_bg_dev);
  const Geo g = make_geo(geom);
  // the column is split at the first level with nord > 0 (divergence_damping.py:307-331)
  int kstart = 0, nonzero_nord = nord;
  for (int k = 0; k < g.nk; ++k)
    if (nord_col_host[k] > 0) {
      kstart = k;
      nonzero_nord = (int)nord_col_host[k];
      break;
    }
  if (nonzero_nord < 0 || nonzero_nord > 3) return PACE_ERR_UNSUPPORTED;
  real* da = (real*)workspace;
  real* db = da + (long)g.sk * (g.nk + 1);
  return launch_divergence_damping(g, *met, u, v, va, damped_rel_vort_bgrid, ua, divg_d, vc, uc, delpc, ke, rel_vort_agrid, dt,
                                   d2_bg_dev, kstart, nonzero_nord, dddmp, d4_bg, da, db, S(stream));
}

int64_t pace_d_sw_workspace_bytes(const pace_geom_t* geom) { return geom ? dsw_workspace_bytes(make_geo(geom)) : 0; }

int pace_d_sw_pingpong_supported(const pace_geom_t* geom, const pace_dsw_config_t* cfg) {
  return (geom && cfg && dsw_pingpong_supported(make_geo(geom), cfg)) ? 1 : 0;
}
int pace_d_sw_wind_outputs_supported(const pace_geom_t* geom, const pace_dsw_config_t* cfg) {
  return pace_d_sw_pingpong_supported(geom, cfg);  // (the kernel that gives the scalars outputs of their own takes the winds too)
}

int pace_d_sw_outputs_supported(const pace_geom_t* geom, const pace_column_t* col, const pace_dsw_config_t* cfg) {
  // the ONE predicate of what launch_d_sw accepts: the query above plus the condition on the column namelist it cannot see
  if (!geom || !col || !cfg || !col->nord_v || !col->nord_w || !col->nord_t) return 0;
  return dsw_outputs_supported(make_geo(geom), col, cfg);
}

int pace_d_sw_prepare(const pace_geom_t* geom, const pace_column_t* col, void* workspace, void* stream) {
  NEED(geom && col && workspace);
  return dsw_prepare(make_geo(geom), col, workspace, S(stream));
}

static int d_sw_entry(int phases, const pace_geom_t* geom, const pace_metrics_t* met, const pace_column_t* col,
                      const pace_dsw_config_t* cfg, void* workspace, const DswFields& f, void* stream) {
  NEED(geom && met && col && cfg && workspace);
  NEED(f.delpc && f.delp && f.pt && f.u && f.v && f.w && f.uc && f.vc && f.ua && f.va && f.divgd && f.mfx && f.mfy && f.cx && f.cy);
  NEED(f.crx && f.cry && f.xfx && f.yfx && f.q_con && f.heat_source && f.diss_est);
  if (cfg->struct_bytes != (int32_t)sizeof(pace_dsw_config_t)) return PACE_ERR_ARG;  // built against another header
  // separate outputs: all four or none, none of them an input
  const int given = (cfg->delp_out != nullptr) + (cfg->pt_out != nullptr) + (cfg->w_out != nullptr) + (cfg->q_con_out != nullptr);
  if (given != 0 && given != 4) return PACE_ERR_ARG;
  if (given && (cfg->delp_out == f.delp || cfg->pt_out == f.pt || cfg->w_out == f.w || cfg->q_con_out == f.q_con)) return PACE_ERR_ARG;
  if (given && ((((uintptr_t)cfg->delp_out | (uintptr_t)cfg->pt_out | (uintptr_t)cfg->w_out | (uintptr_t)cfg->q_con_out) & 15) != 0))
    return PACE_ERR_ARG;  // (16-byte rows, as the header says)
  // ... of the winds: both or none, only with the four, only in a call that runs scalars and winds together
  const int winds = (cfg->u_out != nullptr) + (cfg->v_out != nullptr);
  if (winds == 1 || (winds && !given) || (winds && (cfg->u_out == f.u || cfg->v_out == f.v || cfg->u_out == cfg->v_out))) return PACE_ERR_ARG;
  // (they are written by the kernel of phases 2 + 4 + 8 / 256; a call without 2 and 8 does not touch the winds' outputs)
  if (winds && ((phases & 2) || (phases & 8)) && !((phases & 2) && (phases & 4) && (phases & 8))) return PACE_ERR_ARG;
  return launch_d_sw(make_geo(geom), *met, col, cfg, workspace, phases, f, S(stream));
}

// the ABI signature of the d_sw entry points (include/pace_hip.h), and its field arguments as the bundle the launcher takes
#define DSW_PARAMS                                                                                                        \
  const pace_geom_t *geom, const pace_metrics_t *met, const pace_column_t *col, const pace_dsw_config_t *cfg,            \
      void *workspace, real *delpc, real *delp, real *pt, real *u, real *v, real *w, real *uc, real *vc,  \
      const real *ua, const real *va, real *divgd, real *mfx, real *mfy, real *cx, real *cy, real *crx,   \
      real *cry, real *xfx, real *yfx, real *q_con, const real *zh, real *heat_source, real *diss_est,       \
      double dt, void *stream
#define DSW_FIELDS \
  DswFields { delpc, delp, pt, u, v, w, uc, vc, ua, va, divgd, mfx, mfy, cx, cy, crx, cry, xfx, yfx, q_con, heat_source, diss_est, dt }

int pace_d_sw(DSW_PARAMS) { return d_sw_entry(15, geom, met, col, cfg, workspace, DSW_FIELDS, stream); }
int pace_d_sw_transport(DSW_PARAMS) { return d_sw_entry(3, geom, met, col, cfg, workspace, DSW_FIELDS, stream); }
int pace_d_sw_winds(DSW_PARAMS) { return d_sw_entry(12, geom, met, col, cfg, workspace, DSW_FIELDS, stream); }
int pace_d_sw_phases(int phases, DSW_PARAMS) {
  if (phases < 1 || phases > 256 || ((phases & 1) && (phases & 48)) || ((phases & 4) && (phases & 192)) || ((phases & 256) && phases != 256))
    return PACE_ERR_ARG;  // (1 and 16 / 32, 4 and 64 / 128 are alternatives; 256 stands alone)
  return d_sw_entry(phases, geom, met, col, cfg, workspace, DSW_FIELDS, stream);
}

// d_sw with its wind half on a second stream, in ONE call (the host layer used to make four calls and three event operations
// per d_sw; the host time per substep, 105 - 120 us, is the runtime's launches and did not change).  `prep`: 1 = the whole flux preparation, 32 = its frame (the interior was
// started with phases 16).  Events: the caller's (e.g. torch.cuda.Event.cuda_event), recorded here; afterwards the caller makes
// its stream wait for ev_done before it touches u, v, uc, vc, heat_source, diss_est, delpc or divgd (pace_amd ... d_sw.py join()).
int pace_d_sw_overlapped(int prep, DSW_PARAMS, void* side_stream, void* ev_prep, void* ev_scalars, void* ev_done) {
  const DswFields f = DSW_FIELDS;
  const auto run = [&](int phases, void* on) { return d_sw_entry(phases, geom, met, col, cfg, workspace, f, on); };
#ifdef PACE_EMU
  (void)side_stream; (void)ev_prep; (void)ev_scalars; (void)ev_done;
  if (prep != 1 && prep != 32) return PACE_ERR_ARG;
  return run(prep | 14, stream);
#else
  NEED(side_stream && ev_prep && ev_scalars && ev_done);
  if (prep != 1 && prep != 32) return PACE_ERR_ARG;
  hipStream_t main_s = S(stream), side_s = S(side_stream);
  hipEvent_t e_prep = (hipEvent_t)ev_prep, e_scal = (hipEvent_t)ev_scalars, e_done = (hipEvent_t)ev_done;
  int rc;
  if (geom && cfg && dsw_pingpong_supported(make_geo(geom), cfg)) {
    // the winds are the last pass of the kernel that transports the scalars: one stream, nothing left for the side stream (the
    // kinetic energy there next to vorticity + divergence damping measured slower: profiles/r05_experiments x05)
    if ((rc = run(prep | 14, stream))) return rc;
    return hipEventRecord(e_done, main_s) != hipSuccess ? PACE_ERR_LAUNCH : PACE_OK;
  }
  if ((rc = run(prep, stream))) return rc;  // flux preparation on the caller's stream
  if (hipEventRecord(e_prep, main_s) != hipSuccess || hipStreamWaitEvent(side_s, e_prep, 0) != hipSuccess) return PACE_ERR_LAUNCH;
  if ((rc = run(4, side_stream))) return rc;  // winds A next to the scalar transports
  if ((rc = run(2, stream))) return rc;       // the scalars on the caller's stream
  if (hipEventRecord(e_scal, main_s) != hipSuccess || hipStreamWaitEvent(side_s, e_scal, 0) != hipSuccess) return PACE_ERR_LAUNCH;
  if ((rc = run(8, side_stream))) return rc;  // winds B (they need the new delp) next to whatever the caller launches next
  return hipEventRecord(e_done, side_s) != hipSuccess ? PACE_ERR_LAUNCH : PACE_OK;
#endif
}

int64_t pace_riem_solver3_workspace_bytes(const pace_geom_t* geom) {
  return geom ? riem3_workspace_bytes(make_geo(geom)) : 0;
}

int pace_riem_solver3(const pace_geom_t* geom, void* workspace, int last_call, double dt, const real* cappa,
                      double ptop, const real* zs, const real* ws, real* delz, const real* q_con,
                      const real* delp, const real* pt, real* zh, real* pe, real* ppe, real* pk3, real* pk,
                      real* peln, real* w, double p_fac, void* stream) {
  NEED(geom && workspace && cappa && zs && ws && delz && q_con && delp && pt && zh && pe && ppe && pk3 && pk && peln && w);
  const Geo g = make_geo(geom);
  if (riem_column_supported(g) && !legacy_column_solvers())
    return launch_riem_solver3_column(g, last_call, dt, cappa, ptop, zs, ws, delz, q_con, delp, pt, zh, pe, ppe, pk3, pk, peln, w,
                                      p_fac, S(stream));
  return launch_riem_solver3(g, workspace, last_call, dt, cappa, ptop, zs, ws, delz, q_con, delp, pt, zh, pe, ppe, pk3, pk, peln,
                             w, p_fac, S(stream));
}

int64_t pace_c_sw_workspace_bytes(const pace_geom_t* geom) { return geom ? csw_workspace_bytes(make_geo(geom)) : 0; }

int pace_c_sw(const pace_geom_t* geom, const pace_metrics_t* met, void* workspace, real* delpc, real* ptc,
              real* delp, real* pt, const real* u, const real* v, real* w, real* uc,
              real* vc, real* ua, real* va, real* ut, real* vt, real* divgd, real* omga, double dt2,
              int nord, void* stream) {
  NEED(geom && met && workspace && delpc && ptc && delp && pt && u && v && w && uc && vc && ua && va && ut && vt && divgd && omga);
  return launch_c_sw(make_geo(geom), *met, workspace, delpc, ptc, delp, pt, u, v, w, uc, vc, ua, va, ut, vt, divgd, omga, dt2,
                     nord, S(stream));
}

int pace_c_sw_part(int part, const pace_geom_t* geom, const pace_metrics_t* met, void* workspace, real* delpc, real* ptc,
                   real* delp, real* pt, const real* u, const real* v, real* w, real* uc,
                   real* vc, real* ua, real* va, real* ut, real* vt, real* divgd, real* omga, double dt2,
                   int nord, void* stream) {
  NEED(geom && met && workspace && delpc && ptc && delp && pt && u && v && w && uc && vc && ua && va && ut && vt && divgd && omga);
  if (part < 0 || part > 2) return PACE_ERR_ARG;
  return launch_c_sw(make_geo(geom), *met, workspace, delpc, ptc, delp, pt, u, v, w, uc, vc, ua, va, ut, vt, divgd, omga, dt2,
                     nord, S(stream), part);
}

int pace_d2a2c_vect(const pace_geom_t* geom, const pace_metrics_t* met, void* workspace, real* uc, real* vc,
                    const real* u, const real* v, real* ua, real* va, real* utc, real* vtc, void* stream) {
  NEED(geom && met && workspace && uc && vc && u && v && ua && va && utc && vtc);
  return launch_d2a2c_vect(make_geo(geom), *met, workspace, uc, vc, u, v, ua, va, utc, vtc, S(stream));
}

int64_t pace_riem_solver_c_workspace_bytes(const pace_geom_t* geom) {
  return geom ? riemc_workspace_bytes(make_geo(geom)) : 0;
}

int pace_riem_solver_c(const pace_geom_t* geom, void* workspace, double dt2, const real* cappa, double ptop,
                       const real* hs, const real* ws, const real* ptc, const real* q_con,
                       const real* delpc, real* gz, real* pef, const real* w3, double p_fac, void* stream) {
  NEED(geom && workspace && cappa && hs && ws && ptc && q_con && delpc && gz && pef && w3);
  const Geo g = make_geo(geom);
  if (riem_column_supported(g) && !legacy_column_solvers())
    return launch_riem_solver_c_column(g, dt2, cappa, ptop, hs, ws, ptc, q_con, delpc, gz, pef, w3, p_fac, S(stream));
  return launch_riem_solver_c(g, workspace, dt2, cappa, ptop, hs, ws, ptc, q_con, delpc, gz, pef, w3, p_fac, S(stream));
}

int64_t pace_sim1_solver_workspace_bytes(const pace_geom_t* geom) { return geom ? sim1_workspace_bytes(make_geo(geom)) : 0; }

int pace_sim1_solver(const pace_geom_t* geom, void* workspace, int n_halo, double dt, double p_fac, const real* gamma,
                     const real* cp3, real* pe, const real* delta_mass, const real* pm, const real* pem, real* w,
                     real* dz, const real* potential_temperature, const real* ws, void* stream) {
  NEED(geom && workspace && gamma && cp3 && pe && delta_mass && pm && pem && w && dz && potential_temperature && ws);
  if (n_halo < 0 || n_halo > 3 || geom->nk < 2) return PACE_ERR_ARG;
  return launch_sim1_solver(make_geo(geom), workspace, n_halo, dt, p_fac, gamma, cp3, pe, delta_mass, pm, pem, w, dz,
                            potential_temperature, ws, S(stream));
}

int64_t pace_updatedzc_workspace_bytes(const pace_geom_t* geom) {
  return geom ? updatedzc_workspace_bytes(make_geo(geom)) : 0;
}

int pace_updatedzc(const pace_geom_t* geom, const pace_metrics_t* met, void* workspace, const real* dp_ref,
                   const real* zs, const real* ut, const real* vt, real* gz, real* ws, double dt,
                   void* stream) {
  NEED(geom && met && workspace && dp_ref && zs && ut && vt && gz && ws);
  return launch_updatedzc(make_geo(geom), *met, workspace, dp_ref, zs, ut, vt, gz, ws, dt, S(stream));
}

int64_t pace_updatedzd_workspace_bytes(const pace_geom_t* geom) {
  return geom ? updatedzd_workspace_bytes(make_geo(geom)) : 0;
}

int pace_updatedzd(const pace_geom_t* geom, const pace_metrics_t* met, void* workspace, const pace_updatedzd_k_t* kc,
                   const real* surface_height, real* height, const real* courant_number_x,
                   const real* courant_number_y, const real* x_area_flux, const real* y_area_flux, real* ws,
                   double dt, int hord_tm, void* stream) {
  NEED(geom && met && workspace && kc && surface_height && height && courant_number_x && courant_number_y && x_area_flux &&
       y_area_flux && ws);
  NEED(kc->gk && kc->beta && kc->gamma && kc->damp && kc->nord);
  return launch_updatedzd(make_geo(geom), *met, workspace, kc, surface_height, height, courant_number_x, courant_number_y,
                          x_area_flux, y_area_flux, ws, dt, hord_tm, S(stream));
}

int pace_zero_data(const pace_geom_t* geom, real* mfxd, real* mfyd, real* cxd, real* cyd, real* heat_source,
                   real* diss_estd, int first_timestep, void* stream) {
  NEED(geom && mfxd && mfyd && cxd && cyd && heat_source && diss_estd);
  return launch_zero_data(make_geo(geom), mfxd, mfyd, cxd, cyd, heat_source, diss_estd, first_timestep, S(stream));
}

int pace_interface_pressure_from_toa_pressure_and_thickness(const pace_geom_t* geom, const real* delp, real* pem,
                                                            double ptop, void* stream) {
  NEED(geom && delp && pem);
  return launch_interface_pressure(make_geo(geom), delp, pem, ptop, S(stream));
}

int pace_gz_from_surface_height_and_thicknesses(const pace_geom_t* geom, const real* zs, const real* delz,
                                                real* gz, void* stream) {
  NEED(geom && zs && delz && gz);
  return launch_gz_from_surface(make_geo(geom), zs, delz, gz, S(stream));
}

int pace_compute_geopotential(const pace_geom_t* geom, const real* zh, real* gz, void* stream) {
  NEED(geom && zh && gz);
  return launch_scale_copy(make_geo(geom), zh, gz, phys::GRAV, 1, 2, geom->nk + 1, S(stream));
}

int pace_copy(const pace_geom_t* geom, const real* src, real* dst, void* stream) {
  NEED(geom && src && dst);
  return launch_scale_copy(make_geo(geom), src, dst, 1.0, 0, 3, geom->nk + 1, S(stream));
}

int pace_p_grad_c(const pace_geom_t* geom, const pace_metrics_t* met, real* uc, real* vc, const real* delpc,
                  const real* pkc, const real* gz, double dt2, void* stream) {
  NEED(geom && met && uc && vc && delpc && pkc && gz);
  return launch_p_grad_c(make_geo(geom), *met, uc, vc, delpc, pkc, gz, dt2, S(stream));
}

int64_t pace_nh_p_grad_workspace_bytes(const pace_geom_t* geom) {
  return geom ? nh_p_grad_workspace_bytes(make_geo(geom)) : 0;
}

int pace_nh_p_grad(const pace_geom_t* geom, const pace_metrics_t* met, void* workspace, real* u, real* v,
                   real* pp, real* gz, real* pk3, real* delp, double dt, double ptop, double akap,
                   void* stream) {
  NEED(geom && met && workspace && u && v && pp && gz && pk3 && delp);
  return launch_nh_p_grad(make_geo(geom), *met, workspace, u, v, pp, gz, pk3, delp, dt, ptop, akap, S(stream));
}

int pace_edge_pe(const pace_geom_t* geom, real* pe, const real* delp, double ptop, void* stream) {
  NEED(geom && pe && delp);
  return launch_edge_pe(make_geo(geom), pe, delp, ptop, S(stream));
}

int pace_pk3_halo(const pace_geom_t* geom, real* pk3, const real* delp, double ptop, double akap, void* stream) {
  NEED(geom && pk3 && delp);
  return launch_pk3_halo(make_geo(geom), pk3, delp, ptop, akap, S(stream));
}

int pace_ray_fast(const pace_geom_t* geom, real* u, real* v, real* w, const double* dp, const double* pfull,
                  double dt, double ptop, double rf_cutoff, double tau, int hydrostatic, void* stream) {
  NEED(geom && u && v && w && dp && pfull);
  return launch_ray_fast(make_geo(geom), u, v, w, dp, pfull, dt, ptop, rf_cutoff, tau, hydrostatic, S(stream));
}

int64_t pace_del2cubed_workspace_bytes(const pace_geom_t* geom) {
  return geom ? del2cubed_workspace_bytes(make_geo(geom)) : 0;
}

int pace_del2cubed(const pace_geom_t* geom, const pace_metrics_t* met, void* workspace, real* qdel, double cd,
                   int nmax, void* stream) {
  NEED(geom && met && workspace && qdel);
  return launch_del2cubed(make_geo(geom), *met, workspace, qdel, cd, nmax, S(stream));
}

int pace_apply_diffusive_heating(const pace_geom_t* geom, const real* delp, const real* delz, const real* cappa,
                                 const real* heat_source, real* pt, double delt_time_factor, int nlev,
                                 void* stream) {
  NEED(geom && delp && delz && cappa && heat_source && pt);
  if (nlev < 0 || nlev > geom->nk) return PACE_ERR_ARG;
  return launch_diffusive_heating(make_geo(geom), delp, delz, cappa, heat_source, pt, delt_time_factor, nlev, S(stream));
}

int pace_tracer_flux_compute(const pace_geom_t* geom, const pace_metrics_t* met, const real* cx, const real* cy,
                             real* xfx, real* yfx, void* stream) {
  NEED(geom && met && cx && cy && xfx && yfx);
  return launch_tracer_flux_compute(make_geo(geom), *met, cx, cy, xfx, yfx, S(stream));
}

int pace_tracer_divide_fluxes(const pace_geom_t* geom, real* cxd, real* xfx, real* mfxd, real* cyd, real* yfx,
                              real* mfyd, int n_split, void* stream) {
  NEED(geom && cxd && xfx && mfxd && cyd && yfx && mfyd);
  if (n_split < 1) return PACE_ERR_ARG;
  return launch_tracer_divide(make_geo(geom), cxd, xfx, mfxd, cyd, yfx, mfyd, n_split, S(stream));
}

int pace_apply_mass_flux(const pace_geom_t* geom, const pace_metrics_t* met, const real* dp1, const real* x_mass_flux,
                         const real* y_mass_flux, real* dp2, void* stream) {
  NEED(geom && met && dp1 && x_mass_flux && y_mass_flux && dp2);
  return launch_apply_mass_flux(make_geo(geom), *met, dp1, x_mass_flux, y_mass_flux, dp2, S(stream));
}

int pace_apply_tracer_flux(const pace_geom_t* geom, const pace_metrics_t* met, real* q, const real* dp1,
                           const real* fx, const real* fy, const real* dp2, void* stream) {
  NEED(geom && met && q && dp1 && fx && fy && dp2);
  return launch_apply_tracer_flux(make_geo(geom), *met, q, dp1, fx, fy, dp2, S(stream));
}

int pace_swap_dp(const pace_geom_t* geom, real* dp1, real* dp2, void* stream) {
  NEED(geom && dp1 && dp2);
  return launch_swap_dp(make_geo(geom), dp1, dp2, S(stream));
}

int pace_tracer_cmax(const pace_geom_t* geom, const real* cx, const real* cy, const real* sin_sg5, double* cmax, void* stream) {
  NEED(geom && cx && cy && sin_sg5 && cmax);
  const void* const out = (const void*)cmax;
  if (out == (const void*)cx || out == (const void*)cy || out == (const void*)sin_sg5) return PACE_ERR_ARG;
  return launch_tracer_cmax(make_geo(geom), cx, cy, sin_sg5, cmax, S(stream));
}

int pace_tracer_subcycles(const double* const* cmax_tables, int ntiles, int nk, int max_subcycles, int32_t* out, void* stream) {
  if (!cmax_tables || !out || ntiles < 1 || ntiles > PACE_TRACER_MAX_TILES || nk < 1 || nk > PACE_TRACER_MAX_LEVELS ||
      max_subcycles < 1 || max_subcycles > PACE_TRACER_MAX_SUBCYCLES)
    return PACE_ERR_ARG;
  for (int t = 0; t < ntiles; ++t)
    if (!cmax_tables[t] || (const void*)cmax_tables[t] == (const void*)out) return PACE_ERR_ARG;
  (void)hipGetLastError();
  return launch_tracer_subcycles(cmax_tables, ntiles, nk, max_subcycles, out, S(stream));
}

int pace_tracer_divide_fluxes_levels(const pace_geom_t* geom, real* cxd, real* xfx, real* mfxd, real* cyd, real* yfx, real* mfyd,
                                     const int32_t* ksplt, void* stream) {
  NEED(geom && cxd && xfx && mfxd && cyd && yfx && mfyd && ksplt);
  for (const real* p : {cxd, xfx, mfxd, cyd, yfx, mfyd})
    if ((const void*)p == (const void*)ksplt) return PACE_ERR_ARG;
  return launch_tracer_divide_levels(make_geo(geom), cxd, xfx, mfxd, cyd, yfx, mfyd, ksplt, S(stream));
}

int pace_apply_mass_flux_levels(const pace_geom_t* geom, const pace_metrics_t* met, const real* dp1, const real* x_mass_flux,
                                const real* y_mass_flux, real* dp2, const int32_t* ksplt, int min_subcycles, void* stream) {
  NEED(geom && met && dp1 && x_mass_flux && y_mass_flux && dp2 && ksplt);
  if (min_subcycles < 1) return PACE_ERR_ARG;
  if (dp2 == dp1 || dp2 == x_mass_flux || dp2 == y_mass_flux || (const void*)dp2 == (const void*)ksplt) return PACE_ERR_ARG;
  return launch_apply_mass_flux_levels(make_geo(geom), *met, dp1, x_mass_flux, y_mass_flux, dp2, ksplt, min_subcycles, S(stream));
}

int pace_apply_tracer_flux_levels(const pace_geom_t* geom, const pace_metrics_t* met, real* q, const real* dp1, const real* fx,
                                  const real* fy, const real* dp2, const int32_t* ksplt, int min_subcycles, void* stream) {
  NEED(geom && met && q && dp1 && fx && fy && dp2 && ksplt);
  if (min_subcycles < 1) return PACE_ERR_ARG;
  if (q == dp1 || q == fx || q == fy || q == dp2 || (const void*)q == (const void*)ksplt) return PACE_ERR_ARG;
  return launch_apply_tracer_flux_levels(make_geo(geom), *met, q, dp1, fx, fy, dp2, ksplt, min_subcycles, S(stream));
}

int pace_swap_dp_levels(const pace_geom_t* geom, real* dp1, real* dp2, const int32_t* ksplt, int min_subcycles, void* stream) {
  NEED(geom && dp1 && dp2 && ksplt);
  if (min_subcycles < 1) return PACE_ERR_ARG;
  if (dp1 == dp2 || (const void*)dp1 == (const void*)ksplt || (const void*)dp2 == (const void*)ksplt) return PACE_ERR_ARG;
  return launch_swap_dp_levels(make_geo(geom), dp1, dp2, ksplt, min_subcycles, S(stream));
}

static int halo_check(const pace_geom_t* geom, const pace_halo_desc_t* d, int n) {
  const int ni = geom->n + 7;
  for (int t = 0; t < n; ++t) {
    if (!d[t].field || !d[t].buf || d[t].na < 1 || d[t].nb < 1 || d[t].nk < 1 || d[t].nk > geom->nk + 1) return PACE_ERR_ARG;
    for (int ca = 0; ca < 2; ++ca)
      for (int cb = 0; cb < 2; ++cb) {
        const int a = ca ? d[t].na - 1 : 0, b = cb ? d[t].nb - 1 : 0;
        const int i = d[t].i0 + a * d[t].di_a + b * d[t].di_b, j = d[t].j0 + a * d[t].dj_a + b * d[t].dj_b;
        if (i < 0 || i >= ni || j < 0 || j >= ni) return PACE_ERR_ARG;
      }
  }
  return PACE_OK;
}

int64_t pace_map_single_workspace_bytes(const pace_geom_t* geom) {
  return geom ? map_single_workspace_bytes(make_geo(geom), 1) : 0;
}

int pace_map_single(const pace_geom_t* geom, void* workspace, real* q1, const real* pe1, const real* pe2,
                    const real* qs, double qmin, int kord, int iv, int xstag, int ystag, void* stream) {
  NEED(geom && workspace && q1 && pe1 && pe2);
  return launch_map_fields(make_geo(geom), workspace, &q1, 1, pe1, pe2, qs, qmin, kord, iv, xstag, ystag, S(stream));
}

int64_t pace_mapn_tracer_workspace_bytes(const pace_geom_t* geom, int nq) {
  return (geom && nq > 0) ? map_single_workspace_bytes(make_geo(geom), nq) : 0;
}

int pace_mapn_tracer(const pace_geom_t* geom, void* workspace, real* const* tracers, int nq, const real* pe1,
                     const real* pe2, int kord, void* stream) {
  NEED(geom && workspace && tracers && pe1 && pe2);
  return launch_map_fields(make_geo(geom), workspace, tracers, nq, pe1, pe2, nullptr, 0.0, kord, 0, 0, 0, S(stream));
}

int pace_fillz(const pace_geom_t* geom, real* const* tracers, int nq, const real* dp2, void* stream) {
  NEED(geom && tracers && dp2);
  return launch_fillz(make_geo(geom), tracers, nq, dp2, S(stream));
}

static bool six(const real* const* w) {
  if (!w) return false;
  for (int n = 0; n < 6; ++n)
    if (!w[n]) return false;
  return true;
}

int pace_l2e_prepare(const pace_geom_t* geom, const real* const* water, real* q_con, real* pt, real* cappa, real* delp,
                     real* delz, const real* pe, real* pe1, real* pe2, const real* ak, const real* bk, real* dp2,
                     real* ps, real* pn2, const real* peln, real* pk, double ptop, double akap, double r_vir,
                     void* stream) {
  NEED(geom && six(water) && q_con && pt && cappa && delp && delz && pe && pe1 && pe2 && ak && bk && dp2 && ps && pn2 && peln && pk);
  return launch_l2e_prepare(make_geo(geom), water, q_con, pt, cappa, delp, delz, pe, pe1, pe2, ak, bk, dp2, ps, pn2, peln, pk,
                            ptop, akap, r_vir, S(stream));
}

int pace_l2e_post(const pace_geom_t* geom, const real* const* water, real* q_con, real* pkz, const real* pt,
                  real* cappa, const real* delp, real* delz, real* peln, real* pe0, const real* pn2, double r_vir,
                  void* stream) {
  NEED(geom && six(water) && q_con && pkz && pt && cappa && delp && delz && peln && pe0 && pn2);
  return launch_l2e_post(make_geo(geom), water, q_con, pkz, pt, cappa, delp, delz, peln, pe0, pn2, r_vir, S(stream));
}

int pace_l2e_pressures(const pace_geom_t* geom, int dir, const real* pe, const real* pe1, const real* ak,
                       const real* bk, real* pe0, real* pe3, void* stream) {
  NEED(geom && pe && pe1 && ak && bk && pe0 && pe3);
  if (dir != 0 && dir != 1) return PACE_ERR_ARG;
  return launch_l2e_pressures(make_geo(geom), dir, pe, pe1, ak, bk, pe0, pe3, S(stream));
}

int pace_l2e_finish(const pace_geom_t* geom, const real* const* water, real* pe, const real* pe2, real* pt,
                    const real* pkz, double r_vir, int last_step, void* stream) {
  NEED(geom && six(water) && pe && pe2 && pt && pkz);
  return launch_l2e_finish(make_geo(geom), water, pe, pe2, pt, pkz, r_vir, last_step, S(stream));
}

int pace_l2e_finish_dtmp(const pace_geom_t* geom, const real* const* water, real* pe, const real* pe2, real* pt,
                         const real* pkz, double r_vir, const double* energy_result, void* stream) {
  NEED(geom && six(water) && pe && pe2 && pt && pkz && energy_result);
  return launch_l2e_finish_dtmp(make_geo(geom), water, pe, pe2, pt, pkz, r_vir, energy_result, S(stream));
}

int pace_energy_columns(const pace_geom_t* geom, int mode, const real* const* water, const real* pt, const real* delp,
                        const real* delz, const real* w, const real* u, const real* v, const real* pkz, const real* phis,
                        const real* rsin2, const real* cosa_s, const real* area, real* te0_2d, real* te_2d, real* zsum1,
                        int64_t* words, double r_vir, void* stream) {
  NEED(geom && six(water) && pt && delp && delz && w && u && v && phis && rsin2 && cosa_s && te0_2d);
  if (mode != 0 && mode != 1) return PACE_ERR_ARG;
  const real* const in[] = {water[0], water[1], water[2], water[3], water[4], water[5], pt, delp, delz, w, u, v, pkz, phis, rsin2,
                            cosa_s, area};
  if (mode == 1) {
    if (!(pkz && area && te_2d && zsum1 && words)) return PACE_ERR_ARG;
    if (te_2d == zsum1 || te_2d == te0_2d || zsum1 == te0_2d) return PACE_ERR_ARG;
    if ((const void*)words == (const void*)te_2d || (const void*)words == (const void*)zsum1) return PACE_ERR_ARG;
    for (const real* p : in)
      if (p == te_2d || p == zsum1 || p == te0_2d || (const void*)p == (const void*)words) return PACE_ERR_ARG;
  } else {
    for (const real* p : in)
      if (p == te0_2d) return PACE_ERR_ARG;
  }
  return launch_energy_columns(make_geo(geom), mode, water, pt, delp, delz, w, u, v, pkz, phis, rsin2, cosa_s, area, te0_2d, te_2d,
                               zsum1, words, r_vir, S(stream));
}

int pace_energy_finalize(const int64_t* const* words, int ntiles, double consv_te, double dt_atmos, double* out, void* stream) {
  if (!words || !out || ntiles < 1 || ntiles > PACE_ENERGY_MAX_TILES) return PACE_ERR_ARG;
  for (int t = 0; t < ntiles; ++t)
    if (!words[t] || (const void*)words[t] == (const void*)out) return PACE_ERR_ARG;
  if (!std::isfinite(consv_te) || !(std::isfinite(dt_atmos) && dt_atmos > 0.0)) return PACE_ERR_ARG;
  (void)hipGetLastError();
  return launch_energy_finalize(words, ntiles, consv_te, dt_atmos, out, S(stream));
}

static bool six_rw(real* const* w) {
  if (!w) return false;
  for (int n = 0; n < 6; ++n)
    if (!w[n]) return false;
  return true;
}

int pace_fv_setup_pt(const pace_geom_t* geom, real* const* water, real* q_con, real* pkz, real* pt, real* cappa,
                     const real* delp, const real* delz, real* dp1, void* stream) {
  NEED(geom && six_rw(water) && q_con && pkz && pt && cappa && delp && delz && dp1);
  return launch_fv_setup_pt(make_geo(geom), water, q_con, pkz, pt, cappa, delp, delz, dp1, S(stream));
}

int pace_omega_from_w(const pace_geom_t* geom, const real* delp, const real* delz, const real* w, real* omga,
                      void* stream) {
  NEED(geom && delp && delz && w && omga);
  return launch_omega_from_w(make_geo(geom), delp, delz, w, omga, S(stream));
}

int pace_neg_adj3(const pace_geom_t* geom, real* const* water, real* qcld, real* pt, const real* delp, void* stream) {
  NEED(geom && six_rw(water) && qcld && pt && delp);
  return launch_neg_adj3(make_geo(geom), water, qcld, pt, delp, S(stream));
}

int pace_sat_adjust_tables(double* tables, void* stream) {
  if (!tables) return PACE_ERR_ARG;
  (void)hipGetLastError();
  return launch_sat_adjust_tables(tables, S(stream));
}

int pace_sat_adjust(const pace_geom_t* geom, real* const* water, real* qcld, real* te, real* pt, real* q_con, real* pkz,
                    real* cappa, const real* delp, const real* delz, const real* area, const real* hs, const double* tables,
                    const pace_sat_adjust_params_t* params, int kmp, int last_step, int consv_te, void* stream) {
  NEED(geom && six_rw(water) && qcld && pt && q_con && pkz && cappa && delp && delz && area && hs && tables && params &&
       (te || !consv_te));
  if (params->hydrostatic) return PACE_ERR_UNSUPPORTED;
  if (kmp < 0 || kmp >= geom->nk) return PACE_ERR_ARG;
  return launch_sat_adjust(make_geo(geom), water, qcld, te, pt, q_con, pkz, cappa, delp, delz, area, hs, tables, *params, kmp,
                           last_step, consv_te, S(stream));
}

int pace_dry_convective_adjust(const pace_geom_t* geom, real* const* tracers, real* pt, real* ua, real* va, real* w,
                               real* u_dt, real* v_dt, const real* delp, const real* delz, const real* pkz, const real* peln,
                               const real* pe, int k_sponge, int nwat, double fv_sg_adj, double timestep, void* stream) {
  NEED(geom && tracers && pt && ua && va && w && u_dt && v_dt && delp && delz && pkz && peln && pe);
  for (int n = 0; n < 9; ++n)
    if (!tracers[n]) return PACE_ERR_ARG;
  if (k_sponge < 3 || k_sponge > geom->nk || !(fv_sg_adj > 0.0) || !(timestep > 0.0)) return PACE_ERR_ARG;
  // the externals of m_loop (fv_subgridz.py:794-801)
  const double t_max = k_sponge < (geom->nk < 24 ? geom->nk : 24) ? 315.0 : 325.0;
  const double xvir = nwat == 0 ? 0.0 : phys::ZVIR;
  return launch_dry_convective_adjust(make_geo(geom), tracers, pt, ua, va, w, u_dt, v_dt, delp, delz, pkz, peln, pe, k_sponge,
                                      xvir, t_max, fv_sg_adj, timestep, S(stream));
}

int pace_fill_gfs_delp(const pace_geom_t* geom, const real* delp, real* q, double q_min, void* stream) {
  NEED(geom && delp && q);
  if (geom->nk < 2) return PACE_ERR_ARG;
  return launch_fill_gfs_delp(make_geo(geom), delp, q, q_min, S(stream));
}

int pace_phys_thermo_pressure(const pace_geom_t* geom, const real* const* water, real* pt, real* t_dt, real* pe,
                              const real* delp, real* peln, real* pk, const real* ua, const real* va, real* ps, real* u_srf,
                              real* v_srf, double dt, void* stream) {
  NEED(geom && water && pt && t_dt && pe && delp && peln && pk && ua && va && ps && u_srf && v_srf);
  for (int n = 0; n < 6; ++n)
    if (!water[n]) return PACE_ERR_ARG;
  if (geom->nk < 2) return PACE_ERR_ARG;
  return launch_phys_thermo_pressure(make_geo(geom), water, pt, t_dt, pe, delp, peln, pk, ua, va, ps, u_srf, v_srf, dt,
                                     S(stream));
}

int pace_update_dwinds_phys(const pace_geom_t* geom, real* u, real* v, real* u_dt, real* v_dt, const real* const* vlon,
                            const real* const* vlat, const real* const* es1, const real* const* ew2, const real* edge_vect_w,
                            const real* edge_vect_e, const real* edge_vect_s, const real* edge_vect_n, double dt5,
                            void* stream) {
  NEED(geom && u && v && u_dt && v_dt && vlon && vlat && es1 && ew2 && edge_vect_w && edge_vect_e && edge_vect_s && edge_vect_n);
  for (int m = 0; m < 3; ++m)
    if (!vlon[m] || !vlat[m] || !es1[m] || !ew2[m]) return PACE_ERR_ARG;
  if (geom->n < 4 || geom->n % 2) return PACE_ERR_ARG;  // the edge vectors need a midpoint (geometry.py:726-729)
  return launch_update_dwinds_phys(make_geo(geom), u, v, u_dt, v_dt, vlon, vlat, es1, ew2, edge_vect_w, edge_vect_e,
                                   edge_vect_s, edge_vect_n, dt5, S(stream));
}

int64_t pace_microphysics_workspace_bytes(const pace_geom_t* geom) {
  return (geom && geom_check(geom) == PACE_OK) ? (int64_t)microphysics_workspace_bytes(make_geo(geom)) : 0;
}

int pace_microphysics(const pace_geom_t* geom, void* workspace, const pace_microphysics_config_t* cfg, const real* const* in,
                      real* wmp, real* const* tendencies, real* const* precipitation, void* stream) {
  NEED(geom && workspace && cfg && in && wmp && tendencies && precipitation);
  if (cfg->struct_bytes != (int32_t)sizeof(pace_microphysics_config_t)) return PACE_ERR_ARG;  // built against another header
  if (sizeof(real) != 8) return PACE_ERR_UNSUPPORTED;  // QCMIN, QVMIN are no float32 quantities
  for (int n = 0; n < PACE_MICROPHYSICS_INPUTS; ++n)
    if (!in[n]) return PACE_ERR_ARG;
  for (int n = 0; n < PACE_MICROPHYSICS_TENDENCIES; ++n)
    if (!tendencies[n]) return PACE_ERR_ARG;
  for (int n = 0; n < 4; ++n)
    if (!precipitation[n]) return PACE_ERR_ARG;
  if (cfg->ntimes < 1 || !(cfg->timestep > 0.0) || !(cfg->dts > 0.0)) return PACE_ERR_ARG;
  return launch_microphysics(make_geo(geom), workspace, in, wmp, tendencies, precipitation, *cfg, S(stream));
}

static bool all_set(const void* const* table, int count) {
  for (int n = 0; n < count; ++n)
    if (!table[n]) return false;
  return true;
}

int pace_copy_dycore_to_physics(const pace_geom_t* geom, const real* const* in, real* const* out, void* stream) {
  NEED(geom && in && out);
  if (sizeof(real) != 8) return PACE_ERR_UNSUPPORTED;  // the physics is float64 only (pace_microphysics)
  if (!all_set((const void* const*)in, PACE_PHYSICS_COPY_FIELDS) || !all_set((const void* const*)out, PACE_PHYSICS_COPY_FIELDS))
    return PACE_ERR_ARG;
  return launch_copy_dycore_to_physics(make_geo(geom), in, out, S(stream));
}

int pace_physics_prepare(const pace_geom_t* geom, real* const* tracers, const real* pt, const real* delz, real* delp,
                         const real* omga, real* prsi, real* phii, real* phil, real* delprsi, real* dz, real* wmp,
                         real* const* tendencies, double ptop, int do_microphysics, void* stream) {
  NEED(geom && tracers && pt && delz && delp && prsi && phii && phil && delprsi);
  if (sizeof(real) != 8) return PACE_ERR_UNSUPPORTED;
  if (!all_set((const void* const*)tracers, 8)) return PACE_ERR_ARG;
  if (do_microphysics && !(omga && dz && wmp && tendencies && all_set((const void* const*)tendencies, PACE_MICROPHYSICS_TENDENCIES)))
    return PACE_ERR_ARG;
  return launch_physics_prepare(make_geo(geom), tracers, pt, delz, delp, omga, prsi, phii, phil, delprsi, dz, wmp, tendencies,
                                ptop, do_microphysics != 0, S(stream));
}

int pace_physics_update_state(const pace_geom_t* geom, const real* const* x, const real* const* x_dt, real* const* out, double dt,
                              void* stream) {
  NEED(geom && x && x_dt && out);
  if (sizeof(real) != 8) return PACE_ERR_UNSUPPORTED;
  if (!all_set((const void* const*)x, PACE_PHYSICS_UPDATED_FIELDS) || !all_set((const void* const*)x_dt, PACE_PHYSICS_UPDATED_FIELDS) ||
      !all_set((const void* const*)out, PACE_PHYSICS_UPDATED_FIELDS))
    return PACE_ERR_ARG;
  return launch_physics_update_state(make_geo(geom), x, x_dt, out, dt, S(stream));
}

int pace_physics_tendencies_to_dycore(const pace_geom_t* geom, real* const* tendencies, const real* const* updated,
                                      const real* const* before, real* const* tracers, const real* prsi, real* delp, double rdt,
                                      void* stream) {
  NEED(geom && tendencies && updated && before && tracers && prsi && delp);
  if (sizeof(real) != 8) return PACE_ERR_UNSUPPORTED;
  if (!all_set((const void* const*)tendencies, 3) || !all_set((const void* const*)updated, 9) ||
      !all_set((const void* const*)before, 3) || !all_set((const void* const*)tracers, 6))
    return PACE_ERR_ARG;
  return launch_physics_tendencies_to_dycore(make_geo(geom), tendencies, updated, before, tracers, prsi, delp, rdt, S(stream));
}

int64_t pace_state_extrema_workspace_bytes(const pace_geom_t* geom) {
  return (geom && geom_check(geom) == PACE_OK) ? (int64_t)state_extrema_workspace_bytes(make_geo(geom)) : 0;
}

int pace_state_extrema(const pace_geom_t* geom, const real* const* fields, const int* compute_only, int nfields, void* workspace,
                       double* out, void* stream) {
  NEED(geom && fields && compute_only && workspace && out);
  if (nfields < 1 || nfields > PACE_STATE_EXTREMA_MAX_FIELDS) return PACE_ERR_ARG;
  if (!all_set((const void* const*)fields, nfields)) return PACE_ERR_ARG;
  return launch_state_extrema(make_geo(geom), fields, compute_only, nfields, workspace, out, S(stream));
}

int pace_diag_pack(const pace_geom_t* geom, const pace_diag_item_t* items, int nitems, int out_is_double, void* out,
                   void* stream) {
  NEED(geom && items && out);
  if (nitems < 1 || nitems > PACE_DIAG_MAX_ITEMS) return PACE_ERR_ARG;
  for (int m = 0; m < nitems; ++m) {
    const pace_diag_item_t& it = items[m];
    if (!window_ok(geom, it, true) || it.out_offset < 0) return PACE_ERR_ARG;
    if (it.kind == PACE_DIAG_COLUMN_INTEGRAL && !it.weight) return PACE_ERR_ARG;
  }
  return launch_diag_pack(make_geo(geom), items, nitems, out_is_double, out, S(stream));
}

int pace_plev_diag(const pace_geom_t* geom, const real* peln, const double* log_p, int nlevels, const pace_plev_item_t* items,
                   int nitems, int i0, int j0, int ni, int nj, int out_is_double, void* out, void* stream) {
  NEED(geom && peln && log_p && items && out);
  if (nlevels < 1 || nlevels > PACE_PLEV_MAX_LEVELS || nitems < 1 || nitems > PACE_PLEV_MAX_ITEMS || geom->nk < 2) return PACE_ERR_ARG;
  const int side = geom->n + 7;
  if (i0 < 0 || ni < 1 || ni > side - i0 || j0 < 0 || nj < 1 || nj > side - j0) return PACE_ERR_ARG;
  for (int m = 0; m < nitems; ++m) {
    const pace_plev_item_t& it = items[m];
    if (it.kind != PACE_PLEV_LAYER && it.kind != PACE_PLEV_HEIGHT) return PACE_ERR_ARG;
    if (!it.field || (it.kind == PACE_PLEV_HEIGHT && !it.surface)) return PACE_ERR_ARG;
    if (it.level < 0 || it.level >= nlevels || it.out_offset < 0) return PACE_ERR_ARG;
  }
  return launch_plev_diag(make_geo(geom), peln, log_p, nlevels, items, nitems, i0, j0, ni, nj, out_is_double, out, S(stream));
}

int pace_state_unpack(const pace_geom_t* geom, const pace_unpack_item_t* items, int nitems, const double* in, void* stream) {
  NEED(geom && items && in);
  if (nitems < 1 || nitems > PACE_UNPACK_MAX_ITEMS) return PACE_ERR_ARG;
  for (int m = 0; m < nitems; ++m) {
    const pace_unpack_item_t& it = items[m];
    if (!window_ok(geom, it)) return PACE_ERR_ARG;
    if (it.order != PACE_ORDER_ZFAST && it.order != PACE_ORDER_XFAST) return PACE_ERR_ARG;
    if (it.in_offset < 0 || it.in_step < 1) return PACE_ERR_ARG;
  }
  return launch_state_unpack(make_geo(geom), items, nitems, in, S(stream));
}

static int restart_check(const pace_geom_t* geom, const pace_restart_item_t* items, int nitems) {
  if (!items || nitems < 1 || nitems > PACE_RESTART_MAX_ITEMS) return PACE_ERR_ARG;
  for (int m = 0; m < nitems; ++m)
    if (!window_ok(geom, items[m])) return PACE_ERR_ARG;
  return PACE_OK;
}

int64_t pace_restart_pack_workspace_bytes(const pace_geom_t* geom, const pace_restart_item_t* items, int nitems) {
  if (!geom || geom_check(geom) != PACE_OK || restart_check(geom, items, nitems) != PACE_OK) return 0;
  return (int64_t)restart_pack_workspace_bytes(items, nitems);
}

int pace_restart_pack(const pace_geom_t* geom, const pace_restart_item_t* items, int nitems, int out_type, void* out,
                      uint64_t* sums, void* workspace, void* stream) {
  NEED(geom && items && (out || sums) && (!sums || workspace));
  if (out_type != PACE_RESTART_BE_F64 && out_type != PACE_RESTART_BE_F32) return PACE_ERR_ARG;
  if (restart_check(geom, items, nitems) != PACE_OK) return PACE_ERR_ARG;
  const int esize = out_type == PACE_RESTART_BE_F64 ? 8 : 4;
  for (int m = 0; m < nitems; ++m)
    if (items[m].out_offset < 0 || items[m].out_offset % esize != 0) return PACE_ERR_ARG;
  if (out && (uintptr_t)out % esize != 0) return PACE_ERR_ARG;
  return launch_restart_pack(make_geo(geom), items, nitems, out_type, out, sums, workspace, S(stream));
}

int pace_pe_peln_from_delp(const pace_geom_t* geom, const real* delp, double ptop, real* pe, real* peln, void* stream) {
  NEED(geom && delp && pe && peln);
  return launch_pe_peln_from_delp(make_geo(geom), delp, ptop, pe, peln, S(stream));
}

// the checkpointers' items: `accumulators`: mn / mx / asum are used; `window`: the window and the expected values are
static int ckpt_check(const pace_ckpt_item_t* items, int nitems, bool accumulators, bool window) {
  if (!items || nitems < 1 || nitems > PACE_CKPT_MAX_ITEMS) return PACE_ERR_ARG;
  for (int m = 0; m < nitems; ++m) {
    const pace_ckpt_item_t& it = items[m];
    if (it.ni < 1 || it.nj < 1 || it.nk < 1) return PACE_ERR_ARG;
    if ((int64_t)it.ni * it.nj * it.nk >= ((int64_t)1 << 31)) return PACE_ERR_UNSUPPORTED;
    if (accumulators && (!it.mn || !it.mx || !it.asum)) return PACE_ERR_ARG;
    if (window) {
      if (!it.field || !it.expected || it.ei < 0 || it.ej < 0 || it.ek < 0) return PACE_ERR_ARG;
      if (it.i0 < 0 || it.wi < 1 || it.wi > it.ni - it.i0 || it.j0 < 0 || it.wj < 1 || it.wj > it.nj - it.j0 || it.k0 < 0 ||
          it.wk < 1 || it.wk > it.nk - it.k0)
        return PACE_ERR_ARG;
    }
  }
  return PACE_OK;
}
static int ckpt_check_storage(const pace_ckpt_item_t* items, int nitems) {
  for (int m = 0; m < nitems; ++m) {
    const pace_ckpt_item_t& it = items[m];
    if (!it.field || it.sj < it.ni || it.sk < it.sj * (it.nj - 1) + it.ni) return PACE_ERR_ARG;
  }
  return PACE_OK;
}

int pace_ckpt_accumulate(const pace_ckpt_item_t* items, int nitems, int first, void* stream) {
  int rc = ckpt_check(items, nitems, true, false);
  if (rc == PACE_OK) rc = ckpt_check_storage(items, nitems);
  if (rc != PACE_OK) return rc;
  (void)hipGetLastError();
  return launch_ckpt_accumulate(items, nitems, first, S(stream));
}

int64_t pace_ckpt_thresholds_workspace_bytes(const pace_ckpt_item_t* items, int nitems) {
  if (ckpt_check(items, nitems, false, false) != PACE_OK) return 0;
  return (int64_t)ckpt_thresholds_blocks(items, nitems) * 4 * (int64_t)sizeof(double);
}

int pace_ckpt_thresholds(const pace_ckpt_item_t* items, int nitems, int n_trials, void* workspace, double* out, void* stream) {
  const int rc = ckpt_check(items, nitems, true, false);
  if (rc != PACE_OK) return rc;
  if (n_trials < 1 || !workspace || !out) return PACE_ERR_ARG;
  (void)hipGetLastError();
  return launch_ckpt_thresholds(items, nitems, n_trials, workspace, out, S(stream));
}

int64_t pace_ckpt_validate_workspace_bytes(const pace_ckpt_item_t* items, int nitems) {
  if (ckpt_check(items, nitems, false, true) != PACE_OK) return 0;
  return (int64_t)ckpt_validate_blocks(items, nitems) * 6 * (int64_t)sizeof(double);
}

int pace_ckpt_validate(const pace_ckpt_item_t* items, int nitems, void* workspace, double* out, void* stream) {
  int rc = ckpt_check(items, nitems, false, true);
  if (rc == PACE_OK) rc = ckpt_check_storage(items, nitems);
  if (rc != PACE_OK) return rc;
  if (!workspace || !out) return PACE_ERR_ARG;
  (void)hipGetLastError();
  return launch_ckpt_validate(items, nitems, workspace, out, S(stream));
}

int pace_nudge(const pace_geom_t* geom, const pace_nudge_item_t* items, int nitems, double weight, double dt, int apply,
               void* stream) {
  NEED(geom && items);
  if (nitems < 1 || nitems > PACE_NUDGE_MAX_ITEMS) return PACE_ERR_ARG;
  if (!(weight >= 0.0 && weight <= 1.0) || !std::isfinite(dt)) return PACE_ERR_ARG;
  for (int m = 0; m < nitems; ++m) {
    const pace_nudge_item_t& it = items[m];
    if (!window_ok(geom, it) || !it.ref0) return PACE_ERR_ARG;
    if (!it.tendency && !apply) return PACE_ERR_ARG;
    if (!(std::isfinite(it.timescale) && it.timescale > 0.0)) return PACE_ERR_ARG;
    if (it.field == it.ref0 || it.field == it.ref1 || it.field == it.tendency) return PACE_ERR_ARG;
  }
  return launch_nudge(make_geo(geom), items, nitems, weight, dt, apply, S(stream));
}

int pace_held_suarez(const pace_geom_t* geom, const pace_held_suarez_config_t* cfg, const real* pe, const real* ua, const real* va,
                     const real* pt, const real* sin2lat, const real* cos2lat, real* u_dt, real* v_dt, real* pt_dt, real* teq,
                     void* stream) {
  NEED(geom && cfg && pe && ua && va && pt && sin2lat && cos2lat && u_dt && v_dt && pt_dt);
  if (cfg->struct_bytes != (int32_t)sizeof(pace_held_suarez_config_t)) return PACE_ERR_ARG;
  if (cfg->accumulate != 0 && cfg->accumulate != 1) return PACE_ERR_ARG;
  if (!(std::isfinite(cfg->dt) && cfg->dt >= 0.0)) return PACE_ERR_ARG;
  if (!(cfg->sigma_b >= 0.0 && cfg->sigma_b < 1.0) || !(cfg->p0 > 0.0)) return PACE_ERR_ARG;
  const double rates[] = {cfg->k_f, cfg->k_a, cfg->k_s};
  for (const double rate : rates)
    if (!(std::isfinite(rate) && rate >= 0.0)) return PACE_ERR_ARG;
  const real* const in[] = {pe, ua, va, pt, sin2lat, cos2lat};
  const real* const out[] = {u_dt, v_dt, pt_dt, teq};
  for (int a = 0; a < 4; ++a) {
    if (!out[a]) continue;
    for (const real* p : in)
      if (out[a] == p) return PACE_ERR_ARG;
    for (int b = 0; b < a; ++b)
      if (out[a] == out[b]) return PACE_ERR_ARG;
  }
  return launch_held_suarez(make_geo(geom), *cfg, pe, ua, va, pt, sin2lat, cos2lat, u_dt, v_dt, pt_dt, teq, S(stream));
}

int pace_rayleigh_super(const pace_geom_t* geom, const pace_metrics_t* met, const real* a11, const real* a12, const real* a21,
                        const real* a22, real* u, real* v, real* w, real* pt, const double* factor, double rcv, int conserve,
                        void* stream) {
  NEED(geom && met && a11 && a12 && a21 && a22 && u && v && w && pt && factor);
  if (!met->dx || !met->dy) return PACE_ERR_ARG;
  if (conserve != 0 && conserve != 1) return PACE_ERR_ARG;
  if (conserve && !std::isfinite(rcv)) return PACE_ERR_ARG;
  const real* const fields[] = {u, v, w, pt};
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < a; ++b)
      if (fields[a] == fields[b]) return PACE_ERR_ARG;
  // the leading damped levels, then exactly 1.0 to the bottom
  int kmax = 0;
  while (kmax < geom->nk && factor[kmax] < 1.0) ++kmax;
  for (int k = 0; k < geom->nk; ++k) {
    if (!(factor[k] > 0.0 && factor[k] <= 1.0)) return PACE_ERR_ARG;  // (a NaN fails both)
    if (k >= kmax && factor[k] != 1.0) return PACE_ERR_ARG;
  }
  if (kmax == 0) return PACE_OK;
  return launch_rayleigh_super(make_geo(geom), *met, a11, a12, a21, a22, u, v, w, pt, factor, kmax, rcv, conserve, S(stream));
}

int pace_c2l_ord(const pace_geom_t* geom, const pace_metrics_t* met, int order, const real* u, const real* v,
                 const real* a11, const real* a12, const real* a21, const real* a22, real* ua, real* va,
                 void* stream) {
  NEED(geom && met && u && v && a11 && a12 && a21 && a22 && ua && va);
  if (order != 2 && order != 4) return PACE_ERR_ARG;
  return launch_c2l(make_geo(geom), *met, order, u, v, a11, a12, a21, a22, ua, va, S(stream));
}


int pace_halo_pack(const pace_geom_t* geom, const pace_halo_desc_t* descs, int ndesc, void* stream) {
  NEED(geom && descs && ndesc > 0);
  if (halo_check(geom, descs, ndesc)) return PACE_ERR_ARG;
  return launch_halo_copy(make_geo(geom), descs, ndesc, 0, S(stream));
}

int pace_halo_unpack(const pace_geom_t* geom, const pace_halo_desc_t* descs, int ndesc, void* stream) {
  NEED(geom && descs && ndesc > 0);
  if (halo_check(geom, descs, ndesc)) return PACE_ERR_ARG;
  return launch_halo_copy(make_geo(geom), descs, ndesc, 1, S(stream));
}

int pace_halo_cube(const pace_geom_t* geom, const pace_halo_xfer_t* table_on_device, int n, void* stream) {
  NEED(geom && n >= 0);
  if (n == 0) return PACE_OK;
  if (!table_on_device) return PACE_ERR_ARG;
  return launch_halo_cube(make_geo(geom), table_on_device, n, S(stream));
}

static int cube_xfer(const pace_geom_t* geom, const pace_cube_item_t* table_on_device, int n, int dense_type, void* dense, int scatter,
                     void* stream) {
  NEED(geom && table_on_device && dense);
  if (n < 1 || n > PACE_CUBE_MAX_ITEMS) return PACE_ERR_ARG;
  if (dense_type != PACE_DENSE_F64 && dense_type != PACE_DENSE_F32) return PACE_ERR_ARG;
  return launch_cube_xfer(make_geo(geom), table_on_device, n, dense_type == PACE_DENSE_F64, dense, scatter, S(stream));
}

int pace_cube_gather(const pace_geom_t* geom, const pace_cube_item_t* table_on_device, int n, int dense_type, void* dense,
                     void* stream) {
  return cube_xfer(geom, table_on_device, n, dense_type, dense, 0, stream);
}

int pace_cube_scatter(const pace_geom_t* geom, const pace_cube_item_t* table_on_device, int n, int dense_type, const void* dense,
                      void* stream) {
  return cube_xfer(geom, table_on_device, n, dense_type, (void*)dense, 1, stream);
}

int pace_cube_regrid(const pace_geom_t* geom, const pace_regrid_point_t* points_on_device, int npoints,
                     const pace_regrid_item_t* items_on_device, int n, int dense_type, void* dense, void* stream) {
  NEED(geom && points_on_device && items_on_device && dense);
  if (npoints < 1 || n < 1 || n > PACE_REGRID_MAX_ITEMS) return PACE_ERR_ARG;
  if (dense_type != PACE_DENSE_F64 && dense_type != PACE_DENSE_F32) return PACE_ERR_ARG;
  return launch_cube_regrid(make_geo(geom), points_on_device, npoints, items_on_device, n, dense_type == PACE_DENSE_F64, dense,
                            S(stream));
}

int pace_stencil(const pace_geom_t* geom, const pace_metrics_t* met, int id, void* const* fields, int nfields, const double* scalars,
                 int nscalars, const int* origin, const int* domain, void* stream) {
  NEED(geom && met && fields && origin && domain && nfields >= 1 && nfields <= 16 && nscalars >= 0 && (nscalars == 0 || scalars));
  for (int n = 0; n < nfields; ++n)
    if (!fields[n]) return PACE_ERR_ARG;
  return launch_stencil(make_geo(geom), *met, id, fields, nfields, scalars, nscalars, origin, domain, S(stream));
}

}  // extern "C"
