// Pressure-level diagnostics (`p_select`, this project's extension of the reference's z_select): layer fields and the geometric
// height interpolated to up to PACE_PLEV_MAX_LEVELS pressure surfaces, linearly in log p, for up to PACE_PLEV_MAX_ITEMS output
// planes by ONE launch.  The definitions are include/pace_hip.h's (pace_plev_diag): double arithmetic on the stored values, no
// FMA, no transcendental -- the host hands over log(p) -- and the operation order as written there, so that a numpy restatement
// (tests/plev_reference.py) agrees bit for bit.
//
//   k_plev_diag   1-D grid, 256 threads = 4 waves.  A workgroup takes one column tile of the window (wgmap.h: 64 points in i by
//                 WT_TS_COLUMN = 4 rows in j, one row per wave); a lane owns a column, consecutive lanes consecutive i.
//                   walk    the lane walks peln ONCE, bottom-up, and brackets every target level on the way: the largest k
//                           with peln[k] <= lp (height) and with pm[k] <= lp (layer fields; pm the layers' mean log p) is the
//                           first one met from below.  Per level it keeps the bracket's index and its two log pressures -- in
//                           registers: the loops over the levels are compile-time bounded and unrolled, with p < nlevels as
//                           a predicate -- and divides once after the walk.
//                   items   then item by item (the table travels by value, scalar loads): a LAYER item is two loads at the
//                           lane's bracket (one where it is clamped); the first HEIGHT item of a (delz, phis) pair walks
//                           delz bottom-up, zi[k] = zi[k + 1] - delz[k], and keeps both heights of every level's bracket;
//                           the launcher puts the HEIGHT items of one pair next to each other, so one walk serves them all.
//                   LDS     tile[s][i] of the OUTPUT type at wgmap.h's pitch, two tiles used in turn: one barrier per item.
//                   write   wt_lds_to_runs: runs of 4 contiguous output elements per i.
//
// Nothing outside the window's columns is read (not the halo, not the row padding) and nothing outside an item's ni * nj output
// elements is written.  No atomics, no workspace.  The narrowing is a plain cast.
#include "common.h"
#include "kernels.h"
#include "pack_table.h"
#include "thermo.h"

#ifdef PACE_EMU
#define PLEV_ASSUME(x) ((void)0)
#else
#define PLEV_ASSUME(x) __builtin_assume(x)
#endif

// (by value, like pack_table.h's PackTable: it lies in the kernel-argument segment and is indexed in place)
struct PlevTable {
  pace_plev_item_t item[PACE_PLEV_MAX_ITEMS];
  double log_p[PACE_PLEV_MAX_LEVELS];
  int nitems, nlevels;
  int i0, j0, ni, nj;
};

template <typename OutT>
__global__ void __launch_bounds__(64 * WT_WAVES) k_plev_diag(Geo g, PlevTable tab, const real* __restrict__ peln,
                                                             OutT* __restrict__ out) {
  constexpr int NP = PACE_PLEV_MAX_LEVELS;
  const WindowTile wt = window_tile_of_linear((int)blockIdx.x, tab.ni, tab.nj, 1, false, WT_TS_COLUMN);
  const int sb = wt.sb, ib = wt.ib, wi = wt.wi, ws = wt.ws;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const bool mine = lane < wi && wave < ws;  // this thread has a column
  const int nz = g.nk, nlevels = tab.nlevels;
  const long sk = g.sk;
  const long c = mine ? IDX2(g, tab.i0 + ib + lane, tab.j0 + sb + wave) : 0L;

  __shared__ OutT tile[2 * WT_TS_COLUMN * WT_PITCH];

  // per level: the bracket of the layer fields (kl; tl: its lower log p, then the weight), whether the level is clamped to one
  // layer (bit p of `single`), and the bracket of the height (kh, th)
  int kl[NP], kh[NP];
  double tl[NP], th[NP];
  unsigned single = 0u;
  if (mine) {
    double ul[NP], uh[NP];  // the brackets' upper (k + 1) log pressures
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      kl[p] = -1;
      kh[p] = -1;
      tl[p] = th[p] = ul[p] = uh[p] = 0.0;
    }
    // k = nz - 1: a candidate of the height's bracket only (the layers' stop at nz - 2)
    double e_hi = (double)peln[c + nz * sk];
    double e_lo = (double)peln[c + (nz - 1) * sk];
    const double pm_bot = 0.5 * (e_lo + e_hi);
#pragma unroll
    for (int p = 0; p < NP; ++p)
      if (p < nlevels && e_lo <= tab.log_p[p]) {
        kh[p] = nz - 1;
        th[p] = e_lo;
        uh[p] = e_hi;
      }
    double pm_hi = pm_bot;
    e_hi = e_lo;
#pragma unroll 4  // (the loads of four interfaces in flight)
    for (int k = nz - 2; k >= 1; --k) {
      e_lo = (double)peln[c + k * sk];
      const double pm = 0.5 * (e_lo + e_hi);
#pragma unroll
      for (int p = 0; p < NP; ++p)
        if (p < nlevels) {
          const double lp = tab.log_p[p];
          const bool h = kh[p] < 0 && e_lo <= lp, l = kl[p] < 0 && pm <= lp;
          kh[p] = h ? k : kh[p];
          th[p] = h ? e_lo : th[p];
          uh[p] = h ? e_hi : uh[p];
          kl[p] = l ? k : kl[p];
          tl[p] = l ? pm : tl[p];
          ul[p] = l ? pm_hi : ul[p];
        }
      e_hi = e_lo;
      pm_hi = pm;
    }
    e_lo = (double)peln[c];
    const double pm_top = 0.5 * (e_lo + e_hi);
#pragma unroll
    for (int p = 0; p < NP; ++p)
      if (p < nlevels) {
        const double lp = tab.log_p[p];
        if (kh[p] < 0) {
          kh[p] = 0;
          th[p] = e_lo;
          uh[p] = e_hi;
        }
        if (kl[p] < 0) {
          kl[p] = 0;
          tl[p] = pm_top;
          ul[p] = pm_hi;
        }
        th[p] = (lp - th[p]) / (uh[p] - th[p]);
        tl[p] = (lp - tl[p]) / (ul[p] - tl[p]);
        if (!(lp > pm_top)) {
          kl[p] = 0;
          single |= 1u << p;
        } else if (lp >= pm_bot) {
          kl[p] = nz - 1;
          single |= 1u << p;
        }
      }
  }

  // the heights of the brackets' two interfaces, of the (delz, phis) pair walked last
  double z_lo[NP], z_hi[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) z_lo[p] = z_hi[p] = 0.0;
  const real* walked_delz = nullptr;
  const real* walked_phis = nullptr;

  for (int m = 0; m < tab.nitems; ++m) {
    const pace_plev_item_t& it = tab.item[m];
    const real* __restrict__ q = it.field;
    OutT* const stage = tile + (m & 1) * (WT_TS_COLUMN * WT_PITCH);
    if (mine) {
      double v = 0.0;
      if (it.kind == PACE_PLEV_HEIGHT) {
        if (q != walked_delz || it.surface != walked_phis) {
          walked_delz = q;
          walked_phis = it.surface;
          double zi = (double)it.surface[c] * phys::RGRAV;
#pragma unroll 4
          for (int k = nz - 1; k >= 0; --k) {
            const double z = zi - (double)q[c + k * sk];
#pragma unroll
            for (int p = 0; p < NP; ++p)
              if (p < nlevels) {
                const bool at = kh[p] == k;
                z_lo[p] = at ? z : z_lo[p];
                z_hi[p] = at ? zi : z_hi[p];
              }
            zi = z;
          }
        }
#pragma unroll
        for (int p = 0; p < NP; ++p)
          if (p == it.level) v = z_lo[p] + (z_hi[p] - z_lo[p]) * th[p];
      } else {
        int k = 0;
        double t = 0.0;
        bool one = true;
#pragma unroll
        for (int p = 0; p < NP; ++p)
          if (p == it.level) {
            k = kl[p];
            t = tl[p];
            one = (single >> p) & 1u;
          }
        const double f0 = (double)q[c + k * sk];
        v = f0;
        if (!one) {
          const double f1 = (double)q[c + (k + 1) * sk];
          v = f0 + (f1 - f0) * t;
        }
      }
      stage[wave * WT_PITCH + lane] = (OutT)v;
    }
    __syncthreads();  // (the other tile is free again: a thread got here only after every thread had read it, an item ago)
    PLEV_ASSUME(wi * ws <= 64 * WT_WAVES);  // one pass of wt_lds_to_runs: unrolled for more, the float kernel spilled SGPRs
    wt_lds_to_runs(out + it.out_offset + sb + (long)ib * tab.nj, stage, (long)tab.nj, wi, ws);
  }
}

int launch_plev_diag(const Geo& g, const real* peln, const double* log_p, int nlevels, const pace_plev_item_t* items, int nitems,
                     int i0, int j0, int ni, int nj, int out_is_double, void* out, hipStream_t st) {
  PlevTable tab{};
  tab.nitems = nitems;
  tab.nlevels = nlevels;
  tab.i0 = i0, tab.j0 = j0, tab.ni = ni, tab.nj = nj;
  for (int p = 0; p < nlevels; ++p) tab.log_p[p] = log_p[p];
  // the layer items, then the heights with those of one (delz, phis) pair next to each other: one walk of delz per pair (an
  // item says where its output goes: any order)
  int m = 0;
  for (int r = 0; r < nitems; ++r)
    if (items[r].kind == PACE_PLEV_LAYER) tab.item[m++] = items[r];
  for (int r = 0; r < nitems; ++r) {
    if (items[r].kind != PACE_PLEV_HEIGHT) continue;
    bool seen = false;
    for (int e = 0; e < r && !seen; ++e)
      seen = items[e].kind == PACE_PLEV_HEIGHT && items[e].field == items[r].field && items[e].surface == items[r].surface;
    if (seen) continue;
    for (int e = r; e < nitems; ++e)
      if (items[e].kind == PACE_PLEV_HEIGHT && items[e].field == items[r].field && items[e].surface == items[r].surface)
        tab.item[m++] = items[e];
  }
  const dim3 grid((unsigned)window_tiles(ni, nj, 1, false, WT_TS_COLUMN)), block(64 * WT_WAVES);
  if (out_is_double) hipLaunchKernelGGL(k_plev_diag<double>, grid, block, 0, st, g, tab, peln, (double*)out);
  else hipLaunchKernelGGL(k_plev_diag<float>, grid, block, 0, st, g, tab, peln, (float*)out);
  PACE_CHECK_LAUNCH();
  return PACE_OK;
}
