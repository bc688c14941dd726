"""A numpy restatement of the tracer advection's Courant-number sub-cycling (test infrastructure; include/pace_hip.h has the
contract it restates).

* ``cmax``: per level the maximum over the compute domain of max(|cx|, |cy|) on the levels k < nk // 6 - 1 (the Fortran's
  "k < npz/6", k counted from 1) and of (max(|cx|, |cy|) + 1.0) - sin_sg5 on the others.  numpy's maximum and max propagate a NaN.
* ``subcycles``: int(1.0 + c) of the maximum over the tiles, 0 where c is not finite or the count exceeds max_subcycles; in front
  of them the largest entry and the number of zeros.
* ``advect``: the per-level sequence from the oracle's own pieces -- oracle.tracer.flux_compute, divide_fluxes, apply_mass_flux,
  apply_tracer_flux, swap_dp, oracle.ppm_transport.fvtp2d, oracle.halo -- : the levels that share a count s are gathered into
  compact arrays and go through TracerAdvection's sequence with n_split = s.  So "right" is, level by level, what the fixed path
  would give with that n_split.  Arrays are indexed [i, j, k] over the whole storage (n + 7, n + 7, nk + 1)."""
import numpy as np


def cell_values(cx, cy, sin_sg5, n, nk):
    """The per-cell values, (n, n, nk)."""
    w = slice(3, 3 + n)
    with np.errstate(invalid="ignore"):
        m = np.maximum(np.abs(cx[w, w, :nk]), np.abs(cy[w, w, :nk]))
        wide = (m + 1.0) - sin_sg5[w, w, None]
    plain = np.arange(nk) < nk // 6 - 1
    return np.where(plain[None, None, :], m, wide)


def cmax(cx, cy, sin_sg5, n, nk):
    with np.errstate(invalid="ignore"):
        return cell_values(cx, cy, sin_sg5, n, nk).max(axis=(0, 1))


def subcycles(tables, max_subcycles):
    """tables: one array of nk maxima per tile.  -> int32 [largest, refused, ksplt[0 .. nk - 1]]"""
    with np.errstate(invalid="ignore"):
        c = np.maximum.reduce([np.asarray(t, dtype=np.float64) for t in tables])
    ksplt = []
    for v in c:
        count = int(1.0 + float(v)) if np.isfinite(v) else 0
        ksplt.append(count if 1 <= count <= max_subcycles else 0)
    return np.array([max(ksplt), ksplt.count(0)] + ksplt, dtype=np.int32)


def level_runs(ksplt, it):
    """[(k0, nlev)]: the maximal runs of consecutive levels with ksplt[k] > it."""
    runs, k = [], 0
    while k < len(ksplt):
        if ksplt[k] > it:
            k0 = k
            while k < len(ksplt) and ksplt[k] > it:
                k += 1
            runs.append((k0, k - k0))
        else:
            k += 1
    return runs


def _sequence(grids, tracers, dp1, mfx, mfy, cx, cy, n, nk, n_split):
    """TracerAdvection.__call__ (tracer_2d_1l.py:262-392) with a given n_split, six tiles, in place."""
    from oracle import halo, tracer
    from oracle import ppm_transport as tr

    T = range(6)
    shape = dp1[0].shape
    xfx, yfx = [np.zeros(shape) for _ in T], [np.zeros(shape) for _ in T]
    for t in T:
        tracer.flux_compute(grids[t], cx[t], cy[t], xfx[t], yfx[t], nk)
    if n_split > 1:
        for t in T:
            tracer.divide_fluxes((cx[t], xfx[t], mfx[t], cy[t], yfx[t], mfy[t]), n_split, nk)
    for q in tracers.values():
        halo.halo_update(q, n, nk=nk)
    dp2 = [np.zeros(shape) for _ in T]
    for it in range(n_split):
        for t in T:
            g = grids[t]
            tracer.apply_mass_flux(g, dp1[t], mfx[t], mfy[t], dp2[t], nk)
            for q in tracers.values():
                fx, fy = np.zeros(shape), np.zeros(shape)
                tr.fvtp2d(g, q[t], cx[t], cy[t], xfx[t], yfx[t], fx, fy, 8, x_mass_flux=mfx[t], y_mass_flux=mfy[t], nk=nk)
                tracer.apply_tracer_flux(g, q[t], dp1[t], fx, fy, dp2[t], nk)
        if it != n_split - 1:
            for q in tracers.values():
                halo.halo_update(q, n, nk=nk)
            for t in T:
                tracer.swap_dp(grids[t], dp1[t], dp2[t], nk)


def advect(make_grid, tracers, dp1, mfx, mfy, cx, cy, n, nk, ksplt):
    """The sub-cycled advection of six tiles, in place on the levels 0 .. nk - 1.  make_grid(t, levels) -> the oracle grid of
    tile t with that many levels; tracers: {name: [six arrays]}; the others: [six arrays]; ksplt: one count per level."""
    ksplt = [int(s) for s in ksplt]
    assert len(ksplt) == nk and min(ksplt) >= 1
    for s in sorted(set(ksplt)):
        levels = [k for k in range(nk) if ksplt[k] == s]
        count = len(levels)

        def gather(arrays):
            out = []
            for a in arrays:
                c = np.zeros(a.shape[:2] + (count + 1,))
                c[:, :, :count] = a[:, :, levels]
                out.append(c)
            return out

        compact = {name: gather(arrays) for name, arrays in (("dp1", dp1), ("mfx", mfx), ("mfy", mfy), ("cx", cx), ("cy", cy))}
        compact_tracers = {name: gather(arrays) for name, arrays in tracers.items()}
        _sequence([make_grid(t, count) for t in range(6)], compact_tracers, compact["dp1"], compact["mfx"], compact["mfy"],
                  compact["cx"], compact["cy"], n, count, s)
        for arrays, done in [(dp1, compact["dp1"]), (mfx, compact["mfx"]), (mfy, compact["mfy"]), (cx, compact["cx"]),
                             (cy, compact["cy"])] + [(tracers[name], compact_tracers[name]) for name in tracers]:
            for t in range(6):
                arrays[t][:, :, levels] = done[t][:, :, :count]
