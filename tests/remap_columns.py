"""Input makers for the vertical kernels (test infrastructure): source / target coordinates and fields for MapSingle, MapNTracer,
fillz and neg_adj3 at any size and level count.  Every maker returns full storage arrays (n + 7, n + 7, km + 1).

The remapping kernels (pace_amd/csrc/k_remap.hip) have four places where only the coordinates decide what runs, and one kind of
column for each (KINDS):

    deform    the columns of the C48 / C192 device tests: no ties but at the ends, every target layer inside one or two source
              layers -- the plain path of k_remap_layers (one partial layer above, one below, rarely a whole one between)
    ties      about half of the interior source interfaces EQUAL a target interface bit for bit: the tie rule of k_remap_layers'
              bisection (pe1[L + 1] >= pe2[k]), which is what makes a level block's own start the reference's running index, and
              its `p2b <= p1b` test with equality
    identity  pe1 = pe2: every interface a tie, every target layer exactly one source layer (pl = 0 or 1, pr = 1), every block
              start a tie
    squash    source ~ sigma ** 4, target ~ sigma ** 1.6: near the top one target layer spans many source layers (the `while`
              loop of k_remap_layers runs many times, and the bisection of a block starts deep in the column), near the bottom
              many target layers fall into one source layer (the `p2b <= p1b` branch again and again with one L)

The field of the non-deform kinds changes sign, so the iv = 0 and iv = -1 clamps of k_remap_coefficients engage."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("deform", "ties", "identity", "squash")
PTOP = 300.0


def remap_kb():
    """REMAP_KB of k_remap.hip: the target levels one thread of k_remap_layers takes."""
    with open(os.path.join(ROOT, "pace_amd", "csrc", "k_remap.hip")) as f:
        return int(re.search(r"^#define\s+REMAP_KB\s+(\d+)\b", f.read(), re.M).group(1))


def _sigma(km):
    return np.linspace(0.0, 1.0, km + 1) ** 1.6


def _field(rng, ni, km, offset=0.0):
    """The smooth profile plus noise (so the monotonicity constraints engage); level km is zero."""
    sig = _sigma(km)
    q = np.zeros((ni, ni, km + 1))
    q[:, :, :km] = 250.0 + 40.0 * np.cos(3.0 * np.pi * sig[:km])[None, None, :] + 3.0 * rng.standard_normal((ni, ni, km))
    q[:, :, :km] -= offset
    return q


def remap_columns(n, km, seed, deform):
    """Synthetic columns: hybrid-like target interfaces, a source coordinate deformed by up to `deform` layers, a smooth field
    plus noise (so the monotonicity constraints engage)."""
    rng = np.random.default_rng(seed)
    ni = n + 7
    sig = _sigma(km)
    ps = 1.0e5 * (1.0 + 0.02 * rng.random((ni, ni)))
    pe2 = PTOP + (ps - PTOP)[:, :, None] * sig[None, None, :]
    amp = deform / km * rng.random((ni, ni))
    s1 = sig[None, None, :] + amp[:, :, None] * np.sin(2.0 * np.pi * sig)[None, None, :]
    s1[:, :, 0], s1[:, :, km] = 0.0, 1.0
    pe1 = PTOP + (ps - PTOP)[:, :, None] * s1
    return _field(rng, ni, km), pe1, pe2


def deform_columns(n, km, seed):
    """remap_columns with deform = 3.0 and the source interfaces sorted along k: at 79 levels the sort changes nothing, at a
    few levels three layers of deformation would fold the column.  For: the plain path of k_remap_layers."""
    q, pe1, pe2 = remap_columns(n, km, seed, 3.0)
    pe1 = np.sort(pe1, axis=2)
    assert (np.diff(pe1, axis=2) > 0).all() and np.array_equal(pe1[:, :, [0, km]], pe2[:, :, [0, km]])
    return q, pe1, pe2


def interior_ties(pe1, pe2):
    """(ni, nj, km + 1) bool: source interface k equals target interface k bit for bit, interior interfaces only."""
    t = pe1 == pe2
    t[:, :, 0] = t[:, :, -1] = False
    return t


def ties_columns(n, km, seed):
    """pe1 = pe2 but for about half of the interior interfaces, chosen per column, which move by up to 0.9 of the distance to
    the neighbouring target interface (either direction); the others equal pe2 bit for bit.  For: the bisection's tie rule and
    the `<=` of k_remap_layers.  Asserts what the tests want it for: every column of the compute domain (and of its staggered
    row and column) has an interior tie, and -- where the column has more levels than one block -- some column has one at an
    interface that starts a block of REMAP_KB levels."""
    rng = np.random.default_rng([seed, 1])  # (remap_columns draws from `seed` itself)
    ni = n + 7
    _, _, pe2 = remap_columns(n, km, seed, 0.0)
    move = rng.random((ni, ni, km + 1)) < 0.5
    move[:, :, 0] = move[:, :, km] = False
    # a column whose interior interfaces all move keeps one of them
    full = move[:, :, 1:km].all(axis=2)
    keep = rng.integers(1, km, size=(ni, ni))
    ii, jj = np.nonzero(full)
    move[ii, jj, keep[ii, jj]] = False
    r = 0.9 * (2.0 * rng.random((ni, ni, km + 1)) - 1.0)
    up = np.zeros_like(pe2)
    down = np.zeros_like(pe2)
    up[:, :, :km] = pe2[:, :, 1:] - pe2[:, :, :km]
    down[:, :, 1:] = pe2[:, :, 1:] - pe2[:, :, :km]
    pe1 = np.where(move, pe2 + np.where(r > 0.0, r * up, r * down), pe2)
    pe1 = np.sort(pe1, axis=2)
    assert (np.diff(pe1, axis=2) > 0).all()
    t = interior_ties(pe1, pe2)[3:4 + n, 3:4 + n]
    assert t.any(axis=2).all(), "a column without an interior tie"
    kb = remap_kb()
    if km > kb:
        assert t[:, :, kb::kb].any(), "no tie at the start of a level block"
    return _field(rng, ni, km, 250.0), pe1, pe2


def identity_columns(n, km, seed):
    """pe1 = pe2: every interface a tie.  For: the tie rule at every block start, pl / pr of exactly 0 and 1."""
    rng = np.random.default_rng([seed, 1])
    _, _, pe2 = remap_columns(n, km, seed, 0.0)
    return _field(rng, n + 7, km, 250.0), pe2.copy(), pe2


def squash_columns(n, km, seed):
    """Source interfaces ptop + (ps - ptop) sigma ** 4, target ** 1.6 (sigma = linspace(0, 1, km + 1)).  For: the `while` loop
    of k_remap_layers over many whole source layers (top) and many target layers inside one source layer (bottom)."""
    rng = np.random.default_rng(seed)
    ni = n + 7
    lin = np.linspace(0.0, 1.0, km + 1)
    ps = 1.0e5 * (1.0 + 0.02 * rng.random((ni, ni)))
    pe1 = PTOP + (ps - PTOP)[:, :, None] * (lin ** 4)[None, None, :]
    pe2 = PTOP + (ps - PTOP)[:, :, None] * (lin ** 1.6)[None, None, :]
    return _field(rng, ni, km, 250.0), pe1, pe2


_MAKERS = {"deform": deform_columns, "ties": ties_columns, "identity": identity_columns, "squash": squash_columns}


def columns(kind, n, km, seed):
    return _MAKERS[kind](n, km, seed)


# ---- fillz -----------------------------------------------------------------------------------------------------------------------
FILLZ_PATTERNS = ("none", "scattered", "top", "bottom", "pair", "whole", "mostly", "scattered_dense", "top_and_bottom")


def fillz_tracers(n, km, seed):
    """Nine tracers on the compute domain, (n, n, km) each, and the layer thickness: one pattern of negatives per tracer
    (FILLZ_PATTERNS) -- none; scattered (one value in eight); the top level; the bottom level; two consecutive interior levels;
    the whole column (sum0 <= 0: no rescale); mostly negative with a positive column sum (a large positive value at one interior
    level); scattered, one value in three; top and bottom level."""
    rng = np.random.default_rng(seed)
    dp = 50.0 + 1000.0 * rng.random((n, n, km))
    out = []
    for t, pattern in enumerate(FILLZ_PATTERNS):
        q = 1.0e-3 * (0.1 + rng.random((n, n, km))) * (1.0 + t)  # distinct magnitudes: a swapped batch slot shows
        neg = np.zeros((n, n, km), dtype=bool)
        if pattern == "scattered":
            neg = rng.random((n, n, km)) < 0.125
        elif pattern == "scattered_dense":
            neg = rng.random((n, n, km)) < 1.0 / 3.0
        elif pattern == "top":
            neg[:, :, 0] = True
        elif pattern == "bottom":
            neg[:, :, km - 1] = True
        elif pattern == "top_and_bottom":
            neg[:, :, 0] = neg[:, :, km - 1] = True
        elif pattern == "pair":
            k = rng.integers(1, km - 2, size=(n, n))  # levels k, k + 1 in 1 .. km - 2
            i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
            neg[i, j, k] = neg[i, j, k + 1] = True
        elif pattern == "whole":
            neg[:] = True
        elif pattern == "mostly":
            neg[:] = True
            k = rng.integers(1, km - 1, size=(n, n))
            i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
            neg[i, j, k] = False
            q[i, j, k] *= 40.0 * km
        q = np.where(neg, -q, q)
        if pattern == "mostly":
            assert ((q * dp)[:, :, 1:].sum(axis=2) > 0).all() and ((q < 0).sum(axis=2) == km - 1).all()
        out.append(q)
    return out, dp


# ---- neg_adj3 --------------------------------------------------------------------------------------------------------------------
NEG_ADJ_SPECIES = ("qvapor", "qliquid", "qrain", "qsnow", "qice", "qgraupel", "qcld")


def neg_adj_state(n, km, seed):
    """Mixing ratios 1e-3 (N(0, 1) + 0.4) (a third of them negative), pt in 220 .. 300, random delp: compute-domain arrays
    (n, n, km) by name."""
    rng = np.random.default_rng(seed)
    s = {name: 1.0e-3 * (rng.standard_normal((n, n, km)) + 0.4) for name in NEG_ADJ_SPECIES}
    s["pt"] = 220.0 + 80.0 * rng.random((n, n, km))
    s["delp"] = 50.0 + 1000.0 * rng.random((n, n, km))
    return s
