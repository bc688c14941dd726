"""The remapping and column kernels of DynamicalCore.step_dynamics outside the acoustic loop -- k_remap.hip (MapSingle, MapNTracer,
fillz), k_l2e.hip (LagrangianToEulerian), k_dycore.hip (neg_adj3, CubedToLatLon, fv_setup_pt, omega_from_w), the ord-8 transport
-- at the level counts and windows where their indexing can go wrong, against the oracle.  Every case runs on the emulated
library in the CPU tier and on the device with -m gpu.

What varies here and nowhere else in the suite:
  * the level count: k_remap_interfaces runs its recurrences in chunks of RC = 8 levels with clamped look-ahead loads,
    k_remap_layers gives each thread REMAP_KB = 8 target levels and starts it by bisection, k_remap_coefficients has top-two,
    bottom-two and inner branches; the launchers take nk >= 6 (remap) and nk >= 4 (fillz, neg_adj3).  6 is the minimum (inner
    layers 2 .. 3 only), 7 / 8 / 9 lie below, at and above one chunk and one block, 16 / 17 at two blocks and one level more,
    65 has remainder 1, 128 is sixteen blocks and the deepest bisection.
  * the columns of a row: i = i0 + blockIdx.x * 64 + threadIdx.x.  C64 unstaggered is exactly one block, staggered in x a second
    block with one live lane; C68 has four live lanes in the second block.
  * exact ties between source and target interfaces (tests/remap_columns.py `ties`, `identity`): the bisection of
    k_remap_layers equals the reference's running index only through its tie rule pe1[L + 1] >= pe2[k].
  * iv = 2 (its own coefficient variant), kord 10 with iv -1 / -2, and the x-staggered window.

Bounds: BIT IDENTITY for everything without exp / log (the kernels hold add, multiply, divide and are built without
contraction); LagrangianToEulerian's pt, peln, pk, pkz within test_lagrangian_to_eulerian_emulated's 1e-14 on the emulated
library, and on the device test_lagrangian_to_eulerian_matches_oracle's 1e-11 throughout with the mass fields exact; the
preamble's pkz and pt within test_c2l_and_preamble_kernels_emulated_vs_oracle's 1e-14.  Measured errors: DESIGN.md section 6."""
import numpy as np
import pytest

import remap_columns as rc
from helpers import Env, build_emu, compare, minimal_metrics

BOTH = [pytest.param("emulated", id="emulated"), pytest.param("device", id="gpu", marks=pytest.mark.gpu)]

_libs = {}


def library(which):
    """(library, device) of "emulated" or "device", loaded once."""
    if which not in _libs:
        from pace_amd import _lib

        _libs[which] = (_lib.Library(build_emu()), "cpu") if which == "emulated" else (_lib.load(), "cuda:0")
    return _libs[which]


_envs = {}


def environment(which, n, km):
    """An Env of the library at C<n> x km (the vertical kernels read no metric term)."""
    if (which, n, km) not in _envs:
        lib, device = library(which)
        _envs[which, n, km] = Env(lib, device, minimal_metrics(n), n, km)
    return _envs[which, n, km]


def sync(env):
    if env.qf.device.type == "cuda":
        import torch

        torch.cuda.synchronize()


def outside(shape, win):
    m = np.ones(shape, dtype=bool)
    m[win] = False
    return m


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- the makers ------------------------------------------------------------------------------------------------------------------

def test_column_makers():
    """What the cases below rely on: remap_columns is what tests/test_gpu_parity.py always used (a pinned value), every kind is
    strictly monotone with common ends, `ties` has the ties (the maker asserts them; here: how many, and that they survive at
    every shape of the table), `identity` is one, `squash` really has target layers over many source layers and the reverse, the
    non-deform fields change sign."""
    q, pe1, pe2 = rc.remap_columns(48, 79, 3 + 9 + 1, 3.0)
    assert q.shape == pe1.shape == pe2.shape == (55, 55, 80) and (np.diff(pe1, axis=2) > 0).all()
    assert float(pe2[3, 3, 79]) == 100634.78691302537 and float(pe1[5, 7, 40]) == 37094.41576375667 and float(q[9, 4, 11]) == 288.8057263361583
    kb = rc.remap_kb()
    assert kb == 8
    for n, km in MAP_SHAPES:
        for kind in rc.KINDS:
            q, pe1, pe2 = rc.columns(kind, n, km, 5)
            assert q.shape == pe1.shape == pe2.shape == (n + 7, n + 7, km + 1), (kind, n, km)
            assert (np.diff(pe1, axis=2) > 0).all() and (np.diff(pe2, axis=2) > 0).all(), (kind, n, km)
            assert same(pe1[:, :, [0, km]], pe2[:, :, [0, km]]), (kind, n, km)
            assert (q[:, :, km] == 0).all()
            if kind != "deform":
                assert (q[:, :, :km] > 0).any() and (q[:, :, :km] < 0).any(), (kind, n, km)
            t = rc.interior_ties(pe1, pe2)[3:4 + n, 3:4 + n]
            if kind == "ties":
                frac = t[:, :, 1:km].mean()
                assert 0.3 < frac < 0.7, (n, km, frac)
                assert km <= kb or t[:, :, kb::kb].sum() >= 4, (n, km)
            elif kind == "identity":
                assert t[:, :, 1:km].all()
            else:
                assert not t.any(), (kind, n, km)
    _, pe1, pe2 = rc.columns("squash", 13, 128, 5)
    inside = [(int(((pe1[5, 5] > pe2[5, 5, k]) & (pe1[5, 5] < pe2[5, 5, k + 1])).sum())) for k in range(128)]
    assert max(inside) >= 10 and inside[-1] == 0 and inside[-2] == 0, inside


# ---- MapSingle -------------------------------------------------------------------------------------------------------------------
MAP_SHAPES = [(13, 6), (13, 7), (13, 8), (13, 9), (13, 16), (13, 17), (13, 65), (13, 128), (64, 9), (68, 12)]
CROSS_SHAPES = [(13, 9), (13, 17), (64, 9)]
DIMS = {"unstag": ["x", "y", "z"], "xstag": ["x_interface", "y", "z"], "ystag": ["x", "y_interface", "z"]}
IVS = (1, 0, -1, -2, 2)


def map_single_configs(n, km, stag, kord=None):
    """The table's configurations (kord, iv, kind) at one shape and staggering: the full cross product on CROSS_SHAPES, elsewhere
    (unstaggered only) kord 9 / iv 1 and kord 10 / iv 0 with every kind and iv -2 with `ties`."""
    if (n, km) in CROSS_SHAPES:
        return [(k, iv, kind) for k in ((9, 10) if kord is None else (kord,)) for iv in IVS for kind in rc.KINDS]
    assert stag == "unstag" and kord is None
    return [(9, 1, kind) for kind in rc.KINDS] + [(10, 0, kind) for kind in rc.KINDS] + [(9, -2, "ties")]


_map_cases = {}


def map_single_case(n, km, stag, kord, iv, kind):
    """(q, pe1, pe2, qs, window, expected): storage arrays that hold NaN outside the window (q also at level km; qs is finite
    on the window only), and the oracle's result on the window.  Computed once for both libraries; the tests copy out of them (Quantity.set) and do not write to them."""
    key = (n, km, stag, kord, iv, kind)
    if key not in _map_cases:
        from oracle import remapping

        seed = 1000 * km + 10 * n + 3 * kord + iv + rc.KINDS.index(kind)
        q, pe1, pe2 = rc.columns(kind, n, km, seed)
        win = (slice(3, 3 + n + (stag == "xstag")), slice(3, 3 + n + (stag == "ystag")))
        qs = 0.1 * q[:, :, km - 1]
        out = outside(q.shape[:2], win)
        for a in (q, pe1, pe2, qs):
            a[out] = np.nan
        ref = q[win].copy()
        remapping.map_single(ref, pe1[win], pe2[win], km, kord, iv, qs=qs[win] if iv == -2 else None, qmin=200.0 if iv == 1 else 0.0)
        q[:, :, km] = np.nan
        _map_cases[key] = (q, pe1, pe2, qs, win, ref[:, :, :km])
    return _map_cases[key]


def check_map_single(which, n, km, stag, configs):
    from pace_amd.fv3core.stencils.map_single import MapSingle

    env = environment(which, n, km)
    bad = []
    for kord, iv, kind in configs:
        q, pe1, pe2, qs, win, ref = map_single_case(n, km, stag, kord, iv, kind)
        fq, f1, f2, fs = env.q3(q), env.q3(pe1), env.q3(pe2), env.q2(qs)
        MapSingle(env.stencil_factory, env.qf, kord, iv, DIMS[stag])(fq, f1, f2, qs=fs if iv == -2 else None, qmin=200.0 if iv == 1 else 0.0)
        sync(env)
        got = fq.numpy()
        assert np.isfinite(ref).all()
        if not np.array_equal(got[win][:, :, :km], ref):
            d = np.argwhere(got[win][:, :, :km] != ref)
            bad.append((kord, iv, kind, "window", len(d), "first at", tuple(d[0]), "levels", sorted(set(d[:, 2]))[:6]))
        keep = outside(q.shape, win + (slice(0, km),))
        if not same(got[keep], q[keep]):
            bad.append((kord, iv, kind, "written outside the window"))
        if not (same(f1.numpy(), pe1) and same(f2.numpy(), pe2) and same(fs.numpy(), qs)):
            bad.append((kord, iv, kind, "an input was written"))
    assert not bad, (len(bad), "of", len(configs), bad[:8])


@pytest.mark.parametrize("kord", [9, 10])
@pytest.mark.parametrize("stag", list(DIMS))
@pytest.mark.parametrize("n,km", CROSS_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("which", BOTH)
def test_map_single_cross_product(which, n, km, stag, kord):
    """C13 x 9, C13 x 17 and C64 x 9 (x-staggered: a second block with one live lane): kord {9, 10} x iv {1, 0, -1, -2, 2} x
    every kind of column x the three staggerings, each against the oracle bit for bit on the window; everything outside the
    window (NaN before the call: halo, level km) and every input keeps its bits.  One test per (shape, staggering, kord) runs
    the twenty (iv, kind) pairs and names every one that fails."""
    check_map_single(which, n, km, stag, map_single_configs(n, km, stag, kord))


@pytest.mark.parametrize("n,km", [s for s in MAP_SHAPES if s not in CROSS_SHAPES], ids=lambda v: str(v))
@pytest.mark.parametrize("which", BOTH)
def test_map_single_level_counts(which, n, km):
    """The other level counts (6: the launcher's minimum; 7, 8: below and at one chunk / block; 16: two blocks; 65: remainder 1;
    128: sixteen blocks) and C68 x 12 (two blocks of lanes, four live in the second), unstaggered: kord 9 / iv 1 and kord 10 /
    iv 0 with every kind of column, iv -2 (qs given: finite on the window, NaN outside) with `ties`.  Bit for bit."""
    check_map_single(which, n, km, "unstag", map_single_configs(n, km, "unstag"))


# ---- MapNTracer + fillz ------------------------------------------------------------------------------------------------------------
_mapn_cases = {}


def mapn_case(n, km, kord):
    """Nine distinct tracer fields on `ties` coordinates (some of them with negatives, so that fillz acts), NaN outside the
    compute domain and at level km; the oracle's per-tracer map_single + fillz."""
    key = (n, km, kord)
    if key not in _mapn_cases:
        from oracle import remapping

        q0, pe1, pe2 = rc.columns("ties", n, km, 77 + km + kord)
        rng = np.random.default_rng(n + km + kord)
        win = (slice(3, 3 + n), slice(3, 3 + n))
        out = outside(q0.shape[:2], win)
        dp2 = np.zeros_like(pe2)
        dp2[:, :, :km] = pe2[:, :, 1:] - pe2[:, :, :-1]
        fields = []
        for t in range(9):
            # tracer-like magnitudes, each tracer its own; q0 changes sign, so the odd ones have negatives in most columns
            a = 1.0e-3 * (t + 1) * (np.abs(q0) / 40.0 + 0.05 * rng.random(q0.shape)) if t % 2 == 0 else 1.0e-4 * (t + 1) * (q0 / 40.0 + 0.3)
            a[:, :, km] = 0.0
            fields.append(a)
        for a in fields + [pe1, pe2, dp2]:
            a[out] = np.nan
        refs = []
        for t, a in enumerate(fields):
            q = a[win].copy()
            remapping.map_single(q, pe1[win], pe2[win], km, 9 if t == 5 else kord, 0)
            remapping.fillz(q, dp2[win], km)
            refs.append(q[:, :, :km])
            a[:, :, km] = np.nan
        assert any((a[win][:, :, :km] < 0).any() for a in fields)
        _mapn_cases[key] = (fields, pe1, pe2, dp2, win, refs)
    return _mapn_cases[key]


@pytest.mark.parametrize("kord", [9, 10])
@pytest.mark.parametrize("n,km", [(13, 9), (68, 7)], ids=lambda v: str(v))
@pytest.mark.parametrize("which", BOTH)
def test_mapn_tracer_nine_tracers(which, n, km, kord):
    """MapNTracer with the largest batch the host forms (nine tracers; kord 10: two groups, tracer 5 stays kord 9) + fillz on
    `ties` coordinates at C13 x 9 and C68 x 7 against the oracle's per-tracer map_single + fillz: bit for bit, the nine fields
    distinct (a swapped batch slot shows), nothing written outside the compute domain."""
    from pace_amd.fv3core.stencils.fillz import tracer_variables
    from pace_amd.fv3core.stencils.mapn_tracer import MapNTracer

    env = environment(which, n, km)
    fields, pe1, pe2, dp2, win, refs = mapn_case(n, km, kord)
    assert len(tracer_variables) == 9
    tracers = {name: env.q3(a) for name, a in zip(tracer_variables, fields)}
    op = MapNTracer(env.stencil_factory, env.qf, kord, 9, True, tracers)
    assert sorted(len(v) for v in op._groups.values()) == ([9] if kord == 9 else [1, 8])
    op(env.q3(pe1), env.q3(pe2), env.q3(dp2), tracers)
    sync(env)
    for t, name in enumerate(tracer_variables):
        got = tracers[name].numpy()
        assert np.array_equal(got[win][:, :, :km], refs[t]), (t, name)
        keep = outside(got.shape, win + (slice(0, km),))
        assert same(got[keep], fields[t][keep]), (t, name)
    for a in range(9):
        for b in range(a):
            assert not np.array_equal(refs[a], refs[b])


_fillz_cases = {}


def fillz_case(n, km):
    key = (n, km)
    if key not in _fillz_cases:
        from oracle import remapping

        qs, dp = rc.fillz_tracers(n, km, 31 * n + km)
        refs = []
        for q in qs:
            r = q.copy()
            remapping.fillz(r, dp, km)
            refs.append(r)
        assert sum(not np.array_equal(r, q) for r, q in zip(refs, qs)) >= 7 and np.array_equal(refs[0], qs[0])
        _fillz_cases[key] = (qs, dp, refs)
    return _fillz_cases[key]


@pytest.mark.parametrize("n,km", [(13, 4), (13, 5), (13, 9), (13, 128), (68, 7)], ids=lambda v: str(v))
@pytest.mark.parametrize("which", BOTH)
def test_fillz_nine_patterns(which, n, km):
    """fillz alone (FillNegativeTracerValues, nine tracers in one launch) from its minimum of four levels on: one pattern of
    negatives per tracer (remap_columns.FILLZ_PATTERNS: none, scattered, top, bottom, two consecutive interior levels, the whole
    column -- sum0 <= 0, no rescale --, mostly negative with a positive sum, ...), against the oracle bit for bit; halo and level
    km (NaN) keep their bits."""
    import columns
    from pace_amd.fv3core.stencils.fillz import FillNegativeTracerValues, tracer_variables

    env = environment(which, n, km)
    qs, dp, refs = fillz_case(n, km)
    full = [columns.embed(q, n) for q in qs]
    tracers = {name: env.q3(a) for name, a in zip(tracer_variables, full)}
    FillNegativeTracerValues(env.stencil_factory, env.qf, 9, tracers)(env.q3(columns.embed(dp, n)), tracers)
    sync(env)
    win = (slice(3, 3 + n), slice(3, 3 + n), slice(0, km))
    for t, name in enumerate(tracer_variables):
        got = tracers[name].numpy()
        assert np.array_equal(got[win], refs[t]), (t, rc.FILLZ_PATTERNS[t])
        assert np.isnan(got[outside(got.shape, win)]).all(), (t, rc.FILLZ_PATTERNS[t])


# ---- neg_adj3 --------------------------------------------------------------------------------------------------------------------
_neg_cases = {}


def neg_adj_case(n, km):
    if (n, km) not in _neg_cases:
        from oracle import dycore_parts

        s = rc.neg_adj_state(n, km, 17 * n + km)
        ref = {k: v.copy() for k, v in s.items()}
        dycore_parts.neg_adj3(*[ref[k] for k in rc.NEG_ADJ_SPECIES], ref["pt"], ref["delp"], km)
        _neg_cases[n, km] = (s, ref)
    return _neg_cases[n, km]


@pytest.mark.parametrize("n,km", [(13, 4), (13, 5), (13, 9), (13, 128), (68, 7)], ids=lambda v: str(v))
@pytest.mark.parametrize("which", BOTH)
def test_neg_adj3_level_counts(which, n, km):
    """AdjustNegativeTracerMixingRatio from its minimum of four levels on and at C68: all seven species and pt against
    oracle/dycore_parts.neg_adj3 bit for bit, delp untouched, nothing outside the compute domain written."""
    import columns
    from pace_amd.fv3core.stencils.neg_adj3 import AdjustNegativeTracerMixingRatio

    env = environment(which, n, km)
    s, ref = neg_adj_case(n, km)
    f = {k: env.q3(columns.embed(v, n)) for k, v in s.items()}
    AdjustNegativeTracerMixingRatio(env.stencil_factory, env.qf, False, False)(*[f[k] for k in rc.NEG_ADJ_SPECIES], f["pt"], f["delp"])
    sync(env)
    win = (slice(3, 3 + n), slice(3, 3 + n), slice(0, km))
    for k in rc.NEG_ADJ_SPECIES + ("pt", "delp"):
        got = f[k].numpy()
        assert np.array_equal(got[win], ref[k]), k
        assert np.isnan(got[outside(got.shape, win)]).all(), k
    assert any(not np.array_equal(ref[k], s[k]) for k in rc.NEG_ADJ_SPECIES) and not np.array_equal(ref["pt"], s["pt"])


# ---- LagrangianToEulerian ----------------------------------------------------------------------------------------------------------
L2E_CASES = [(13, 6, False), (13, 8, True), (13, 17, False), (68, 9, False), (13, 128, True)]
L2E_EXACT = ("delp", "pe", "ps", "u", "v", "w", "delz", "q_con", "cappa")
L2E_LOG = ("pt", "peln", "pk", "pkz")
_l2e_cases = {}


def l2e_case(n, km, last_step):
    """(inputs, tracer inputs, ak, bk, ptop, the oracle's fields, the oracle's tracers)."""
    key = (n, km, last_step)
    if key not in _l2e_cases:
        from helpers import l2e_synthetic_case
        from oracle import constants as oc
        from oracle import remapping

        f, tr, ak, bk, ptop = l2e_synthetic_case(n, km)
        assert (f["delp"][2:4 + n, 2:4 + n, :km] > 0).all(), "a folded column"
        rf, rt = {k: v.copy() for k, v in f.items()}, {k: v.copy() for k, v in tr.items()}
        remapping.lagrangian_to_eulerian(rf, rt, ak, bk, ptop, oc.KAPPA, oc.ZVIR, last_step, n, km, o=3, nq=8)
        _l2e_cases[key] = (f, tr, ak, bk, ptop, rf, rt)
    return _l2e_cases[key]


@pytest.mark.parametrize("n,km,last_step", L2E_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("which", BOTH)
def test_lagrangian_to_eulerian_level_counts(which, n, km, last_step):
    """The whole LagrangianToEulerian sequence (k_l2e.hip, the remaps of pt, eight tracers, w, delz and the two staggered
    winds, fillz) on helpers.l2e_synthetic_case at the remap's minimum of six levels, at one block, at two blocks + 1, at C68
    and at 128 levels, against oracle/remapping.lagrangian_to_eulerian.  Emulated: masses, pe, ps, the winds, w, delz, q_con,
    cappa and all tracers bit for bit; pt, peln, pk, pkz within 1e-14.  Device: 1e-11 throughout, delp, pe, ps exact."""
    from pace_amd import synthetic
    from pace_amd.fv3core import RemappingConfig
    from pace_amd.fv3core.stencils.remapping import LagrangianToEulerian
    from pace_amd.util import constants as c

    lib, device = library(which)
    f, tr, ak, bk, ptop, rf, rt = l2e_case(n, km, last_step)
    env = Env(lib, device, synthetic.tile_metrics(n, km), n, km)
    qf = {k: (env.q3(v) if v.ndim == 3 else env.q2(v)) for k, v in f.items()}
    qt = {k: env.q3(v) for k, v in tr.items()}
    op = LagrangianToEulerian(env.stencil_factory, env.qf, RemappingConfig(), None, 8, None, qt)
    op(qt, qf["pt"], qf["delp"], qf["delz"], qf["peln"], qf["u"], qf["v"], qf["w"], qf["cappa"], qf["q_con"], qf["qcld"],
       qf["pkz"], qf["pk"], qf["pe"], qf["phis"], qf["ps"], qf["wsd"], env.kq(ak), env.kq(bk), None, ptop, c.KAPPA, c.ZVIR, last_step,
       0.0, 100.0)
    sync(env)
    cw = (slice(3, 3 + n), slice(3, 3 + n))
    wins = {"u": (slice(3, 3 + n), slice(3, 4 + n)), "v": (slice(3, 4 + n), slice(3, 3 + n))}
    pairs = {}
    for name in L2E_EXACT + L2E_LOG:
        got, ref = qf[name].numpy()[wins.get(name, cw)], rf[name][wins.get(name, cw)]
        if got.ndim == 3:
            kk = km + 1 if name in ("pe", "peln", "pk") else km
            got, ref = got[:, :, :kk], ref[:, :, :kk]
        pairs[name] = (got, ref)
    for name in tr:
        pairs[name] = (qt[name].numpy()[cw][:, :, :km], rt[name][cw][:, :, :km])
    exact = L2E_EXACT + tuple(tr) if which == "emulated" else ("delp", "pe", "ps")
    tol = 1e-14 if which == "emulated" else 1e-11
    errs = {}
    for name, (got, ref) in pairs.items():
        assert np.isfinite(ref).all(), name
        errs[name] = compare(ref, got, near_zero=1e-18) if got.ndim == 3 else compare(ref, got)
    print(f"L2E {which} C{n} x {km} last_step={int(last_step)} " + " ".join(f"{k}={e:.1e}" for k, e in errs.items() if e > 0.0))
    for name, (got, ref) in pairs.items():
        if name in exact:
            assert np.array_equal(got, ref), (name, errs[name])
        assert errs[name] < tol, (name, errs[name])
    assert len(tr) == 8 and not np.array_equal(rf["pt"], f["pt"])


# ---- CubedToLatLon and the preamble ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("n,nz", [(13, 3), (64, 2), (68, 5)], ids=lambda v: str(v))
@pytest.mark.parametrize("which", BOTH)
def test_c2l_and_preamble_windows(which, n, nz, order):
    """helpers.check_c2l_and_preamble (the body of test_c2l_and_preamble_kernels_emulated_vs_oracle) where the rows leave the
    first 64-lane block: k_c2l's order-2 window is n + 2 wide, so C64 puts two lanes into a second block, C68 six (order 4,
    fv_setup_pt, omega_from_w: four); C13 x 3 is an odd size with fewer levels than anything else runs.  The wind transform
    bit for bit, the preamble within 1e-14."""
    from helpers import check_c2l_and_preamble

    lib, device = library(which)
    errs = check_c2l_and_preamble(lib, device, n, nz, order)
    if errs:
        print(f"PREAMBLE {which} C{n} x {nz} " + " ".join(f"{k}={e:.1e}" for k, e in errs.items()))


# ---- the ord-8 transport -----------------------------------------------------------------------------------------------------------
ORD8_SHAPES = [pytest.param("emulated", 40, 3, id="emulated-40-3")] + [
    pytest.param("device", n, nz, id=f"gpu-{n}-{nz}", marks=pytest.mark.gpu) for n, nz in ((13, 33), (40, 3), (72, 8))]


@pytest.mark.parametrize("which,n,nz", ORD8_SHAPES)
def test_ord8_transport_at_device_chain_shapes(which, n, nz):
    """helpers.check_ord8_transport (the body of test_ord8_transport_matches_oracle_c96) at the sizes of
    tests/test_gpu_device_paths.py DEVICE_CHAIN_SHAPES at which the general transport kernel runs: one partial tile (13 x 33),
    2 x 2 partial tiles with fewer levels than a map's group of eight (40 x 3), 3 x 3 tiles with the reorder (72 x 8).  Both
    fluxes bit for bit."""
    from helpers import check_ord8_transport
    from test_gpu_device_paths import DEVICE_CHAIN_SHAPES

    assert (n, nz) in DEVICE_CHAIN_SHAPES
    lib, device = library(which)
    check_ord8_transport(lib, device, n, nz)
