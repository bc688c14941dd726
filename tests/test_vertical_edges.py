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
preamble's pkz and pt within test_c2l_and_preamble_kernels_emulated_vs_oracle's 1e-14.  Measured errors: DESIGN.md section 6.

The second half of the module runs the same operators on the float32-storage library (library(which, "f32")) against
float32(oracle(float32 inputs)), each output in the class F32_TABLE gives it, and the four kernels of k_l2e.hip one by one with
either storage type."""
import numpy as np
import pytest

import remap_columns as rc
from helpers import Env, build_emu, build_emu_f32, compare, minimal_metrics

BOTH = [pytest.param("emulated", id="emulated"), pytest.param("device", id="gpu", marks=pytest.mark.gpu)]

_libs = {}


def library(which, storage=None):
    """(library, device) of "emulated" or "device", loaded once; storage="f32": the float32-storage build."""
    assert storage in (None, "f32")
    if (which, storage) not in _libs:
        from pace_amd import _lib

        if which == "emulated":
            _libs[which, storage] = (_lib.Library(build_emu_f32() if storage else build_emu()), "cpu")
        else:
            _libs[which, storage] = (_lib.load(32) if storage else _lib.load(), "cuda:0")
        assert _libs[which, storage][0].real_bytes == (4 if storage else 8)
    return _libs[which, storage]


_envs = {}


def environment(which, n, km, storage=None):
    """An Env of the library at C<n> x km (the vertical kernels read no metric term)."""
    if (which, n, km, storage) not in _envs:
        lib, device = library(which, storage)
        _envs[which, n, km, storage] = Env(lib, device, minimal_metrics(n), n, km)
    return _envs[which, n, km, storage]


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
    # float32 storage: a top layer whose interfaces differ by more than a factor of two (their float difference is not exact
    # there) -- ptop = 300 Pa under a first interface of thousands at 6 ... 17 levels (not at 65, where the first layer is
    # 126 Pa thick, nor in `squash`, 315 Pa).  (k_remap.hip forms its one difference of two `real` interfaces, DP(k), for the bottom two
    # layers only; their ratio stays below two, so what the float32 cases see of it is the quotient DP(km - 2) / DP(km - 1).)
    share = {}
    for n, km, stag in F32_MAP_SHAPES:
        for _, _, kind in f32_map_configs(n, km):
            _, pe1, _ = rc.columns(kind, n, km, 5)
            top = pe1.astype(np.float32)[3:3 + n, 3:3 + n]
            share[n, km, kind] = float((top[:, :, 1] > 2.0 * top[:, :, 0]).mean())
            assert (top[:, :, km] < 2.0 * top[:, :, km - 1]).all(), (n, km, kind)
    assert share[13, 6, "ties"] == 1.0 and share[13, 9, "deform"] == 1.0 and share[13, 9, "identity"] == 1.0, share
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


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("n,nz", [(13, 3), (64, 2), (68, 5)], ids=lambda v: str(v))
@pytest.mark.parametrize("which", BOTH)
def test_c2l_and_preamble_windows_f32(which, n, nz, order):
    """The same on the float32-storage library against float32(oracle(float32 inputs)) (helpers.check_c2l_and_preamble with
    storage="f32"): ua, va of both orders, q_con, cappa, dp1 and omga in the exact class -- k_c2l, k_fv_setup_pt and
    k_omega_from_w are one pass from loads to stores --, pkz and pt (exp, log) in the last-place class.  Float32 rows are padded to
    32 elements: C13 32, C64 and C68 96 (the float64 cases: 32, 80, 80)."""
    from helpers import check_c2l_and_preamble

    lib, device = library(which, "f32")
    errs = check_c2l_and_preamble(lib, device, n, nz, order, storage="f32")
    if errs:
        print(f"PREAMBLE f32 {which} C{n} x {nz} differ: " + " ".join(f"{k}={e}" for k, e in errs.items()))


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


# ======================================================================================================================
# float32 storage: the same operators on libpace_hip_f32.so / libpace_emu_f32.so against float32(oracle(float32 inputs))
# ======================================================================================================================
# The definitions are those of tests/test_f32_operators.py (module docstring there): inputs rounded with opchain.f32 and held as
# float64 for the oracle, outputs an operator only writes NaN before the call, classes exact / last-place / staged, S(v) from the
# oracle alone fed opchain.f32_neighbours of its inputs (two draws, fixed seed), bound opchain.staged_bound with factor 2.
# Classified by reading the kernels (pace_amd/csrc):
#   k_remap.hip   k_remap_interfaces stores the copy of the field (a1), the interface values (qi) and the elimination's
#                 multipliers (gw) in the `real` workspace, k_remap_coefficients reads a1 and qi back and stores a2, a3, a4 there,
#                 k_remap_layers reads a1 .. a4 back: every remapped value is staged.  k_fillz stores each level once it is final
#                 and reads the column back for the final rescale.
#   k_dycore.hip  k_fix_neg_water is one pass per cell (qliquid, qsnow, qice, pt: exact); k_neg_columns then reads qgraupel,
#                 qrain and qvapor back from `real` storage and sweeps them, and qcld, in place, level by level.
#   k_l2e.hip     k_l2e_prepare forms the target interfaces from ak, bk and ps = pe[km] in double and stores them once (pe, ps,
#                 delp: exact; pk = exp(akap log(pe2)), peln = log(pe2): last place).  pt is stored as real before it is remapped
#                 on log-pressure coordinates that are real themselves, and everything k_l2e_post and k_l2e_finish form (q_con,
#                 cappa, pkz, the final pt) is made of remapped fields: staged, exp / log included -- the issue that asked for
#                 this table put pt and pkz into the last-place class; no remapped value can be there.
#   k_fvtp2d.hip  the ord-8 transport's fluxes: F32_ORD8 below.
# kord 10 picks a reconstruction by comparing second differences (set_exts: |2 a1 - (a2 + a3)| > |a2 - a3|), on values read back
# from `real` storage; S holds the oracle's own flips under one ulp of input noise, and the bound held with factor 2 at every
# shape below (measured: DESIGN.md section 6).
F32_SEED = 20250201
_REMAP = "a1, the interface values and a2, a3, a4 go through the real workspace of k_remap_interfaces / _coefficients / _layers"
F32_TABLE = {
    ("MapSingle", "q"): ("staged", _REMAP),
    ("MapNTracer", "q"): ("staged", _REMAP + "; k_fillz reads the column back from real storage for its rescale"),
    ("fillz", "q"): ("staged", "k_fillz stores each level as real once it is final and reads the column back for the final rescale"),
    **{("neg_adj3", v): ("exact", None) for v in ("qliquid", "qsnow", "qice", "pt", "delp")},
    **{("neg_adj3", v): ("staged", "k_neg_columns reads back what k_fix_neg_water stored as real and sweeps the column in place")
       for v in ("qvapor", "qrain", "qgraupel", "qcld")},
    **{("l2e", v): ("exact", None) for v in ("delp", "pe", "ps")},
    **{("l2e", v): ("last-place", None) for v in ("pk", "peln")},
    **{("l2e", v): ("staged", _REMAP + "; pt and the log-pressure coordinates are real fields before the remap")
       for v in ("pt", "pkz", "q_con", "cappa", "u", "v", "w", "delz", "tracers")},
}
# float32 rows are padded to 32 elements (float64: 16): the strides the cases below reach
F32_STRIDES = {13: 32, 40: 64, 64: 96, 68: 96}
_f32_rows = []


def f32_class(op, var):
    from test_f32_operators import EXACT, LAST, staged

    kind, why = F32_TABLE[op, var]
    return {"exact": EXACT, "last-place": LAST}.get(kind) or staged(why)


def f32_response(oracle, inputs, ref, draws=2, hold=(), common_ends=None):
    """S per output: max |oracle(inputs (+) one float32 ulp) - oracle(inputs)| over `draws` draws.  oracle: dict -> dict.
    hold: inputs that are not state (the K-tables ak, bk: the chain's noise leaves the column tables alone as well, and a moved
    bk[km] = 1 would take the bottom target interface off the bottom source interface).  common_ends = (source, target): the two
    coordinates keep their common top and bottom interface (the source's follow the target's), which is what makes them a remap."""
    from opchain import f32_neighbours

    S = dict.fromkeys(ref, 0.0)
    for draw in range(draws):
        rng = np.random.default_rng(F32_SEED + draw)
        noisy = {k: (f32_neighbours(v, rng) if isinstance(v, np.ndarray) and k not in hold else v) for k, v in inputs.items()}
        if common_ends:
            src, dst = common_ends
            noisy[src][:, :, [0, -1]] = noisy[dst][:, :, [0, -1]]
        noisy = oracle(noisy)
        for k in ref:
            d = float(np.abs(noisy[k] - ref[k]).max())
            assert np.isfinite(d), k
            S[k] = max(S[k], d)
    return S


def f32_judge(tag, op, var, got, ref, S, wrong, key=None):
    from opchain import f32
    from test_f32_operators import judge, show

    row, bad = judge(f32_class(op, key or var), np.ascontiguousarray(got), f32(ref), S)
    show("f32 " + tag, op, var, row)
    _f32_rows.append((tag, op, var, row))
    if bad:
        wrong.append((tag, op, var, bad))


def f32_untouched(got, before, win):
    """Outside `win` the float32 field still holds the bits of float32(before)."""
    keep = outside(got.shape, win)
    return np.array_equal(got.view(np.uint32)[keep], before.astype(np.float32).view(np.uint32)[keep])


# ---- MapSingle ---------------------------------------------------------------------------------------------------------------------
F32_MAP_SHAPES = [(13, 6, "unstag"), (13, 9, "unstag"), (13, 17, "unstag"), (13, 65, "unstag"), (64, 9, "xstag"), (68, 12, "unstag")]


def f32_map_configs(n, km):
    """kord 9 / iv 1, kord 10 / iv 0 and iv -2 on `ties`; at 13 x 9 the first two on all four kinds of column."""
    kinds = rc.KINDS if (n, km) == (13, 9) else ("ties",)
    return [(9, 1, kind) for kind in kinds] + [(10, 0, kind) for kind in kinds] + [(9, -2, "ties")]


_f32_map_cases = {}


def f32_map_case(n, km, stag, kord, iv, kind):
    """map_single_case's columns rounded to float32: (inputs, window, float64 oracle on them, S)."""
    from opchain import f32
    from oracle import remapping

    key = (n, km, stag, kord, iv, kind)
    if key not in _f32_map_cases:
        q, pe1, pe2, qs, win, _ = map_single_case(n, km, stag, kord, iv, kind)
        inp = {"q": f32(q), "pe1": f32(pe1), "pe2": f32(pe2), "qs": f32(qs)}
        assert (np.diff(inp["pe1"][win], axis=2) > 0).all() and (np.diff(inp["pe2"][win], axis=2) > 0).all()

        def oracle(a, store=None):
            r = a["q"][win].copy()
            r[:, :, km] = 0.0
            remapping.map_single(r, a["pe1"][win], a["pe2"][win], km, kord, iv, qs=a["qs"][win] if iv == -2 else None,
                                 qmin=200.0 if iv == 1 else 0.0, store=store)
            return {"q": r[:, :, :km]}

        ref = oracle(inp)
        assert np.isfinite(ref["q"]).all()
        S = f32_response(oracle, inp, ref, common_ends=("pe1", "pe2"))
        _f32_map_cases[key] = (inp, win, ref, S, oracle(inp, store=f32)["q"])
    return _f32_map_cases[key]


def limiter_columns(ref, stored, S, factor=2.0):
    """(ni, nj) bool, from the oracle alone: the columns in which the oracle that rounds its intermediates where the kernels store
    them (oracle/remapping.py `store`) leaves the staged bound around the plain oracle.  The profile's limiters compare an
    interface value with its neighbouring layer means (apply_constraints) and the signs of products of differences
    (posdef_constraint_iv1, remap_constraint, set_exts for kord 10); where two of these nearly tie -- with a source layer a
    thousandth of its neighbours the interface value nearly equals the layer mean above -- ONE rounding of the stored interface
    value picks the other branch, and the two branches differ by the size of the layer-to-layer differences, not by S.  Noise on
    the inputs moves the interface value and the layer mean together and rarely shows such a tie, so S does not contain it."""
    from opchain import staged_bound

    return (np.abs(stored - ref) > staged_bound(float(np.abs(ref).max()), S, factor)).any(axis=2)


def check_map_single_f32(lib, device, env, n, km, stag, tag):
    from pace_amd.fv3core.stencils.map_single import MapSingle

    assert env.qf.row_stride == F32_STRIDES[n]
    wrong = []
    for kord, iv, kind in f32_map_configs(n, km):
        inp, win, ref, S, stored = f32_map_case(n, km, stag, kord, iv, kind)
        fq, f1, f2, fs = env.q3(inp["q"]), env.q3(inp["pe1"]), env.q3(inp["pe2"]), env.q2(inp["qs"])
        MapSingle(env.stencil_factory, env.qf, kord, iv, DIMS[stag])(fq, f1, f2, qs=fs if iv == -2 else None, qmin=200.0 if iv == 1 else 0.0)
        sync(env)
        got = fq.numpy()
        t = f"{tag} C{n} x {km} {stag} kord={kord} iv={iv} {kind}"
        # the staged bound against float32(oracle), but for the columns the oracle itself marks (limiter_columns)
        plain = ~limiter_columns(ref["q"], stored, S["q"])
        assert plain.mean() > 0.99, (t, int((~plain).sum()))
        f32_judge(t + f" limiter_columns={int((~plain).sum())}", "MapSingle", "q", got[win][:, :, :km][plain], ref["q"][plain], S["q"], wrong)
        # ... and, everywhere, bit for bit what the oracle gives when it rounds where the kernels store
        w = got[win][:, :, :km]
        if not np.array_equal(w, stored.astype(np.float32)):
            from test_f32_operators import ulps

            u = ulps(w, stored.astype(np.float32))
            wrong.append((t, f"not the storing oracle bit for bit: {int((u != 0).sum())} of {u.size} differ, by up to {int(u.max())} ulp"))
        if not f32_untouched(got, inp["q"], win + (slice(0, km),)):
            wrong.append((t, "written outside the window"))
        if not all(f32_untouched(f.numpy(), inp[k], ()) for f, k in ((f1, "pe1"), (f2, "pe2"), (fs, "qs"))):
            wrong.append((t, "an input was written"))
    return wrong


@pytest.mark.parametrize("n,km,stag", F32_MAP_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("which", BOTH)
def test_map_single_f32(which, n, km, stag):
    """MapSingle with float32 storage at the remap's minimum of six levels, around one chunk and one block (9, 17), with remainder
    one (65), at C64 staggered in x (a second block with one live lane) and at C68: staged bound on the window, nothing outside
    it written, no input written."""
    lib, device = library(which, "f32")
    wrong = check_map_single_f32(lib, device, environment(which, n, km, "f32"), n, km, stag, which)
    assert not wrong, wrong


# ---- MapNTracer + fillz, fillz, neg_adj3 ---------------------------------------------------------------------------------------------
_f32_mapn = {}


def f32_mapn_case(n, km, kord):
    from opchain import f32
    from oracle import remapping

    key = (n, km, kord)
    if key not in _f32_mapn:
        fields, pe1, pe2, dp2, win, _ = mapn_case(n, km, kord)
        inp = {"pe1": f32(pe1), "pe2": f32(pe2), "dp2": f32(dp2), **{f"q{t}": f32(a) for t, a in enumerate(fields)}}

        def oracle(a, store=None):
            out = {}
            for t in range(9):
                q = a[f"q{t}"][win].copy()
                q[:, :, km] = 0.0
                remapping.map_single(q, a["pe1"][win], a["pe2"][win], km, 9 if t == 5 else kord, 0, store=store)
                if store is not None:
                    q = store(q)  # (the remapped field is a real field before k_fillz reads it)
                remapping.fillz(q, a["dp2"][win], km)
                out[f"q{t}"] = q[:, :, :km]
            return out

        ref = oracle(inp)
        _f32_mapn[key] = (inp, win, ref, f32_response(oracle, inp, ref, common_ends=("pe1", "pe2")), oracle(inp, store=f32))
    return _f32_mapn[key]


@pytest.mark.parametrize("kord", [9, 10])
@pytest.mark.parametrize("n,km", [(13, 9), (68, 7)], ids=lambda v: str(v))
@pytest.mark.parametrize("which", BOTH)
def test_mapn_tracer_nine_tracers_f32(which, n, km, kord):
    """MapNTracer (nine tracers, kord 10: two groups) + fillz with float32 storage: every tracer within the staged bound of
    float32(oracle's map_single + fillz), nothing outside the compute domain written."""
    from pace_amd.fv3core.stencils.fillz import tracer_variables
    from pace_amd.fv3core.stencils.mapn_tracer import MapNTracer

    env = environment(which, n, km, "f32")
    inp, win, ref, S, stored = f32_mapn_case(n, km, kord)
    tracers = {name: env.q3(inp[f"q{t}"]) for t, name in enumerate(tracer_variables)}
    MapNTracer(env.stencil_factory, env.qf, kord, 9, True, tracers)(env.q3(inp["pe1"]), env.q3(inp["pe2"]), env.q3(inp["dp2"]), tracers)
    sync(env)
    wrong = []
    for t, name in enumerate(tracer_variables):
        got = tracers[name].numpy()
        plain = ~limiter_columns(ref[f"q{t}"], stored[f"q{t}"], S[f"q{t}"])
        assert plain.mean() > 0.99, (t, int((~plain).sum()))
        f32_judge(f"{which} C{n} x {km} kord={kord} limiter_columns={int((~plain).sum())}", "MapNTracer", f"q{t}",
                  got[win][:, :, :km][plain], ref[f"q{t}"][plain], S[f"q{t}"], wrong, key="q")
        if not f32_untouched(got, inp[f"q{t}"], win + (slice(0, km),)):
            wrong.append((t, name, "written outside the window"))
    assert not wrong, wrong


F32_COLUMN_SHAPES = [(13, 4), (13, 9), (68, 7)]
_f32_fillz = {}


def f32_fillz_case(n, km):
    from opchain import f32
    from oracle import remapping

    if (n, km) not in _f32_fillz:
        qs, dp, _ = fillz_case(n, km)
        inp = {"dp": f32(dp), **{f"q{t}": f32(q) for t, q in enumerate(qs)}}

        def oracle(a):
            out = {}
            for t in range(9):
                out[f"q{t}"] = a[f"q{t}"].copy()
                remapping.fillz(out[f"q{t}"], a["dp"], km)
            return out

        ref = oracle(inp)
        _f32_fillz[n, km] = (inp, ref, f32_response(oracle, inp, ref))
    return _f32_fillz[n, km]


@pytest.mark.parametrize("n,km", F32_COLUMN_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("which", BOTH)
def test_fillz_nine_patterns_f32(which, n, km):
    """fillz alone with float32 storage, the nine patterns of negatives: staged bound; halo and level km keep their NaN."""
    import columns
    from pace_amd.fv3core.stencils.fillz import FillNegativeTracerValues, tracer_variables

    env = environment(which, n, km, "f32")
    inp, ref, S = f32_fillz_case(n, km)
    tracers = {name: env.q3(columns.embed(inp[f"q{t}"], n)) for t, name in enumerate(tracer_variables)}
    FillNegativeTracerValues(env.stencil_factory, env.qf, 9, tracers)(env.q3(columns.embed(inp["dp"], n)), tracers)
    sync(env)
    win = (slice(3, 3 + n), slice(3, 3 + n), slice(0, km))
    wrong = []
    for t, name in enumerate(tracer_variables):
        got = tracers[name].numpy()
        f32_judge(f"{which} C{n} x {km} {rc.FILLZ_PATTERNS[t]}", "fillz", f"q{t}", got[win], ref[f"q{t}"], S[f"q{t}"], wrong, key="q")
        if not np.isnan(got[outside(got.shape, win)]).all():
            wrong.append((t, "written outside the window"))
    # the pattern without negatives is returned as it came, whatever the class allows
    assert np.array_equal(tracers[tracer_variables[0]].numpy()[win], inp["q0"].astype(np.float32))
    assert not wrong, wrong


_f32_neg = {}


def f32_neg_adj_case(n, km):
    from opchain import f32
    from oracle import dycore_parts

    if (n, km) not in _f32_neg:
        s, _ = neg_adj_case(n, km)
        inp = {k: f32(v) for k, v in s.items()}

        def oracle(a):
            r = {k: v.copy() for k, v in a.items()}
            dycore_parts.neg_adj3(*[r[k] for k in rc.NEG_ADJ_SPECIES], r["pt"], r["delp"], km)
            return r

        ref = oracle(inp)
        _f32_neg[n, km] = (inp, ref, f32_response(oracle, inp, ref))
    return _f32_neg[n, km]


@pytest.mark.parametrize("n,km", F32_COLUMN_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("which", BOTH)
def test_neg_adj3_f32(which, n, km):
    """AdjustNegativeTracerMixingRatio with float32 storage: what k_fix_neg_water alone decides (qliquid, qsnow, qice, pt) and
    delp exact, the four species of the column sweeps staged; nothing outside the compute domain written."""
    import columns
    from pace_amd.fv3core.stencils.neg_adj3 import AdjustNegativeTracerMixingRatio

    env = environment(which, n, km, "f32")
    inp, ref, S = f32_neg_adj_case(n, km)
    f = {k: env.q3(columns.embed(v, n)) for k, v in inp.items()}
    AdjustNegativeTracerMixingRatio(env.stencil_factory, env.qf, False, False)(*[f[k] for k in rc.NEG_ADJ_SPECIES], f["pt"], f["delp"])
    sync(env)
    win = (slice(3, 3 + n), slice(3, 3 + n), slice(0, km))
    wrong = []
    for k in rc.NEG_ADJ_SPECIES + ("pt", "delp"):
        got = f[k].numpy()
        f32_judge(f"{which} C{n} x {km}", "neg_adj3", k, got[win], ref[k], S[k], wrong)
        if not np.isnan(got[outside(got.shape, win)]).all():
            wrong.append((k, "written outside the window"))
    assert not wrong, wrong


# ---- LagrangianToEulerian ------------------------------------------------------------------------------------------------------------
F32_L2E_CASES = [(13, 6, False), (13, 8, True), (68, 9, False)]
_f32_l2e = {}


def f32_l2e_windows(n, km):
    cw = (slice(3, 3 + n), slice(3, 3 + n))
    wins = {"u": (slice(3, 3 + n), slice(3, 4 + n)), "v": (slice(3, 4 + n), slice(3, 3 + n))}
    return {name: wins.get(name, cw) + ((slice(0, km + 1 if name in ("pe", "peln", "pk") else km),) if name != "ps" else ())
            for name in L2E_EXACT + L2E_LOG}, cw + (slice(0, km),)


def f32_l2e_case(n, km, last_step):
    from opchain import f32
    from oracle import constants as oc
    from oracle import remapping

    key = (n, km, last_step)
    if key not in _f32_l2e:
        f, tr, ak, bk, ptop, _, _ = l2e_case(n, km, last_step)
        inp = {**{k: f32(v) for k, v in f.items()}, **{"tracer_" + k: f32(v) for k, v in tr.items()}, "ak": f32(ak), "bk": f32(bk)}
        ptop = float(inp["ak"][0])
        wins, tw = f32_l2e_windows(n, km)

        def oracle(a):
            rf = {k: a[k].copy() for k in f}
            rt = {k: a["tracer_" + k].copy() for k in tr}
            remapping.lagrangian_to_eulerian(rf, rt, a["ak"], a["bk"], ptop, oc.KAPPA, oc.ZVIR, last_step, n, km, o=3, nq=8)
            return {**{k: rf[k][w] for k, w in wins.items()}, **{"tracer_" + k: rt[k][tw] for k in tr}}

        ref = oracle(inp)
        assert all(np.isfinite(v).all() for v in ref.values())
        _f32_l2e[key] = (inp, list(f), list(tr), ptop, ref, f32_response(oracle, inp, ref, hold=("ak", "bk")))
    return _f32_l2e[key]


@pytest.mark.parametrize("n,km,last_step", F32_L2E_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("which", BOTH)
def test_lagrangian_to_eulerian_f32(which, n, km, last_step):
    """The whole LagrangianToEulerian sequence with float32 storage at the remap's minimum of six levels, at one block as the
    last step (moist_pt_last_step) and at C68 x 9: delp, pe, ps exact; pk, peln within the last place (1 float32 ulp, at most 1e-4
    of the window different); everything that is remapped or made of remapped fields staged (F32_TABLE)."""
    from pace_amd import synthetic
    from pace_amd.fv3core import RemappingConfig
    from pace_amd.fv3core.stencils.remapping import LagrangianToEulerian
    from pace_amd.util import constants as c

    from opchain import f32_dict

    lib, device = library(which, "f32")
    inp, fields, names, ptop, ref, S = f32_l2e_case(n, km, last_step)
    env = Env(lib, device, f32_dict(synthetic.tile_metrics(n, km)), n, km)
    assert env.qf.row_stride == F32_STRIDES[n]
    qf = {k: (env.q3(inp[k]) if inp[k].ndim == 3 else env.q2(inp[k])) for k in fields}
    qt = {k: env.q3(inp["tracer_" + k]) for k in names}
    op = LagrangianToEulerian(env.stencil_factory, env.qf, RemappingConfig(), None, 8, None, qt)
    op(qt, qf["pt"], qf["delp"], qf["delz"], qf["peln"], qf["u"], qf["v"], qf["w"], qf["cappa"], qf["q_con"], qf["qcld"],
       qf["pkz"], qf["pk"], qf["pe"], qf["phis"], qf["ps"], qf["wsd"], env.kq(inp["ak"]), env.kq(inp["bk"]), None, ptop, c.KAPPA, c.ZVIR,
       last_step, 0.0, 100.0)
    sync(env)
    wins, tw = f32_l2e_windows(n, km)
    tag = f"{which} C{n} x {km} last_step={int(last_step)}"
    wrong = []
    for name, w in wins.items():
        f32_judge(tag, "l2e", name, qf[name].numpy()[w], ref[name], S[name], wrong)
    for name in names:
        f32_judge(tag, "l2e", name, qt[name].numpy()[tw], ref["tracer_" + name], S["tracer_" + name], wrong, key="tracers")
    assert not wrong, wrong
    assert len(names) == 8


@pytest.mark.parametrize("n,km", [(13, 6), (64, 6), (68, 9)], ids=lambda v: str(v))
@pytest.mark.parametrize("storage", [None, "f32"], ids=["f64", "f32"])
@pytest.mark.parametrize("which", BOTH)
def test_l2e_kernels_one_by_one(which, storage, n, km):
    """k_l2e_prepare, k_l2e_post, k_l2e_pressures (both directions) and k_l2e_finish (last step and not) on their own, with
    either storage type (helpers.check_l2e_kernels): everything without exp / log bit for bit, pt, pn2, pk and pkz in the last
    place.  This is where the float32 build's condensate sums, the pair sums of k_l2e_pressures and k_l2e_post's -delz * delp
    can be seen on their own: in the whole sequence they disappear in the staged class.  C64: the staggered column ie + 1 of
    the v-direction pressures is the one live lane of a second block; C68: five lanes."""
    from helpers import check_l2e_kernels

    lib, device = library(which, storage)
    report = check_l2e_kernels(lib, device, n, km, storage)
    print(f"L2E kernels {which} {storage or 'f64'} C{n} x {km} " + " ".join(f"{k}={v}" for k, v in report.items() if v))


def test_f32_last_place_shapes_hold_against_the_transcendentals_last_place():
    """No kernel here.  The last-place class allows 1 float32 ulp on at most 1e-4 of a window; this checks that at the shapes
    used here a change of one float64 ulp in the result of numpy's own exp / log changes the float32 value of no element at all
    (so the class is a condition on the kernel, not something the shapes can fail on their own): LagrangianToEulerian's pk and
    peln from the target interfaces.  (The preamble's pkz and pt: helpers.check_c2l_and_preamble checks the same in place.)"""
    from oracle import constants as oc

    for n, km, last_step in F32_L2E_CASES:
        _, _, _, _, ref, _ = f32_l2e_case(n, km, last_step)
        for name in ("pk", "peln"):
            v = ref[name]
            for moved in (np.nextafter(v, np.inf), np.nextafter(v, -np.inf)):
                flips = int((moved.astype(np.float32) != v.astype(np.float32)).sum())
                assert flips <= 1e-4 * v.size, (n, km, name, flips)
    assert oc.KAPPA > 0


# ---- the ord-8 transport ---------------------------------------------------------------------------------------------------------
F32_ORD8 = [pytest.param("emulated", 13, 5, id="emulated-13-5"), pytest.param("device", 40, 3, id="gpu-40-3", marks=pytest.mark.gpu)]


@pytest.mark.parametrize("which,n,nz", F32_ORD8)
def test_ord8_transport_f32(which, n, nz):
    """helpers.check_ord8_transport with storage="f32": the monotone transport's two fluxes against float32(oracle)."""
    from helpers import check_ord8_transport

    lib, device = library(which, "f32")
    report = check_ord8_transport(lib, device, n, nz, storage="f32")
    for k, row in report.items():
        print(f"F32OPS f32 {which} C{n} x {nz} ord8.{k} {row}")
