"""The float32-storage library's operators, one by one, against float32(oracle) -- not against a tolerance of the field's size.

libpace_hip_f32.so / tests/emu/libpace_emu_f32.so keep fields, metrics and K-tables as float and compute in registers in double.
tests/opchain.py's chain with storage="f32" is the float64 oracle on float32-rounded metrics, column tables and state, rounded
again at every operator boundary: each `before` is exactly what ProductOps._load puts into the float32 fields, each `after` is
float32(oracle(before)).  Every (operator, output) then sits in exactly one class (TABLE):

  exact       got == float32(ref) bit for bit on the window of opchain's checks: the float64 suite holds the operator bit-identical
              to the oracle in this tier, and nothing between the operator's loads and the store of this output passes through
              `real` storage (decided by reading the kernel);
  last-place  device operators with exp / log / pow whose only difference from the oracle is the float64 last place: every element
              within 1 float32 ulp of float32(ref), at most 1e-4 of the window's elements different at all.  A float64 last-place
              difference flips a float32 rounding with probability ~1e-8 per element: the expected count at these shapes is below
              one; the cap is a condition, not a tolerance;
  staged      an intermediate goes through `real` storage (named in TABLE): max |got - float32(ref)| <= 2^-23 max |ref| + f S(v),
              f = 2.  S(v) = max |oracle(before (+) noise)[v] - oracle(before)[v]|, where (+) noise moves every non-zero float32
              input to a float32 neighbour, up or down at random (fixed seed, the larger of two draws): what ONE rounding of the
              inputs does to this output, from the reference alone.  2^-23 max |ref| is one float32 ulp of the magnitude for the
              output's own rounding; f = 2 because a kernel that stages rounds once more per stage than the oracle's single input
              rounding, and two draws sample the response rather than bound it.  A larger f has its reason beside it; never above 8.

ws3 (updatedzc) and wsd (updatedzd) are (zs - bottom height) / dt with the bottom height read back from `real` storage.  Against
the oracle, which uses the unrounded height, every element differs: by 0.2 to 1.8 % of max |ws| at 13 x 5 and 48 x 3 (3.5e4 to
3.0e5 u, u = 2^-24 max |ws|), by 17 % (ws3, 2.8e6 u) and 24 % (wsd, 4.0e6 u) at 13 x 33 -- and the oracle's own response S to one
ulp of input noise is four to six times that at every shape (test_ws_is_ill_conditioned_in_float32_heights).  They are staged
like the rest (error / S 0.16 to 0.25), which says little about the kernel at such an S; so they are ADDITIONALLY pinned exactly,
as the oracle's two expressions (oracle/vertical.py update_dz_c / update_dz_d) applied to the bottom height the operator itself
stored (ws_of_stored_bottom).

Outputs an operator only writes hold NaN before the call (opchain.WRITE_ONLY); every output is float32; all 15 operators are seen.
Measured error / S per output on both tiers: DESIGN.md section 6.
"""
import ctypes as C

import numpy as np
import pytest

import opchain
from helpers import build_emu_f32
from opchain import Chain, ProductOps, f32, f32_neighbours, poisoned

SEED = 20240905
MAX_FACTOR = 8.0
LAST_PLACE_FRACTION = 1e-4

EXACT, LAST = ("exact", None, None, None), ("last-place", None, None, None)


def staged(why, factor=2.0, flips=None):
    """flips: additionally, every element within 1 float32 ulp of float32(ref) and at most this fraction different at all."""
    assert factor <= MAX_FACTOR
    return ("staged", why, factor, flips)


def tier(emulated, device):
    return {"emulated": emulated, "device": device}


# ---- the intermediates (pace_amd/csrc), by operator -------------------------------------------------------------------------------
# d2a2c_vect / c_sw (k_csw.hip): pass A (k_d2a2c_a) stores utmp, vtmp, ua, va as real; pass B reads them back and stores uc / vc
# (workspace ucw, vcw), ut, vt; pass C (k_csw_transport) reads ut, vt, ucw, vcw back for the fluxes, the kinetic energy and the
# vorticity (both real), pass D reads those.  k_csw_tile keeps all of it in LDS as double, but the band around the tiles is in every
# checked window.
_CSW_A = staged("utmp / vtmp and ua / va are stored as real by pass A (k_d2a2c_a) and read back by pass B")
_CSW_C = ("ut / vt are stored as real by pass B and read back by the transport pass (k_csw_transport) on the band; under emulation "
          "the effect stays below the rounding of delpc and ptc at (13, 5) and (48, 3) and shows as 1 ulp on 1e-4 of delpc at (48, 8)")
_CSW_D = staged("uc / vc of pass B (workspace ucw / vcw), the kinetic energy and the vorticity are stored as real before pass D")
# d_sw (k_dsw.hip launch_d_sw): the flux preparation stores the contravariant winds (workspace ut, vt) and crx, cry, xfx, yfx as
# real; every transport reads those back.  General family: the mass fluxes (fx, fy) and the flux-form updates (gx, gy, fx2) are real
# fields between k_fvtp2d_scalars3 and k_finish_scalars.  Lean family: one kernel from the Courant numbers to the four scalars
# and the winds, but the Courant numbers and area fluxes it loads are the stored ones.
_DSW_FX = staged("the contravariant winds (workspace ut / vt) are stored as real by the flux preparation's frame workgroups and read "
                 "back by the ones that form the Courant numbers and area fluxes")
_DSW_SCALAR = staged("crx, cry, xfx, yfx are read back from real storage by the transport of either family; in the general one the "
                     "mass fluxes (workspace fx, fy) and the flux-form updates (gx, gy, fx2) are real fields between "
                     "k_fvtp2d_scalars3 and k_finish_scalars as well.  (Measured under emulation with the fused kernel: pt and q_con "
                     "bit-identical, delp and w 1 ulp on 1e-4 of the points)")
_DSW_MASS = staged("crx, cry, xfx, yfx are read back from real storage; the mass fluxes accumulate into the caller's real field")
_DSW_WIND = staged("kinetic energy, relative vorticity (workspace ke, wk) and the damped vorticity vort_b are real fields between "
                   "k_ke_vorticity, k_divdamp_fused and the vorticity transport; the split order adds umid / vmid and ut2 / vt2")
_DSW_HEAT = staged("the heating's terms (workspace dw, heat_s) and the winds before the update are stored as real before the heating "
                   "is formed; a difference of kinetic-energy-sized terms")
_DSW_DELPC = staged("k_divdamp_halo_state_lds / _mem replays the reference's in-place passes from divg_d, uc and vc as k_divdamp_fused "
                    "stored them (real), on the full contract's halo")
# riem_solver3's w and perturbation pressure: no real-storage intermediate.  The column solver eliminates in another order than the
# oracle (the float64 suite holds the operator to 5e-6, not bit for bit, under emulation too), and both outputs are small
# differences of large terms: float64 differences of ~1e-11 of the magnitude flip a float32 rounding on ~5e-5 of the points,
# too many for the last-place cap at a few thousand points.  So the class is "staged" (S is ~7e3 u here: the bound alone is 1e-3 of
# the field), and ON TOP of it every element is within 1 float32 ulp with at most 1e-3 of them different at all.  The fraction
# from the formats, not from a run: the two eliminations differ by a few float64 roundings per level, ~1e-15 ... 1e-14 of the terms
# they add up; w and the perturbation pressure are 1e-3 ... 1e-4 of those terms (10 Pa of 1e5 Pa), so the float64 difference is
# ~1e-11 of the output, and a difference d of the output flips its float32 rounding with probability d / 2^-23: ~2e-4 per element.
# 1e-3 leaves a factor 5.
RIEM3_FLIPS = 1e-3
_RIEM3_SMALL = staged("no real-storage intermediate: the solver's order of elimination differs from the oracle's in float64, and this "
                      "output is a small difference of large terms", flips=RIEM3_FLIPS)
_ZD = staged("the Courant numbers and area fluxes interpolated to the interfaces (workspace crx_i, cry_i, xfx_i, yfx_i) are stored as "
             "real by k_spline_to_interfaces_* and read back by the transport; measured under emulation: bit-identical")
_NH = staged("pkc, gz and pk3 averaged to the corners (a2b_ord4) are stored as real and read back by the wind update")

TABLE = {
    **{("d2a2c_vect", v): _CSW_A for v in ("uc", "vc", "ua", "va", "utc", "vtc")},
    **{("c_sw", v): _CSW_A for v in ("ua", "va", "ut", "vt")},
    **{("c_sw", v): staged(_CSW_C) for v in ("delpc", "ptc", "omga")},
    ("c_sw", "uc"): _CSW_D, ("c_sw", "vc"): _CSW_D,
    ("c_sw", "divgd"): staged("uc / vc of pass B are stored as real (workspace ucw / vcw) before the divergence is formed"),
    # gz_new goes through the workspace as real, but k_updatedzc_column only copies it or replaces it by (level below + DZ_MIN):
    # re-rounding a float32 value changes nothing, and the limiter is idle in this state
    ("updatedzc", "gz"): EXACT,
    # (and pinned exactly to the oracle's expression on that stored height: ws_of_stored_bottom)
    ("updatedzc", "ws3"): staged("the bottom height gz[:, :, km] is stored as real (workspace gz_new) and k_updatedzc_column forms ws "
                                 "from the value it reads back; the oracle from the unrounded height"),
    ("updatedzd", "wsd"): staged("the bottom height zh[:, :, km] is stored as real by the transport's height epilogue (or "
                                 "k_apply_height_fluxes) and k_height_column forms ws from the value it reads back"),
    ("riem_solver_c", "pkc"): tier(EXACT, LAST), ("riem_solver_c", "gz"): tier(EXACT, LAST),
    ("p_grad_c", "uc"): EXACT, ("p_grad_c", "vc"): EXACT,
    **{("d_sw", v): _DSW_SCALAR for v in ("delp", "pt", "w", "q_con")},
    **{("d_sw", v): _DSW_FX for v in ("crx", "cry", "xfx", "yfx", "cxd", "cyd")},
    ("d_sw", "mfxd"): _DSW_MASS, ("d_sw", "mfyd"): _DSW_MASS,
    ("d_sw", "u"): _DSW_WIND, ("d_sw", "v"): _DSW_WIND,
    ("d_sw", "heat_source"): _DSW_HEAT, ("d_sw", "diss_estd"): _DSW_HEAT,
    # the work fields: k_divdamp_fused runs the nord passes in LDS as double and stores the last pass's uc, vc and divergence once
    ("d_sw", "uc"): EXACT, ("d_sw", "vc"): EXACT, ("d_sw", "divgd"): EXACT,
    ("d_sw", "vt"): _DSW_DELPC,
    ("updatedzd", "zh"): _ZD,
    **{("riem_solver3", v): tier(EXACT, LAST) for v in ("delz", "zh", "pk3", "pe", "pk", "peln")},
    ("riem_solver3", "w"): _RIEM3_SMALL, ("riem_solver3", "pkc"): _RIEM3_SMALL,
    ("edge_pe", "pe"): EXACT,
    ("pk3_halo", "pk3"): staged("pe is staged in pk3 as real by k_pk3_halo_scan and read back by k_pk3_halo_pow"),
    ("compute_geopotential", "gz"): EXACT,
    ("nh_p_grad", "u"): _NH, ("nh_p_grad", "v"): _NH,
    ("nh_p_grad", "pkc"): EXACT, ("nh_p_grad", "gz"): EXACT, ("nh_p_grad", "pk3"): EXACT,
    # (the damping table rf, dp, p_ref is built on the host in double and passed by value: k_acoustic.hip launch_ray_fast)
    ("ray_fast", "u"): tier(EXACT, LAST), ("ray_fast", "v"): tier(EXACT, LAST), ("ray_fast", "w"): tier(EXACT, LAST),
    ("del2cubed", "heat_source"): staged("every iteration of k_del2cubed_iter stores the field as real for the next one"),
    ("apply_diffusive_heating", "pt"): tier(EXACT, LAST),
}


def resolve(spec, ctx):
    while isinstance(spec, dict):
        (key,) = [k for k in spec if k in ctx]
        spec = spec[key]
    return spec


# ---- the oracle, once per shape ----------------------------------------------------------------------------------------------
_oracle = {}


def cut(a, win, nk):
    return a[win][:, :, :nk] if a.ndim == 3 else a[win]


def oracle_cases(n, nz, draws=2):
    """(chain, cases, S) of the float32-storage chain at C<n> x nz, computed once and shared by the tiers: S[(operator, output)]
    is the oracle's response to storage noise over the checked window (module docstring)."""
    if (n, nz) not in _oracle:
        chain = Chain(n, nz, storage="f32")
        cases = list(chain.cases())
        by = {c.name: c for c in cases}
        S = {}
        for draw in range(draws):
            rng = np.random.default_rng(SEED + draw)
            for c in Chain(n, nz, storage="f32").cases(inject=lambda name: {k: f32_neighbours(v, rng) for k, v in by[name].before.items()}):
                for var, win, nk, _, _ in c.checks:
                    d = float(np.abs(cut(c.raw[var], win, nk) - cut(by[c.name].raw[var], win, nk)).max())
                    assert np.isfinite(d), (c.name, var)
                    S[c.name, var] = max(S.get((c.name, var), 0.0), d)
        _oracle[n, nz] = (chain, cases, S)
    return _oracle[n, nz]


def ulps(a, b):
    """The distance of two float32 arrays in units of the last place (NaN on either side: a huge number)."""
    def ordered(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(ordered(np.ascontiguousarray(a)) - ordered(np.ascontiguousarray(b)))
    d[np.isnan(a) | np.isnan(b)] = 2 ** 40
    return d


def judge(cls, got, ref, S):
    """One output against float32(ref) in its class.  Returns (row of measurements, None or what is wrong)."""
    kind, _, factor, flips = cls
    assert got.dtype == np.float32, got.dtype
    ref32 = ref.astype(np.float32)
    assert np.array_equal(ref32.astype(np.float64), ref), "the oracle's `after` is not a float32 value"
    fill = np.abs(ref) >= opchain.F32_MAX  # (pk3's fill where the window holds it: kept bit for bit, and not a magnitude)
    if fill.any():
        assert np.array_equal(got[fill], ref32[fill]), "the fill value changed"
        got, ref, ref32 = got[~fill], ref[~fill], ref32[~fill]
    u = ulps(got, ref32)
    ndiff, worst = int((u != 0).sum()), int(u.max()) if u.size else 0
    err = float(np.abs(got.astype(np.float64) - ref).max()) if np.isfinite(got).all() else np.inf
    scale = float(np.abs(ref).max())
    row = dict(cls=kind, differ=ndiff, of=int(u.size), ulps=worst, err_in_u=err / (2.0 ** -24 * scale + 1e-300),
               err_over_S=err / S if S > 0 else (0.0 if err == 0 else np.inf))
    wrong = None
    if kind == "exact":
        if not np.array_equal(got, ref32):
            wrong = "not bit-identical"
    elif kind == "last-place":
        if worst > 1 or ndiff > LAST_PLACE_FRACTION * u.size:
            wrong = "beyond the float64 last place"
    else:
        bound = opchain.staged_bound(scale, S, factor)
        row["bound_over_S"] = bound / S if S > 0 else np.inf
        if not err <= bound:
            wrong = f"error {err:.3e} above 2^-23 max|ref| + {factor:g} S = {bound:.3e}"
        elif flips is not None and (worst > 1 or ndiff > flips * u.size):
            wrong = f"{ndiff} of {u.size} differ, by up to {worst} ulp: more than 1 ulp on {flips:g} of the elements"
    return row, wrong


def ws_of_stored_bottom(case, f, dt, km):
    """ws3 == float32((zs - gz_out[:, :, km]) x (1 / dt2)) on compute +- 1, wsd == float32((zs - zh_out[:, :, km]) / dt) on the
    compute domain: the oracle's two expressions (oracle/vertical.py update_dz_c, update_dz_d) on the bottom height the operator
    itself stored, bit for bit.  Returns None or what is wrong."""
    var, hv = ("ws3", "gz") if case.name == "updatedzc" else ("wsd", "zh")
    (win,) = [c[1] for c in case.checks if c[0] == var]
    got, zs, bottom = f[var].numpy(), case.before["zs"], f[hv].numpy().astype(np.float64)[:, :, km]
    want = ((zs - bottom) * (1.0 / (0.5 * dt)) if var == "ws3" else (zs - bottom) / dt).astype(np.float32)
    if got.dtype != np.float32 or not np.array_equal(got[win], want[win]):
        return f"{var} is not float32 of the oracle's expression on the stored bottom height ({int(ulps(got[win], want[win]).max())} ulp)"
    return None


def show(tag, name, var, row):
    print(f"F32OPS {tag} {name}.{var} {row['cls']} differ={row['differ']}/{row['of']} ulps={row['ulps']} "
          f"err={row['err_in_u']:.2f}u err/S={row['err_over_S']:.3g}")


# ---- the libraries -----------------------------------------------------------------------------------------------------------
_libs = {}


def library(which):
    """(float32-storage library, device) of "emulated" or "device", loaded once."""
    if which not in _libs:
        from pace_amd import _lib

        _libs[which] = (_lib.Library(build_emu_f32()), "cpu") if which == "emulated" else (_lib.load(32), "cuda")
        assert _libs[which][0].real_bytes == 4
    return _libs[which]


# the device shapes: the smallest at which each transport family and c_sw's tile-and-band form run (test_gpu_device_paths.py
# launch_facts); float32 row strides 32, 64, 96 and 128 elements; 96 is the only one with the 32 x 24 fused kernel, which
# BASELINE configuration 5 is benchmarked on.  Emulated: the general kernel on a partial tile, and the 16 x 24 fused kernel with
# c_sw's tile kernel.  (Level-count branches and the column solver's instances: test_gpu_device_paths.py, not repeated here.)
LEAN = {13: False, 48: True, 72: False, 96: True}
CHAIN_SHAPES = [pytest.param("emulated", 13, 5, id="emulated-13x5"), pytest.param("emulated", 48, 3, id="emulated-48x3")] + [
    pytest.param("device", n, nz, id=f"gpu-{n}x{nz}", marks=pytest.mark.gpu) for n, nz in ((13, 33), (48, 8), (72, 3), (96, 3))]


@pytest.mark.parametrize("which,n,nz", CHAIN_SHAPES)
def test_f32_operator_chain_vs_float32_of_oracle(which, n, nz):
    """All 15 operators of the acoustic loop body on the float32-storage library, each output in the class TABLE gives it."""
    lib, device = library(which)
    chain, cases, S = oracle_cases(n, nz)
    ops = ProductOps(lib, device, chain)
    lean = lib.cdll.pace_d_sw_wind_outputs_supported(C.byref(ops.dsw._geom), C.byref(ops.dsw._cfg)) == 1
    assert lean == LEAN[n], (n, lean)
    assert ops.env.qf.row_stride == 32 * ((n + 7 + 31) // 32), ops.env.qf.row_stride
    ctx = {which}
    tag = f"{which} n={n} nz={nz}"
    seen, wrong = [], []
    for case in cases:
        f = ops.run(case.name, poisoned(case))
        for var, win, nk, _, _ in case.checks:
            got = cut(f[var].numpy(), win, nk)
            row, bad = judge(resolve(TABLE[case.name, var], ctx), got, cut(case.after[var], win, nk), S[case.name, var])
            show(tag, case.name, var, row)
            if bad:
                wrong.append((case.name, var, bad, row))
        if case.name in ("updatedzc", "updatedzd"):  # ws3 / wsd additionally, and exactly
            bad = ws_of_stored_bottom(case, f, chain.dt, nz)
            if bad:
                wrong.append((case.name, bad))
        seen.append(case.name)
    assert not wrong, wrong
    assert len(seen) == 15 and len(set(seen)) == 15


def test_every_output_has_one_class():
    """TABLE covers every (operator, output) of the chain's checks, resolves to one class on either tier, and every entry that
    is not exact names its intermediate."""
    chain = Chain(13, 3, storage="f32")
    keys = {(c.name, chk[0]) for c in chain.cases() for chk in c.checks}
    assert keys == set(TABLE), (keys ^ set(TABLE))
    for key, spec in TABLE.items():
        for which in ("emulated", "device"):
            kind, why, factor, _ = resolve(spec, {which})
            assert kind in ("exact", "last-place", "staged"), key
            assert kind != "last-place" or which == "device", key
            assert kind != "staged" or (why and 0 < factor <= MAX_FACTOR), key


def test_ws_is_ill_conditioned_in_float32_heights():
    """No kernel here: why ws3 / wsd cannot be held to float32(oracle).  ws = (zs - bottom height) / dt is a difference of two
    heights of ~1e3 m that agree to ~1e-2 m, over a few seconds.  The oracle's two expressions (oracle/vertical.py update_dz_c,
    update_dz_d) applied to the float32-rounded bottom height and to the unrounded one differ by up to half a float32 ulp of the
    height over dt, and the oracle's own response S to one float32 ulp of noise on its inputs is larger than that.  Recorded
    (u = 2^-24 max |ws|) at 13 x 5: ws3 3.0e5 u = 1.8 % of the field (S 1.2e6 u), wsd 3.5e4 u = 0.2 % (S 1.4e5 u); at 48 x 3:
    9.7e4 u = 0.6 % (S 3.9e5 u) and 4.9e4 u = 0.3 % (S 2.8e5 u).  Asserted: between 1e4 u and 1e6 u at these two shapes, a
    decade either side of what is recorded.  (With 33 levels the same difference is 2.8e6 u and 4.0e6 u, 17 and 24 % of the field:
    the module docstring.)  A kernel that stores the height as float32 and forms ws from the stored value is therefore as good as
    float32 heights allow; test_f32_operator_chain_vs_float32_of_oracle pins it to exactly that expression."""
    for n, nz in ((13, 5), (48, 3)):
        chain, cases, S = oracle_cases(n, nz)
        by = {c.name: c for c in cases}
        for name, var, hv, lo, rdt in (("updatedzc", "ws3", "gz", 1, 1.0 / (0.5 * chain.dt)), ("updatedzd", "wsd", "zh", 0, None)):
            case = by[name]
            win = opchain._win(n, lo, lo)
            zs, bottom = case.before["zs"][win], case.raw[hv][win][:, :, nz]
            form = (lambda h: (zs - h) * rdt) if rdt else (lambda h: (zs - h) / chain.dt)
            assert np.array_equal(form(bottom), case.raw[var][win])  # the oracle's expression, on the oracle's height
            diff = np.abs(form(f32(bottom)) - form(bottom))
            u = 2.0 ** -24 * float(np.abs(form(bottom)).max())
            print(f"F32OPS conditioning n={n} nz={nz} {var}: rounded height {diff.max() / u:.3g} u = {diff.max() / (u * 2 ** 24):.2%} of the "
                  f"field, S = {S[name, var] / u:.3g} u")
            assert 1e4 * u < diff.max() < 1e6 * u, (var, diff.max() / u)
            # where it comes from: half an ulp of the height, over dt
            assert diff.max() <= 2.0 ** -24 * float(np.abs(bottom).max()) / (0.5 * chain.dt if rdt else chain.dt) * (1 + 1e-12)
            assert S[name, var] > diff.max(), (var, S[name, var] / u)  # one ulp of input noise moves the oracle further


STANDALONE = [pytest.param("emulated", 13, 5, id="emulated-13x5"), pytest.param("device", 48, 8, id="gpu-48x8", marks=pytest.mark.gpu)]


@pytest.mark.parametrize("which,n,nz", STANDALONE)
def test_f32_standalone_operators_vs_float32_of_oracle(which, n, nz):
    """XPiecewiseParabolic / YPiecewiseParabolic (iord 5, 6, 8: one pass from loads to stores) equal float32(oracle) bit for bit
    and write nothing outside origin .. origin + domain.  DivergenceDamping: divgd, uc, vc exact (k_divdamp_fused runs the passes
    in LDS in double and stores the last one once); vort_b, ke, delpc staged (the relative vorticity averaged to the corners and
    the damped vorticity are real fields; delpc: the halo-state kernel replays the passes from stored values).  Sim1Solver's w,
    dz, pe staged: the column kernel keeps its elimination coefficients in five real workspace fields (k_sim1.hip Sim1Work).
    (opchain.check_standalone_operators with storage="f32".)"""
    lib, device = library(which)
    report = {}
    errs = opchain.check_standalone_operators(lib, device, n, nz, exact=True, storage="f32", report=report)
    for name, r in report.items():
        print(f"F32OPS {which} n={n} nz={nz} standalone {name} staged err={r['err_in_u']:.2f}u err/S={r['err_over_S']:.3g}")
    assert {f"{a}ppm{o}" for a in "xy" for o in (5, 6, 8)} <= set(errs)
    assert all(errs[f"{a}ppm{o}"] == 0.0 for a in "xy" for o in (5, 6, 8)), errs
    assert len(report) == 6 + 6, sorted(report)


# ---- the two height updates where their flux terms are not negligible ----------------------------------------------------------
# On the chain's state the advective terms of updatedzc / updatedzd are 1e-4 of the heights they update, and smooth: an error of
# one float32 rounding in a flux, or in the interface winds the fluxes are made of, does not reach the last place of gz or zh
# (the flux of a nearly uniform height cancels against the change of the cell's area).  Here the heights are multiplied, column by
# column, by 1 +- 2^-4 in a checkerboard and the winds (updatedzc: ut, vt) or Courant numbers and area fluxes (updatedzd) by
# 1024 -- Courant numbers of 0.1 to 0.3 -- so that the fluxes decide the result.  updatedzd runs with hord_tm = 6 (the
# transport kernel's height epilogue) and with hord_tm = 8, the only way to k_fvtp2d + k_delnflux + k_apply_height_fluxes, which
# the chain never takes.  With 33 levels the dp_ref pairs of updatedzc's interface winds have sums that are no float32 values: this
# case found `dp_ref[k - 1] + dp_ref[k]` and its like evaluated in float by the float32 build (k_acoustic.hip pavg), 1 ulp of gz
# on 19 of 7650 points.
ROUGH_SHAPE = (13, 33)
ROUGH = [("updatedzc", 0), ("updatedzd", 6), ("updatedzd", 8)]
_rough = {}


def rough_cases():
    """{(operator, hord_tm): (OpCase, {output: S})} on the chain's `before` of the operator, roughened as described above."""
    if not _rough:
        from oracle import vertical

        n, nz = ROUGH_SHAPE
        chain, cases, _ = oracle_cases(n, nz)
        by = {c.name: c for c in cases}
        g, dt = chain.g, chain.dt
        i, j = np.indices(by["updatedzc"].before["zs"].shape)
        board = 1.0 + 2.0 ** -4 * np.where((i + j) % 2 == 0, 1.0, -1.0)

        def oracle(name, b, hord):
            a = {k: v.copy() for k, v in b.items()}
            if name == "updatedzc":
                a["zh"][:-1, :-1, :] = a["gz"][:-1, :-1, :]
                vertical.update_dz_c(g, g.dp_ref, a["zs"], a["ut"], a["vt"], a["gz"], a["ws3"], 0.5 * dt)
            else:
                vertical.update_dz_d(g, chain.col, g.dp_ref, a["zs"], a["zh"], a["crx"], a["cry"], a["xfx"], a["yfx"], a["wsd"], dt, hord_tm=hord)
            return a

        for name, hord in ROUGH:
            outs = ("gz", "ws3") if name == "updatedzc" else ("zh", "wsd")
            b = {k: v.copy() for k, v in by[name].before.items()}
            for k in (("ut", "vt") if name == "updatedzc" else ("crx", "cry", "xfx", "yfx")):
                b[k] *= 1024.0
            for k in ("gz", "zh", "zs"):
                b[k] = f32(b[k] * (board[:, :, None] if b[k].ndim == 3 else board))
            raw = oracle(name, b, hord)
            checks = [c for c in by[name].checks if c[0] in outs]
            assert len(checks) == 2 and all(np.isfinite(cut(raw[var], win, nk)).all() for var, win, nk, _, _ in checks)
            S = dict.fromkeys(outs, 0.0)
            for draw in range(2):
                rng = np.random.default_rng(SEED + draw)
                noisy = oracle(name, {k: f32_neighbours(v, rng) for k, v in b.items()}, hord)
                for var, win, nk, _, _ in checks:
                    S[var] = max(S[var], float(np.abs(cut(noisy[var], win, nk) - cut(raw[var], win, nk)).max()))
            _rough[name, hord] = (opchain.OpCase(name, b, opchain.f32_dict(raw), checks), S)
    return _rough


@pytest.mark.parametrize("which", [pytest.param("emulated", id="emulated"), pytest.param("device", id="gpu", marks=pytest.mark.gpu)])
def test_f32_height_updates_with_rough_heights_and_large_courant_numbers(which):
    """updatedzc's gz: exact (one pass from ut, vt, gz, dp_ref to gz_new).  updatedzd's zh, hord_tm 6 and 8: staged -- the
    interface Courant numbers and area fluxes (crx_i, cry_i, xfx_i, yfx_i) are real fields, and with hord_tm = 8 so are the four
    flux fields fx, fy, fx2, fy2 between k_fvtp2d, k_delnflux and k_apply_height_fluxes.  ws3 / wsd: staged as in TABLE, and the
    oracle's expression on the stored bottom height, exactly."""
    from pace_amd.fv3core.stencils.updatedzd import UpdateHeightOnDGrid

    n, nz = ROUGH_SHAPE
    lib, device = library(which)
    chain = oracle_cases(n, nz)[0]
    ops = ProductOps(lib, device, chain)
    env = ops.env
    dzd = {6: ops.dzd, 8: UpdateHeightOnDGrid(env.stencil_factory, env.qf, env.damping, env.grid_data, 0, 8,
                                              {k: env.kq(v) for k, v in chain.col.items()})}
    wrong = []
    for (name, hord), (case, S) in rough_cases().items():
        ops.dzd = dzd.get(hord, ops.dzd)
        f = ops.run(name, poisoned(case))
        for var, win, nk, _, _ in case.checks:
            cls = resolve(TABLE[name, var], {which})
            if var == "zh":
                cls = staged("crx_i, cry_i, xfx_i, yfx_i (and fx, fy, fx2, fy2 with hord_tm = 8) are real fields")
            row, bad = judge(cls, cut(f[var].numpy(), win, nk), cut(case.after[var], win, nk), S[var])
            show(f"{which} rough n={n} nz={nz} hord_tm={hord}", name, var, row)
            if bad:
                wrong.append((name, hord, var, bad, row))
        bad = ws_of_stored_bottom(case, f, chain.dt, nz)
        if bad:
            wrong.append((name, hord, bad))
    assert not wrong, wrong
