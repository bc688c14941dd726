"""The column kernels past one 64-lane block, against the reference: C68 inputs assembled from the columns of the C12 fixtures
(tests/columns.py), the expectation for every column the reference's output for its source column.

k_microphysics, k_physics_prepare, k_dry_convective_adjust and k_sat_adjust run one thread per column, i = is + blockIdx.x * 64 +
threadIdx.x; the C12 and C20 cases never leave block 0, and the larger cases compare with the emulated build of the same source
or check conservation only.  C68 is two blocks per row, the second with four of its 64 lanes: the smallest size that reaches
blockIdx.x > 0.  Every check here runs on the emulated library in the CPU tier and on the device with -m gpu.

Bounds: those of the C12 tests, imported with their helpers -- the microphysics by the reference's `Microph` line (MAX_ERROR =
2.2e-8 in the reference's relative measure, the NEAR_ZERO table); the saturation adjustment by TranslateSatAdjust3d's 2e-11 (the
emulated library also by test_sat_adjust_emulated's 2e-12 and 1e-13); BIT IDENTITY for the dry convective adjustment, the
physics-to-dycore coupling, the Physics shell's fields before the microphysics and its forward Euler.

Copies: every copy of one source column has to hold the same bits, and those of the same library's run on the untiled C12
fixture, in every output that is compared with a tolerance.  The emulator runs one thread at a time, so on the device this is
the check that sees columns interfering with each other (two columns that share workspace, a race) below the bound.

Measured, worst over the cases (every test prints its own).  Microphysics, the emulated library: udt 1.8e-11, vdt 5.2e-11
(mptime), the species' tendencies <= 5e-13, pt_dt 1.3e-12, wmp 1.9e-15, precipitation 7.8e-15 -- the figures of C12, as they
have to be (each case 1.1 to 1.7 s); the saturation adjustment: qliquid 1.0e-12, qrain 1.3e-13, the rest <= 1e-13, as at C12.
The MI355X, Microphysics at C68, worst over the five cases: qv_dt 5.8e-13, ql_dt 2.1e-13, qr_dt 1.8e-13, qi_dt 4.6e-12, qs_dt
2.4e-13, qg_dt 2.3e-11 (sub2), udt 1.2e-10 and vdt 5.2e-11 (mptime), pt_dt 1.8e-12 (dry), wmp 2.3e-15, precipitation 7.3e-14
(ice, mptime) -- per case and per variable the device's figures at C12.  Physics at C68: vdt 2.3e-11, udt 1.4e-11, qg_dt
9.7e-13, wmp 2.3e-13, the other tendencies <= 2.8e-13 (C12: the same).  SatAdjust3d at C68, worst over the five cases: qcld
5.2e-13 (rad), te 1.5e-13 (consv), qliquid 9.3e-14, q_con 9.2e-14, qrain 7.7e-14, qice 5.3e-14, qsnow 3.0e-14, qgraupel 2.7e-14,
qvapor 2.0e-14, pt 3.4e-15, pkz 2.7e-15, cappa 1.1e-15.  The copy checks have no figure, they are bit identity: on the emulated
library and on the device no value of any output differs between the copies of a column or from the C12 run, in all five
Microphysics cases, the Physics call and the five SatAdjust3d cases; the dry convective adjustment (seven cases) and
PhysicsToDycore equal the gathered reference bit for bit on both.  The 19 device tests take 2.6 s together."""
import numpy as np
import pytest

import columns
import test_fv_subgridz as sgz
import test_microphysics as mph
import test_physics as phy
import test_physics_coupling as cpl
import test_sat_adjust as sat
from helpers import build_emu, golden

mgp = phy.mgp

N, NZ = 68, 79
CMAP = columns.column_map(N, seed=68)
BOTH = [pytest.param("emulated", id="emulated"), pytest.param("device", id="gpu", marks=pytest.mark.gpu)]

_libs = {}


def library(which):
    """(library, device) of "emulated" or "device", loaded once."""
    if which not in _libs:
        from pace_amd import _lib

        _libs[which] = (_lib.Library(build_emu()), "cpu") if which == "emulated" else (_lib.load(), "cuda:0")
    return _libs[which]


def gather(a):
    return columns.gather(a, CMAP)


# ---- the map -------------------------------------------------------------------------------------------------------------------

def test_column_map():
    columns.check_column_map(CMAP, N)
    si, sj = CMAP
    counts = np.bincount((si * 12 + sj).ravel(), minlength=144)
    assert counts.min() == 32 and counts.max() == 33 and (si[64:].size, len(np.unique((si * 12 + sj)[64:]))) == (272, 144)
    again = columns.column_map(N, seed=68)
    assert np.array_equal(again[0], si) and np.array_equal(again[1], sj)
    other = columns.column_map(N, seed=1)
    assert not np.array_equal(other[0], si)
    columns.check_column_map(columns.column_map(20, seed=3), 20)
    # gather and embed
    a = np.arange(144.0).reshape(12, 12)
    assert np.array_equal(gather(a), si * 12.0 + sj)
    b = np.arange(144.0 * 5).reshape(12, 12, 5)
    g = gather(b)
    assert g.shape == (N, N, 5) and np.array_equal(g[65, 7], b[si[65, 7], sj[65, 7]])
    full = columns.embed(g, N)
    assert full.shape == (N + 7, N + 7, 6) and np.array_equal(full[3:3 + N, 3:3 + N, :5], g) and np.isnan(full).sum() == full.size - g.size
    assert columns.embed(gather(a), N).shape == (N + 7, N + 7)
    d = columns.gather_all({"x": b, "k_sel": np.arange(12), "s": 1.0}, CMAP)
    assert d["x"].shape == (N, N, 5) and d["k_sel"].shape == (12,) and d["s"] == 1.0
    # check_copies sees one differing copy, and a tiled output that is consistent but not the untiled run's
    columns.check_copies(g, b, CMAP, "clean")
    bad = g.copy()
    bad[66, 3, 2] = np.nextafter(bad[66, 3, 2], np.inf)
    with pytest.raises(AssertionError, match="between copies"):
        columns.check_copies(bad, b, CMAP, "one copy off")
    with pytest.raises(AssertionError, match="untiled"):
        columns.check_copies(g, b + 1.0, CMAP, "another run")


# ---- Microphysics --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", mph.TAGS)
@pytest.mark.parametrize("which", BOTH)
def test_microphysics_c68(which, tag):
    """All five cases at C68 x 79 against the gathered reference outputs within the reference's bound; the fields the reference
    leaves alone keep their bits and nothing is written outside the compute domain; every copy of a source column holds the
    bits of the same library's C12 run."""
    lib, device = library(which)
    cfg = mph.CASES[tag]
    inp12 = mph.case_inputs(tag)
    inp = columns.gather_all(inp12, CMAP)
    out, op = mph.run(lib, device, inp, [cfg["timestep"]], cfg["mp_time"], n=N)
    assert op._ntimes == (2 if tag in ("sub2", "mptime") else 1)
    mph.check_against_reference(tag, out, inp, f"{which} C68", n=N, gather=gather)
    out12, _ = mph.run(lib, device, inp12, [cfg["timestep"]], cfg["mp_time"])
    for name in mph.OUT:
        columns.check_copies(mph.window(out, name, N), mph.window(out12, name), CMAP, (tag, name))


# ---- Physics: prepare, the microphysics, update_physics_state_with_tendencies ------------------------------------------------

@pytest.mark.parametrize("which", BOTH)
def test_physics_c68(which):
    """The three parts of the Physics call at C68 x 79 from the physics_c12_pre / post fixtures: every `pre` field (wmp included)
    to the bit and the tendencies zero after prepare; after the call `pre` but wmp still to the bit, the tendencies and wmp within
    the `Microph` bound, the forward Euler exact, nothing outside the domain; copies of the tendencies, wmp and the updated
    fields bit-identical with the C12 run."""
    lib, device = library(which)
    inp12 = phy.inputs()
    inp = columns.gather_all(inp12, CMAP)
    pre, post, _ = mgp.run_operators(lib, device, inp, phy.ptop(), N, NZ)
    want_pre = columns.gather_all(phy.golden("pre"), CMAP)
    phy.check_pre(pre, n=N, want=want_pre)
    for name in phy.TEND:
        assert (phy.window(pre[name], name, N, NZ) == 0).all(), name
    phy.check_nothing_outside(pre, N)
    assert np.array_equal(pre["land"], columns.embed(inp["land"], N), equal_nan=True)
    phy.check_pre(post, [name for name in phy.PRE if name != "wmp"], n=N, want=want_pre)
    phy.check_tendencies(post, columns.gather_all(phy.golden("post"), CMAP), f"{which} C68", N)
    phy.check_euler(post, N)
    phy.check_nothing_outside(post, N)
    _, post12, _ = mgp.run_operators(lib, device, inp12, phy.ptop())
    for name in phy.TEND + ["wmp"] + phy.UPDATED:
        columns.check_copies(phy.window(post[name], name, N, NZ), phy.window(post12[name], name, 12, NZ), CMAP, name)


# ---- PhysicsToDycore ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", BOTH)
def test_physics_to_dycore_c68(which):
    """C68 x 79 from physics_c12_coupled: the dycore side and the fixture's physics side gathered, every coupled field to the
    bit, nothing outside the compute domain."""
    lib, device = library(which)
    inp = columns.gather_all(cpl.inputs(), CMAP)
    side = columns.gather_all(cpl.fixture_physics_side(), CMAP)
    entry = columns.gather_all(cpl.entry_tendencies(), CMAP)
    got = mgp.run_coupling(lib, device, inp, side, entry, N, NZ)
    cpl.check_coupled(got, columns.gather_all(cpl.golden("coupled"), CMAP), N, NZ)


# ---- DryConvectiveAdjustment -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", sgz.CASES + ["base_r32"])
@pytest.mark.parametrize("which", BOTH)
def test_dry_convective_adjust_c68(which, tag):
    """Every case of tests/test_fv_subgridz.py at C68 x 79: bit equality with the gathered expectation; halo, the extra level and
    the levels from k_sponge on keep their bits.  pe has the one element the operator reads."""
    lib, device = library(which)
    d, inp12 = sgz.case(tag), sgz.inputs()
    if tag == "base_r32":
        inp12 = sgz.rounded(inp12)
    out, full = sgz.run_case(lib, device, d, columns.gather_all(inp12, CMAP), n=N)
    assert np.isfinite(full["pe"]).sum() == 1 and np.isfinite(full["pe"][3, 3, 0])
    sgz.check_bitwise(d, out, full, inp12, tag, n=N, gather=gather)


# ---- SatAdjust3d -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", sat.CASES)
@pytest.mark.parametrize("which", BOTH)
def test_sat_adjust_c68(which, tag):
    """The five cases at C68 with the fixture's levels and kmp: TranslateSatAdjust3d's 2e-11 (the emulated library also to
    test_sat_adjust_emulated's 2e-12 overall and 1e-13 for pt, pkz, cappa, qvapor); everything outside the window holds what it
    held; copies bit-identical with the C12 run."""
    lib, device = library(which)
    d12 = golden("satadj_c12.npz")
    d = columns.gather_all(d12, CMAP)
    out, full = sat.run_sat_adjust(lib, device, d, tag, n=N)
    worst = sat.check_sat_adjust(d, out, full, tag, 2e-11, n=N)
    print(which, "C68", tag, " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    if which == "emulated":
        assert max(worst.values()) < 2e-12, worst
        assert max(worst[k] for k in ("pt", "pkz", "cappa", "qvapor")) < 1e-13, worst
    out12, _ = sat.run_sat_adjust(lib, device, d12, tag)
    kmp, nk = int(d["kmp"]), len(d["k_sel"])
    for name in sat.SA_OUT:
        columns.check_copies(out[name][3:3 + N, 3:3 + N, kmp:nk], out12[name][3:15, 3:15, kmp:nk], CMAP, (tag, name))
