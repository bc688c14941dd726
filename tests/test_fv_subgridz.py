"""The dry convective adjustment (DryConvectiveAdjustment, k_subgridz.hip) against runs of the reference
(tools/make_golden_fvsubgridz.py): the emulated library on the CPU, the gfx950 library with -m gpu.

The operator has no transcendental, and the reference's two `**` (x ** 2, (1 - r) ** 2.0) are products in the interpreter's run
(the tool's numpy restatement, which writes them as products, reproduces every output of every case bit for bit), so every
comparison with the reference in fp64 is BIT EQUALITY."""
import os
import types

import numpy as np
import pytest

from helpers import GOLDEN, Env, build_emu, build_emu_f32, compare, golden, minimal_metrics

N, NZ = 12, 79
TRACERS = ["qvapor", "qliquid", "qrain", "qice", "qsnow", "qgraupel", "qo3mr", "qsgs_tke", "qcld"]
MIXED = TRACERS + ["ua", "va", "w"]
IN3 = ["delp", "delz", "pkz", "peln", "pt"] + MIXED[9:] + TRACERS
OUT = ["pt", "ua", "va", "w"] + TRACERS + ["u_dt", "v_dt"]
CASES = ["base", "full", "top", "all", "pe1", "nwat0"]
C = slice(3, 3 + N)


@pytest.fixture(scope="module")
def emu_lib():
    from pace_amd import _lib

    return _lib.Library(build_emu())


@pytest.fixture(scope="module")
def emu_f32_lib():
    from pace_amd import _lib

    return _lib.Library(build_emu_f32())


@pytest.fixture(scope="module")
def lib():
    from pace_amd import _lib

    return _lib.load()


def inputs():
    d = {}
    for m in range(3):
        d.update(golden(f"fvsubgridz_c12_in{m}.npz"))
    return {n: d["in_" + n] for n in IN3}


def rounded(inp):
    return {n: v.astype(np.float32).astype(np.float64) for n, v in inp.items()}


def case(tag):
    d = golden(f"fvsubgridz_c12_{tag}.npz")
    if os.path.exists(os.path.join(GOLDEN, f"fvsubgridz_c12_{tag}_b.npz")):
        d.update(golden(f"fvsubgridz_c12_{tag}_b.npz"))
    return d


def expected(d, name, inp):
    """The reference's output on (compute domain, levels < k_sponge): stored whole, or as the points that differ from the input."""
    ks = int(d["k_sponge"])
    base = inp[name][:, :, :ks] if name in inp else np.zeros((N, N, ks))
    if "out_" + name in d:
        return d["out_" + name]
    out = np.ascontiguousarray(base).copy()
    out.ravel()[d[f"out_{name}__idx"]] = d[f"out_{name}__val"]
    return out


def embed(inp, pe00, n=N):
    """The inputs in NaN-filled storage; of pe only the element the operator reads is set."""
    full = {}
    for name in IN3 + ["pe", "u_dt", "v_dt"]:
        a = np.full((n + 7, n + 7, NZ + 1), np.nan)
        if name in inp:
            a[3:3 + n, 3:3 + n, :inp[name].shape[2]] = inp[name]
        full[name] = a
    full["pe"][3, 3, 0] = pe00
    return full


def run_case(lib, device, d, inp, tensors=False, n_sponge="fixture", n=N):
    """DryConvectiveAdjustment with the case's arguments on `inp` (n x n columns; the operator reads no metric term, so any size
    other than the fixture's gets minimal ones); returns (outputs, storage before the call) as full arrays."""
    from pace_amd.fv3core import DryConvectiveAdjustment

    env = Env(lib, device, golden("grid_c12_tile0.npz") if n == N else minimal_metrics(n), n, NZ)
    full = embed(inp, float(d["pe00"]), n)
    q = {k: env.q3(v) for k, v in full.items()}
    if n_sponge == "fixture":
        n_sponge = None if int(d["n_sponge"]) < 0 else int(d["n_sponge"])
    op = DryConvectiveAdjustment(env.stencil_factory, env.qf, int(d["nwat"]), int(d["fv_sg_adj"]), n_sponge, False)
    fields = {k: (v.data if tensors else v) for k, v in q.items()}
    state = types.SimpleNamespace(**{k: v for k, v in fields.items() if k not in ("u_dt", "v_dt")})
    op(state, fields["u_dt"], fields["v_dt"], float(d["timestep"]))
    if device != "cpu":
        import torch

        torch.cuda.synchronize()
    return {k: v.numpy() for k, v in q.items()}, full


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def check_bitwise(d, out, full, inp, tag, n=N, gather=None):
    """`inp`: the fixture's C12 inputs (the expectation is stored against them); gather: what takes a C12 window to the n x n
    one the operator ran on (tests/columns.py), none at C12."""
    ks = int(d["k_sponge"])
    for name in OUT:
        ref, got = expected(d, name, inp), out[name][3:3 + n, 3:3 + n, :ks]
        if gather is not None:
            ref = gather(ref)
        same = bits(ref) == bits(got)
        assert same.all(), (tag, name, int((~same).sum()), "points differ; worst", compare(ref, got))
    check_outside(out, full, ks, tag, n=n)


def check_outside(out, full, ks, tag, f32=False, n=N):
    """Halo, the extra level and levels >= k_sponge keep their bits, in every field the operator is given."""
    outside = np.ones((n + 7, n + 7, NZ + 1), dtype=bool)
    outside[3:3 + n, 3:3 + n, :ks] = False
    for name in full:
        before = full[name].astype(np.float32).astype(np.float64) if f32 else full[name]
        where = outside if name in OUT else np.ones_like(outside)
        assert np.array_equal(out[name][where], before[where], equal_nan=True), (tag, name, "changed outside the window")


# ---- the fixture itself --------------------------------------------------------------------------------------------------

def test_fixture_coverage():
    """The counts tools/make_golden_fvsubgridz.py stored (over (column, level, sweep) of case base, from its restatement of the
    operator after that reproduced the reference's run bit for bit) reach what the inputs were built for."""
    d = case("base")
    cov = {k[4:]: (int(v[0]), int(v[1])) for k, v in d.items() if k.startswith("cov_")}
    need = {"mixing": 500, "not_mixing": 500, "mixing_level1": 10, "mixing_level2": 10, "mixing_level3": 10,
            "factor_decides_level1": 5, "factor_decides_level2": 5, "factor_decides_level3": 5, "t_max_branch": 10,
            "t_min_branch_clamped": 10, "t_min_decides_pe1": 10, "t_max_decides_top": 10, "ri_ref_capped": 10, "ri_ref_uncapped": 10,
            "tracers_nonzero_in_mixed_columns": 1, "negative_condensate": 1}
    for name, least in need.items():
        assert cov[name][1] >= least and cov[name][0] >= cov[name][1], (name, cov[name])
    # what can be recounted from the stored arrays: outputs that t_min alone decides, and the blending of case base
    inp = inputs()
    base, pe1, full = d, case("pe1"), case("full")
    differ = np.zeros((N, N, 48), dtype=bool)
    for name in OUT:
        differ |= bits(expected(base, name, inp)) != bits(expected(pe1, name, inp))
    assert int(differ.sum()) == cov["t_min_decides_pe1"][0]
    assert float(base["timestep"]) / float(base["fv_sg_adj"]) < 1 <= float(full["timestep"]) / float(full["fv_sg_adj"])
    assert int(case("top")["k_sponge"]) == 10 and int(case("all")["k_sponge"]) == NZ and int(case("nwat0")["nwat"]) == 0
    assert float(pe1["pe00"]) == 1.0 and float(base["pe00"]) >= 2.0


# ---- the emulated library --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", CASES)
def test_dry_convective_adjust_emulated(emu_lib, tag):
    """Every output of every case equals the reference's run bit for bit; nothing outside origin (isc, jsc, 0), domain
    (nx, ny, k_sponge) changes."""
    d, inp = case(tag), inputs()
    out, full = run_case(emu_lib, "cpu", d, inp)
    check_bitwise(d, out, full, inp, tag)


def test_dry_convective_adjust_rounded_inputs_emulated(emu_lib):
    """base_r32: the reference's run on base's inputs rounded to float32 -- the float64 build on the same inputs, bit for bit."""
    d, inp = case("base_r32"), rounded(inputs())
    out, full = run_case(emu_lib, "cpu", d, inp)
    check_bitwise(d, out, full, inp, "base_r32")


def test_dry_convective_adjust_f32_emulated(emu_f32_lib, emu_lib):
    """The float32-storage build on base's inputs against the reference's run on the same inputs rounded to float32 (base_r32):
    equal inputs, fp64 arithmetic in both, so what is left is the float32 rounding of the stored outputs (6e-8); held to
    test_f32.py's one-operator bound 2e-5 on every output, no point left out.  The same against the float64 build on the
    rounded inputs."""
    d, inp = case("base_r32"), inputs()
    r = rounded(inp)
    out, full = run_case(emu_f32_lib, "cpu", d, inp)
    ref64, _ = run_case(emu_lib, "cpu", d, r)
    ks = int(d["k_sponge"])
    for name in OUT:
        got = out[name][C, C, :ks]
        e = compare(expected(d, name, r), got)
        print(name, "against the reference on rounded inputs", e)
        assert e < 2e-5, (name, e)
        e = compare(ref64[name][C, C, :ks], got)
        assert e < 2e-5, (name, "float64 build on float32-rounded inputs", e)
    check_outside(out, full, ks, "f32", f32=True)


# ---- the host layer ----------------------------------------------------------------------------------------------------------

def test_exported_and_configured():
    import pace_amd.fv3core as fv3core
    from pace_amd.fv3core.stencils.fv_subgridz import DryConvectiveAdjustment

    assert fv3core.DryConvectiveAdjustment is DryConvectiveAdjustment
    cfg = fv3core.DynamicalCoreConfig()
    assert cfg.fv_sg_adj == -1 and not cfg.do_dry_convective_adjustment
    assert fv3core.DynamicalCoreConfig(fv_sg_adj=600).do_dry_convective_adjustment
    assert cfg.n_sponge == cfg.acoustic_dynamics.d_grid_shallow_water.n_sponge == 48
    names = [a.arg_name for a in DryConvectiveAdjustment.arg_specs]
    assert sorted(names) == sorted(IN3 + ["pe", "u_dt", "v_dt"])
    assert {a.intent for a in DryConvectiveAdjustment.arg_specs} == {"in", "inout"}


def test_hydrostatic_refused(emu_lib):
    from pace_amd.fv3core import DryConvectiveAdjustment

    env = Env(emu_lib, "cpu", golden("grid_c12_tile0.npz"), N, NZ)
    with pytest.raises(NotImplementedError):
        DryConvectiveAdjustment(env.stencil_factory, env.qf, 6, 600, 48, True)


def test_fewer_than_three_levels_is_a_no_op(emu_lib):
    """n_sponge = 2: the Fortran's early return (the reference's call would raise AttributeError): every bit stays."""
    d, inp = case("base"), inputs()
    out, full = run_case(emu_lib, "cpu", d, inp, n_sponge=2)
    for name in full:
        assert np.array_equal(out[name], full[name], equal_nan=True), name


def test_quantities_and_tensors_give_the_same(emu_lib):
    d, inp = case("base"), inputs()
    out_q, _ = run_case(emu_lib, "cpu", d, inp)
    out_t, _ = run_case(emu_lib, "cpu", d, inp, tensors=True)
    for name in out_q:
        assert np.array_equal(out_q[name], out_t[name], equal_nan=True), name


def test_layout_and_type_are_checked(emu_lib):
    """Every field, pe and peln included, has to be of the library's storage type and layout."""
    import torch

    from pace_amd.fv3core import DryConvectiveAdjustment

    d = case("base")
    env = Env(emu_lib, "cpu", golden("grid_c12_tile0.npz"), N, NZ)
    op = DryConvectiveAdjustment(env.stencil_factory, env.qf, 6, 600, 48, False)
    for bad in ("pe", "peln", "qcld", "v_dt"):
        for wrong in (torch.zeros((N + 7, N + 7, NZ + 1), dtype=torch.float64),  # C order: not the library's layout
                      env.q3().data.to(torch.float32)):
            q = {k: env.q3() for k in IN3 + ["pe", "u_dt", "v_dt"]}
            q[bad] = wrong
            state = types.SimpleNamespace(**{k: v for k, v in q.items() if k not in ("u_dt", "v_dt")})
            with pytest.raises(ValueError):
                op(state, q["u_dt"], q["v_dt"], float(d["timestep"]))


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("tag", CASES + ["base_r32"])
def test_dry_convective_adjust_gpu(lib, tag):
    """The same parity on the device, all seven cases (base_r32: the float64 library on the rounded inputs): bit equality --
    division and multiplication are IEEE on gfx950 and the build does not contract."""
    d, inp = case(tag), inputs()
    if tag == "base_r32":
        inp = rounded(inp)
    out, full = run_case(lib, "cuda:0", d, inp)
    check_bitwise(d, out, full, inp, tag)


def run_c192(lib, device, s, n, nk, k_sponge, timestep):
    from pace_amd.fv3core import DryConvectiveAdjustment

    metrics = {"area": np.full((n + 7, n + 7), 2.7e9), "da_min": 2.7e9, "da_min_c": 2.7e9,
               **{k: np.zeros((n + 7, n + 7)) for k in ("del6_u", "del6_v", "divg_u", "divg_v")}}
    env = Env(lib, device, metrics, n, nk)
    q = {k: env.q3(v) for k, v in s.items()}
    op = DryConvectiveAdjustment(env.stencil_factory, env.qf, 6, 600, k_sponge, False)
    op(types.SimpleNamespace(**{k: v for k, v in q.items() if k not in ("u_dt", "v_dt")}), q["u_dt"], q["v_dt"], timestep)
    if device != "cpu":
        import torch

        torch.cuda.synchronize()
    return {k: v.numpy() for k, v in q.items()}


@pytest.mark.gpu
def test_dry_convective_adjust_c192_gpu(lib, emu_lib):
    """C192 x 79, n_sponge = 48, timestep >= fv_sg_adj: the device's output equals the emulated library's bit for bit on the whole
    storage; every output finite; some point changes; the column sums of delp * q over the window are conserved for each of the
    twelve mixed quantities to 1e-13 of the sum of delp * |q| (each flux leaves one level and enters the next, divided by their
    own delp, and |h0 / delp| never exceeds the difference of the two levels' values, so six roundings per level and sweep stay
    near 1e-15 of that scale; 1e-13 is the margin of the saturation adjustment's conservation test)."""
    from pace_amd import synthetic

    n, nk, ks = 192, NZ, 48
    s = synthetic.convective_state(n, nk)
    out = run_c192(lib, "cuda:0", s, n, nk, ks, 900.0)
    emu = run_c192(emu_lib, "cpu", s, n, nk, ks, 900.0)
    for name in s:
        assert np.array_equal(bits(out[name]), bits(emu[name])), (name, "device and emulation differ")
    win = (slice(3, 3 + n), slice(3, 3 + n), slice(0, ks))
    for name in OUT:
        assert np.isfinite(out[name][win]).all(), name
    assert not np.array_equal(out["qvapor"][win], s["qvapor"][win])
    assert np.count_nonzero(out["u_dt"][win]) > 1000
    dp = s["delp"][win]
    for name in MIXED:
        before, after = (dp * s[name][win]).sum(axis=2), (dp * out[name][win]).sum(axis=2)
        scale = (dp * np.abs(s[name][win])).sum(axis=2)
        e = float(np.max(np.abs(after - before) / scale))
        print(name, "column sum changes by", e)
        assert e < 1e-13, (name, e)
    outside = np.ones(out["pt"].shape, dtype=bool)
    outside[win] = False
    for name in s:
        where = outside if name in OUT else np.ones_like(outside)
        assert np.array_equal(out[name][where], s[name][where]), name
