"""CopyDycoreToPhysics and PhysicsToDycore (pace_amd.stencils.physics_coupling, k_physics.hip) against a run of the reference
(tools/make_golden_physics.py, part `coupled`: fill_gfs_delp, then prepare_tendencies_and_update_tracers) and against
tools/physics_np.py, which a test here holds to that run bit for bit; on the device also the other two kernels of k_physics.hip
at sizes the fixture does not reach.

Bound: BIT IDENTITY -- none of these kernels contains a transcendental.  The one exception is the C20 chain's tendencies, which
come out of the microphysics: the device against the emulated library within the reference's `Microph` line (MAX_ERROR,
NEAR_ZERO of tests/test_microphysics.py's generator, imported); measured on the MI355X: at most 2.5e-10 (vdt)."""
import os
import sys
import types

import numpy as np
import pytest

from helpers import ROOT, build_emu, build_emu_f32

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_physics as mgp  # noqa: E402
import physics_np as npr  # noqa: E402
from make_golden_microphysics import MAX_ERROR, TEND, load_split  # noqa: E402
from make_golden_physics import COUPLED, DT, DYCORE_TEND, LAYER_IN, N, NZ, PRE, UPDATED, bits, embed, window  # noqa: E402


@pytest.fixture(scope="module")
def emu_lib():
    from pace_amd import _lib

    return _lib.Library(build_emu())


@pytest.fixture(scope="module")
def lib():
    from pace_amd import _lib

    return _lib.load()


_cache = {}


def golden(part):
    if part not in _cache:
        _cache[part] = load_split(f"physics_c12_{part}")
    return _cache[part]


def inputs():
    if "inputs" not in _cache:
        _cache["inputs"] = mgp.dycore_inputs()
    return _cache["inputs"]


def fixture_physics_side():
    return mgp.coupling_inputs(inputs(), golden("post"), golden("pre"))


def entry_tendencies(shape=(N, N, NZ)):
    return mgp.coupling_tendencies(shape)


def assert_same_bits(got, want, what):
    assert got.shape == want.shape, what
    diff = bits(got) != bits(want)
    assert not diff.any(), (what, int(diff.sum()), "values differ; first at", tuple(np.argwhere(diff)[0]))


def check_coupled(got_full, want, n=N, nk=NZ):
    for name in COUPLED:
        assert_same_bits(window(got_full[name], name, n, nk), want[name], name)
    for name in COUPLED:  # the storage was NaN outside the compute domain and on level nk
        outside = np.ones(got_full[name].shape, dtype=bool)
        outside[3:3 + n, 3:3 + n, :nk] = False
        assert np.isnan(got_full[name][outside]).all(), (name, "written outside the compute domain")


# ---- the restatement -------------------------------------------------------------------------------------------------------------

def test_numpy_restatement_equals_the_reference():
    want = mgp.numpy_coupled(inputs(), fixture_physics_side(), entry_tendencies())
    ref = golden("coupled")
    for name in COUPLED:
        assert_same_bits(want[name], ref[name], name)
    # fill_gfs_delp had work, the tracers and the air mass changed
    assert not np.array_equal(ref["physics_updated_specific_humidity"], golden("post")["physics_updated_specific_humidity"])
    assert (ref["delp"] != inputs()["delp"]).mean() > 0.5 and (ref["qrain"] != inputs()["qrain"]).any()


# ---- the emulated library ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tensors", [False, True])
def test_coupling_fixture_fed_emulated(emu_lib, tensors):
    got = mgp.run_coupling(emu_lib, "cpu", inputs(), fixture_physics_side(), entry_tendencies(), tensors=tensors)
    check_coupled(got, golden("coupled"))


def test_tendencies_are_accumulated(emu_lib):
    """With zero on entry the result is (t1 - t0) * rdt; with values on entry it is those plus that product, rounded once --
    which is entry + (result from zero) in fp64, to the bit.  Everything else does not depend on the entry values."""
    phy = fixture_physics_side()
    zero = {name: np.zeros((N, N, NZ)) for name in DYCORE_TEND}
    from_zero = mgp.run_coupling(emu_lib, "cpu", inputs(), phy, zero)
    check_coupled(from_zero, mgp.numpy_coupled(inputs(), phy, zero))
    ref, entry = golden("coupled"), entry_tendencies()
    for name in DYCORE_TEND:
        increment = window(from_zero[name], name, N, NZ)
        assert np.count_nonzero(increment) > 100 and (entry[name] != 0).any(), name
        assert_same_bits(entry[name] + increment, ref[name], name)
    for name in COUPLED[3:]:
        assert_same_bits(window(from_zero[name], name, N, NZ), ref[name], name)


def test_rdt_follows_the_namelist(emu_lib):
    from pace_amd.stencils import PhysicsToDycore

    env = mgp.make_env(emu_lib, "cpu", inputs()["area"], N, NZ, 300.0)
    assert PhysicsToDycore(env.stencil_factory, env.qf, mgp.namelist(dt_atmos=450))._rdt == 1.0 / 450.0
    phy = fixture_physics_side()
    got = mgp.run_coupling(emu_lib, "cpu", inputs(), phy, entry_tendencies(), dt_atmos=450)
    want = mgp.numpy_coupled(inputs(), phy, entry_tendencies(), rdt=1.0 / 450.0)
    check_coupled(got, want)
    assert not np.array_equal(want["pt_dt"], golden("coupled")["pt_dt"])


def distinct_fields(n, nk, offset):
    """Sixteen full arrays of finite values, every element different from its counterpart at another offset."""
    shape = (n + 7, n + 7, nk + 1)
    i, j, k = np.meshgrid(*[np.arange(m) for m in shape], indexing="ij")
    return {name: offset + 16.0 * (i + shape[0] * (j + shape[1] * k)) + m for m, name in enumerate(LAYER_IN)}


def run_copy(lib, device, n, nk):
    from pace_amd.stencils import CopyDycoreToPhysics

    env = mgp.make_env(lib, device, np.ones((n, n)), n, nk, 300.0)
    src = distinct_fields(n, nk, 0.5)
    dycore = types.SimpleNamespace(**{name: env.q3(v) for name, v in src.items()})
    state = mgp.physics_state(env, {}, n, nk)
    CopyDycoreToPhysics(env.stencil_factory, env.qf)(dycore, state)
    mgp.sync(device)
    out = mgp.state_arrays(state)
    inside = np.zeros((n + 7, n + 7, nk + 1), dtype=bool)
    inside[3:3 + n + 1, 3:3 + n + 1, :nk] = True
    for name in LAYER_IN:
        assert np.array_equal(out[name][inside], src[name][inside]), name
        assert np.isnan(out[name][~inside]).all(), (name, "copied outside (n + 1, n + 1, nk)")
        assert np.array_equal(mgp.to_numpy(getattr(dycore, name)), src[name]), name
    for name in out:
        if name not in LAYER_IN:
            assert np.isnan(out[name]).all(), (name, "touched by the copy")


def test_copy_covers_its_domain_and_nothing_else(emu_lib):
    run_copy(emu_lib, "cpu", N, NZ)


def test_refusals_and_checks(emu_lib):
    import torch

    from pace_amd import _lib, stencils
    from pace_amd.stencils import physics_coupling

    assert stencils.CopyDycoreToPhysics is physics_coupling.CopyDycoreToPhysics
    assert stencils.PhysicsToDycore is physics_coupling.PhysicsToDycore
    env = mgp.make_env(emu_lib, "cpu", inputs()["area"], N, NZ, 300.0)
    with pytest.raises(NotImplementedError, match="layout"):
        stencils.PhysicsToDycore(env.stencil_factory, env.qf, mgp.namelist(layout=(2, 2)))
    f32 = _lib.Library(build_emu_f32())
    env32 = mgp.make_env(f32, "cpu", inputs()["area"], N, NZ, 300.0)
    with pytest.raises(NotImplementedError, match="float64"):
        stencils.PhysicsToDycore(env32.stencil_factory, env32.qf, mgp.namelist())
    with pytest.raises(NotImplementedError, match="float64"):
        stencils.CopyDycoreToPhysics(env32.stencil_factory, env32.qf)
    # layout and type
    op = stencils.PhysicsToDycore(env.stencil_factory, env.qf, mgp.namelist())
    copy = stencils.CopyDycoreToPhysics(env.stencil_factory, env.qf)
    wrongs = [torch.zeros((N + 7, N + 7, NZ + 1), dtype=torch.float64), env.q3().data.to(torch.float32), env.q2().data, None]
    for wrong in wrongs:
        dycore = types.SimpleNamespace(**{name: env.q3() for name in LAYER_IN})
        state = mgp.physics_state(env, {}, N, NZ, fill=1.0)
        tend = [env.q3(), env.q3(), env.q3()]
        with pytest.raises(ValueError):
            op(dycore, state, tend[0], wrong, tend[2])
        state.prsi = wrong
        with pytest.raises(ValueError):
            op(dycore, state, *tend)
        dycore.qo3mr = wrong
        with pytest.raises(ValueError):
            copy(dycore, mgp.physics_state(env, {}, N, NZ, fill=1.0))


# ---- on the GPU --------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_coupling_fixture_fed_gpu(lib):
    got = mgp.run_coupling(lib, "cuda:0", inputs(), fixture_physics_side(), entry_tendencies())
    check_coupled(got, golden("coupled"))


def synthetic_tendencies(shape):
    """Tendencies for the forward Euler where no microphysics runs: exact multiples of 2 ** -20, different per field."""
    from pace_amd import synthetic

    return {name: synthetic.microphysics_tendencies(shape, m) * 2.0 ** 20 for m, name in enumerate(TEND)}


def run_kernels_without_microphysics(lib, device, n, nk):
    """Copy, Physics.prepare, Physics.update (on tendencies set in between) and PhysicsToDycore on one set of objects, each
    against tools/physics_np.py to the bit."""
    from pace_amd.physics import Physics
    from pace_amd.stencils import CopyDycoreToPhysics

    inp = mgp.dycore_inputs(n, nk)
    env = mgp.make_env(lib, device, inp["area"], n, nk, 300.0)
    nml = mgp.namelist(n, nk)
    dycore = types.SimpleNamespace(**{name: env.q3(embed(inp[name], n)) for name in LAYER_IN})
    state = mgp.physics_state(env, {"land": inp["land"]}, n, nk)
    CopyDycoreToPhysics(env.stencil_factory, env.qf)(dycore, state)
    physics = Physics(env.stencil_factory, env.qf, env.grid_data, nml, ["microphysics"])
    physics.prepare(state)
    mgp.sync(device)
    pre = mgp.state_arrays(state)
    want, (hi, lo) = mgp.numpy_pre(inp, 300.0)
    for name in PRE:
        assert_same_bits(window(pre[name], name, n, nk), want[name], name)
    for name in TEND:
        assert (window(pre[name], name, n, nk) == 0).all(), name
    tendencies = synthetic_tendencies(inp["pt"].shape)
    for name, v in tendencies.items():
        mgp.set_field(getattr(state.microphysics, name), embed(v, n))
    physics.update(state, DT)
    mgp.sync(device)
    post = mgp.state_arrays(state)
    want.update(tendencies)
    npr.update_physics_state_with_tendencies(want, DT)
    for name in UPDATED:
        assert_same_bits(window(post[name], name, n, nk), want[name], name)
        assert not np.array_equal(want[name], want[dict((o, x) for x, _, o in npr.UPDATED)[name]]), name
    for name, a in post.items():
        if name != "land":
            outside = np.ones(a.shape, dtype=bool)
            outside[3:3 + n, 3:3 + n, :nk + 1 if name in ("prsi", "phii") else nk] = False
            # (the copy's domain is one row and one column wider: it carries the NaN of the dycore's storage there)
            assert np.isnan(a[outside]).all(), name
    entry = mgp.coupling_tendencies(inp["pt"].shape)
    got = mgp.couple(env, nml, dycore, state, entry, n, device)
    phy = {name: window(post[name], name, n, nk) for name in UPDATED + ["ua", "va", "pt", "prsi"]}
    want_coupled = mgp.numpy_coupled(inp, phy, entry)
    for name in COUPLED:
        assert np.isfinite(want_coupled[name]).all(), name
    check_coupled(got, want_coupled, n, nk)
    return int(hi.sum()), int(lo.sum())


def test_kernels_without_microphysics_c20_emulated(emu_lib):
    """C20 x 7 on the emulated library: nk is no multiple of the level chunks (4 and 8), 20 of 64 lanes."""
    run_kernels_without_microphysics(emu_lib, "cpu", 20, 7)


@pytest.mark.gpu
def test_kernels_without_microphysics_c68_gpu(lib):
    """C68 x 7: two blocks per row (blockIdx.x > 0, which C12 and C20 never reach), the second with 4 of 64 lanes (5 in the
    copy); nk = 7 is no multiple of the level chunks (4 in the column sweeps, 8 in the pointwise kernels)."""
    run_copy(lib, "cuda:0", 68, 7)
    run_kernels_without_microphysics(lib, "cuda:0", 68, 7)


@pytest.mark.gpu
def test_chain_c20_gpu(lib, emu_lib):
    """C20 x 79, Copy -> Physics -> PhysicsToDycore on one set of objects: every output finite, `pre` equal to numpy to the bit,
    the coupling equal to numpy applied to the operator's own physics output, the tendencies and wmp within the `Microph`
    bound of the emulated library's, the forward Euler exact."""
    n, nk = 20, NZ
    inp = mgp.dycore_inputs(n, nk)
    pre, post, coupled = mgp.run_operators(lib, "cuda:0", inp, 300.0, n, nk)
    want, _ = mgp.numpy_pre(inp, 300.0)
    for name in PRE:
        assert_same_bits(window(pre[name], name, n, nk), want[name], name)
    for name in TEND + ["wmp"] + UPDATED:
        assert np.isfinite(window(post[name], name, n, nk)).all(), name
    for x, x_dt, out in npr.UPDATED:
        w = lambda name: window(post[name], name, n, nk)  # noqa: E731
        assert_same_bits(w(out), w(x) + w(x_dt) * DT, out)
    phy = {name: window(post[name], name, n, nk) for name in UPDATED + ["ua", "va", "pt", "prsi"]}
    want_coupled = mgp.numpy_coupled(inp, phy, mgp.coupling_tendencies(inp["pt"].shape))
    for name in COUPLED:
        assert np.isfinite(want_coupled[name]).all(), name
    check_coupled(coupled, want_coupled, n, nk)
    _, emu_post, _ = mgp.run_operators(emu_lib, "cpu", inp, 300.0, n, nk)
    errs = mgp.tendency_errors({name: window(emu_post[name], name, n, nk) for name in TEND + ["wmp"]}, post, n, nk)
    print("device against emulation, C20", " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    for name, e in errs.items():
        assert e <= MAX_ERROR, (name, e)
    assert np.count_nonzero(window(post["qi_dt"], "qi_dt", n, nk)) > 10000
