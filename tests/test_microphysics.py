"""The GFDL cloud microphysics (pace_amd.physics.Microphysics, k_microphys.hip) against runs of the reference
(tools/make_golden_microphysics.py): the emulated library on the CPU, the gfx950 library with -m gpu.

Bound: the reference's comparison, 2|a - b| / (|a| + |b|), against the reference's own `Microph` device line
(physics/tests/savepoint/translate/overrides/standard.yaml): max_error 2.2e-8; near-zero ql_dt 1e-8, qr_dt 1e-9, udt / vdt 1e-8,
everything else (qg_dt, the precipitation and wmp included) 1e-18.  The same bound for the emulated library and the device.
The generator holds the reference against itself, inputs perturbed by 1e-15, to a quarter of it (cond_* in the fixtures).
State fields the reference leaves alone have to keep their bits.

Measured (worst over the five cases; every test prints its own): the emulated library udt 1.8e-11, vdt 5.2e-11, the species'
tendencies <= 5e-13, pt_dt 1.3e-12, wmp 1.9e-15, precipitation 7.8e-15; the MI355X udt 1.2e-10, vdt 5.2e-11, qg_dt 2.3e-11,
qi_dt 4.6e-12, the other species <= 5.8e-13, pt_dt 1.8e-12, wmp 2.3e-15, precipitation 7.3e-14; the device against the emulated
library at C20 x 79 udt 1.4e-11.  The bound stays the reference's.  The workspace tests (NaN on entry, reuse across cases) are bit
identity against a fresh operator and hold on the emulated library and on the MI355X for every case."""
import ctypes as C
import dataclasses
import os
import re
import sys
import types

import numpy as np
import pytest

from helpers import ROOT, Env, build_emu, build_emu_f32, compare, minimal_metrics

sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_microphysics import CASES, COVERAGE, MAX_ERROR, NEAR_ZERO, OUT, PRECIP, STATE3, TEND, load_split  # noqa: E402

N, NZ = 12, 79
TAGS = list(CASES)
CONDENSATES = ["qliquid", "qrain", "qice", "qsnow", "qgraupel"]


@pytest.fixture(scope="module")
def emu_lib():
    from pace_amd import _lib

    return _lib.Library(build_emu())


@pytest.fixture(scope="module")
def lib():
    from pace_amd import _lib

    return _lib.load()


_cache = {}


def fixture_inputs():
    if "in" not in _cache:
        _cache["in"] = {k[3:]: v for k, v in load_split("microphysics_c12_in").items()}
    return _cache["in"]


def case(tag):
    if tag not in _cache:
        _cache[tag] = load_split(f"microphysics_c12_{tag}")
    return _cache[tag]


def case_inputs(tag):
    """The state, the tendencies and area at entry as the generator had them: the stored ones; `dry` without condensate;
    `accum` with the tendencies of pace_amd.synthetic.microphysics_tendencies (exact in any arithmetic)."""
    from pace_amd import synthetic

    inp = dict(fixture_inputs())
    shape = inp["pt"].shape
    if CASES[tag]["dry"]:
        for name in CONDENSATES + ["qcld"]:
            inp[name] = np.zeros(shape)
        inp["delprsi"] = inp["delp"].copy()
    for m, name in enumerate(TEND):
        inp[name] = synthetic.microphysics_tendencies(shape, m) if CASES[tag]["accum"] else np.zeros(shape)
    return inp


def embed(a, n, fill=np.nan):
    nk = a.shape[2] if a.ndim == 3 else 0
    full = np.full((n + 7, n + 7, nk + 1) if a.ndim == 3 else (n + 7, n + 7), fill)
    if a.ndim == 3:
        full[3:3 + n, 3:3 + n, :nk] = a
    else:
        full[3:3 + n, 3:3 + n] = a
    return full


def make_env(lib, device, area, n, nk):
    return Env(lib, device, minimal_metrics(n, embed(area, n, 1.0)), n, nk)


def namelist(mp_time=225.0, **kw):
    from pace_amd.physics import PhysicsConfig

    values = dict(dt_atmos=225, hydrostatic=False, npx=N + 1, npy=N + 1, npz=NZ, nwat=6, do_qa=True, mp_time=mp_time)
    values.update(kw)
    return PhysicsConfig(**values)


def make_state(env, inp, n, tensors=False):
    """A MicrophysicsState on NaN-filled storage (whatever is read outside the compute domain shows), the tendencies set."""
    from pace_amd.physics import MicrophysicsState

    q = {name: env.q3(embed(inp[name], n)) for name in STATE3}
    land = env.q2(embed(inp["land"], n))
    tendency = env.q3()
    pick = (lambda f: f.data) if tensors else (lambda f: f)
    state = MicrophysicsState(*[pick(q[name]) for name in STATE3[:13]], pick(q["delprsi"]), pick(q["wmp"]), pick(q["dz"]),
                              pick(tendency), pick(land))
    for name in TEND:
        f = getattr(state, name)
        full = embed(inp[name], n)
        if tensors:
            import torch

            f.copy_(torch.as_tensor(full, dtype=f.dtype).to(f.device))
        else:
            f.set(full)
    return state


def to_numpy(f):
    return f.numpy() if hasattr(f, "dims") else f.detach().cpu().numpy()


def run(lib, device, inp, timesteps, mp_time=225.0, tensors=False, op=None, n=N, nk=NZ):
    """Microphysics on `inp`, once per entry of `timesteps` on one object; returns (every field after the calls as full arrays,
    the operator)."""
    from pace_amd.physics import Microphysics

    env = make_env(lib, device, inp["area"], n, nk)
    if op is None:
        op = Microphysics(env.stencil_factory, env.qf, env.grid_data, namelist(mp_time))
    state = make_state(env, inp, n, tensors)
    for timestep in timesteps:
        op(state, timestep)
    if device != "cpu":
        import torch

        torch.cuda.synchronize()
    out = {name: to_numpy(getattr(state, name)) for name in STATE3 + TEND + ["land"]}
    for name in PRECIP:
        out[name] = getattr(op, "_" + name).numpy()
    return out, op


def window(out, name, n=N, nk=NZ):
    if name in PRECIP:
        return out[name][3:3 + n, 3:3 + n, 0]
    return out[name][3:3 + n, 3:3 + n, :nk]


def check_against_reference(tag, out, inp, what, n=N, gather=None):
    """gather: what takes the fixture's C12 window to the n x n one the operator ran on (tests/columns.py), none at C12."""
    d = case(tag)
    worst = {}
    for name in OUT:
        ref = d["out_" + name] if gather is None else gather(d["out_" + name])
        worst[name] = compare(ref, window(out, name, n), near_zero=NEAR_ZERO.get(name, 1e-18))
    print(what, tag, " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for name, e in worst.items():
        assert e <= MAX_ERROR, (tag, name, e)
    check_untouched(out, inp, n)


def check_untouched(out, inp, n=N, nk=NZ):
    """The state fields the reference leaves alone keep their bits; nothing outside the compute domain is written (wmp and
    the tendencies were NaN there), and the precipitation holds the column's value on every level."""
    for name in STATE3 + ["land"]:
        if name != "wmp":
            assert np.array_equal(out[name], embed(inp[name], n), equal_nan=True), (name, "changed")
    outside = np.ones((n + 7, n + 7, nk + 1), dtype=bool)
    outside[3:3 + n, 3:3 + n, :nk] = False
    for name in TEND + ["wmp"]:
        assert np.isnan(out[name][outside]).all(), (name, "written outside the compute domain")
    for name in PRECIP:
        f = out[name][3:3 + n, 3:3 + n, :nk]
        assert (f == f[:, :, :1]).all(), name


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- the fixture itself --------------------------------------------------------------------------------------------------

def test_fixture_coverage():
    """Every branch count tools/make_golden_microphysics.py took on case base is above zero, the reference against its own
    perturbed run stayed within a quarter of the bound for every compared variable of every case, and the cases are what the
    tests take them for."""
    d = case("base")
    cov = {k[4:]: int(v) for k, v in d.items() if k.startswith("cov_")}
    assert sorted(cov) == sorted(COVERAGE)
    for name, count in cov.items():
        assert count > 0, name
    for tag in TAGS:
        c = case(tag)
        for name in OUT:
            assert float(c["cond_" + name]) <= MAX_ERROR / 4, (tag, name)
            assert np.isfinite(c["out_" + name]).all(), (tag, name)
    assert float(case("sub2")["timestep"]) == 2 * float(case("sub2")["mp_time"]) == 450.0
    assert float(case("mptime")["timestep"]) == 2 * float(case("mptime")["mp_time"]) == 225.0
    inp = fixture_inputs()
    assert set(np.unique(inp["land"])) == {0.0, 0.4, 1.0} and (inp["omga"] != 0).any()
    assert all((inp[name] < 0).any() for name in CONDENSATES + ["qvapor"])
    # columns without one species each (the no_fall paths of case base), and every tendency of the dry case's falls is none
    for name in CONDENSATES[1:]:
        col_max = np.abs(inp[name]).max(axis=2)
        assert (col_max == 0).any() and (col_max > 0).any(), name
    for name in PRECIP:
        assert (case("dry")["out_" + name] == 0).all() and (d["out_" + name] > 0).any(), name
    for name in TEND:
        if name != "qa_dt":
            assert np.count_nonzero(d["out_" + name]) > 1000, name


# ---- the emulated library --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", TAGS)
def test_microphysics_emulated(emu_lib, tag):
    inp = case_inputs(tag)
    out, _ = run(emu_lib, "cpu", inp, [CASES[tag]["timestep"]], CASES[tag]["mp_time"])
    check_against_reference(tag, out, inp, "emulated")


def test_two_calls_with_different_timesteps_equal_fresh_objects(emu_lib):
    """_update_timestep_if_needed: 225 s then 450 s on one object (the second call on the first one's tendencies and wmp) gives
    the bits of two fresh objects doing the same, and the factors follow the reference's _set_timestep."""
    from pace_amd.physics import Microphysics

    inp = case_inputs("base")
    both, op = run(emu_lib, "cpu", inp, [225.0, 450.0])
    assert (op._ntimes, op._dts, op._timestep, op._cfg.ntimes, op._cfg.dts) == (2, 225.0, 450.0, 2, 225.0)
    assert op._fac_imlt == 1.0 - np.exp(-0.5 * 225.0 / 600.0) == op._cfg.fac_imlt
    first, _ = run(emu_lib, "cpu", inp, [225.0])
    again = dict(inp)
    for name in TEND + ["wmp"]:
        again[name] = window(first, name)
    env = make_env(emu_lib, "cpu", inp["area"], N, NZ)
    fresh = Microphysics(env.stencil_factory, env.qf, env.grid_data, namelist())
    second, _ = run(emu_lib, "cpu", again, [450.0], op=fresh)
    for name in TEND + ["wmp"] + PRECIP:
        assert np.array_equal(bits(window(both, name)), bits(window(second, name))), name
    # ... and it is what the reference's run with 450 s gives from zero tendencies, where the first call had none to add
    assert not np.array_equal(window(both, "qv_dt"), window(first, "qv_dt"))


def test_tendencies_are_accumulated(emu_lib):
    """accum: what is passed in stays in; the result is the entry value plus case base's tendency to the bit (qa_dt is set
    to zero, udt and vdt keep level 0)."""
    inp = case_inputs("accum")
    out, _ = run(emu_lib, "cpu", inp, [225.0])
    base, _ = run(emu_lib, "cpu", case_inputs("base"), [225.0])
    for name in TEND:
        got, add = window(out, name), window(base, name)
        want = np.zeros_like(got) if name == "qa_dt" else inp[name] + add
        assert np.array_equal(bits(got), bits(want)), name
    assert np.array_equal(window(out, "udt")[:, :, 0], inp["udt"][:, :, 0]) and (inp["udt"][:, :, 0] != 0).any()
    assert np.array_equal(bits(window(out, "wmp")), bits(window(base, "wmp")))


def test_quantities_and_tensors_give_the_same(emu_lib):
    inp = case_inputs("base")
    out_q, _ = run(emu_lib, "cpu", inp, [225.0])
    out_t, _ = run(emu_lib, "cpu", inp, [225.0], tensors=True)
    for name in out_q:
        assert np.array_equal(out_q[name], out_t[name], equal_nan=True), name


def test_state_copies_the_tendency(emu_lib):
    env = make_env(emu_lib, "cpu", fixture_inputs()["area"], N, NZ)
    state = make_state(env, case_inputs("base"), N)
    ptrs = {getattr(state, name).data.data_ptr() for name in TEND}
    assert len(ptrs) == len(TEND)


# ---- the workspace between calls -----------------------------------------------------------------------------------------------
# The sixteen work arrays live in one workspace the operator allocates once (zeros) and hands to every call.  A work array the
# kernel read before its first write of that call would see zeros in a fresh operator and the previous step's values in a model
# run.  So: the workspace poisoned with NaN, and the workspace as another case left it, both against a fresh operator, bit for bit
# on the whole storage of every field.

def run_copied(lib, device, inp, tag, op=None, poison=False):
    """run() on case `tag`'s timestep, the arrays copied (on the CPU they are views, the precipitation's of the operator's own
    storage, which the next call writes); poison: the operator's workspace filled with NaN before the call."""
    from pace_amd.physics import Microphysics

    if poison:
        env = make_env(lib, device, inp["area"], N, NZ)
        op = Microphysics(env.stencil_factory, env.qf, env.grid_data, namelist(CASES[tag]["mp_time"]))
        op._workspace.fill_(float("nan"))
    out, op = run(lib, device, inp, [CASES[tag]["timestep"]], CASES[tag]["mp_time"], op=op)
    return {name: np.array(a) for name, a in out.items()}, op


def assert_same_storage(got, want, what):
    assert sorted(got) == sorted(want)
    for name in got:
        differ = bits(got[name]) != bits(want[name])
        assert not differ.any(), (what, name, int(differ.sum()), "values differ; first at", tuple(np.argwhere(differ)[0]))


def check_poisoned_workspace(lib, device, tag):
    inp = case_inputs(tag)
    fresh, _ = run_copied(lib, device, inp, tag)
    poisoned, op = run_copied(lib, device, inp, tag, poison=True)
    assert_same_storage(poisoned, fresh, f"{tag}, workspace NaN on entry")
    for name in OUT:
        assert np.isfinite(window(poisoned, name)).all(), (tag, name)
    return op


def check_reuse_across_cases(lib, device, first, second):
    """`first` then `second` on one operator: the second call gives what a fresh operator gives on the same inputs."""
    _, op = run_copied(lib, device, case_inputs(first), first)
    assert float(op._workspace.abs().max()) > 0  # (the first call left something behind)
    inp = case_inputs(second)
    reused, _ = run_copied(lib, device, inp, second, op=op)
    fresh, _ = run_copied(lib, device, inp, second)
    assert_same_storage(reused, fresh, f"{second} after {first} on one operator")


@pytest.mark.parametrize("tag", TAGS)
def test_nan_in_the_workspace_changes_nothing_emulated(emu_lib, tag):
    check_poisoned_workspace(emu_lib, "cpu", tag)


@pytest.mark.parametrize("first,second", [("base", "dry"), ("dry", "base")])
def test_workspace_reused_across_cases_emulated(emu_lib, first, second):
    """dry skips every fall path: what base left in the work arrays of the falls is still there to be read."""
    check_reuse_across_cases(emu_lib, "cpu", first, second)


# ---- the host layer ----------------------------------------------------------------------------------------------------------

def test_exported_names_and_config():
    import pace_amd.physics as physics
    import pace_amd.physics.stencils.microphysics as module

    assert physics.Microphysics is module.Microphysics and physics.MicrophysicsState is module.MicrophysicsState
    cfg = physics.PhysicsConfig()
    assert (cfg.mp_time, cfg.tice, cfg.c_paut, cfg.ccn_l, cfg.ccn_o, cfg.tau_imlt, cfg.rthresh) == (225.0, 273.16, 0.5, 300.0, 100.0, 600.0,
                                                                                                     1e-05)
    assert (cfg.do_qa, cfg.do_sedi_w, cfg.use_ppm, cfg.irain_f, cfg.layout) == (False, True, False, 0, (1, 1))
    nml = types.SimpleNamespace(dt_atmos=450, npz=63, vi_max=0.5)
    got = physics.PhysicsConfig.from_namelist(nml)
    assert (got.dt_atmos, got.npz, got.vi_max, got.do_qa, got.vr_max) == (450, 63, 0.5, True, 16.0)
    assert {f.name for f in dataclasses.fields(cfg)} >= set(module.REQUIRED_SWITCHES)


def test_header_and_binding_agree_on_the_entry_points():
    from pace_amd import _lib

    text = open(os.path.join(ROOT, "include", "pace_hip.h")).read()
    for name in ("pace_microphysics_workspace_bytes", "pace_microphysics"):
        assert re.search(rf"\b{name}\s*\(", text) and name in _lib.EXPORTED_SYMBOLS
    body = re.search(r"typedef struct \{([^}]*)\} pace_microphysics_config_t;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for kind, names in re.findall(r"\b(int32_t|double)\s+([^;]+);", body):
        for item in names.split(","):
            name, dims = re.match(r"\s*(\w+)((?:\[\d+\])*)", item).groups()
            fields.append((name, kind, int(np.prod([int(x) for x in re.findall(r"\d+", dims)] or [1]))))
    bound = [(name, "int32_t" if t is C.c_int32 else "double", C.sizeof(t) // (4 if t is C.c_int32 else 8))
             for name, t in _lib.MicrophysicsConfig._fields_]
    assert fields == bound
    assert C.sizeof(_lib.MicrophysicsConfig) == 8 + 8 * sum(count for _, kind, count in fields if kind == "double")
    assert int(re.search(r"#define PACE_MICROPHYSICS_INPUTS (\d+)", text).group(1)) == len(_lib.MICROPHYSICS_INPUTS)
    assert int(re.search(r"#define PACE_MICROPHYSICS_TENDENCIES (\d+)", text).group(1)) == len(_lib.MICROPHYSICS_TENDENCIES)
    assert list(_lib.MICROPHYSICS_TENDENCIES) == TEND


def test_other_switch_values_are_refused(emu_lib):
    from pace_amd.physics import Microphysics
    from pace_amd.physics.stencils.microphysics import REQUIRED_SWITCHES

    env = make_env(emu_lib, "cpu", fixture_inputs()["area"], N, NZ)
    assert len(REQUIRED_SWITCHES) == 18
    for name, value in REQUIRED_SWITCHES.items():
        other = 1 if name == "irain_f" else (not value)
        with pytest.raises(NotImplementedError, match=name):
            Microphysics(env.stencil_factory, env.qf, env.grid_data, namelist(**{name: other}))
    nml = namelist()
    nml.hydrostatic = True
    with pytest.raises(NotImplementedError, match="hydrostatic"):
        Microphysics(env.stencil_factory, env.qf, env.grid_data, nml)
    with pytest.raises(NotImplementedError, match="layout"):
        Microphysics(env.stencil_factory, env.qf, env.grid_data, namelist(layout=(2, 2)))
    Microphysics(env.stencil_factory, env.qf, env.grid_data, namelist(vi_max=0.5, tau_imlt=300.0, ccn_l=270.0))  # any number


def test_float32_library_is_refused():
    """QCMIN = 1e-12 and QVMIN = 1e-20 are no float32 quantities: the constructor refuses the float32 build, and so does the
    entry point (the library still builds and links with the kernel in it)."""
    from pace_amd import _lib
    from pace_amd.physics import Microphysics

    f32 = _lib.Library(build_emu_f32())
    env = make_env(f32, "cpu", fixture_inputs()["area"], N, NZ)
    with pytest.raises(NotImplementedError, match="float64"):
        Microphysics(env.stencil_factory, env.qf, env.grid_data, namelist())
    cfg = _lib.MicrophysicsConfig()
    cfg.struct_bytes, cfg.ntimes, cfg.timestep, cfg.dts = C.sizeof(cfg), 1, 225.0, 225.0
    q = env.q3()
    ptrs = lambda count: (C.c_void_p * count)(*[q.data.data_ptr()] * count)  # noqa: E731
    from pace_amd.util.grid import geom_struct

    with pytest.raises(_lib.PaceError, match="unsupported"):
        f32.call("pace_microphysics", C.byref(geom_struct(env.qf)), q.data.data_ptr(), C.byref(cfg), ptrs(13), q.data.data_ptr(),
                 ptrs(10), ptrs(4), None)


def test_struct_bytes_mismatch_is_refused(emu_lib):
    inp = case_inputs("base")
    _, op = run(emu_lib, "cpu", inp, [225.0])
    env = make_env(emu_lib, "cpu", inp["area"], N, NZ)
    state = make_state(env, inp, N)
    op._cfg.struct_bytes -= 8
    from pace_amd import _lib

    with pytest.raises(_lib.PaceError, match="invalid argument"):
        op(state, 225.0)


def test_layout_and_type_are_checked(emu_lib):
    import torch

    from pace_amd.physics import Microphysics

    inp = case_inputs("base")
    env = make_env(emu_lib, "cpu", inp["area"], N, NZ)
    op = Microphysics(env.stencil_factory, env.qf, env.grid_data, namelist())
    for bad in ("pt", "delprsi", "wmp", "qr_dt", "land"):
        wrongs = [torch.zeros((N + 7, N + 7, NZ + 1), dtype=torch.float64), env.q3().data.to(torch.float32)]
        if bad == "land":
            wrongs = [torch.zeros((N + 7, N + 7), dtype=torch.float64), env.q3().data]
        for wrong in wrongs:
            state = make_state(env, inp, N)
            setattr(state, bad, wrong)
            with pytest.raises(ValueError):
                op(state, 225.0)


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_microphysics_gpu(lib, tag):
    """Every case on the device against the reference's run: C12 x 79 is 144 columns, twelve partial waves; sub2 and mptime
    run two sub-steps."""
    inp = case_inputs(tag)
    out, op = run(lib, "cuda:0", inp, [CASES[tag]["timestep"]], CASES[tag]["mp_time"])
    assert op._ntimes == (2 if tag in ("sub2", "mptime") else 1)
    check_against_reference(tag, out, inp, "device")


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_nan_in_the_workspace_changes_nothing_gpu(lib, tag):
    check_poisoned_workspace(lib, "cuda:0", tag)


@pytest.mark.gpu
@pytest.mark.parametrize("first,second", [("base", "dry"), ("dry", "base")])
def test_workspace_reused_across_cases_gpu(lib, first, second):
    check_reuse_across_cases(lib, "cuda:0", first, second)


@pytest.mark.gpu
def test_microphysics_c20_device_against_emulation_gpu(lib, emu_lib):
    """C20 x 79, 400 columns (a multiple of neither 64 nor 256), pace_amd.synthetic's columns and fill, the tendencies non-zero on
    entry: the device against the emulated library within the bound, every output finite, the untouched fields bit-identical.
    (Two sub-steps on the device: sub2 and mptime above.)  The inputs meet the fixtures' condition: the emulated library against
    itself on inputs perturbed by 1e-15 (four draws) stays at or below 3.0e-9 (udt) for every variable, a seventh of the bound."""
    from pace_amd import synthetic

    n = 20
    pt, delp, delz = synthetic.microphysics_columns(n, NZ)
    inp = synthetic.microphysics_state(pt, delp, delz)
    for m, name in enumerate(TEND):
        inp[name] = synthetic.microphysics_tendencies(pt.shape, m)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    inp["area"] = 2.0e10 * (1.0 + 0.3 * np.sin(0.3 * i + 0.2 * j))
    dev, _ = run(lib, "cuda:0", inp, [225.0], n=n)
    emu, _ = run(emu_lib, "cpu", inp, [225.0], n=n)
    worst = {}
    for name in OUT:
        a, b = window(emu, name, n), window(dev, name, n)
        assert np.isfinite(b).all(), name
        worst[name] = compare(a, b, near_zero=NEAR_ZERO.get(name, 1e-18))
    print("device against emulation, C20", " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for name, e in worst.items():
        assert e <= MAX_ERROR, (name, e)
    check_untouched(dev, inp, n)
    assert np.count_nonzero(window(dev, "rain", n)) > 300 and np.count_nonzero(window(dev, "qi_dt", n)) > 10000
