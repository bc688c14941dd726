"""The Physics shell (pace_amd.physics.Physics / PhysicsState, k_physics.hip) against a run of the reference
(tools/make_golden_physics.py: tile 0 of C12 x 79) and, where no fixture exists, against tools/physics_np.py, which a test here
holds to the fixture bit for bit.  The emulated library on the CPU, the gfx950 library with -m gpu.

Bounds.  BIT IDENTITY for everything without a transcendental: the fields as they are before the microphysics (`pre`) and the
forward Euler, physics_updated_x == x + x_dt * dt evaluated in numpy on the operator's own x and x_dt.  The ten tendencies and
wmp after the call: the reference's `Microph` line of tests/test_microphysics.py (MAX_ERROR, NEAR_ZERO, imported).  The
physics_updated_* fields are not compared with the fixture in the relative metric: species that q + q_dt * dt nearly removes
cancel, and the reference against itself on inputs perturbed by 1e-15 is 8e-7 apart there; bit-exact inputs, tendencies at
their bound and a bit-exact forward Euler pin the same thing without the cancellation.

Measured (every test prints its own): tendencies and wmp against the fixture, the emulated library at most 2.3e-11 (vdt), the
MI355X at most 2.3e-11 (vdt; qg_dt 9.7e-13, wmp 2.3e-13); everything else is equal to the bit on both."""
import ctypes as C
import dataclasses
import os
import re
import sys

import numpy as np
import pytest

from helpers import ROOT, build_emu, build_emu_f32

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_physics as mgp  # noqa: E402
import physics_np as npr  # noqa: E402
from make_golden_microphysics import MAX_ERROR, TEND, load_split  # noqa: E402
from make_golden_physics import N, NZ, DT, PRE, UPDATED, bits, embed, window  # noqa: E402


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


def ptop():
    return float(golden("pre")["ptop"])


def emulated_parts(emu_lib):
    """Copy, prepare, the microphysics, update on the emulated library, once for the tests that look at it."""
    if "emulated" not in _cache:
        _cache["emulated"] = mgp.run_operators(emu_lib, "cpu", inputs(), ptop())
    return _cache["emulated"]


def assert_same_bits(got, want, what):
    assert got.shape == want.shape, what
    diff = bits(got) != bits(want)
    assert not diff.any(), (what, int(diff.sum()), "values differ; first at", tuple(np.argwhere(diff)[0]))


def check_pre(pre_full, names=PRE, n=N, nk=NZ, want=None):
    want = golden("pre") if want is None else want
    for name in names:
        assert_same_bits(window(pre_full[name], name, n, nk), want[name], name)


def check_tendencies(post_full, ref, what, n=N, nk=NZ):
    errs = mgp.tendency_errors(ref, post_full, n, nk)
    print(what, " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    for name, e in errs.items():
        assert e <= MAX_ERROR, (name, e)


def check_euler(post_full, n=N, nk=NZ, dt=DT):
    for x, x_dt, out in npr.UPDATED:
        w = lambda name: window(post_full[name], name, n, nk)  # noqa: E731
        assert_same_bits(w(out), w(x) + w(x_dt) * dt, out)


def check_nothing_outside(full, n=N, nk=NZ, skip=()):
    """Storage was NaN outside the compute domain and on level nk of the layer fields: it still is; prsik is not touched."""
    for name, a in full.items():
        if name == "land" or name in skip:
            continue
        outside = np.ones(a.shape, dtype=bool)
        outside[3:3 + n, 3:3 + n, :nk + 1 if name in ("prsi", "phii") else nk] = False
        if name == "prsik":
            outside[...] = True
        assert np.isnan(a[outside]).all(), (name, "written outside its domain")


# ---- the fixture and the restatement ---------------------------------------------------------------------------------------

def test_fixture_meets_the_generators_conditions():
    pre, post = golden("pre"), golden("post")
    for part in ("pre", "post", "coupled"):
        for name, v in golden(part).items():
            assert np.isfinite(v).all(), (part, name)
    s, (hi, lo) = mgp.numpy_pre(inputs(), ptop())
    assert hi.sum() > 100 and lo.sum() > 100
    assert (pre["qvapor"] < 0).sum() > 100 and (pre["qvapor"] < 1e-10).any()
    assert (post["physics_updated_specific_humidity"] < 1e-9).any()
    assert pre["prsi"].shape == pre["phii"].shape == (N, N, NZ + 1) and pre["delp"].shape == (N, N, NZ)
    assert (pre["prsi"][:, :, 0] == ptop()).all() and (pre["phii"][:, :, NZ] == 0).all()


def test_numpy_restatement_equals_the_reference():
    """tools/physics_np.py against the run of the reference, bit for bit: every field before the microphysics, and the forward
    Euler on the reference's own tendencies."""
    s, _ = mgp.numpy_pre(inputs(), ptop())
    pre, post = golden("pre"), golden("post")
    for name in PRE:
        assert_same_bits(s[name], pre[name], name)
    for name in TEND:
        assert (s[name] == 0).all()
        s[name] = post[name]
    npr.update_physics_state_with_tendencies(s, DT)
    for name in UPDATED:
        assert_same_bits(s[name], post[name], name)


# ---- the emulated library ----------------------------------------------------------------------------------------------------

def test_prepare_bits_emulated(emu_lib):
    pre, _, _ = emulated_parts(emu_lib)
    check_pre(pre)
    for name in TEND:
        assert (window(pre[name], name, N, NZ) == 0).all(), name
    check_nothing_outside(pre)
    assert np.array_equal(pre["land"], embed(inputs()["land"], N), equal_nan=True)


def test_tendencies_and_forward_euler_emulated(emu_lib):
    _, post, _ = emulated_parts(emu_lib)
    check_tendencies(post, golden("post"), "emulated")
    check_euler(post)
    check_nothing_outside(post)
    check_pre(post, [name for name in PRE if name != "wmp"])


def test_whole_call_equals_its_parts_emulated(emu_lib):
    """Physics.__call__ is prepare, the microphysics, update: the same bits as the three run one by one."""
    _, parts, _ = emulated_parts(emu_lib)
    _, whole, _ = mgp.run_operators(emu_lib, "cpu", inputs(), ptop(), whole=True)
    for name in parts:
        assert np.array_equal(bits(parts[name]), bits(whole[name])), name


def run_prepare(lib, device, inp, top, packages, n=N, nk=NZ, tensors=False, state_packages=("microphysics",)):
    """Physics(active_packages=packages) up to the microphysics on a state that holds `inp` (no copy kernel); returns the full
    arrays."""
    from pace_amd.physics import Physics

    env = mgp.make_env(lib, device, inp["area"], n, nk, top)
    state = mgp.physics_state(env, inp, n, nk, packages=state_packages, tensors=tensors)
    op = Physics(env.stencil_factory, env.qf, env.grid_data, mgp.namelist(n, nk), list(packages))
    if packages:
        op.prepare(state)
    else:
        op(state, DT)  # without packages the whole call is the statein part
    mgp.sync(device)
    return mgp.state_arrays(state)


def test_without_packages_only_the_statein_runs(emu_lib):
    """active_packages = []: the same `pre` bits, and dz, wmp, the tendencies and physics_updated_* keep their NaN."""
    inp = inputs()
    out = run_prepare(emu_lib, "cpu", inp, ptop(), [])
    check_pre(out, [name for name in PRE if name not in ("dz", "wmp")])
    for name in ["dz", "wmp"] + TEND + UPDATED:
        assert np.isnan(out[name]).all(), name
    check_nothing_outside(out)
    # ... and a state without a microphysics part does as well
    again = run_prepare(emu_lib, "cpu", inp, ptop(), [], state_packages=())
    for name in again:
        assert np.array_equal(bits(again[name]), bits(out[name])), name


def test_quantities_and_tensors_give_the_same_bits(emu_lib):
    a = run_prepare(emu_lib, "cpu", inputs(), ptop(), ["microphysics"])
    b = run_prepare(emu_lib, "cpu", inputs(), ptop(), ["microphysics"], tensors=True)
    for name in a:
        assert np.array_equal(bits(a[name]), bits(b[name])), name
    check_pre(b)


# ---- the host layer ------------------------------------------------------------------------------------------------------------

REFERENCE_FIELDS = {  # the reference's PhysicsState, in its order: name -> (metadata name, units)
    "qvapor": ("specific_humidity", "kg/kg"), "qliquid": ("cloud_water_mixing_ratio", "kg/kg"),
    "qice": ("cloud_ice_mixing_ratio", "kg/kg"), "qrain": ("rain_mixing_ratio", "kg/kg"), "qsnow": ("snow_mixing_ratio", "kg/kg"),
    "qgraupel": ("graupel_mixing_ratio", "kg/kg"), "qo3mr": ("ozone_mixing_ratio", "kg/kg"),
    "qsgs_tke": ("turbulent_kinetic_energy", "m**2/s**2"), "qcld": ("cloud_fraction", ""), "pt": ("air_temperature", "degK"),
    "delp": ("pressure_thickness_of_atmospheric_layer", "Pa"), "delz": ("vertical_thickness_of_atmospheric_layer", "m"),
    "ua": ("eastward_wind", "m/s"), "va": ("northward_wind", "m/s"), "w": ("vertical_wind", "m/s"),
    "omga": ("vertical_pressure_velocity", "Pa/s"),
    "physics_updated_specific_humidity": ("physics_updated_specific_humidity", "kg/kg"),
    "physics_updated_qliquid": ("physics_updated_liquid_water_mixing_ratio", "kg/kg"),
    "physics_updated_qice": ("physics_updated_ice_water_mixing_ratio", "kg/kg"),
    "physics_updated_qrain": ("physics_updated_rain_water_mixing_ratio", "kg/kg"),
    "physics_updated_qsnow": ("physics_updated_snow_mixing_ratio", "kg/kg"),
    "physics_updated_qgraupel": ("physics_updated_graupel_mixing_ratio", "kg/kg"),
    "physics_updated_cloud_fraction": ("physics_cloud_fraction", ""), "physics_updated_pt": ("physics_air_temperature", "degK"),
    "physics_updated_ua": ("physics_eastward_wind", "m/s"), "physics_updated_va": ("physics_northward_wind", "m/s"),
    "delprsi": ("model_level_pressure_thickness_in_physics", "Pa"), "phii": ("interface_geopotential_height", "m"),
    "phil": ("layer_geopotential_height", "m"), "dz": ("geopotential_height_thickness", "m"),
    "wmp": ("layer_mean_vertical_velocity_microph", "m/s"), "prsi": ("interface_pressure", "Pa"),
    "prsik": ("log_interface_pressure", "Pa"), "land": ("land_mask", "-"),
}


def test_physics_state_init_zeros(emu_lib):
    import pace_amd.physics as physics
    from pace_amd.physics.physics_state import PhysicsState
    from pace_amd.physics.stencils.physics import Physics
    from pace_amd.util import constants

    assert physics.PhysicsState is PhysicsState and physics.Physics is Physics
    env = mgp.make_env(emu_lib, "cpu", inputs()["area"], N, NZ, 300.0)
    state = PhysicsState.init_zeros(env.qf, ["microphysics"])
    declared = [f for f in dataclasses.fields(PhysicsState)]
    assert [f.name for f in declared] == list(REFERENCE_FIELDS)
    for f in declared:
        name, units = REFERENCE_FIELDS[f.name]
        dims = [constants.X_DIM, constants.Y_DIM]
        if f.name != "land":
            dims.append(constants.Z_INTERFACE_DIM if f.name in ("phii", "prsi", "prsik") else constants.Z_DIM)
        assert (f.metadata["name"], f.metadata["units"], f.metadata["dims"]) == (name, units, dims), f.name
        storage = getattr(state, f.name)
        assert tuple(storage.shape) == ((N + 7, N + 7) if f.name == "land" else (N + 7, N + 7, NZ + 1)) and not storage.any()
    mp = state.microphysics
    for name in ("pt", "qvapor", "qliquid", "qrain", "qice", "qsnow", "qgraupel", "qcld", "ua", "va", "delp", "delz", "omga",
                 "delprsi", "wmp", "dz", "land"):
        assert getattr(mp, name) is getattr(state, name), name
    ptrs = {getattr(mp, name).data.data_ptr() for name in TEND}
    assert len(ptrs) == len(TEND)
    assert PhysicsState.init_zeros(env.qf, []).microphysics is None
    assert not hasattr(PhysicsState, "xr_dataset")
    # init_from_storages: Quantity objects over the given storages
    storages = {f.name: getattr(state, f.name) for f in declared}
    other = PhysicsState.init_from_storages(storages, env.sizer, env.qf, ["microphysics"])
    assert other.phii.extent == (N, N, NZ + 1) and other.pt.extent == (N, N, NZ) and other.pt.origin == (3, 3, 0)
    assert other.pt.data.data_ptr() == state.pt.data_ptr() and other.microphysics.pt is other.pt


def test_refusals(emu_lib):
    from pace_amd import _lib
    from pace_amd.physics import Physics
    from pace_amd.util.grid import geom_struct

    env = mgp.make_env(emu_lib, "cpu", inputs()["area"], N, NZ, 300.0)
    make = lambda nml, packages=("microphysics",), e=env: Physics(e.stencil_factory, e.qf, e.grid_data, nml, list(packages))  # noqa: E731
    for nwat in (0, 5, 7):
        with pytest.raises(NotImplementedError, match="nwat"):
            make(mgp.namelist(nwat=nwat), ())
    with pytest.raises(NotImplementedError, match="hydrostatic"):
        make(mgp.namelist(hydrostatic=True))
    with pytest.raises(NotImplementedError, match="layout"):
        make(mgp.namelist(layout=(2, 2)), ())
    with pytest.raises(NotImplementedError):
        make(mgp.namelist(), ("microphysics", "pbl"))
    op = make(mgp.namelist())
    assert (op._nwat, op._p00, op._ptop, op._do_microphysics) == (6, 1.0e5, 300.0, True)
    f32 = _lib.Library(build_emu_f32())
    env32 = mgp.make_env(f32, "cpu", inputs()["area"], N, NZ, 300.0)
    with pytest.raises(NotImplementedError, match="float64"):
        make(mgp.namelist(), (), env32)
    # ... and so do the entry points of the float32 build
    q = env32.q3()
    table = lambda count: (C.c_void_p * count)(*[q.data.data_ptr()] * count)  # noqa: E731
    p, geom = q.data.data_ptr(), C.byref(geom_struct(env32.qf))
    with pytest.raises(_lib.PaceError, match="unsupported"):
        f32.call("pace_physics_prepare", geom, table(8), p, p, p, p, p, p, p, p, p, p, table(10), 300.0, 1, None)
    with pytest.raises(_lib.PaceError, match="unsupported"):
        f32.call("pace_physics_update_state", geom, table(10), table(10), table(10), 225.0, None)
    with pytest.raises(_lib.PaceError, match="unsupported"):
        f32.call("pace_copy_dycore_to_physics", geom, table(16), table(16), None)
    with pytest.raises(_lib.PaceError, match="unsupported"):
        f32.call("pace_physics_tendencies_to_dycore", geom, table(3), table(9), table(3), table(6), p, p, 1.0 / 225.0, None)


def test_layout_and_type_are_checked(emu_lib):
    import torch

    from pace_amd.physics import Physics

    env = mgp.make_env(emu_lib, "cpu", inputs()["area"], N, NZ, 300.0)
    op = Physics(env.stencil_factory, env.qf, env.grid_data, mgp.namelist(), ["microphysics"])
    wrongs = [torch.zeros((N + 7, N + 7, NZ + 1), dtype=torch.float64), env.q3().data.to(torch.float32), env.q2().data, None]
    for bad in ("qo3mr", "pt", "prsi", "phil", "wmp", "physics_updated_pt"):
        for wrong in wrongs:
            state = mgp.physics_state(env, inputs(), N, NZ, fill=1.0)
            setattr(state, bad, wrong)
            with pytest.raises(ValueError):
                op.prepare(state)
                op.update(state, DT)
    state = mgp.physics_state(env, inputs(), N, NZ, fill=1.0)
    state.microphysics.qr_dt = wrongs[0]
    with pytest.raises(ValueError):
        op.prepare(state)
    with pytest.raises(ValueError):
        op.prepare(mgp.physics_state(env, inputs(), N, NZ, packages=(), fill=1.0))


def test_header_and_binding_agree_on_the_entry_points():
    from pace_amd import _lib

    text = open(os.path.join(ROOT, "include", "pace_hip.h")).read()
    for name in ("pace_copy_dycore_to_physics", "pace_physics_prepare", "pace_physics_update_state",
                 "pace_physics_tendencies_to_dycore"):
        proto = re.search(rf"\bint {name}\s*\(([^;]*)\);", text).group(1)
        assert name in _lib.EXPORTED_SYMBOLS
        assert len(proto.split(",")) == len(_lib._PROTOS[name][1]), name
    assert int(re.search(r"#define PACE_PHYSICS_COPY_FIELDS (\d+)", text).group(1)) == len(_lib.PHYSICS_COPY_FIELDS) == 16
    assert int(re.search(r"#define PACE_PHYSICS_UPDATED_FIELDS (\d+)", text).group(1)) == len(_lib.PHYSICS_UPDATED) == 10
    assert [tuple(row) for row in _lib.PHYSICS_UPDATED] == [tuple(row) for row in npr.UPDATED]
    assert list(_lib.PHYSICS_COPY_FIELDS) == npr.COPIED
    assert sorted(x_dt for _, x_dt, _ in _lib.PHYSICS_UPDATED) == sorted(TEND)


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_physics_c12_gpu(lib):
    """The whole Physics call on the device against the reference's run: C12 x 79 is 144 columns, 12 of 64 lanes of a block
    active.  `pre` bits (wmp, which the microphysics transports, by its bound), tendency bounds, forward-Euler bits."""
    _, post, _ = mgp.run_operators(lib, "cuda:0", inputs(), ptop(), whole=True)
    check_pre(post, [name for name in PRE if name != "wmp"])
    check_tendencies(post, golden("post"), "device")
    check_euler(post)
    check_nothing_outside(post)


@pytest.mark.gpu
def test_prepare_c12_gpu(lib):
    """Physics.prepare alone on the device: every `pre` field, wmp included, to the bit; the tendencies zero."""
    out = run_prepare(lib, "cuda:0", inputs(), ptop(), ["microphysics"])
    check_pre(out)
    for name in TEND:
        assert (window(out[name], name, N, NZ) == 0).all(), name
    check_nothing_outside(out)
