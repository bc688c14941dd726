"""pace_amd.fv3core.GeosDycoreWrapper (reference: fv3core/pace/fv3core/initialization/geos_wrapper.py, tests/main/fv3core/
test_init_from_geos.py): a host model's numpy arrays in, one DynamicalCore step, a dictionary of numpy arrays out.

The six-tile runs are C12 x 79 on six ThreadComm ranks in one process; on the GPU they run in a child process with a time
limit.  The wrapper is compared bit for bit with the step done by hand: a DycoreState filled by numpy window assignment
(restated here from the reference's slices), step_dynamics with the same configuration, the outputs cut with numpy.
"""
import copy
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers  # noqa: E402
from helpers import ROOT, build_emu, build_emu_f32  # noqa: E402

N, NZ, H = 12, 79, 3
ARGUMENTS = ("u", "v", "w", "delz", "pt", "delp", "q", "ps", "pe", "pk", "peln", "pkz", "phis", "q_con", "omga", "ua", "va", "uc", "vc",
             "mfxd", "mfyd", "cxd", "cyd", "diss_estd")
TRACERS = ("qvapor", "qliquid", "qice", "qrain", "qsnow", "qgraupel", "qcld")  # q[..., 0:7]
CENTRED = ("w", "ua", "va", "delz", "pt", "delp", "q_con", "omga", "diss_estd")
OUTPUTS = ("u", "v", "w", "ua", "va", "uc", "vc", "delz", "pt", "delp", "mfxd", "mfyd", "cxd", "cyd", "ps", "pe", "pk", "peln", "pkz",
           "phis", "q_con", "omga", "diss_estd") + TRACERS
# the dycore_config of the reference's test (test_init_from_geos.py:27-77)
REFERENCE_DYCORE_CONFIG = {
    "a_imp": 1.0, "beta": 0.0, "consv_te": 0.0, "d2_bg": 0.0, "d2_bg_k1": 0.2, "d2_bg_k2": 0.1, "d4_bg": 0.15, "d_con": 1.0, "d_ext": 0.0,
    "dddmp": 0.5, "delt_max": 0.002, "do_sat_adj": True, "do_vort_damp": True, "fill": True, "hord_dp": 6, "hord_mt": 6, "hord_tm": 6,
    "hord_tr": 8, "hord_vt": 6, "hydrostatic": False, "k_split": 1, "ke_bg": 0.0, "kord_mt": 9, "kord_tm": -9, "kord_tr": 9, "kord_wz": 9,
    "n_split": 1, "nord": 3, "nwat": 6, "p_fac": 0.05, "rf_cutoff": 3000.0, "rf_fast": True, "tau": 10.0, "vtdm4": 0.06, "z_tracer": True,
    "do_qa": True, "tau_i2s": 1000.0, "tau_g2v": 1200.0, "ql_gen": 0.001, "ql_mlt": 0.002, "qs_mlt": 1e-06, "qi_lim": 1.0, "dw_ocean": 0.1,
    "dw_land": 0.15, "icloud_f": 0, "tau_l2v": 300.0, "tau_v2l": 90.0, "fv_sg_adj": 0, "n_sponge": 48}


def reference_namelist(nz=91, **dycore):
    """The namelist of the reference's test as a plain dict (there it is wrapped in an f90nml.Namelist, which is a dict)."""
    return {"stencil_config": {"compilation_config": {"backend": "numpy", "rebuild": False, "validate_args": True,
                                                      "format_source": False, "device_sync": False}},
            "initialization": {"type": "baroclinic"}, "nx_tile": N, "nz": nz, "dt_atmos": 225, "minutes": 15, "layout": [1, 1],
            "dycore_config": dict(REFERENCE_DYCORE_CONFIG, **dycore)}


def fortran_namelist(nz=91, **core):
    """The same settings as a Fortran model holds them: groups, npx / npy / npz in fv_core_nml, the rest where FV3 keeps it."""
    gfdl = ("tau_i2s", "tau_g2v", "ql_gen", "ql_mlt", "qs_mlt", "qi_lim", "dw_ocean", "dw_land", "icloud_f", "tau_l2v", "tau_v2l", "do_qa")
    core_nml = {k: v for k, v in REFERENCE_DYCORE_CONFIG.items() if k not in gfdl}
    core_nml.update(npx=N + 1, npy=N + 1, npz=nz, ntiles=6, layout=[1, 1])
    core_nml.update(core)
    return {"coupler_nml": {"dt_atmos": 225, "months": 0, "calendar": "julian"}, "fv_core_nml": core_nml,
            "gfdl_cloud_microphysics_nml": {k: REFERENCE_DYCORE_CONFIG[k] for k in gfdl}}


def source_shapes(n=N, nz=NZ):
    full = n + 2 * H
    shapes = {"u": (full, full + 1, nz), "v": (full + 1, full, nz), "uc": (full + 1, full, nz), "vc": (full, full + 1, nz),
              "mfxd": (n + 1, n, nz), "mfyd": (n, n + 1, nz), "cxd": (n + 1, full, nz), "cyd": (full, n + 1, nz),
              "ps": (full, full), "phis": (full, full), "pe": (n + 2, n + 2, nz + 1), "pk": (n, n, nz + 1), "peln": (n, n, nz + 1),
              "pkz": (n, n, nz), "q": (full, full, nz, 7)}
    shapes.update({name: (full, full, nz) for name in CENTRED})
    return shapes


def output_shapes(n=N, nz=NZ):
    """geos_wrapper.py:382-440 (_allocate_output_dir)."""
    full = n + 2 * H
    shapes = {"u": (full, full + 1, nz), "v": (full + 1, full, nz), "uc": (full + 1, full, nz), "vc": (full, full + 1, nz),
              "mfxd": (n + 1, n, nz), "mfyd": (n, n + 1, nz), "cxd": (n + 1, full, nz), "cyd": (full, n + 1, nz),
              "ps": (full, full), "phis": (full, full), "pe": (n + 2, n + 2, nz + 1), "pk": (n, n, nz + 1), "peln": (n, n, nz + 1),
              "pkz": (n, n, nz)}
    shapes.update({name: (full, full, nz) for name in CENTRED + TRACERS})
    return shapes


@pytest.fixture(scope="module")
def emu_lib():
    from pace_amd import _lib

    return _lib.Library(build_emu())


@pytest.fixture(scope="module")
def emu_lib_f32():
    from pace_amd import _lib

    return _lib.Library(build_emu_f32())


class CountingLib:
    """A library whose entry-point calls are counted (tests/test_diagnostics.py)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def call(self, name, *args):
        self.calls.append(name)
        return self._lib.call(name, *args)


def counted(wrapper):
    """-> (h2d, d2h): the lists the wrapper's one host-to-device and the packer's one device-to-host copy append their sizes to."""
    h2d, d2h = [], []
    to_device, to_host = wrapper._to_device, wrapper._packer._to_host

    def counted_to_device(staging, staged):
        h2d.append(staging.numel())
        to_device(staging, staged)

    def counted_to_host(packed, host):
        d2h.append(packed.numel())
        to_host(packed, host)

    wrapper._to_device, wrapper._packer._to_host = counted_to_device, counted_to_host
    return h2d, d2h


# ---- the reference's test, restated ---------------------------------------------------------------------------------------------
def test_geos_wrapper_as_the_reference_tests_it(emu_lib):
    """test_init_from_geos.py: C12 x 91, its namelist, NullComm(0, 6), all-ones arguments (no physical state: CPU tier only)."""
    from pace_amd import fv3core
    from pace_amd.util import NullComm

    counting = CountingLib(emu_lib)
    wrapper = fv3core.GeosDycoreWrapper(reference_namelist(), NullComm(rank=0, total_ranks=6, fill_value=0.0), "numpy", lib=counting)
    assert isinstance(wrapper, fv3core.GeosDycoreWrapper)
    assert isinstance(wrapper.dynamical_core, fv3core.DynamicalCore) and isinstance(wrapper.dycore_state, fv3core.DycoreState)
    assert isinstance(wrapper.dycore_config, fv3core.DynamicalCoreConfig) and wrapper.dycore_config.npz == 91
    assert wrapper.communicator.rank == 0 and wrapper.dycore_state.bdt == 225.0
    h2d, d2h = counted(wrapper)
    arguments = [np.ones(source_shapes(nz=91)[name]) for name in ARGUMENTS]
    del counting.calls[:]
    output_dict = wrapper(*arguments)
    assert isinstance(output_dict["u"], np.ndarray)
    assert tuple(output_dict) == OUTPUTS and len(output_dict) == 30
    for name, shape in output_shapes(nz=91).items():
        a = output_dict[name]
        assert isinstance(a, np.ndarray) and a.shape == shape and a.dtype == np.float64 and a.flags.c_contiguous, name
    # phis is input only: ones over the compute domain, the halo as the state was made
    assert np.array_equal(output_dict["phis"][H:H + N, H:H + N], np.ones((N, N))) and output_dict["phis"][0, 0] == 0.0
    # apart from what step_dynamics makes: one unpack launch, one pack launch, one copy each way
    assert counting.calls[0] == "pace_state_unpack" and counting.calls[-1] == "pace_diag_pack"
    assert counting.calls.count("pace_state_unpack") == 1 and counting.calls.count("pace_diag_pack") == 1
    assert len(h2d) == 1 and len(d2h) == 1 and d2h[0] == sum(int(np.prod(s)) for s in output_shapes(nz=91).values())
    timer = wrapper.perf_collector.timestep_timer
    assert {name: timer.hits.get(name) for name in ("move_to_pace", "dycore", "move_to_fortran")} == \
        {"move_to_pace": 1, "dycore": 1, "move_to_fortran": 1}
    assert wrapper.output_dict is output_dict


# ---- the namelist -----------------------------------------------------------------------------------------------------------------
def test_namelist_forms():
    from pace_amd.fv3core import DynamicalCoreConfig

    flat, groups = DynamicalCoreConfig.from_f90nml(reference_namelist()), DynamicalCoreConfig.from_f90nml(fortran_namelist())
    assert flat == groups
    assert (flat.npx, flat.npy, flat.npz, flat.layout, flat.dt_atmos, flat.do_sat_adj, flat.fv_sg_adj) == (13, 13, 91, (1, 1), 225.0, True, 0)
    assert flat.acoustic_dynamics.d_grid_shallow_water.n_sponge == 48 and flat.acoustic_dynamics.riemann.p_fac == 0.05
    # an unknown key is dropped: `minutes`, `calendar`, the stencil_config group; a known one still counts
    assert DynamicalCoreConfig.from_f90nml(reference_namelist(who_knows=3)) == flat
    assert DynamicalCoreConfig.from_f90nml(reference_namelist(n_split=5)).acoustic_dynamics.n_split == 5
    with pytest.raises(ValueError, match="duplicate keys: k_split"):
        DynamicalCoreConfig.from_f90nml(dict(fortran_namelist(), other_nml={"k_split": 2}))
    with pytest.raises(ValueError, match="n_split"):
        DynamicalCoreConfig.from_f90nml(reference_namelist(n_split="many"))
    with pytest.raises(ValueError, match="hord_tr"):
        DynamicalCoreConfig.from_f90nml(fortran_namelist(hord_tr=8.5))
    with pytest.raises(KeyError, match="nx_tile or fv_core_nml"):
        DynamicalCoreConfig.from_f90nml({"dt_atmos": 225, "dycore_config": {"k_split": 1}})


def test_constructor_refusals(emu_lib):
    from pace_amd import fv3core
    from pace_amd.util import NullComm

    def make(namelist):
        return fv3core.GeosDycoreWrapper(namelist, NullComm(0, 6), "numpy", lib=emu_lib)

    missing = reference_namelist()
    del missing["dycore_config"]["k_split"]
    with pytest.raises(KeyError, match="Cannot find k_split in namelist"):
        make(missing)
    missing = fortran_namelist()
    del missing["fv_core_nml"]["k_split"]
    with pytest.raises(KeyError, match="Cannot find k_split in namelist"):
        make(missing)
    with pytest.raises(NotImplementedError, match="layout"):
        make(dict(reference_namelist(), layout=[2, 2]))
    with pytest.raises(NotImplementedError, match="layout"):
        make(fortran_namelist(layout=[2, 2]))
    with pytest.raises(ValueError, match="duplicate keys"):
        make(dict(fortran_namelist(), other_nml={"n_split": 2}))


def test_wrong_shapes_name_the_argument(emu_lib):
    from pace_amd import fv3core
    from pace_amd.util import NullComm

    wrapper = fv3core.GeosDycoreWrapper(reference_namelist(nz=NZ), NullComm(0, 6), "numpy", lib=emu_lib)
    shapes = source_shapes()
    good = {name: np.ones(shapes[name]) for name in ARGUMENTS}
    for name, shape in (("pe", (N + 6, N + 6, NZ + 1)), ("pe", (N + 2, N + 2, NZ)), ("q", (N + 6, N + 6, NZ)), ("ps", (N + 6, N + 6, 1)),
                        ("u", shapes["v"]), ("diss_estd", (N, N, NZ))):
        arguments = dict(good, **{name: np.ones(shape)})
        with pytest.raises(ValueError, match=rf"^{name}: "):
            wrapper(*[arguments[a] for a in ARGUMENTS])


# ---- against the step done by hand ----------------------------------------------------------------------------------------------
def step_namelist():
    """The reference test's settings at 79 levels, without the saturation adjustment (the baroclinic case's configuration)."""
    return reference_namelist(nz=NZ, do_sat_adj=False)


def arguments_for(tile, arrays, second=False):
    """The 24 arguments cut from the baroclinic state of `tile` (helpers.generated_inputs: whole storages, (n + 7, n + 7, nz + 1))
    to the shapes a host model passes; what that state does not have is a smooth deterministic pattern.  second: another state
    -- the winds damped, the air a little warmer, the tracers scaled."""
    full = N + 2 * H
    shape = arrays["delp"].shape
    i, j, k = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), np.arange(shape[2]), indexing="ij")
    pattern = 0.5 + 0.5 * np.sin(0.31 * i + 0.17 * j + 0.23 * k + tile)
    fields = {name: np.array(arrays[name]) for name in "u v w delz pt delp pe pk peln phis uc vc ua va ps qvapor".split()}
    fields.update({name: f * (arrays["delp"] > 0) for name, f in helpers.dycore_condensates(tile, shape).items()})
    fields.update(pkz=1.0 + pattern, q_con=1e-4 * pattern, omga=0.01 * (pattern - 0.5), diss_estd=1e-3 * pattern,
                  mfxd=10.0 * pattern, mfyd=-10.0 * pattern, cxd=0.1 * pattern, cyd=-0.1 * pattern)
    if second:
        for name in ("u", "v", "uc", "vc", "ua", "va"):
            fields[name] = 0.9 * fields[name]
        fields["pt"] = fields["pt"] + 0.5 * pattern
        fields["w"] = fields["w"] + 0.01 * (pattern - 0.5)
        for name in TRACERS:
            fields[name] = 0.97 * fields[name]
    c = slice(H, H + N)
    out = {"u": fields["u"][:full, :full + 1, :NZ], "v": fields["v"][:full + 1, :full, :NZ],
           "uc": fields["uc"][:full + 1, :full, :NZ], "vc": fields["vc"][:full, :full + 1, :NZ],
           "mfxd": fields["mfxd"][H:H + N + 1, c, :NZ], "mfyd": fields["mfyd"][c, H:H + N + 1, :NZ],
           "cxd": fields["cxd"][H:H + N + 1, :full, :NZ], "cyd": fields["cyd"][:full, H:H + N + 1, :NZ],
           "ps": fields["ps"][:full, :full], "phis": fields["phis"][:full, :full],
           "pe": fields["pe"][H - 1:H + N + 1, H - 1:H + N + 1, :], "pk": fields["pk"][c, c, :], "peln": fields["peln"][c, c, :],
           "pkz": fields["pkz"][c, c, :NZ], "q": np.stack([fields[name][:full, :full, :NZ] for name in TRACERS], axis=-1)}
    out.update({name: fields[name][:full, :full, :NZ] for name in CENTRED})
    shapes = source_shapes()
    assert all(out[name].shape == shapes[name] for name in ARGUMENTS)
    return [np.ascontiguousarray(out[name]) for name in ARGUMENTS]


def ordered(arguments, order):
    """C: as they are; F: every argument np.asfortranarray; mixed: every second one."""
    if order == "C":
        return arguments
    return [np.asfortranarray(a) if order == "F" or m % 2 == 0 else a for m, a in enumerate(arguments)]


def assign_by_hand(state, arguments):
    """The reference's window assignments (geos_wrapper.py:207-270) in numpy on the host, field by field."""
    c, c1 = slice(H, H + N), slice(H, H + N + 1)
    a = dict(zip(ARGUMENTS, arguments))
    cuts = {"u": a["u"][c, c1], "v": a["v"][c1, c], "uc": a["uc"][c1, c], "vc": a["vc"][c, c1], "mfxd": a["mfxd"], "mfyd": a["mfyd"],
            "cxd": a["cxd"][:, c], "cyd": a["cyd"][c, :], "ps": a["ps"][c, c], "phis": a["phis"][c, c], "pk": a["pk"], "peln": a["peln"],
            "pkz": a["pkz"]}
    cuts.update({name: a[name][c, c] for name in CENTRED})
    cuts.update({name: a["q"][c, c, :, t] for t, name in enumerate(TRACERS)})
    for name, values in cuts.items():
        q = getattr(state, name)
        storage = np.array(q.numpy())
        view = storage[tuple(slice(o, o + e) for o, e in zip(q.origin, q.extent))]
        assert view.shape == values.shape, name
        view[...] = values.astype(storage.dtype)
        q.set(storage)
    storage = np.array(state.pe.numpy())
    storage[H - 1:H + N + 1, H - 1:H + N + 1, :] = a["pe"].astype(storage.dtype)
    state.pe.set(storage)


def cut_by_hand(state):
    """The reference's output slices (geos_wrapper.py:282-378) in numpy, as float64."""
    c, c1 = slice(H, H + N), slice(H, H + N + 1)
    d = {name: np.array(getattr(state, name).numpy()) for name in OUTPUTS}
    out = {"u": d["u"][:-1, :, :-1], "v": d["v"][:, :-1, :-1], "uc": d["uc"][:, :-1, :-1], "vc": d["vc"][:-1, :, :-1],
           "mfxd": d["mfxd"][c1, c, :-1], "mfyd": d["mfyd"][c, c1, :-1], "cxd": d["cxd"][c1, :-1, :-1], "cyd": d["cyd"][:-1, c1, :-1],
           "ps": d["ps"][:-1, :-1], "phis": d["phis"][:-1, :-1], "pe": d["pe"][H - 1:H + N + 1, H - 1:H + N + 1, :],
           "pk": d["pk"][c, c, :], "peln": d["peln"][c, c, :], "pkz": d["pkz"][c, c, :-1]}
    out.update({name: d[name][:-1, :-1, :-1] for name in CENTRED + TRACERS})
    return {name: np.ascontiguousarray(out[name]).astype(np.float64) for name in OUTPUTS}


def sync(device):
    if device != "cpu":
        import torch

        torch.cuda.synchronize()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def run_by_hand(lib, device, steps):
    """Per tile: the outputs after each of `steps` steps, the arguments of step m assigned before it."""
    import datetime

    from pace_amd.fv3core import DycoreState, DynamicalCore, DynamicalCoreConfig
    from pace_amd.tile import setup_factories
    from pace_amd.util import CubedSphereCommunicator, run_tiles
    from pace_amd.util.grid import DampingCoefficients, GridData, MetricTerms

    generated = helpers.generated_inputs(N, NZ)

    def program(comm):
        tile = comm.Get_rank()
        config = DynamicalCoreConfig.from_f90nml(step_namelist())
        cube = CubedSphereCommunicator(comm, device=device, lib=lib)
        _, qf, _, sf = setup_factories(lib, device, N, NZ, communicator=cube)
        metric_terms = MetricTerms(quantity_factory=qf, communicator=cube)
        grid_data = GridData.new_from_metric_terms(metric_terms)
        damping = DampingCoefficients.new_from_metric_terms(metric_terms, grid_data)
        state = DycoreState.init_zeros(quantity_factory=qf)
        core = DynamicalCore(cube, grid_data, sf, qf, damping, config, state.phis, state, datetime.timedelta(seconds=config.dt_atmos))
        outs = []
        for m in range(steps):
            assign_by_hand(state, arguments_for(tile, generated[tile][1], second=m == 1))
            core.step_dynamics(state)
            sync(device)
            outs.append(cut_by_hand(state))
        return outs

    return run_tiles(6, program)


def run_wrapper(lib, device, orders):
    """Per tile: (the outputs of one wrapper after each call, call m with the arguments of step m in orders[m]; the counts of
    the last call)."""
    from pace_amd import fv3core
    from pace_amd.util import run_tiles

    generated = helpers.generated_inputs(N, NZ)

    def program(comm):
        tile = comm.Get_rank()
        counting = CountingLib(lib)
        wrapper = fv3core.GeosDycoreWrapper(copy.deepcopy(step_namelist()), comm, "hip:gfx950", lib=counting, device=device)
        h2d, d2h = counted(wrapper)
        outs = []
        for m, order in enumerate(orders):
            del counting.calls[:], h2d[:], d2h[:]
            out = wrapper(*ordered(arguments_for(tile, generated[tile][1], second=m == 1), order))
            outs.append({name: a.copy() for name, a in out.items()})  # (the next call overwrites them)
        counts = (counting.calls.count("pace_state_unpack"), counting.calls.count("pace_diag_pack"), len(h2d), len(d2h))
        return outs, counts

    return run_tiles(6, program)


def wrapper_against_hand(lib, device, runs):
    """runs: the orders of each wrapper's calls.  -> [(run, tile, call, name) that differ], facts."""
    steps = max(len(orders) for orders in runs)
    want = run_by_hand(lib, device, steps)
    different, facts = [], []
    for orders in runs:
        got = run_wrapper(lib, device, orders)
        for tile in range(6):
            outs, counts = got[tile]
            facts.append((orders, tile, counts, [tuple(out) for out in outs]))
            for m, out in enumerate(outs):
                for name in OUTPUTS:
                    a, b = out[name], want[tile][m][name]
                    if a.shape != b.shape or a.dtype != np.float64 or not np.array_equal(bits(a), bits(b)):
                        different.append((orders, tile, m, name))
    # the second step did something, and so did the second set of arguments
    moved = all(not np.array_equal(want[t][0]["pt"], want[t][-1]["pt"]) for t in range(6)) if steps > 1 else None
    finite = all(np.isfinite(want[t][m][name]).all() for t in range(6) for m in range(steps) for name in ("pt", "u", "delp", "qvapor"))
    return different, facts, moved, finite


# C then a mix of orders on one wrapper (the second call: halos and untouched fields carry over); every argument F-ordered
RUNS_F64 = (("C", "mixed"), ("F",))
RUNS_F32 = (("mixed",),)


def check_against_hand(result, runs):
    different, facts, moved, finite = result
    assert different == [], different[:12]
    assert len(facts) == 6 * len(runs) and finite and moved in (True, None)
    for orders, tile, counts, names in facts:
        assert counts == (1, 1, 1, 1), (orders, tile, counts)
        assert all(n == OUTPUTS for n in names)


def test_wrapper_is_the_step_by_hand_emulated(emu_lib):
    check_against_hand(wrapper_against_hand(emu_lib, "cpu", RUNS_F64), RUNS_F64)


def test_wrapper_is_the_step_by_hand_f32_emulated(emu_lib_f32):
    check_against_hand(wrapper_against_hand(emu_lib_f32, "cpu", RUNS_F32), RUNS_F32)


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------
def _child_main(what, out_path):
    from pace_amd import _lib

    if what == "f64":
        result = wrapper_against_hand(_lib.load(), "cuda", RUNS_F64)
    elif what == "f32":
        result = wrapper_against_hand(_lib.load(32), "cuda", RUNS_F32)
    else:
        raise ValueError(what)
    with open(out_path, "wb") as f:
        pickle.dump(result, f)


def run_in_child(what, tmp_path, timeout=300):
    """A fresh process, a time limit, the child's output in the error when it fails (tests/test_driver.py)."""
    out = os.path.join(str(tmp_path), f"{what}.pkl")
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); "
            f"import test_geos_wrapper; test_geos_wrapper._child_main({what!r}, {out!r})")
    p = subprocess.run([sys.executable, "-X", "faulthandler", "-c", code], capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError(f"child run {what!r} failed (rc {p.returncode}):\n{p.stdout[-4000:]}\n{p.stderr[-8000:]}")
    with open(out, "rb") as f:
        return pickle.load(f)


@pytest.mark.gpu
def test_wrapper_is_the_step_by_hand_gpu(tmp_path):
    check_against_hand(run_in_child("f64", tmp_path), RUNS_F64)


@pytest.mark.gpu
def test_wrapper_is_the_step_by_hand_f32_gpu(tmp_path):
    check_against_hand(run_in_child("f32", tmp_path), RUNS_F32)
