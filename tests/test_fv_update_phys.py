"""The end of a dycore-only time step (pace_amd.stencils: UpdateAtmosphereState, ApplyPhysicsToDycore, AGrid2DGridPhysics;
k_updphys.hip) against a run of the reference on six C12 x 79 tiles (tools/make_golden_fvupdatephys.py), and at larger sizes
against the numpy restatement that reproduced that run bit for bit (tools/fv_update_phys_np.py): the emulated library on the
CPU, the gfx950 libraries with -m gpu.

Inputs are not stored: the state is pace_amd's generated one, changed and given tendencies by integer formulas
(fv_update_phys_np.perturb / tendencies), exactly as the generator built them.  The operators get the REFERENCE's grid terms
(drivergrid_c12.npz, the grid_* of acoustic_c12_tile*.npz), so that equal inputs meet equal arithmetic.

Bounds: BIT EQUALITY over the whole storage of every field passed -- the arithmetic of fill_gfs_delp, moist_cv, the pe sum
and the wind update has no transcendental, and pace_c2l_ord is bit-identical on equal inputs -- except peln = log(pe) and
pk = exp(KAPPA * peln), held to the relative error 1e-14 that the reference's own Translate tests apply by default.
Measured worst case with the emulated library (glibc log / exp against numpy's): peln 0.0, pk 1.4e-16; on an MI355X: peln 0.0,
pk 1.8e-16."""
import os
import pickle
import subprocess
import sys
import types

import numpy as np
import pytest

from helpers import ROOT, build_emu, build_emu_f32, golden

sys.path.insert(0, os.path.join(ROOT, "tools"))
import fv_update_phys_np as npr  # noqa: E402
import make_golden_fvupdatephys as gen  # noqa: E402

N, NZ, DT = gen.N, gen.NZ, gen.DT
WINDOWS = gen.WINDOWS
C = slice(3, 3 + N)
TOL_LOG = 1e-14
WATER = gen.WATER
FIELDS3 = WATER + ["pt", "pe", "delp", "peln", "pk", "u", "v", "ua", "va", "u_dt", "v_dt", "t_dt"]
FIELDS2 = ["ps", "u_srf", "v_srf"]
GRID_TERMS = ("vlon", "vlat", "es1", "ew2", "edge_vect_w", "edge_vect_e", "edge_vect_s", "edge_vect_n")


@pytest.fixture(scope="module")
def emu_lib():
    from pace_amd import _lib

    return _lib.Library(build_emu())


@pytest.fixture(scope="module")
def emu_f32_lib():
    from pace_amd import _lib

    return _lib.Library(build_emu_f32())


# ---- fixtures, inputs, expectations ----------------------------------------------------------------------------------------
_cache = {}


def inputs(chain=False):
    """chain: the state of the fixture in which DycoreToPhysics runs the dry convective adjustment first."""
    if ("in", chain) not in _cache:
        _cache[("in", chain)] = gen.build_inputs(N, NZ, chain=chain)
    return [{k: v.copy() for k, v in s.items()} for s in _cache[("in", chain)]]


def fixture(t, chain=False):
    stem = f"fvupdatephys_chain_c12_tile{t}" if chain else f"fvupdatephys_c12_tile{t}"
    d = golden(stem + ".npz")
    if os.path.exists(os.path.join(ROOT, "tests", "golden", stem + "_b.npz")):
        d.update(golden(stem + "_b.npz"))
    return d


def ref_grids():
    """Per tile: the reference's driver grid terms and the metric terms CubedToLatLon reads, as captured from its MetricTerms."""
    if "grids" not in _cache:
        dg = golden("drivergrid_c12.npz")
        out = []
        for t in range(6):
            g = {k: dg[f"{k}_tile{t}"] for k in GRID_TERMS}
            g["metrics"] = {k[5:]: v for k, v in golden(f"acoustic_c12_tile{t}.npz").items() if k.startswith("grid_")}
            g.update({k: g["metrics"][k] for k in ("dx", "dy", "a11", "a12", "a21", "a22")})
            out.append(g)
        _cache["grids"] = out
    return _cache["grids"]


def expected_all(chain=False):
    """Per tile, name -> the whole storage after the reference's [DycoreToPhysics and] UpdateAtmosphereState: the inputs with
    the stored windows put in; peln, pk from the stored pe with numpy (what the reference's run gave); the halos of u, v from
    the six windows."""
    if ("exp", chain) in _cache:
        return _cache[("exp", chain)]
    from pace_amd.util.gridgen.positions import exchange_vector

    inp = inputs(chain)
    windows = gen.CHAIN_WINDOWS if chain else WINDOWS
    out = []
    for t in range(6):
        d, e = fixture(t, chain), {}
        for name in list(inp[t]) + ["u_srf", "v_srf"]:
            before = inp[t][name] if name in inp[t] else np.zeros((N + 7, N + 7))
            e[name] = before.copy()
            if name in windows and name not in ("peln", "pk"):
                w = windows[name]
                e[name][w] = gen_unpack(d, "out_" + name, before[w])
        e["peln"][C, C, 1:] = np.log(e["pe"][C, C, 1:])
        e["pk"][C, C, 1:] = np.exp(npr.KAPPA * e["peln"][C, C, 1:])
        out.append(e)
    exchange_vector([e["u"][:, :, :NZ] for e in out], [e["v"][:, :, :NZ] for e in out], N, "d")
    _cache[("exp", chain)] = out
    return out


def gen_unpack(d, key, before):
    from make_golden_fvsubgridz import unpack

    return unpack(d, key, before)


def check(name, got, ref, tag, tol=TOL_LOG):
    """Bit equality over the whole array (NaN equals NaN); peln, pk: relative error <= tol = 1e-14."""
    if name in ("peln", "pk"):
        with np.errstate(all="ignore"):
            err = np.abs(got - ref) / np.abs(ref)
        err = np.where(got == ref, 0.0, err)
        worst = float(np.nanmax(err))
        print(tag, name, "worst relative error", worst)
        assert worst <= tol and np.array_equal(np.isnan(got), np.isnan(ref)), (tag, name, worst)
        return
    a, b = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(ref, dtype=np.float64)
    same = (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))
    assert same.all(), (tag, name, int((~same).sum()), "points differ, first at", tuple(np.argwhere(~same)[0]),
                        float(a[~same][0]), float(b[~same][0]))


def nan_outside(a, window, levels=None):
    """`a` with NaN everywhere outside (window, levels): what an operator must not read."""
    out = np.full(a.shape, np.nan)
    w = tuple(window) + ((slice(0, levels),) if levels is not None and a.ndim == 3 else ())
    out[w] = a[w]
    return out


# ---- one tile's program -----------------------------------------------------------------------------------------------------
def namelist(n=N, dt=DT):
    return types.SimpleNamespace(npx=n + 1, npy=n + 1, layout=(1, 1), dt_atmos=dt, c2l_ord=4)


def tile_program(comm, lib, device, inp, grid, what, n=N, nz=NZ, dt=DT, tensors=False):
    """what: "fill" (UpdateAtmosphereState without tendencies), "winds" (AGrid2DGridPhysics alone), "apply"
    (ApplyPhysicsToDycore), "update" (DycoreToPhysics without the adjustment, then UpdateAtmosphereState with tendencies),
    "chain" (the same with the dry convective adjustment, fv_sg_adj = 600, n_sponge = 48).  Returns name -> array."""
    import torch

    from pace_amd import stencils
    from pace_amd.tile import Env
    from pace_amd.util import CubedSphereCommunicator
    from pace_amd.util.grid import DriverGridData

    env = Env(lib, device, grid["metrics"], n, nz)
    cube = CubedSphereCommunicator(comm, device=device, lib=lib)
    info = DriverGridData.new_from_grid_variables(**{k: grid[k] for k in GRID_TERMS}, quantity_factory=env.qf)
    q = {k: (env.q3(v) if v.ndim == 3 else env.q2(v)) for k, v in inp.items()}
    f = {k: (v.data if tensors else v) for k, v in q.items()}
    state = types.SimpleNamespace(**{k: v for k, v in f.items() if k not in ("u_dt", "v_dt", "t_dt")})
    tend = types.SimpleNamespace(u_dt=f["u_dt"], v_dt=f["v_dt"])
    nl = namelist(n, dt)
    extra = {}
    if what == "winds":
        stencils.AGrid2DGridPhysics(env.stencil_factory, env.qf, cube.partitioner.tile, cube.rank, nl, info)(f["u"], f["v"], f["u_dt"], f["v_dt"])
    elif what == "apply":
        op = stencils.ApplyPhysicsToDycore(env.stencil_factory, env.qf, env.grid_data, nl, cube, info, state, f["u_dt"], f["v_dt"])
        op(state, f["u_dt"], f["v_dt"], f["t_dt"], dt)
        extra = {"u_srf": op._u_srf.numpy(), "v_srf": op._v_srf.numpy()}
    else:
        from pace_amd.fv3core import DynamicalCoreConfig

        if what in ("update", "chain"):
            cfg = DynamicalCoreConfig(npx=n + 1, npy=n + 1, npz=nz, fv_sg_adj=gen.FV_SG_ADJ)
            assert cfg.n_sponge == gen.N_SPONGE and cfg.nwat == 6
            stencils.DycoreToPhysics(env.stencil_factory, env.qf, cfg, what == "chain", True)(state, None, tend, dt)
        op = stencils.UpdateAtmosphereState(env.stencil_factory, env.grid_data, nl, cube, info, state, env.qf, True, what != "fill", tend)
        op(state, None, f["u_dt"], f["v_dt"], f["t_dt"], dt)
        a = op._apply_physics_to_dycore
        extra = {"u_srf": a._u_srf.numpy(), "v_srf": a._v_srf.numpy()}
    if device != "cpu":
        torch.cuda.synchronize()
    out = {k: v.numpy().astype(np.float64) for k, v in q.items()}
    out.update({k: v.astype(np.float64) for k, v in extra.items()})
    return out


def six_tiles(lib, device, inps, grids, what, **kw):
    from pace_amd.util import run_tiles

    return run_tiles(6, lambda comm: tile_program(comm, lib, device, inps[comm.Get_rank()], grids[comm.Get_rank()], what, **kw))


# ---- what each stage starts from and has to give --------------------------------------------------------------------------
def case_fill():
    """fill_gfs_delp alone: delp, qvapor with NaN in the one row / column of the storage the full domain does not cover."""
    inp, exp = inputs(), expected_all()
    full = (slice(0, N + 6), slice(0, N + 6))
    for s in inp:
        for k in ("delp", "qvapor"):
            s[k] = nan_outside(s[k], full)
    want = [{k: (nan_outside(e[k], full) if k == "qvapor" else s[k]) for k in s} for s, e in zip(inp, exp)]
    return inp, want


def case_winds():
    """AGrid2DGridPhysics alone: u_dt, v_dt with the one-point halo the update gives them (corners as they were), NaN beyond it
    and on level nz; u, v NaN outside the points they are updated on."""
    from pace_amd.util.gridgen.positions import exchange_scalar

    inp, exp = inputs(), expected_all()
    for k in ("u_dt", "v_dt"):
        exchange_scalar([s[k][:, :, :NZ] for s in inp], N, n_pts=1)
    H1 = WINDOWS["u_dt"]
    want = []
    for s, e in zip(inp, exp):
        for k in ("u_dt", "v_dt"):
            s[k] = nan_outside(s[k], H1, NZ)
        for k in ("u", "v"):
            s[k] = nan_outside(s[k], WINDOWS[k], NZ)
        w = {k: v for k, v in s.items()}
        for k in ("u", "v"):
            w[k] = nan_outside(e[k], WINDOWS[k], NZ)
        for k in ("u_dt", "v_dt"):
            w[k] = s[k].copy()
            w[k][H1 + (slice(0, NZ),)] = 0.0
        want.append(w)
    return inp, want


def case_apply():
    """ApplyPhysicsToDycore: the state as fill_gfs_delp leaves it."""
    inp, exp = inputs(), expected_all()
    for s, e in zip(inp, exp):
        s["qvapor"] = e["qvapor"].copy()
    return inp, exp


def case_update():
    return inputs(), expected_all()


def case_chain():
    return inputs(True), expected_all(True)


CASES = {"fill": case_fill, "winds": case_winds, "apply": case_apply, "update": case_update, "chain": case_chain}


def run_and_check(lib, device, what, tensors=False):
    inp, want = CASES[what]()
    outs = six_tiles(lib, device, inp, ref_grids(), what, tensors=tensors)
    check_outputs(outs, want, what)


def check_outputs(outs, want, what):
    for t in range(6):
        for name, ref in want[t].items():
            if name in ("u_srf", "v_srf") and what in ("fill", "winds"):
                continue
            check(name, outs[t][name], ref, (what, "tile", t))


# ---- the fixture itself --------------------------------------------------------------------------------------------------
def test_fixture_coverage():
    """Each of fill_gfs_delp's four branches is taken in at least 10 columns of the six tiles (counted by the generator with
    the restatement after that reproduced the reference's run), and a recount on the rebuilt inputs gives the stored counts."""
    d = fixture(0)
    cov = {b: (int(d["cov_" + b][0]), int(d["cov_" + b][1])) for b in npr.BRANCHES}
    for b, (count, least) in cov.items():
        assert least >= 10 and count >= least, (b, count, least)
    again = {b: 0 for b in npr.BRANCHES}
    for s in inputs():
        for b, m in npr.fill_gfs_delp(s["delp"], s["qvapor"], 1.0e-9).items():
            again[b] += int(m.sum())
    assert again == {b: c[0] for b, c in cov.items()}
    q = np.concatenate([s["qvapor"][C, C, :NZ].ravel() for s in inputs()])
    assert (q < 0).sum() > 1000 and ((q >= 0) & (q < 1e-9)).sum() > 1000


@pytest.mark.parametrize("chain", [False, True])
def test_restatement_reproduces_the_fixture(chain):
    """tools/fv_update_phys_np.py on the rebuilt inputs and the reference's grid terms gives the stored outputs bit for bit
    (peln, pk: both sides are numpy's); with the adjustment first, the fixture says in how many columns it acted."""
    mine, _ = gen.restated(inputs(chain), ref_grids())
    exp = expected_all(chain)
    for t in range(6):
        for name in exp[t]:
            assert gen.bits_equal(mine[t][name], exp[t][name]), (t, name)
    if chain:
        assert 100 <= int(fixture(0, True)["cov_adjusted_columns"][0]) <= 5 * N * N


# ---- the emulated library ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["fill", "winds", "apply", "update", "chain"])
def test_six_tiles_emulated(emu_lib, what):
    """fill_gfs_delp alone, AGrid2DGridPhysics alone, ApplyPhysicsToDycore, UpdateAtmosphereState after DycoreToPhysics --
    without ("update") and with ("chain") the dry convective adjustment -- against the reference's runs."""
    run_and_check(emu_lib, "cpu", what)


def test_quantities_and_tensors_give_the_same(emu_lib):
    run_and_check(emu_lib, "cpu", "update", tensors=True)


def rounded(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def run_kernels_one_tile(lib, inp, grid, n=N, nz=NZ, dt=DT, device="cpu", fill=True):
    """fill_gfs_delp (if `fill`), the column kernel and the wind kernels on ONE tile, without halo updates and CubedToLatLon."""
    import ctypes

    import torch

    from pace_amd import stencils
    from pace_amd.fv3core.stencils._common import dptr
    from pace_amd.fv3core.stencils.fillz import pointer_table
    from pace_amd.tile import Env
    from pace_amd.util import CubedSphereCommunicator, LoopbackComm
    from pace_amd.util.grid import DriverGridData, geom_struct

    env = Env(lib, device, grid["metrics"], n, nz)
    info = DriverGridData.new_from_grid_variables(**{k: grid[k] for k in GRID_TERMS}, quantity_factory=env.qf)
    q = {k: (env.q3(v) if v.ndim == 3 else env.q2(v)) for k, v in inp.items()}
    q["u_srf"], q["v_srf"] = env.q2(), env.q2()
    geom = geom_struct(env.qf)
    stream = None if device == "cpu" else ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if fill:
        lib.call("pace_fill_gfs_delp", ctypes.byref(geom), dptr(q["delp"]), dptr(q["qvapor"]), 1.0e-9, stream)
    lib.call("pace_phys_thermo_pressure", ctypes.byref(geom), pointer_table([q[k] for k in WATER]),
             *[dptr(q[k]) for k in ("pt", "t_dt", "pe", "delp", "peln", "pk", "ua", "va", "ps", "u_srf", "v_srf")], float(dt), stream)
    cube = CubedSphereCommunicator(LoopbackComm(rank=0, total_ranks=6), device=device, lib=lib)
    stencils.AGrid2DGridPhysics(env.stencil_factory, env.qf, cube.partitioner.tile, 0, namelist(n, dt), info)(q["u"], q["v"], q["u_dt"], q["v_dt"])
    if device != "cpu":
        torch.cuda.synchronize()
    return {k: v.numpy().astype(np.float64) for k, v in q.items()}


def restated_one_tile(inp, grid, dt=DT, store=np.float64):
    """store=np.float32: on float32-valued inputs and grid terms, every field rounded to float32 where it is stored."""
    s = {k: v.copy() for k, v in inp.items()}
    n = s["delp"].shape[0] - 7
    npr.fill_gfs_delp(s["delp"], s["qvapor"], 1.0e-9, store)
    s["u_srf"], s["v_srf"] = np.zeros((n + 7, n + 7)), np.zeros((n + 7, n + 7))
    npr.apply_before_halo(s, s["t_dt"], dt, s["u_srf"], s["v_srf"])
    npr.update_dwinds_phys(s["u"], s["v"], s["u_dt"], s["v_dt"], grid, 0.5 * dt)
    return s if store == np.float64 else {k: rounded(v) for k, v in s.items()}


# peln, pk in float32 storage: 1e-14 on the fp64 value, then one rounding to float32 (half an ulp = 2 ** -24 relative)
TOL_LOG_F32 = TOL_LOG + 2.0 ** -24


def rounded_grid(grid):
    return {k: (rounded(v) if k in GRID_TERMS else v) for k, v in grid.items()}


def check_f32(got, want, tag, skip=("ua", "va")):
    """The float32 library's outputs (widened) against a float32 restatement: EQUAL, whole storage; peln, pk to TOL_LOG_F32.
    ua, va: CubedToLatLon reads the stored, rounded u, v and has no float32 restatement."""
    for name, ref in want.items():
        if name not in skip:
            check(name, got[name], ref, tag, tol=TOL_LOG_F32)


def rounded_case(t=0):
    inp, grid = inputs()[t], ref_grids()[t]
    rin = {k: rounded(v) for k, v in inp.items()}
    rgrid = {k: (rounded(v) if k in GRID_TERMS else v) for k, v in grid.items()}
    return inp, grid, rin, rgrid


@pytest.mark.parametrize("t", range(6))
def test_f32_fill_gfs_delp_and_kernels_against_the_restatement_emulated(emu_f32_lib, t):
    """The float32-storage build, fill_gfs_delp included, on every tile's float32-rounded inputs against the restatement
    that rounds to float32 at every store (fill_gfs_delp: after each of its statements; q_min is float32(1e-9) in both):
    EQUAL over the whole storage of every field, peln / pk to 1e-14 + 2 ** -24."""
    inp, grid = inputs()[t], ref_grids()[t]
    rin, rgrid = {k: rounded(v) for k, v in inp.items()}, rounded_grid(grid)
    got = run_kernels_one_tile(emu_f32_lib, rin, grid)
    want = restated_one_tile(rin, rgrid, store=np.float32)
    check_f32(got, want, ("f32", "tile", t))
    # a clamped level holds float32(1e-9), the threshold the next call compares with: it is not "below q_min" again
    assert (got["qvapor"][:18, :18, 1:NZ] == float(np.float32(1.0e-9))).sum() > 100


def test_f32_storage_emulated(emu_f32_lib, emu_lib):
    """The float32-storage build against the float64 build on the float32-rounded inputs (grid terms included), its outputs
    rounded once to float32: EQUAL, since the arithmetic and the pe carry are fp64 registers in both.  The column and the
    wind kernels (fill_gfs_delp's sweeps re-read stored, rounded values: it is not part of this comparison)."""
    inp, grid, rin, rgrid = rounded_case()
    ref = run_kernels_one_tile(emu_lib, rin, rgrid, fill=False)
    got = run_kernels_one_tile(emu_f32_lib, rin, grid, fill=False)
    for name in ["pt", "t_dt", "pe", "peln", "pk", "ps", "u_srf", "v_srf", "u", "v", "u_dt", "v_dt"]:
        assert np.array_equal(got[name], rounded(ref[name]), equal_nan=True), (name, "float32 build differs")


# ---- the host layer ----------------------------------------------------------------------------------------------------------
def test_refusals(emu_lib):
    from pace_amd import stencils
    from pace_amd.fv3core import DynamicalCoreConfig
    from pace_amd.tile import Env
    from pace_amd.util import CubedSphereCommunicator, LoopbackComm
    from pace_amd.util.grid import DriverGridData

    grid = ref_grids()[0]
    env = Env(emu_lib, "cpu", grid["metrics"], N, NZ)
    cube = CubedSphereCommunicator(LoopbackComm(rank=0, total_ranks=6), device="cpu", lib=emu_lib)
    info = DriverGridData.new_from_grid_variables(**{k: grid[k] for k in GRID_TERMS}, quantity_factory=env.qf)
    state = types.SimpleNamespace(u=env.q3(), v=env.q3())
    tend = types.SimpleNamespace(u_dt=env.q3(), v_dt=env.q3())
    cfg = DynamicalCoreConfig(npx=N + 1, npy=N + 1, npz=NZ)
    with pytest.raises(NotImplementedError):
        stencils.UpdateAtmosphereState(env.stencil_factory, env.grid_data, namelist(), cube, info, state, env.qf, False, True, tend)
    with pytest.raises(NotImplementedError):
        stencils.DycoreToPhysics(env.stencil_factory, env.qf, cfg, False, False)
    bad = namelist()
    bad.layout = (2, 2)
    with pytest.raises(NotImplementedError):
        stencils.UpdateAtmosphereState(env.stencil_factory, env.grid_data, bad, cube, info, state, env.qf, True, True, tend)
    with pytest.raises(NotImplementedError):
        stencils.ApplyPhysicsToDycore(env.stencil_factory, env.qf, env.grid_data, bad, cube, info, state, tend.u_dt, tend.v_dt)
    with pytest.raises(NotImplementedError):
        stencils.AGrid2DGridPhysics(env.stencil_factory, env.qf, cube.partitioner.tile, 0, bad, info)
    # the constructors that are not refused build
    stencils.UpdateAtmosphereState(env.stencil_factory, env.grid_data, namelist(), cube, info, state, env.qf, True, False, tend)
    assert stencils.CubedToLatLon is __import__("pace_amd.fv3core.stencils.c2l_ord", fromlist=["x"]).CubedToLatLon
    assert stencils.fv_update_phys.ApplyPhysicsToDycore is stencils.ApplyPhysicsToDycore
    assert stencils.update_dwind_phys.AGrid2DGridPhysics is stencils.AGrid2DGridPhysics
    assert stencils.update_atmos_state.UpdateAtmosphereState is stencils.UpdateAtmosphereState


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------
def generated_case(n, nz=NZ, chain=False):
    """Inputs and pace_amd's own grid terms at any size, per tile."""
    from pace_amd.util import gridgen

    inp = gen.build_inputs(n, nz, chain=chain)
    grids = []
    for t, terms in enumerate(gridgen.tiles(n, nz)):
        g = {k: terms[k] for k in GRID_TERMS}
        g["metrics"] = {k: v for k, v in terms.items() if k not in ("ee1", "ee2", "es1", "ew2")}
        g.update({k: terms[k] for k in ("dx", "dy", "a11", "a12", "a21", "a22")})
        grids.append(g)
    return inp, grids


def _gpu_child(what, out_path):
    """Runs in a child process (six tiles = six host threads sharing one device, like helpers.run_in_child)."""
    from pace_amd import _lib

    kind, arg = what.split(":")
    lib = _lib.load(32 if kind.endswith("32") else 64)
    if kind == "fixture64":
        result = {w: six_tiles(lib, "cuda", CASES[w]()[0], ref_grids(), w) for w in ("fill", "winds", "apply", "update", "chain")}
    elif kind == "fixture32":  # (the float32 library: the update without the adjustment, on the rounded inputs)
        result = six_tiles(lib, "cuda", [{k: rounded(v) for k, v in s.items()} for s in inputs()], ref_grids(), "update")
    elif kind == "six64":
        inp, grids = generated_case(int(arg), chain=True)
        result = six_tiles(lib, "cuda", inp, grids, "chain", n=int(arg))
    elif kind == "six32":
        inp, grids = generated_case(int(arg))
        result = six_tiles(lib, "cuda", [{k: rounded(v) for k, v in s.items()} for s in inp], grids, "update", n=int(arg))
    else:
        inp, grids = generated_case(int(arg))
        result = run_kernels_one_tile(lib, inp[0], grids[0], n=int(arg), device="cuda")
    with open(out_path, "wb") as f:
        pickle.dump(result, f)


def gpu_child(what, tmp_path):
    out = os.path.join(str(tmp_path), "out.pkl")
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); "
            f"import test_fv_update_phys as m; m._gpu_child({what!r}, {out!r})")
    p = subprocess.run([sys.executable, "-X", "faulthandler", "-c", code], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-6000:])
    with open(out, "rb") as f:
        return pickle.load(f)


@pytest.mark.gpu
def test_six_tiles_fixture_gpu(tmp_path):
    """The six-tile comparisons of the emulated library on the device (libpace_hip.so), six tiles on one GPU through
    pace_amd.util.run_tiles: the same bounds."""
    outs = gpu_child("fixture64:0", tmp_path)
    for what in ("fill", "winds", "apply", "update", "chain"):
        check_outputs(outs[what], CASES[what]()[1], what)


@pytest.mark.gpu
def test_six_tiles_fixture_f32_gpu(tmp_path):
    """libpace_hip_f32.so: DycoreToPhysics (no adjustment) + UpdateAtmosphereState on six tiles, the float32-rounded fixture
    inputs and the reference's grid terms rounded, against the float32 restatement (gen.restated, store = float32): EQUAL over
    the whole storage of every field -- qvapor after fill_gfs_delp, pt, t_dt, pe, ps, the surface winds, u and v with the
    halos CubedToLatLon's update gives them, u_dt and v_dt after their halo update and the zeroing -- peln, pk to
    1e-14 + 2 ** -24.  ua, va are not compared (CubedToLatLon reads the stored, rounded u, v)."""
    outs = gpu_child("fixture32:0", tmp_path)
    rin = [{k: rounded(v) for k, v in s.items()} for s in inputs()]
    mine, _ = gen.restated(rin, [rounded_grid(g) for g in ref_grids()], N, NZ, DT, store=np.float32)
    for t in range(6):
        check_f32(outs[t], mine[t], ("fixture f32", "tile", t))


def _check_generated(outs, n):
    inp, grids = generated_case(n, chain=True)
    mine, _ = gen.restated(inp, grids, n, NZ, DT)
    changed = 0
    for t in range(6):
        for name in mine[t]:
            check(name, outs[t][name], mine[t][name], ("generated", n, "tile", t))
        changed += int((mine[t]["qcld"] != inp[t]["qcld"]).any(axis=2).sum())
    assert changed > 100, "the adjustment did not act"


@pytest.mark.gpu
@pytest.mark.parametrize("n", [48, 96])
def test_six_generated_tiles_gpu(tmp_path, n):
    """DycoreToPhysics (with the dry convective adjustment) + UpdateAtmosphereState on six generated tiles at C48 (partial
    64-lane rows) and C96 x 79 against the restatement on the same inputs, whole storage: bit equality, peln / pk to 1e-14."""
    _check_generated(gpu_child(f"six64:{n}", tmp_path), n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [48, 96])
def test_six_generated_tiles_f32_gpu(tmp_path, n):
    """libpace_hip_f32.so at C48 and C96 x 79, six tiles: the update without the adjustment (which has no float32
    restatement) on the rounded generated inputs against the float32 restatement, as test_six_tiles_fixture_f32_gpu."""
    outs = gpu_child(f"six32:{n}", tmp_path)
    inp, grids = generated_case(n)
    rin = [{k: rounded(v) for k, v in s.items()} for s in inp]
    mine, _ = gen.restated(rin, [rounded_grid(g) for g in grids], n, NZ, DT, store=np.float32)
    for t in range(6):
        check_f32(outs[t], mine[t], ("generated f32", n, "tile", t))


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [64, 32])
def test_one_tile_c192_gpu(tmp_path, precision):
    """The three kernels on one generated tile at C192 x 79 against the restatement (no halo update, no CubedToLatLon), whole
    storage; the float32 library on the rounded inputs against the float32 restatement, fill_gfs_delp included: equal."""
    n = 192
    inp, grids = generated_case(n)
    if precision == 64:
        got = gpu_child(f"one64:{n}", tmp_path)
        want = restated_one_tile(inp[0], grids[0])
        for name in FIELDS3 + FIELDS2:
            check(name, got[name], want[name], ("c192", name))
        return
    got = gpu_child(f"one32:{n}", tmp_path)
    rin = {k: rounded(v) for k, v in inp[0].items()}
    check_f32(got, restated_one_tile(rin, rounded_grid(grids[0]), store=np.float32), ("c192 f32",), skip=())
