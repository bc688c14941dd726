"""The five stencils of k_tracer.hip one by one, and TracerAdvection whole away from C12, on the float64 and the float32-storage
library, emulated and on the device.

The stencils are driven through the C entry points TracerAdvection uses (pace_tracer_flux_compute, pace_tracer_divide_fluxes,
pace_apply_mass_flux, pace_apply_tracer_flux, pace_swap_dp) on one tile without a communicator, in the order of
TracerAdvection.__call__ but with given tracer fluxes instead of the transport (that one: tests/test_vertical_edges.py
test_ord8_transport_at_device_chain_shapes).  The reference is oracle/tracer.py's function of the same name.  With float32 storage
every input is a float32 value (opchain.f32, the metric terms included) and the reference is float32(oracle(inputs)); the state
is rounded again after every stencil, as `real` fields do.

Every output is in the EXACT class of tests/test_f32_operators.py in both storage types: each stencil is one pass from its loads
to one store per output, without a transcendental.  Asserted per stencil call:
  * bit identity with the reference on the written window;
  * every cell outside the window keeps the bits it held (NaN wherever the stencil does not read: an input's halo, level nk, an
    output that is only written), and every input keeps its bits.  The windows: the compute domain for the two `apply` stencils
    and the swap, (n + 1) x (n + 6) and (n + 6) x (n + 1) for flux_compute's xfx and yfx; divide_fluxes writes the whole storage
    plane, the reference's origin_full, domain_full(add=(1, 1, 0)): exactly that, levels 0 .. nk - 1.

What the shapes reach: flux_compute, divide and swap_dp map a flat index over the padded plane to (i, j) (PLANE_IJK), the two
`apply` stencils use 64 x 4 patches (PATCH_IJK); both read the staggered column ie + 1.  C13: an odd size, one block per row.
C64: i = ie + 1 = 67 is the one live flux lane of a second 64-lane patch (and lanes 64 .. 70 of the plane).  C68: five compute
lanes 64 .. 70 there.  Row strides (elements): float64 rows are padded to 16, float32 rows to 32 -- C13 32 / 32 (20 points), C64 80 / 96 (71),
C68 80 / 96 (75; asserted below).  nk = 1, 5, 3, 2 levels; n_split 1 (no sub-cycling: one pass, no swap) and 3.

Found by this module: k_apply_mass_flux and k_apply_tracer_flux evaluated their whole expression in float in
the float32 build, every operand being a `real` load.
"""
import ctypes as C

import numpy as np
import pytest

import opchain
from helpers import Env, build_emu, build_emu_f32, oracle_grid
from opchain import f32, f32_dict, f32_neighbours

SEED = 20250131
SHAPES = [(13, 1), (13, 5), (64, 3), (68, 2)]
STRIDES = {("f64", 13): 32, ("f64", 64): 80, ("f64", 68): 80, ("f32", 13): 32, ("f32", 64): 96, ("f32", 68): 96}
LIBS = [pytest.param("emulated", "f64", id="emulated-f64"), pytest.param("emulated", "f32", id="emulated-f32"),
        pytest.param("device", "f64", id="gpu-f64", marks=pytest.mark.gpu), pytest.param("device", "f32", id="gpu-f32", marks=pytest.mark.gpu)]

_libs = {}


def library(which, storage):
    """(library, device) of "emulated" or "device" with "f64" or "f32" storage, loaded once."""
    if (which, storage) not in _libs:
        from pace_amd import _lib

        if which == "emulated":
            _libs[which, storage] = (_lib.Library(build_emu_f32() if storage == "f32" else build_emu()), "cpu")
        else:
            _libs[which, storage] = (_lib.load(32) if storage == "f32" else _lib.load(), "cuda")
        assert _libs[which, storage][0].real_bytes == (4 if storage == "f32" else 8)
    return _libs[which, storage]


def stored(a, storage):
    """What a `real` field holds of a float64 array, as float64."""
    return f32(a) if storage == "f32" else np.asarray(a, dtype=np.float64)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def keep(a, win, nk):
    """`a` with NaN everywhere but on the (i, j) window `win`, levels 0 .. nk - 1."""
    out = np.full(a.shape, np.nan)
    w = win + (slice(0, nk),)
    out[w] = a[w]
    return out


# ---- the stencil sequence and its reference, once per (shape, n_split, storage) ---------------------------------------------------
ARGS = {"flux_compute": ("cx", "cy", "xfx", "yfx"), "divide": ("cx", "xfx", "mfx", "cy", "yfx", "mfy"),
        "apply_mass_flux": ("dp1", "mfx", "mfy", "dp2"), "apply_tracer_flux": ("q", "dp1", "fx", "fy", "dp2"), "swap_dp": ("dp1", "dp2")}
_cases = {}


def stencil_cases(n, nk, n_split, storage):
    """(metrics, [(stencil, before, after, {output: window})]): `before` is what the fields hold (float64 arrays of storable
    values, NaN wherever the stencil must neither read nor write), `after` the oracle's result on a copy of it, unrounded."""
    key = (n, nk, n_split, storage)
    if key in _cases:
        return _cases[key]
    from oracle import tracer
    from pace_amd import synthetic

    metrics = synthetic.tile_metrics(n, nk)
    if storage == "f32":
        metrics = f32_dict(metrics)
    g = oracle_grid(metrics, n, nk)
    rng = np.random.default_rng(SEED + 1000 * n + 10 * nk + n_split)
    shape = (n + 7, n + 7, nk + 1)
    area, dp = float(metrics["area"][3:3 + n, 3:3 + n].mean()), 1000.0

    def field(lo, hi):
        a = stored(lo + (hi - lo) * rng.random(shape), storage)
        a[:, :, nk] = np.nan
        return a

    cw = opchain._win(n)
    xw, yw, bw = opchain._win(n, 0, 0, 1, 0), opchain._win(n, 0, 0, 0, 1), opchain._win(n, 0, 0, 1, 1)
    xfw, yfw = (slice(3, 4 + n), slice(0, n + 6)), (slice(0, n + 6), slice(3, 4 + n))
    full = (slice(0, n + 7), slice(0, n + 7))
    nan = np.full(shape, np.nan)
    cases = []

    def step(name, before, wins, fn):
        after = {k: v.copy() for k, v in before.items()}
        fn(after)
        cases.append((name, before, after, wins))
        return {k: stored(v, storage) for k, v in after.items()}

    # sign-changing Courant numbers: both branches of flux_compute in every row
    cx, cy = field(-0.6, 0.6), field(-0.6, 0.6)
    b = {"cx": keep(cx, xfw, nk), "cy": keep(cy, yfw, nk), "xfx": nan.copy(), "yfx": nan.copy()}
    for a, w in ((b["cx"], xfw), (b["cy"], yfw)):
        row = a[w][:, :, 0]
        assert ((row > 0).any(axis=0) & (row < 0).any(axis=0)).all()
    step("flux_compute", b, {"xfx": xfw, "yfx": yfw}, lambda a: tracer.flux_compute(g, a["cx"], a["cy"], a["xfx"], a["yfx"], nk))
    # divide_fluxes: the whole plane of all six
    b = {"cx": cx, "cy": cy, "xfx": field(-0.6 * area, 0.6 * area), "yfx": field(-0.6 * area, 0.6 * area),
         "mfx": field(-0.1 * area * dp, 0.1 * area * dp), "mfy": field(-0.1 * area * dp, 0.1 * area * dp)}
    d = step("divide", b, dict.fromkeys(ARGS["divide"], full), lambda a: tracer.divide_fluxes([a[k] for k in ARGS["divide"]], n_split, nk))
    mfx, mfy = keep(d["mfx"], bw, nk), keep(d["mfy"], bw, nk)
    dp1, dp2, q = keep(field(0.8 * dp, 1.2 * dp), cw, nk), nan.copy(), keep(field(1.0e-4, 1.0e-2), cw, nk)
    for it in range(n_split):
        s = step("apply_mass_flux", {"dp1": dp1, "mfx": mfx, "mfy": mfy, "dp2": dp2}, {"dp2": cw},
                 lambda a: tracer.apply_mass_flux(g, a["dp1"], a["mfx"], a["mfy"], a["dp2"], nk))
        dp2 = s["dp2"]
        assert (dp2[cw][:, :, :nk] > 0.3 * dp).all()
        fx = keep(field(-1.0e-3 * area * dp, 1.0e-3 * area * dp), bw, nk)
        fy = keep(field(-1.0e-3 * area * dp, 1.0e-3 * area * dp), bw, nk)
        s = step("apply_tracer_flux", {"q": q, "dp1": dp1, "fx": fx, "fy": fy, "dp2": dp2}, {"q": cw},
                 lambda a: tracer.apply_tracer_flux(g, a["q"], a["dp1"], a["fx"], a["fy"], a["dp2"], nk))
        q = s["q"]
        if it != n_split - 1:
            s = step("swap_dp", {"dp1": dp1, "dp2": dp2}, {"dp1": cw, "dp2": cw}, lambda a: tracer.swap_dp(g, a["dp1"], a["dp2"], nk))
            dp1, dp2 = s["dp1"], s["dp2"]
    _cases[key] = (metrics, cases)
    return _cases[key]


def call_stencil(lib, env, geom, met, name, f, n_split):
    from pace_amd.fv3core.stencils._common import dptr

    p = [dptr(f[k]) for k in ARGS[name]]
    if name == "flux_compute":
        lib.call("pace_tracer_flux_compute", C.byref(geom), C.byref(met), *p, None)
    elif name == "divide":
        lib.call("pace_tracer_divide_fluxes", C.byref(geom), *p, int(n_split), None)
    elif name == "swap_dp":
        lib.call("pace_swap_dp", C.byref(geom), *p, None)
    else:
        lib.call("pace_" + name, C.byref(geom), C.byref(met), *p, None)
    if env.qf.device.type == "cuda":
        import torch

        torch.cuda.synchronize()


def check_tracer_stencils(lib, device, n, nk, n_split, storage):
    """Every stencil call of the sequence against the oracle, in the exact class.  Returns [what is wrong]."""
    from pace_amd.util.grid import geom_struct
    from test_f32_operators import ulps

    metrics, cases = stencil_cases(n, nk, n_split, storage)
    env = Env(lib, device, metrics, n, nk)
    assert env.qf.row_stride == STRIDES[storage, n], env.qf.row_stride
    geom, met = geom_struct(env.qf), env.grid_data.c_struct()
    real = np.float32 if storage == "f32" else np.float64
    wrong = []
    for number, (name, before, after, wins) in enumerate(cases):
        f = {k: env.q3(before[k]) for k in ARGS[name]}
        call_stencil(lib, env, geom, met, name, f, n_split)
        for k in ARGS[name]:
            got, want = f[k].numpy(), after[k].astype(real)
            assert got.dtype == real and got.shape == want.shape
            if k not in wins:
                if not np.array_equal(bits(got), bits(before[k].astype(real))):
                    wrong.append((number, name, k, "an input was written"))
                continue
            w = wins[k] + (slice(0, nk),)
            assert np.isfinite(after[k][w]).all(), (name, k)
            if not np.array_equal(bits(got[w]), bits(want[w])):
                u = ulps(got[w], want[w]) if storage == "f32" else (got[w] != want[w])
                wrong.append((number, name, k, f"{int((u != 0).sum())} of {u.size} differ on the window, worst {int(u.max())} ulp"))
            out = np.ones(got.shape, dtype=bool)
            out[w] = False
            # (outside the window the oracle leaves what `before` held: the same array there)
            if not np.array_equal(bits(got)[out], bits(before[k].astype(real))[out]):
                wrong.append((number, name, k, f"{int((bits(got)[out] != bits(before[k].astype(real))[out]).sum())} cells written outside the window"))
    return wrong, [c[0] for c in cases]


@pytest.mark.parametrize("n_split", [1, 3])
@pytest.mark.parametrize("n,nk", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("which,storage", LIBS)
def test_tracer_stencils_one_by_one(which, storage, n, nk, n_split):
    """flux_compute, divide_fluxes, then n_split times apply_mass_flux, apply_tracer_flux and (but for the last) swap_dp, each
    on the oracle's state before it: bit for bit on the window, nothing else written (module docstring)."""
    lib, device = library(which, storage)
    wrong, seen = check_tracer_stencils(lib, device, n, nk, n_split, storage)
    assert not wrong, wrong
    assert seen == ["flux_compute", "divide"] + (["apply_mass_flux", "apply_tracer_flux", "swap_dp"] * n_split)[:-1]


# ---- TracerAdvection whole, six tiles at C13 x 5 -------------------------------------------------------------------------------------
WHOLE_SHAPE = (13, 5)
WHOLE_OUT = ("qvapor", "q2", "dp1", "mfxd", "mfyd", "cxd", "cyd")
_whole = {}


def whole_inputs(storage):
    """Per tile {name: array} on opchain.six_tile_inputs' geometry and masses: two tracers (one of them sign-changing), random
    sign-changing Courant numbers and mass fluxes small enough that the layer mass stays positive over the three sub-cycles."""
    n, nz = WHOLE_SHAPE
    m, tiles = opchain.six_tile_inputs(n, nz)
    rng = np.random.default_rng(SEED)
    area = m["area"][:, :, None]
    ins = []
    for t, (a, _) in enumerate(tiles):
        d = {"dp1": a["delp"].copy(), "qvapor": 1.0e-2 * a["pt"] / np.abs(a["pt"]).max() * (1.0 + 0.2 * rng.random(a["pt"].shape)),
             "q2": 1.0e-3 * (rng.random(a["pt"].shape) - 0.3)}
        d["cxd"], d["cyd"] = rng.uniform(-0.5, 0.5, a["pt"].shape), rng.uniform(-0.5, 0.5, a["pt"].shape)
        d["mfxd"], d["mfyd"] = 0.3 * d["cxd"] * d["dp1"] * area, 0.3 * d["cyd"] * d["dp1"] * area
        ins.append({k: stored(v, storage) for k, v in d.items()})
    return (f32_dict(m) if storage == "f32" else m), ins


def oracle_whole(m, ins):
    from oracle import tracer

    n, nz = WHOLE_SHAPE
    grids = [oracle_grid(m, n, nz) for _ in range(6)]
    f = {k: [d[k].copy() for d in ins] for k in WHOLE_OUT}
    tracer.tracer_advection(grids, {"qvapor": f["qvapor"], "q2": f["q2"]}, f["dp1"], f["mfxd"], f["mfyd"], f["cxd"], f["cyd"], n, nz)
    return f


def whole_case(storage):
    """(metrics, inputs, the oracle's outputs, S): S[name] is the oracle's response over the six tiles' checked windows to one
    float32 rounding of the state it is given (two draws of opchain.f32_neighbours, fixed seed); float32 storage only."""
    if storage not in _whole:
        m, ins = whole_inputs(storage)
        ref = oracle_whole(m, ins)
        S = {}
        if storage == "f32":
            for draw in range(2):
                rng = np.random.default_rng(SEED + 1 + draw)
                noisy = oracle_whole(m, [{k: f32_neighbours(v, rng) for k, v in d.items()} for d in ins])
                for k in WHOLE_OUT:
                    for t in range(6):
                        w = whole_window(k)
                        S[k] = max(S.get(k, 0.0), float(np.abs(noisy[k][t][w] - ref[k][t][w]).max()))
        _whole[storage] = (m, ins, ref, S)
    return _whole[storage]


def whole_window(k):
    n, nz = WHOLE_SHAPE
    return opchain._win(n, 0, 0, int(k in ("mfxd", "cxd")), int(k in ("mfyd", "cyd"))) + (slice(0, nz),)


@pytest.mark.parametrize("which,storage", LIBS)
def test_tracer_advection_six_tiles_c13(which, storage):
    """TracerAdvection on six C13 x 5 tiles through the cube communicator (one device, or emulated) against
    oracle.tracer.tracer_advection: the first whole run at a size that is odd and not C12.  float64: bit for bit, like the C12
    golden test.  float32: the divided mass fluxes and Courant numbers exact (one product); the tracers and dp1 staged -- the
    area fluxes, the transport's fluxes fx / fy, dp2 and the tracer between sub-cycles are `real` fields -- against
    opchain.staged_bound with factor 2 and S from the oracle alone."""
    from helpers import run_tracer_tiles
    from test_f32_operators import EXACT, judge, show, staged

    n, nz = WHOLE_SHAPE
    lib, device = library(which, storage)
    m, ins, ref, S = whole_case(storage)
    outs = run_tracer_tiles(lib, device, [m] * 6, ins, n, nz)
    wrong = []
    for k in WHOLE_OUT:
        w = whole_window(k)
        for t in range(6):
            got, want = outs[t][k][w], ref[k][t][w]
            assert np.isfinite(want).all(), (k, t)
            if storage == "f64":
                if not np.array_equal(got, want):
                    wrong.append((k, t, int((got != want).sum()), float(np.abs(got - want).max())))
                continue
            cls = EXACT if k in ("mfxd", "mfyd", "cxd", "cyd") else staged(
                "xfx / yfx, the transport's fx / fy, dp2 and the tracer between sub-cycles are real fields")
            row, bad = judge(cls, got, f32(want), S[k])
            show(f"{which} tracer_advection n={n} nz={nz} tile={t}", "TracerAdvection", k, row)
            if bad:
                wrong.append((k, t, bad, row))
    assert not wrong, wrong
