"""pace_amd.stencils.HeldSuarezForcing on a C12 x 7 state (tile 0 of the C12 grid: tests/golden/grid_c12_tile0.npz).

* one pace_held_suarez launch per call and nothing else: no other entry point, no upload, the two planes' storages and values
  untouched; the planes equal np.sin(lat) ** 2 / np.cos(lat) ** 2 of grid_data.lat_agrid as the library stores them;
* the result is the restatement's (tests/held_suarez_reference.py) with the device's teq, for a DycoreState-like namespace;
* the contraction, float64 library, heating_scale = 1.  With u = 2 ** -53, D = T - teq and r = kt dt / (1 + kt dt) <= 1 the
  kernel's pt_dt = -fl(fl(kt fl(D)) / fl(1 + fl(kt dt))) is -(kt D / (1 + kt dt)) (1 + e) with |e| <= 5 u to first order (five
  roundings), so T + dt pt_dt - teq = D / (1 + kt dt) - e r D exactly.  The test forms the left side in double as
  fl(fl(T + fl(dt pt_dt)) - teq): three roundings of at most u dt |pt_dt| <= u |D|, u (|T| + |D|) and u |D|; the right side
  fl(fl(D) / fl(1 + fl(kt dt))) carries four roundings of a value <= |D|.  Together
      |lhs - rhs| <= u (5 |D| + |D| + (|T| + |D|) + |D| + 4 |D|) = u (|T| + 12 |D|),
  doubled for the second-order terms.  Likewise ua + dt u_dt against ua / (1 + kv dt) with T = D = ua.  Hence
  |T_new - teq| <= |T - teq| + that bound everywhere, for dt = 225 and for dt = 1e6 (where forward Euler would overshoot:
  k_s dt = 2.9);
* the winds above sigma_b get tendencies of exactly zero magnitude;
* a state with pt = teq (the device's own teq output) and zero winds gets all-zero tendencies -- in the float32 library pt holds
  the NARROWED teq, within half a float32 ulp of the double the kernel forms, so there |pt_dt| <= kt (ulp32(teq) / 2) (1 + 2 ** -22);
* the refusals of the configuration, the constructor and the call.

Every check is a function of the device: the CPU tier calls it with the emulation libraries, the GPU tier with the product's."""
import dataclasses
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import ROOT, build_emu, build_emu_f32  # noqa: E402
import held_suarez_reference as ref  # noqa: E402

N, NK = 12, 7
U = 2.0 ** -53


class SpyLib:
    """A library whose entry-point calls are counted."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def call(self, name, *args):
        self.calls.append(name)
        return self._lib.call(name, *args)


def _lib(device, which):
    from pace_amd import _lib

    if device == "cpu":
        return _lib.Library(build_emu() if which == 0 else build_emu_f32())
    return _lib.load() if which == 0 else _lib.load(32)


def _sync(device):
    if device != "cpu":
        import torch

        torch.cuda.synchronize()


def setup(device, which, **kw):
    from pace_amd.stencils import HeldSuarezForcing
    from pace_amd.tile import Env

    lib = SpyLib(_lib(device, which))
    metrics = dict(np.load(os.path.join(ROOT, "tests", "golden", "grid_c12_tile0.npz"), allow_pickle=False))
    env = Env(lib, device, metrics, N, NK)
    forcing = HeldSuarezForcing(env.stencil_factory, env.qf, env.grid_data, **kw)
    rng = np.random.default_rng(3)
    shape = (N + 7, N + 7, NK + 1)
    ps = rng.uniform(95000.0, 103000.0, shape[:2] + (1,))
    values = dict(pe=300.0 + (ps - 300.0) * (np.arange(NK + 1) / NK) ** 0.5, ua=rng.uniform(-50.0, 50.0, shape),
                  va=rng.uniform(-50.0, 50.0, shape), pt=rng.uniform(180.0, 320.0, shape))
    state = types.SimpleNamespace(**{name: env.q3(a) for name, a in values.items()})
    out = types.SimpleNamespace(u_dt=env.q3(), v_dt=env.q3(), pt_dt=env.q3(), teq=env.q3())
    return lib, env, forcing, state, out


def host(ns):
    return {name: np.array(q.numpy()) for name, q in vars(ns).items()}


def constants(forcing, dt):
    c = forcing.config
    return ref.Constants(dt=dt, heating_scale=forcing.heating_scale, **dataclasses.asdict(c))


def check_operator(device, which):
    from pace_amd import _launch

    lib, env, forcing, state, out = setup(device, which)
    real = np.float32 if lib.real_bytes == 4 else np.float64
    lat = np.asarray(env.grid_data.lat_agrid)
    assert isinstance(env.grid_data.lat_agrid, np.ndarray) and lat.shape == (N + 7, N + 7)
    s2, c2 = np.array(forcing.sin2lat.numpy()), np.array(forcing.cos2lat.numpy())
    assert s2.dtype == real and np.array_equal(s2, (np.sin(lat) ** 2).astype(real)) and np.array_equal(c2, (np.cos(lat) ** 2).astype(real))
    assert forcing.heating_scale == ref.CV_AIR / ref.CP_AIR
    # ---- one launch per call, nothing uploaded
    uploads = []
    real_upload = _launch.upload_table
    _launch.upload_table = lambda *a, **k: (uploads.append(1), real_upload(*a, **k))[1]
    pointers = (forcing.sin2lat.ptr, forcing.cos2lat.ptr)
    try:
        lib.calls.clear()
        forcing(state, out.u_dt, out.v_dt, out.pt_dt, 225.0, teq=out.teq)
        first = host(out)
        forcing(state, out.u_dt, out.v_dt, out.pt_dt, 225.0, accumulate=True)
        _sync(device)
    finally:
        _launch.upload_table = real_upload
    assert lib.calls == ["pace_held_suarez"] * 2 and uploads == []
    assert pointers == (forcing.sin2lat.ptr, forcing.cos2lat.ptr)
    assert np.array_equal(s2, forcing.sin2lat.numpy()) and np.array_equal(c2, forcing.cos2lat.numpy())
    # ---- the restatement with the device's teq; the second call added the same values to the first's
    h = host(state)
    c = constants(forcing, 225.0)
    zeros = np.zeros((N + 7, N + 7, NK + 1), real)
    cs = slice(3, 3 + N)
    teq64 = first["teq"][cs, cs, :NK].astype(np.float64)
    assert (teq64 >= 200.0).all() and (teq64 == 200.0).mean() > 0.05 and (teq64 > 200.0).mean() > 0.05
    want = ref.held_suarez(c, h["pe"], h["ua"], h["va"], h["pt"], s2, c2, zeros, zeros, zeros, zeros, N, NK, 0, teq=teq64)
    twice = ref.held_suarez(c, h["pe"], h["ua"], h["va"], h["pt"], s2, c2, first["u_dt"], first["v_dt"], first["pt_dt"], None, N, NK,
                            1, teq=teq64)
    second = host(out)
    for m, name in enumerate(("u_dt", "v_dt") + (("pt_dt",) if lib.real_bytes == 8 else ())):
        assert np.array_equal(first[name], want[m]) and np.array_equal(second[name], twice[m]), name
    assert np.array_equal(second["teq"], first["teq"])  # (not written without teq=)
    # ---- the winds above sigma_b: exactly zero
    t = ref.terms(c, h["pe"], s2, c2, N, NK)
    above = t["sigma"] < c.sigma_b
    assert 0.05 < above.mean() < 0.95
    for name in ("u_dt", "v_dt"):
        assert (first[name][cs, cs, :NK][above] == 0.0).all() and (first[name][cs, cs, :NK][~above & (t["h"] > 0)] != 0.0).all()
    # ---- a timedelta is a number of seconds
    from datetime import timedelta

    forcing(state, out.u_dt, out.v_dt, out.pt_dt, timedelta(seconds=225))
    _sync(device)
    assert all(np.array_equal(host(out)[name], first[name]) for name in ("u_dt", "v_dt", "pt_dt"))
    # ---- pt = teq and no wind: nothing to relax
    state.pt.set(first["teq"])
    state.ua.set(zeros)
    state.va.set(zeros)
    forcing(state, out.u_dt, out.v_dt, out.pt_dt, 225.0)
    _sync(device)
    rest = host(out)
    assert (rest["u_dt"] == 0.0).all() and (rest["v_dt"] == 0.0).all()
    if lib.real_bytes == 8:
        assert (rest["pt_dt"] == 0.0).all()
    else:
        half = 0.5 * np.spacing(first["teq"][cs, cs, :NK]).astype(np.float64)
        assert (np.abs(rest["pt_dt"][cs, cs, :NK]) <= t["kt"] * half * (1.0 + 2.0 ** -22)).all()


def check_contraction(device):
    lib, env, forcing, state, out = setup(device, 0, constant_volume=False)
    assert forcing.heating_scale == 1.0
    h = host(state)
    s2, c2 = np.array(forcing.sin2lat.numpy()), np.array(forcing.cos2lat.numpy())
    cs = (slice(3, 3 + N), slice(3, 3 + N), slice(0, NK))
    for dt in (225.0, 1.0e6):
        forcing(state, out.u_dt, out.v_dt, out.pt_dt, dt, teq=out.teq)
        _sync(device)
        got = {name: a[cs] for name, a in host(out).items()}
        t = ref.terms(constants(forcing, dt), h["pe"], s2, c2, N, NK)
        for tendency, old, target, rate in (("pt_dt", h["pt"][cs], got["teq"], t["kt"]), ("u_dt", h["ua"][cs], 0.0, t["kv"]),
                                            ("v_dt", h["va"][cs], 0.0, t["kv"])):
            lhs = (old + dt * got[tendency]) - target
            rhs = (old - target) / (1.0 + rate * dt)
            bound = 2.0 * U * (np.abs(old) + 12.0 * np.abs(old - target))
            print(f"dt {dt:g} {tendency}: |lhs - rhs| at most {np.abs(lhs - rhs).max():.3e}, {(np.abs(lhs - rhs) / bound).max():.3f} of the bound")
            assert (np.abs(lhs - rhs) <= bound).all(), (dt, tendency, float((np.abs(lhs - rhs) / bound).max()))
            assert (np.abs(lhs) <= np.abs(old - target) + bound).all(), (dt, tendency)
        assert (t["kt"] * dt).max() > (2.0 if dt > 1e5 else 0.0)  # (1e6 s is past forward Euler's stability limit)


def check_refusals(device):
    from pace_amd.stencils import HeldSuarezConfig, HeldSuarezForcing

    assert HeldSuarezConfig() == HeldSuarezConfig(p0=1e5, kappa=ref.RDGAS / ref.CP_AIR, sigma_b=0.7, k_f=1 / 86400, k_a=1 / (40 * 86400),
                                                  k_s=1 / (4 * 86400), delta_t_y=60.0, delta_theta_z=10.0, t0=315.0, t_strat=200.0)
    for kw in (dict(sigma_b=-0.1), dict(sigma_b=1.0), dict(sigma_b=float("nan")), dict(p0=0.0), dict(p0=-1.0), dict(k_f=-1e-6),
               dict(k_a=float("inf")), dict(k_s=float("nan")), dict(t0="warm"), dict(sigma_b=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            HeldSuarezConfig(**kw)
    lib, env, forcing, state, out = setup(device, 0)
    with pytest.raises(ValueError, match="HeldSuarezConfig"):
        HeldSuarezForcing(env.stencil_factory, env.qf, env.grid_data, {"sigma_b": 0.7})
    with pytest.raises(ValueError, match="lat_agrid"):
        HeldSuarezForcing(env.stencil_factory, env.qf, types.SimpleNamespace())
    with pytest.raises(ValueError, match="lat_agrid"):
        HeldSuarezForcing(env.stencil_factory, env.qf, types.SimpleNamespace(lat_agrid=np.zeros((N, N))))
    lib.calls.clear()
    for dt in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="timestep"):
            forcing(state, out.u_dt, out.v_dt, out.pt_dt, dt)
    with pytest.raises(ValueError, match="3-D"):
        forcing(state, out.u_dt, out.v_dt, forcing.sin2lat, 225.0)
    with pytest.raises(ValueError, match="layout"):
        forcing(state, out.u_dt, out.v_dt, out.pt_dt.data.clone().contiguous(), 225.0)
    with pytest.raises(ValueError, match="needs every field"):
        forcing(state, out.u_dt, None, out.pt_dt, 225.0)
    assert lib.calls == []
    from pace_amd import _lib

    with pytest.raises(_lib.PaceError, match="invalid argument"):  # an output that is an input
        forcing(state, state.ua, out.v_dt, out.pt_dt, 225.0)


@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_operator_emulated(library):
    check_operator("cpu", library)


def test_contraction_emulated():
    check_contraction("cpu")


def test_refusals_emulated():
    check_refusals("cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_operator_on_the_gpu(library):
    check_operator("cuda", library)


@pytest.mark.gpu
def test_contraction_on_the_gpu():
    check_contraction("cuda")


@pytest.mark.gpu
def test_refusals_on_the_gpu():
    check_refusals("cuda")
