"""pace_amd.fv3core.RayleighSuper on a C12 x 19 state (tile 0 of the C12 grid: tests/golden/grid_c12_tile0.npz, whose ptop is 300 Pa
and whose first 19 levels reach 9.2 hPa; rf_cutoff = 3000 Pa damps the first seven).

* factors(dt) against a scalar restatement with the math module (tests/rayleigh_reference.py): entries exactly 1.0 where
  pfull >= rf_cutoff; elsewhere rf (rates(dt)) agrees to a relative 1e-12 and f is exactly 1 / (1 + rf) (check_factors has the derivation); the table is formed
  once per dt and is read-only;
* one call is one pace_rayleigh_super -- in the emulation's launch log two kernels with conserve, one without, none when no level
  lies above rf_cutoff -- and nothing else: no other entry point, no upload, no host copy of a device field after construction;
* the result is the restatement's, bit for bit, over the raw storages;
* the refusals: hydrostatic, tau <= 0, rf_cutoff <= ptop, a dt that is negative or not finite, a field of another layout.

Every check is a function of the device: the CPU tier calls it with the emulation libraries, the GPU tier with the product's."""
import contextlib
import math
import os
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import ROOT, build_emu, build_emu_f32  # noqa: E402
import rayleigh_reference as ref  # noqa: E402

N, NK = 12, 19
RF_CUTOFF, TAU, DT = 3000.0, 10.0, 225.0
PLANES = ("dx", "dy", "a11", "a12", "a21", "a22")


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


@contextlib.contextmanager
def launch_log(device, out):
    """The emulation names every kernel launch on stderr while PACE_EMU_LAUNCH_LOG is set: out receives the names."""
    if device != "cpu":
        yield
        return
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+") as f:
        os.dup2(f.fileno(), 2)
        os.environ["PACE_EMU_LAUNCH_LOG"] = "1"
        try:
            yield
        finally:
            del os.environ["PACE_EMU_LAUNCH_LOG"]
            os.dup2(saved, 2)
            os.close(saved)
            f.seek(0)
            out.extend(line.split()[2] for line in f if line.startswith("[emu launch]"))


def setup(device, which, **kw):
    from pace_amd.fv3core import RayleighSuper
    from pace_amd.tile import Env

    lib = SpyLib(_lib(device, which))
    metrics = dict(np.load(os.path.join(ROOT, "tests", "golden", "grid_c12_tile0.npz"), allow_pickle=False))
    env = Env(lib, device, metrics, N, NK)
    args = dict(rf_cutoff=RF_CUTOFF, tau=TAU, ptop=env.grid_data.ptop)
    args.update(kw)
    damping = RayleighSuper(env.stencil_factory, env.qf, env.grid_data, **args)
    rng = np.random.default_rng(4)
    shape = (N + 7, N + 7, NK + 1)
    values = dict(u=rng.uniform(-50.0, 50.0, shape), v=rng.uniform(-50.0, 50.0, shape), w=rng.uniform(-5.0, 5.0, shape),
                  pt=rng.uniform(180.0, 320.0, shape))
    fields = {name: env.q3(a) for name, a in values.items()}
    return lib, env, damping, fields


def raw(q):
    a = q._base.detach().cpu().numpy().copy()
    return a.transpose(*range(a.ndim)[::-1])


def check_factors(device):
    """rf = c * sin(x) ** 2 with c = dt / tau0 and x = 0.5 * pi * log(q) / log(q0), q = rf_cutoff / pfull, q0 = rf_cutoff / ptop.
    Both sides form q, q0, c and the products and quotients by the same correctly rounded operations on the same numbers; they
    differ only in log and sin, numpy's against the math module's, each within about 1 ulp of the true value.  A relative
    perturbation e of log(q) is a relative e of x; d ln(sin(x) ** 2) / d ln(x) = 2 x cot(x), at most 2 in magnitude on (0, pi / 2].
    So rf differs by at most 2 * (2 * 1 ulp for the two logarithms + roundings) + 2 * 1 ulp for the sine: some 10 ulp = 1e-15;
    the conditioning of log(q) in q (1 / log(q), large only as pfull -> rf_cutoff, where rf -> 0) does not enter, since q is the same
    number on both sides.  1e-12 leaves three orders of magnitude and still catches a wrong constant, level or formula.  rf is
    compared as rates(dt) gives it; factors(dt) is exactly 1.0 / (1.0 + rf) of it."""
    lib, env, damping, _ = setup(device, 0)
    pfull = np.asarray(env.grid_data.p, dtype=np.float64)[:NK]
    ptop = float(env.grid_data.ptop)
    assert ptop == 300.0 and (pfull < RF_CUTOFF).sum() == 7 and (np.diff(pfull) > 0).all()
    for dt in (DT, 1800.0, 0.0):
        table = damping.factors(dt)
        want_f, want_rf, kmax = ref.factors(list(pfull), dt, TAU, RF_CUTOFF, ptop)
        assert table.dtype == np.float64 and table.shape == (NK,) and kmax == 7
        assert (table[kmax:] == 1.0).all() and not table.flags.writeable
        assert damping.factors(dt) is table  # formed once
        rf = damping.rates(dt)
        assert rf.shape == (NK,) and (rf[kmax:] == 0.0).all() and np.array_equal(table, 1.0 / (1.0 + rf))
        for k in range(kmax):
            assert table[k] == 1.0 / (1.0 + rf[k])
            if dt > 0.0:
                assert 0.0 < table[k] < 1.0 and want_rf[k] > 0.0
                assert abs(rf[k] - want_rf[k]) <= 1e-12 * want_rf[k], (dt, k, rf[k], want_rf[k])
            else:
                assert table[k] == 1.0 and rf[k] == 0.0
        if dt > 0.0:
            assert (np.diff(table[:kmax]) > 0).all()  # the damping weakens toward rf_cutoff
    # at the model top sin ** 2 is nearly 1: rf = dt / tau0 there
    assert abs(1.0 / damping.factors(DT)[0] - 1.0 - DT / (TAU * 86400.0)) < 0.2 * DT / (TAU * 86400.0)
    assert lib.calls == []
    # rf_cutoff above every level: all damped; below the first level: none
    _, _, everything, _ = setup(device, 0, rf_cutoff=1.0e5)
    assert (everything.factors(DT) < 1.0).all()
    _, _, nothing, _ = setup(device, 0, rf_cutoff=400.0)
    assert (nothing.factors(DT) == 1.0).all()


def check_operator(device, which):
    from pace_amd import _launch
    from pace_amd.fv3core.stencils import rayleigh_super as _common

    for conserve in (True, False):
        lib, env, damping, fields = setup(device, which, conserve=conserve)
        _sync(device)
        before = {name: raw(q) for name, q in fields.items()}
        planes = [raw(getattr(env.grid_data, name)) for name in PLANES]
        uploads, copies, kernels = [], [], []
        real_upload, real_column = _launch.upload_table, _common.host_column
        _launch.upload_table = lambda *a, **k: (uploads.append(1), real_upload(*a, **k))[1]
        _common.host_column = lambda *a, **k: (copies.append(1), real_column(*a, **k))[1]
        try:
            lib.calls.clear()
            with launch_log(device, kernels):
                damping(fields["u"], fields["v"], fields["w"], fields["pt"], DT)
                _sync(device)
        finally:
            _launch.upload_table, _common.host_column = real_upload, real_column
        assert lib.calls == ["pace_rayleigh_super"] and uploads == [] and copies == []
        if device == "cpu":
            assert kernels == (["k_rayleigh_heat", "k_rayleigh_scale<false>"] if conserve else ["k_rayleigh_scale<true>"]), kernels
        after = {name: raw(q) for name, q in fields.items()}
        want = ref.rayleigh_super(before["u"], before["v"], before["w"], before["pt"], *planes, damping.factors(DT), N,
                                  conserve=conserve)
        for name, expected in zip(("u", "v", "w", "pt"), want):
            assert np.array_equal(after[name], expected), (name, conserve)
        cs = slice(3, 3 + N)
        # (float32: next to rf_cutoff f is within half a float32 ulp of 1 and f * u rounds back to u)
        assert (after["u"][cs, 3:4 + N, :6] != before["u"][cs, 3:4 + N, :6]).all()
        assert ((after["pt"][cs, cs, :3] > before["pt"][cs, cs, :3]).mean() > 0.8) == conserve  # (float32: a small heat rounds away)
        assert (after["pt"] >= before["pt"]).all()
        for name, plane in zip(PLANES, planes):
            assert np.array_equal(raw(getattr(env.grid_data, name)), plane), name
    # no level above rf_cutoff: the entry point is called, nothing is launched, nothing moves
    lib, env, damping, fields = setup(device, which, rf_cutoff=400.0)
    before = {name: raw(q) for name, q in fields.items()}
    kernels = []
    with launch_log(device, kernels):
        damping(fields["u"], fields["v"], fields["w"], fields["pt"], DT)
        _sync(device)
    assert kernels == [] and all(np.array_equal(raw(q), before[name]) for name, q in fields.items())


def check_refusals(device):
    from pace_amd.fv3core import RayleighSuper

    lib, env, damping, fields = setup(device, 0)
    make = lambda **kw: RayleighSuper(env.stencil_factory, env.qf, env.grid_data,  # noqa: E731
                                      **dict(dict(rf_cutoff=RF_CUTOFF, tau=TAU, ptop=300.0), **kw))
    with pytest.raises(NotImplementedError, match="hydrostatic"):
        make(hydrostatic=True)
    for tau in (0.0, -10.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tau"):
            make(tau=tau)
    for cutoff in (300.0, 100.0, float("nan")):
        with pytest.raises(ValueError, match="rf_cutoff"):
            make(rf_cutoff=cutoff)
    with pytest.raises(ValueError, match="rf_cutoff"):
        make(ptop=0.0)
    lib.calls.clear()
    for dt in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="timestep"):
            damping(fields["u"], fields["v"], fields["w"], fields["pt"], dt)
    with pytest.raises(ValueError, match="layout"):
        damping(fields["u"], fields["v"], fields["w"], fields["pt"].data.clone().contiguous(), DT)
    assert lib.calls == []
    from pace_amd import _lib

    with pytest.raises(_lib.PaceError, match="invalid argument"):  # two of the four are one array
        damping(fields["u"], fields["u"], fields["w"], fields["pt"], DT)
    assert math.isclose(damping._rcv, ref.RCV, rel_tol=0, abs_tol=0)


def test_factors_emulated():
    check_factors("cpu")


@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_operator_emulated(library):
    check_operator("cpu", library)


def test_refusals_emulated():
    check_refusals("cpu")


@pytest.mark.gpu
def test_factors_on_the_gpu():
    check_factors("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_operator_on_the_gpu(library):
    check_operator("cuda", library)


@pytest.mark.gpu
def test_refusals_on_the_gpu():
    check_refusals("cuda")
