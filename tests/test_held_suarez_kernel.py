"""pace_held_suarez (pace_amd/csrc/k_heldsuarez.hip): the Held-Suarez forcing as one launch.

Every storage -- pe, ua, va, pt, the two planes, the three tendencies and teq -- is random-filled over its WHOLE base (row padding,
halo and level nk included); pe is physical on the compute domain (ps uniform in [95000, 103000], pe[k] = 300 + (ps - 300) *
(k / nk) ** 0.5), the latitudes are uniform in [-pi/2, pi/2], pt in [180, 320], the winds in [-50, 50].  The test asserts that
each side of both selects (the t_strat clamp, sigma above / below sigma_b) holds at least 5 % of the cells.

Shapes: C12 x 2, C13 x 7 (odd rows, misaligned row starts), C68 x 5 (rows longer than 64 lanes: a second, partly idle pass),
C12 x 19 (19, 7, 5 are primes and 2 is the smallest level count: for every level chunk > 1 one of them is no multiple of it; with
the chunk of 8 that is built, 19 = 8 + 8 + 3).

* u_dt, v_dt over their whole raw storages BIT FOR BIT against the numpy restatement (tests/held_suarez_reference.py): they involve
  no transcendental.  pt_dt likewise against the restatement fed with the DEVICE's teq, in the float64 library bit for bit.  In
  the float32 library the stored teq is the narrowed one while pt_dt was formed from the double: there the double lies within
  half a float32 ulp of the stored value, pt_dt as computed (every operation rounded) is a non-decreasing function of teq -- a
  difference, a product with kt >= 0, a quotient by 1 + kt dt > 0, a product with heating_scale >= 0, a negation, the sum with the
  old value and the narrowing are all monotone, and so is each one's rounding -- so the device's pt_dt must lie between the
  restatement's at teq - ulp32 / 2 and at teq + ulp32 / 2, both ends included, compared as stored float32 values.  Elements
  outside the compute domain's nk levels keep their random values; accumulate 0 and 1, teq given and NULL, dt 0 and 225,
  heating_scale 1 and CV_AIR / CP_AIR; the inputs are unchanged afterwards.
* teq against the restatement with numpy's log and exp, to a bound derived PER CELL.  With q = pm / p0 (the same correctly
  rounded operations on both sides), u(v) the spacing of doubles at |v| plus the error already carried, and the measured maxima of
  profiles/r06_transcendental_accuracy.txt (lean_log 0.546 ulp, lean_exp 0.548 ulp; glibc's, which numpy calls, 0.515 and 0.506):
      e_lp = (0.546 + 0.515) u(lp)                             both logarithms against the true one
      e_a  = kappa e_lp + u(a)                a = kappa * lp   two roundings of half an ulp each
      e_pk = pk expm1(e_a) + (0.548 + 0.506) u(pk)             the true exp is e_a-Lipschitz in relative terms
      e_b  = delta_theta_z e_lp + u(b)        b = delta_theta_z * lp
      e_m  = c2 e_b + u(m)                    m = b * c2
      e_d  = e_m + u(d)                       d = (t0 - delta_t_y * s2) - m      the minuend is the same on both sides
      e_x  = |d| e_pk + pk e_d + e_d e_pk + u(x)               x = d * pk
  and the clamp max(x, t_strat) is 1-Lipschitz, so |teq_device - teq_numpy| <= e_x in every cell.  For these inputs e_x is 2.5 to 5.3
  ulp of teq; the measured maximum is printed (DESIGN.md 4.23 records it).  A cell whose numpy x lies more than e_x below
  t_strat must be exactly t_strat, and no teq is below t_strat.  Float32 library: the narrowed values differ by at most one
  float32 ulp.
* a NaN planted in pt makes a NaN in that cell's pt_dt only; in one pe interface, NaN in the two layers that touch it; in ps, NaN
  in its whole column and nowhere else.
* every PACE_ERR_ARG of the header; the header against the binding.

Every check is a function of the device: the CPU tier calls it with the emulation libraries, the GPU tier with the product's."""
import ctypes as C
import dataclasses
import itertools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import ROOT, build_emu, build_emu_f32  # noqa: E402
import held_suarez_reference as ref  # noqa: E402

X, Y, Z = "x", "y", "z"
SHAPES = ((12, 2), (13, 7), (68, 5), (12, 19))
LOG_ULP, EXP_ULP, LIBM_LOG_ULP, LIBM_EXP_ULP = 0.546, 0.548, 0.515, 0.506  # profiles/r06_transcendental_accuracy.txt


def _libs(device):
    from pace_amd import _lib

    if device == "cpu":
        return [_lib.Library(build_emu()), _lib.Library(build_emu_f32())]
    return [_lib.load(), _lib.load(32)]


def _stream(device):
    if device == "cpu":
        return None
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same(got, want):
    """Bits where the expected value is no NaN, NaN-ness where it is."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


class Case:
    """The storages of one launch shape on the device, random-filled; `host` keeps what was stored, indexed [i, j, k]."""

    INPUTS = ("pe", "ua", "va", "pt", "s2", "c2")
    OUTPUTS = ("u_dt", "v_dt", "pt_dt", "teq")

    def __init__(self, lib, device, n, nk, seed):
        import torch

        from pace_amd import _launch
        from pace_amd.util import QuantityFactory, SubtileGridSizer

        self.lib, self.device, self.n, self.nk = lib, device, n, nk
        self.np_real = np.float32 if lib.real_bytes == 4 else np.float64
        factory = QuantityFactory(SubtileGridSizer(n, n, nk), device, torch.float32 if lib.real_bytes == 4 else torch.float64)
        rng = np.random.default_rng(seed)
        self.q = {name: factory.zeros([X, Y] if name in ("s2", "c2") else [X, Y, Z], "") for name in self.INPUTS + self.OUTPUTS}
        self.geom = _launch.geometry([self.q["pe"]], str, "")
        shape3 = tuple(self.q["pe"]._base.shape)[::-1]  # (padded row, n + 7, nk + 1)
        cs = slice(3, 3 + n)
        pe = rng.uniform(-300.0, 300.0, shape3)
        ps = rng.uniform(95000.0, 103000.0, (n, n, 1))
        pe[cs, cs, :] = 300.0 + (ps - 300.0) * (np.arange(nk + 1) / nk) ** 0.5
        lat = rng.uniform(-np.pi / 2, np.pi / 2, shape3[:2])
        values = dict(pe=pe, ua=rng.uniform(-50.0, 50.0, shape3), va=rng.uniform(-50.0, 50.0, shape3),
                      pt=rng.uniform(180.0, 320.0, shape3), s2=np.sin(lat) ** 2, c2=np.cos(lat) ** 2,
                      u_dt=rng.uniform(-1e-3, 1e-3, shape3), v_dt=rng.uniform(-1e-3, 1e-3, shape3),
                      pt_dt=rng.uniform(-1e-3, 1e-3, shape3), teq=rng.uniform(-300.0, 300.0, shape3))
        self.host = {}
        for name, a in values.items():
            self.put(name, a)

    def put(self, name, a):
        import torch

        a = np.ascontiguousarray(a.astype(self.np_real))
        self.q[name]._base.copy_(torch.as_tensor(np.ascontiguousarray(a.transpose(*range(a.ndim)[::-1]))))
        self.host[name] = a

    def raw(self, name):
        a = self.q[name]._base.detach().cpu().numpy().copy()
        return a.transpose(*range(a.ndim)[::-1])

    def config(self, c, accumulate):
        from pace_amd import _lib

        cfg = _lib.HeldSuarezConfig(struct_bytes=C.sizeof(_lib.HeldSuarezConfig), accumulate=accumulate)
        for f in dataclasses.fields(c):
            setattr(cfg, f.name, getattr(c, f.name))
        return cfg

    def launch(self, c, accumulate, with_teq=True):
        """The outputs refilled with what they held at first, then one launch. -> the four raw storages after it."""
        for name in self.OUTPUTS:
            self.put(name, self.host[name])
        cfg = self.config(c, accumulate)
        q = self.q
        self.lib.call("pace_held_suarez", C.byref(self.geom), C.byref(cfg), *[q[name].ptr for name in self.INPUTS],
                      q["u_dt"].ptr, q["v_dt"].ptr, q["pt_dt"].ptr, q["teq"].ptr if with_teq else None, _stream(self.device))
        if self.device != "cpu":
            import torch

            torch.cuda.synchronize()
        return {name: self.raw(name) for name in self.OUTPUTS}

    def expected(self, c, accumulate, with_teq, **given):
        h = self.host
        out = ref.held_suarez(c, h["pe"], h["ua"], h["va"], h["pt"], h["s2"], h["c2"], h["u_dt"], h["v_dt"], h["pt_dt"],
                              h["teq"] if with_teq else None, self.n, self.nk, accumulate, **given)
        return dict(zip(self.OUTPUTS, out))

    def window(self, a):
        return a[3:3 + self.n, 3:3 + self.n, :self.nk]

    def check(self, c, accumulate, with_teq, device_teq):
        """One launch against the restatement over the whole raw storages; device_teq: the teq storage of a launch with it."""
        got = self.launch(c, accumulate, with_teq)
        where = (self.n, self.nk, self.lib.real_bytes, c.dt, c.heating_scale, accumulate, with_teq)
        teq64 = self.window(device_teq).astype(np.float64)
        want = self.expected(c, accumulate, with_teq, teq=teq64)
        for name in ("u_dt", "v_dt"):
            assert same(got[name], want[name]), (name,) + where + (int((_bits(got[name]) != _bits(want[name])).sum()),)
        if self.lib.real_bytes == 8:
            assert same(got["pt_dt"], want["pt_dt"]), ("pt_dt",) + where + (int((_bits(got["pt_dt"]) != _bits(want["pt_dt"])).sum()),)
        else:  # (the module's docstring: monotone in teq, whose double lies within half a float32 ulp of the stored value)
            half = 0.5 * np.spacing(np.abs(self.window(device_teq))).astype(np.float64)
            lo = self.expected(c, accumulate, with_teq, teq=teq64 - half)["pt_dt"]
            hi = self.expected(c, accumulate, with_teq, teq=teq64 + half)["pt_dt"]
            nan = np.isnan(lo) | np.isnan(hi)
            assert np.array_equal(np.isnan(got["pt_dt"]), nan), ("pt_dt NaN",) + where
            outside = ~nan & ((got["pt_dt"] < lo) | (got["pt_dt"] > hi))
            assert not outside.any(), ("pt_dt",) + where + (int(outside.sum()),)
            untouched = np.ones(lo.shape, bool)
            self.window(untouched)[...] = False
            assert np.array_equal(_bits(got["pt_dt"])[untouched], _bits(self.host["pt_dt"])[untouched]), ("pt_dt outside",) + where
        if with_teq:
            assert np.array_equal(_bits(got["teq"]), _bits(device_teq)), ("teq",) + where  # the same bits in every launch
            assert same(got["teq"], want["teq"])  # ... and nothing outside the window
        else:
            assert np.array_equal(_bits(got["teq"]), _bits(self.host["teq"])), ("teq written",) + where
        for name in self.INPUTS:
            assert np.array_equal(_bits(self.raw(name)), _bits(self.host[name])), (name, "changed") + where
        return got


def teq_bound(c, t):
    """e_x of the module's docstring per cell, from the restatement's terms (numpy's log and exp)."""
    def u(v, carried=0.0):
        return np.spacing(np.abs(v) + carried)

    lp, pk, c2 = t["lp"], t["pk"], t["c2"]
    e_lp = (LOG_ULP + LIBM_LOG_ULP) * u(lp)
    a = c.kappa * lp
    e_a = c.kappa * e_lp + u(a, c.kappa * e_lp)
    e_pk = pk * np.expm1(e_a) + (EXP_ULP + LIBM_EXP_ULP) * u(pk, pk * np.expm1(e_a))
    b = c.delta_theta_z * lp
    e_b = c.delta_theta_z * e_lp + u(b, c.delta_theta_z * e_lp)
    m = b * c2
    e_m = c2 * e_b + u(m, c2 * e_b)
    d = (c.t0 - c.delta_t_y * t["s2"]) - m
    e_d = e_m + u(d, e_m)
    carried = np.abs(d) * e_pk + pk * e_d + e_d * e_pk
    return carried + u(t["x"], carried)


def check_kernel(device, only=None):
    worst = {}
    for which, lib in enumerate(_libs(device)):
        if only is not None and only != which:
            continue
        for seed, (n, nk) in enumerate(SHAPES):
            case = Case(lib, device, n, nk, 10 + seed)
            base = ref.Constants()
            t = ref.terms(base, case.host["pe"], case.host["s2"], case.host["c2"], n, nk)
            clamped, frictional = float((t["x"] < base.t_strat).mean()), float((t["hx"] > 0.0).mean())
            print(f"C{n} x {nk}: {clamped:.1%} of the cells on the t_strat clamp, {frictional:.1%} above sigma_b")
            assert 0.05 <= clamped <= 0.95 and 0.05 <= frictional <= 0.95, (n, nk, clamped, frictional)
            device_teq = case.launch(base, 0, True)["teq"]
            # ---- teq against numpy's log and exp
            got, want, bound = case.window(device_teq).astype(np.float64), t["teq"], teq_bound(base, t)
            if lib.real_bytes == 8:
                ulps = np.abs(got - want) / np.spacing(want)
                worst[(n, nk)] = float(ulps.max())
                print(f"  teq: at most {ulps.max():.3f} ulp from the restatement with numpy's log and exp; the derived bound is "
                      f"{(bound / np.spacing(want)).min():.2f} to {(bound / np.spacing(want)).max():.2f} ulp")
                assert (np.abs(got - want) <= bound).all(), (n, nk, float((np.abs(got - want) / bound).max()))
            else:
                want32 = want.astype(np.float32)
                assert (np.abs(got - want32.astype(np.float64)) <= np.spacing(want32).astype(np.float64)).all(), (n, nk)
            assert (got[t["x"] < base.t_strat - bound] == base.t_strat).all() and (got >= base.t_strat).all()
            if lib.real_bytes == 8:
                assert (got[t["x"] > base.t_strat + bound] > base.t_strat).all()
            # ---- the tendencies, every combination
            for dt, scale, accumulate, with_teq in itertools.product((0.0, 225.0), (1.0, ref.CV_AIR / ref.CP_AIR), (0, 1),
                                                                     (True, False)):
                case.check(dataclasses.replace(base, dt=dt, heating_scale=scale), accumulate, with_teq, device_teq)
    return worst


def check_specials(device, only=None):
    for which, lib in enumerate(_libs(device)):
        if only is not None and only != which:
            continue
        n, nk = 13, 7
        c = ref.Constants()
        cs = slice(3, 3 + n)
        plain = Case(lib, device, n, nk, 20)

        def planted(name, index):
            case = Case(lib, device, n, nk, 20)
            a = case.host[name].copy()
            a[index] = np.nan
            case.put(name, a)
            device_teq = case.launch(c, 0, True)["teq"]
            got = case.check(c, 1, True, device_teq)
            return {k: np.isnan(v) for k, v in got.items()}

        def only_at(mask, index):
            want = np.zeros(mask.shape, bool)
            want[index] = True
            return np.array_equal(mask, want)

        assert not any(np.isnan(v).any() for v in plain.launch(c, 0, True).values())
        # pt: that cell's pt_dt only
        nan = planted("pt", (3 + 5, 3 + 11, 4))
        assert only_at(nan["pt_dt"], (3 + 5, 3 + 11, 4)) and not (nan["u_dt"].any() or nan["v_dt"].any() or nan["teq"].any())
        # one pe interface: the two layers that touch it, in everything
        nan = planted("pe", (3 + 12, 3 + 0, 3))
        for name in Case.OUTPUTS:
            assert only_at(nan[name], (3 + 12, 3 + 0, slice(2, 4))), name
        # ps: its whole column of the tendencies (teq does not read ps, but ps is also the lowest layer's lower interface)
        nan = planted("pe", (3 + 0, 3 + 12, nk))
        for name in ("u_dt", "v_dt", "pt_dt"):
            assert only_at(nan[name], (3 + 0, 3 + 12, slice(0, nk))), name
        assert only_at(nan["teq"], (3 + 0, 3 + 12, nk - 1))
        # a NaN outside the compute domain -- halo, row padding, level nk of the layer fields -- reaches nothing
        case = Case(lib, device, n, nk, 20)
        for name in ("ua", "va", "pt", "pe", "s2", "c2"):
            a = np.full(case.host[name].shape, np.nan, case.np_real)
            a[cs, cs] = case.host[name][cs, cs]
            if name in ("ua", "va", "pt"):
                a[:, :, nk] = np.nan
            case.put(name, a)
        got = case.launch(c, 0, True)
        assert all(np.array_equal(_bits(got[name]), _bits(plain.launch(c, 0, True)[name])) for name in Case.OUTPUTS)


def check_refusals(device):
    from pace_amd import _lib

    lib = _libs(device)[0]
    case = Case(lib, device, 12, 5, 30)
    c = ref.Constants()
    q = case.q
    names = Case.INPUTS + Case.OUTPUTS

    def call(geom=case.geom, cfg=None, **kw):
        cfg = case.config(c, 1) if cfg is None else cfg
        for key in [k for k in kw if k not in names]:
            setattr(cfg, key, kw.pop(key))
        pointers = [kw.get(name, q[name].ptr) for name in names]
        lib.call("pace_held_suarez", None if geom is None else C.byref(geom), None if cfg is False else C.byref(cfg), *pointers,
                 _stream(device))

    inf, nan = float("inf"), float("nan")
    bad = [dict(geom=None), dict(cfg=False)]
    bad += [{name: None} for name in names if name != "teq"]
    bad += [dict(struct_bytes=0), dict(struct_bytes=C.sizeof(_lib.HeldSuarezConfig) - 8), dict(struct_bytes=C.sizeof(_lib.HeldSuarezConfig) + 8)]
    bad += [dict(dt=-1.0), dict(dt=inf), dict(dt=nan)]
    bad += [dict(sigma_b=-0.1), dict(sigma_b=1.0), dict(sigma_b=1.5), dict(sigma_b=nan)]
    bad += [dict(p0=0.0), dict(p0=-1.0e5), dict(p0=nan)]
    bad += [{rate: value} for rate in ("k_f", "k_a", "k_s") for value in (-1.0e-6, inf, nan)]
    bad += [dict(accumulate=2), dict(accumulate=-1)]
    bad += [{out: q[other].ptr} for out in Case.OUTPUTS for other in names if other != out]  # an output is an input or another output
    for kw in bad:
        with pytest.raises(_lib.PaceError, match="invalid argument"):
            call(**kw)
    if device != "cpu":
        import torch

        torch.cuda.synchronize()
    for name in names:  # nothing is written on error
        assert np.array_equal(_bits(case.raw(name)), _bits(case.host[name])), name
    # what is accepted: teq NULL, dt 0, sigma_b 0, rates 0, two inputs that are one array
    call(teq=None, dt=0.0, sigma_b=0.0, k_f=0.0, k_a=0.0, k_s=0.0, va=q["ua"].ptr)
    if device != "cpu":
        import torch

        torch.cuda.synchronize()


@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_kernel_against_numpy_emulated(library):
    check_kernel("cpu", library)


@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_specials_emulated(library):
    check_specials("cpu", library)


def test_refusals_emulated():
    check_refusals("cpu")


def test_header_and_binding_agree_on_the_entry_point():
    from pace_amd import _lib

    text = open(os.path.join(ROOT, "include", "pace_hip.h")).read()
    declared = set(re.findall(r"\b(pace_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert set(_lib.EXPORTED_SYMBOLS) <= declared and "pace_held_suarez" in _lib.EXPORTED_SYMBOLS
    proto = re.search(r"\bint pace_held_suarez\s*\(([^;]*)\);", text).group(1)
    assert len(proto.split(",")) == len(_lib._PROTOS["pace_held_suarez"][1]) == 13
    body = re.search(r"typedef struct \{([^}]*)\} pace_held_suarez_config_t;", text).group(1)
    fields = re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", body))
    assert fields == [name for name, _ in _lib.HeldSuarezConfig._fields_]
    assert C.sizeof(_lib.HeldSuarezConfig) == 8 + 12 * 8 and _lib.HeldSuarezConfig.dt.offset == 8
    assert [name for name, _ in _lib.HeldSuarezConfig._fields_][2:] == [f.name for f in dataclasses.fields(ref.Constants)]


@pytest.mark.gpu
@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_kernel_against_numpy_on_the_gpu(library):
    check_kernel("cuda", library)


@pytest.mark.gpu
@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_specials_on_the_gpu(library):
    check_specials("cuda", library)


@pytest.mark.gpu
def test_refusals_on_the_gpu():
    check_refusals("cuda")
