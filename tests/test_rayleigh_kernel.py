"""pace_rayleigh_super (pace_amd/csrc/k_rayleigh.hip): the rf_fast = false sponge damping, heat launch then wind launch.

Every storage -- u, v, w, pt and the six metric planes -- is filled over its WHOLE base (row padding, halo and level nk included).
Inside the windows the kernel may read (u on (n, n + 1) points, v on (n + 1, n), w and pt on (n, n), the planes on (n + 1, n + 1),
levels < kmax) the values are physical: winds in [-50, 50], w in [-5, 5], pt in [180, 320], dx, dy in [1e4, 2e4], a11 .. a22 in
[-1, 1].  Everywhere else -- the halo, the row padding, level nk, the levels from kmax on, u beyond row n + 1, v beyond column n + 1 --
the "hostile" fill puts a NaN or a huge finite number (1e300; float32: 1e38), half and half: a read there turns a result into a NaN
or an infinity, a write there changes a finite sentinel.

Shapes: C12 x 2, C13 x 7 (odd width, misaligned row starts), C68 x 5 (two 64-lane segments and a partial row group), C12 x 19
(19 = 4 level chunks of 4 and one of 3).  Factor tables: kmax 0 (every factor 1.0), 1, partial (about nk / 2) and nk, conserve 0
and 1, both libraries.

* the whole raw storage of u, v, w, pt BIT FOR BIT against the sequential restatement (tests/rayleigh_reference.py); the metric
  planes are unchanged; a second run from the same inputs gives the same bits;
* f == 1.0 on every level leaves every bit alone;
* one NaN in u inside the window reaches exactly the two adjacent cells' pt and its own u;
* every PACE_ERR_ARG of the header, and the buffers are untouched after all of them;
* the restatement's ua / va are oracle.dycore_parts.c2l_ord2's, bit for bit;
* the invariant: pace_c2l_ord order 2 on the winds before and after; per cell (pt_new - pt_old) / rcv + 0.5 * (KE_new - KE_old)
  against a bound counted from the roundings (check_invariant's docstring).

Every check is a function of the device: the CPU tier calls it with the emulation libraries, the GPU tier with the product's."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import ROOT, build_emu, build_emu_f32  # noqa: E402
import rayleigh_reference as ref  # noqa: E402

X, Y, Z = "x", "y", "z"
SHAPES = ((12, 2), (13, 7), (68, 5), (12, 19))
PLANES = ("dx", "dy", "a11", "a12", "a21", "a22")
FIELDS = ("u", "v", "w", "pt")
U64, U32 = 2.0 ** -53, 2.0 ** -24


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


def _sync(device):
    if device != "cpu":
        import torch

        torch.cuda.synchronize()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same(got, want):
    """Bits where the expected value is no NaN, NaN-ness where it is."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def table(nk, kmax, seed=0):
    f = np.ones(nk)
    f[:kmax] = np.sort(np.random.default_rng(100 + seed).uniform(0.5, 0.999, kmax))
    return f


class Case:
    """The storages of one shape on the device; `host` keeps what was stored, indexed [i, j, k].  kmax: the levels whose windows
    hold physical values; hostile: NaN / huge outside the windows, otherwise physical values everywhere; positive: winds and
    a11 .. a22 all positive (no cancellation in the A-grid winds)."""

    def __init__(self, lib, device, n, nk, seed, kmax=None, hostile=True, positive=False, pt0=None):
        import torch

        from pace_amd import _launch, _lib
        from pace_amd.util import QuantityFactory, SubtileGridSizer

        self.lib, self.device, self.n, self.nk = lib, device, n, nk
        self.np_real = np.float32 if lib.real_bytes == 4 else np.float64
        factory = QuantityFactory(SubtileGridSizer(n, n, nk), device, torch.float32 if lib.real_bytes == 4 else torch.float64)
        rng = np.random.default_rng(seed)
        self.q = {name: factory.zeros([X, Y] if name in PLANES else [X, Y, Z], "") for name in PLANES + FIELDS}
        self.geom = _launch.geometry([self.q["u"]], str, "")
        shape3 = tuple(self.q["u"]._base.shape)[::-1]  # (padded row, n + 7, nk + 1)
        shape2 = shape3[:2]
        lo = 10.0 if positive else -50.0
        values = dict(u=rng.uniform(lo, 50.0, shape3), v=rng.uniform(lo, 50.0, shape3), w=rng.uniform(-5.0, 5.0, shape3),
                      pt=rng.uniform(180.0, 320.0, shape3) if pt0 is None else np.full(shape3, pt0),
                      dx=rng.uniform(1.0e4, 2.0e4, shape2), dy=rng.uniform(1.0e4, 2.0e4, shape2))
        for name in PLANES[2:]:
            values[name] = rng.uniform(0.5 if positive else -1.0, 1.0, shape2)
        if hostile:
            huge = 1.0e38 if lib.real_bytes == 4 else 1.0e300
            kmax = nk if kmax is None else kmax
            cs, st = slice(3, 3 + n), slice(3, 3 + n + 1)
            windows = dict(u=(cs, st), v=(st, cs), w=(cs, cs), pt=(cs, cs), dx=(cs, st), dy=(st, cs))
            for name, a in values.items():
                inside = np.zeros(a.shape, bool)
                if a.ndim == 3:
                    inside[windows[name] + (slice(0, kmax),)] = True
                else:
                    inside[windows.get(name, (cs, cs))] = True
                bad = np.where(rng.uniform(size=a.shape) < 0.5, np.nan, huge * rng.uniform(0.5, 1.0, a.shape) * rng.choice([-1.0, 1.0], a.shape))
                values[name] = np.where(inside, a, bad)
        self.host = {}
        for name, a in values.items():
            self.put(name, a)
        self.metrics = _lib.Metrics()
        self.metrics.dx, self.metrics.dy = self.q["dx"].ptr, self.q["dy"].ptr

    def put(self, name, a):
        import torch

        a = np.ascontiguousarray(a.astype(self.np_real))
        self.q[name]._base.copy_(torch.as_tensor(np.ascontiguousarray(a.transpose(*range(a.ndim)[::-1]))))
        self.host[name] = a

    def raw(self, name):
        a = self.q[name]._base.detach().cpu().numpy().copy()
        return a.transpose(*range(a.ndim)[::-1])

    def call(self, factor, conserve=1, rcv=ref.RCV, geom=True, met=True, **pointers):
        factor = None if factor is None else np.ascontiguousarray(factor, dtype=np.float64)
        args = [pointers.get(name, self.q[name].ptr) for name in PLANES[2:] + FIELDS]
        self.lib.call("pace_rayleigh_super", C.byref(self.geom) if geom else None, C.byref(self.metrics) if met else None, *args,
                      None if factor is None else factor.ctypes.data_as(C.POINTER(C.c_double)), rcv, conserve, _stream(self.device))
        _sync(self.device)

    def launch(self, factor, conserve=1):
        """The four fields refilled with what they held at first, then one call. -> their raw storages after it."""
        for name in FIELDS:
            self.put(name, self.host[name])
        self.call(factor, conserve)
        return {name: self.raw(name) for name in FIELDS}

    def expected(self, factor, conserve=1):
        h = self.host
        out = ref.rayleigh_super(h["u"], h["v"], h["w"], h["pt"], *[h[name] for name in PLANES], factor, self.n, conserve=bool(conserve))
        return dict(zip(FIELDS, out))

    def changed(self, names=PLANES + FIELDS):
        return [name for name in names if not np.array_equal(_bits(self.raw(name)), _bits(self.host[name]))]


def check_kernel(device, only=None):
    for which, lib in enumerate(_libs(device)):
        if only is not None and only != which:
            continue
        for seed, (n, nk) in enumerate(SHAPES):
            for kmax in sorted({0, 1, (nk + 1) // 2, nk}):
                case = Case(lib, device, n, nk, 10 + seed, kmax=kmax)
                factor = table(nk, kmax, seed)
                for conserve in (1, 0):
                    where = (n, nk, kmax, conserve, lib.real_bytes)
                    got, want = case.launch(factor, conserve), case.expected(factor, conserve)
                    for name in FIELDS:
                        assert same(got[name], want[name]), (name,) + where + (int((_bits(got[name]) != _bits(want[name])).sum()),)
                        touched = _bits(got[name]) != _bits(case.host[name])
                        assert not touched[:, :, kmax:].any(), (name, "level >= kmax") + where
                    if kmax > 0:  # the windows hold finite results, and something moved
                        cs = slice(3, 3 + n)
                        assert np.isfinite(got["pt"][cs, cs, :kmax]).all() and np.isfinite(got["u"][cs, 3:4 + n, :kmax]).all()
                        assert (got["u"][cs, 3:4 + n, :kmax] != case.host["u"][cs, 3:4 + n, :kmax]).all()
                        assert (got["v"][3:4 + n, cs, :kmax] != case.host["v"][3:4 + n, cs, :kmax]).all()
                        assert (got["pt"][cs, cs, :kmax] > case.host["pt"][cs, cs, :kmax]).mean() > (0.9 if conserve else -1)
                        if not conserve:
                            assert np.array_equal(_bits(got["pt"]), _bits(case.host["pt"]))
                    else:
                        assert all(np.array_equal(_bits(got[name]), _bits(case.host[name])) for name in FIELDS), where
                    assert case.changed(PLANES) == [], where
                    again = case.launch(factor, conserve)
                    assert all(np.array_equal(_bits(again[name]), _bits(got[name])) for name in FIELDS), ("second run",) + where


def check_specials(device, only=None):
    for which, lib in enumerate(_libs(device)):
        if only is not None and only != which:
            continue
        n, nk, kmax = 13, 7, 4
        factor = table(nk, kmax)
        plain = Case(lib, device, n, nk, 20, hostile=False)
        base = plain.launch(factor)
        assert all(np.isfinite(a).all() for a in base.values())
        # one NaN in u inside the window: the two cells that share the face, and itself
        for (i, j, k) in ((3 + 5, 3 + 6, 2), (3 + 0, 3 + 12, 0), (3 + 12, 3 + 1, 3)):
            case = Case(lib, device, n, nk, 20, hostile=False)
            a = case.host["u"].copy()
            a[i, j, k] = np.nan
            case.put("u", a)
            got, want = case.launch(factor), case.expected(factor)
            for name in FIELDS:
                assert same(got[name], want[name]), name
            nan_pt = np.zeros(a.shape, bool)
            nan_pt[i, j, k] = nan_pt[i, j - 1, k] = True
            nan_u = np.zeros(a.shape, bool)
            nan_u[i, j, k] = True
            assert np.array_equal(np.isnan(got["pt"]), nan_pt) and np.array_equal(np.isnan(got["u"]), nan_u)
            assert not np.isnan(got["v"]).any() and not np.isnan(got["w"]).any()
        # the last row of u (j = n) belongs to one cell only; a NaN in v's last column likewise
        case = Case(lib, device, n, nk, 20, hostile=False)
        a, b = case.host["u"].copy(), case.host["v"].copy()
        a[3 + 4, 3 + n, 1] = np.nan
        b[3 + n, 3 + 7, 1] = np.nan
        case.put("u", a)
        case.put("v", b)
        got = case.launch(factor)
        nan_pt = np.zeros(a.shape, bool)
        nan_pt[3 + 4, 3 + n - 1, 1] = nan_pt[3 + n - 1, 3 + 7, 1] = True
        assert np.array_equal(np.isnan(got["pt"]), nan_pt)
        assert int(np.isnan(got["u"]).sum()) == 1 and int(np.isnan(got["v"]).sum()) == 1
        # a NaN one place outside the windows reaches nothing: u in row n + 2, v in column n + 2, level kmax, the halo
        case = Case(lib, device, n, nk, 20, hostile=False)
        for name, index in (("u", (3 + 4, 3 + n + 1, 1)), ("v", (3 + n + 1, 3 + 7, 1)), ("u", (3 + 4, 3 + 4, kmax)),
                            ("w", (2, 3 + 4, 0)), ("pt", (3 + 4, 2, 0)), ("v", (3 + 4, 3 + n, 0)), ("u", (3 + n, 3 + 4, 0))):
            a = case.host[name].copy()
            a[index] = np.nan
            case.put(name, a)
        got = case.launch(factor)
        for name in FIELDS:
            finite = ~np.isnan(case.host[name])
            assert np.array_equal(_bits(got[name])[finite], _bits(base[name])[finite]), name
            assert np.array_equal(np.isnan(got[name]), ~finite), name
        # f == 1.0 on every level: every bit stays
        hostile = Case(lib, device, n, nk, 21)
        for conserve in (0, 1):
            got = hostile.launch(np.ones(nk), conserve)
            assert all(np.array_equal(_bits(got[name]), _bits(hostile.host[name])) for name in FIELDS)


def check_restatement_against_the_oracle():
    """The restatement's ua / va are oracle.dycore_parts.c2l_ord2's on the compute domain, bit for bit."""
    sys.path.insert(0, ROOT)
    from oracle import dycore_parts

    n, nk = 13, 3
    rng = np.random.default_rng(5)
    shape = (n + 7, n + 7, nk + 1)
    u, v = rng.uniform(-50, 50, shape), rng.uniform(-50, 50, shape)
    planes = [rng.uniform(1e4, 2e4, shape[:2]), rng.uniform(1e4, 2e4, shape[:2])] + [rng.uniform(-1, 1, shape[:2]) for _ in range(4)]
    ua, va = dycore_parts.c2l_ord2(u, v, *planes, n, nk)
    cs = slice(3, 3 + n)
    for k in range(nk):
        mine = ref.a_grid_winds(u, v, *planes, n, k)
        assert np.array_equal(_bits(mine[0]), _bits(ua[cs, cs, k])) and np.array_equal(_bits(mine[1]), _bits(va[cs, cs, k]))


def check_invariant(device, only=None):
    """Energy: what the winds lose the temperature gains.  With every wind, a11 .. a22, dx and dy positive no sum in the A-grid winds
    cancels, so every computed quantity carries a RELATIVE error; u = 2 ** -53, first order, K = the exact KE_old of the stored inputs:

      ua (k_c2l<2>, also the heat kernel's): wu = u * dx (1), wu0 + wu1 (1), dx0 + dx1 (1), the quotient (1), 2.0 * exact:
          u1 within 4 u; a11 * u1 (1), the sum (1): ua within 6 u.
      KE_old = (ua * ua + va * va) + w * w: the squares 2 * 6 + 1 = 13 u, their sum 14 u, w * w 1 u, the sum 15 u.
      the heat: g = 1.0 - f * f carries at most u * (f * f + g) <= u absolute; H = ((0.5 * KE_old) * g) * rcv two roundings; the test
          divides pt_new - pt_old by rcv (1).  With pt_old = 0 the sum pt_old + H and the difference are exact, so
          A = (pt_new - pt_old) / rcv = 0.5 * KE_old * (1 - f * f) within 0.5 * K * (1 + 3 g) u <= 2 u K.
      the new winds f * u (1 each): their exact A-grid winds are f * ua within u, computed 7 u; KE_new = f * f * K within
          2 * 7 + 1 + 1 = 16 u for the winds' part, 2 * 1 + 1 = 3 u for w's, the sum 17 u.
      D = A + 0.5 * (KE_new - KE_old): exactly 0.5 * f * f * K * (theta_new - theta_old) <= 0.5 * (17 + 15) u K = 16 u K, plus A's
          2 u K, plus the test's difference KE_new - KE_old (1, of at most K, halved): 0.5 u K.  The final sum's rounding is u * |D|.

    |D| <= 18.5 u K, asserted as 19 u KE_old (the second-order terms, about 300 u * u K, sit in the half u).  The float32 library
    narrows the new winds and w (KE_new: 2 s, s = 2 ** -24), pace_c2l_ord's outputs (KE_old and KE_new: 2 s each) and pt_new (A: s):
    0.5 * (2 + 2) s K + 0.5 * 2 s K + 0.5 s K = 3.5 s K more, asserted as 19 u + 4 s.

    With a physical pt_old the sum pt_old + H is rounded once more -- at most the storage's unit roundoff times |pt_new|, divided by
    rcv; the difference of two temperatures within a factor of two of each other is exact -- and the bound gains exactly that
    term, which is no multiple of KE_old."""
    for which, lib in enumerate(_libs(device)):
        if only is not None and only != which:
            continue
        s = U32 if lib.real_bytes == 4 else 0.0
        for seed, (n, nk) in enumerate(SHAPES):
            for pt0 in (0.0, None):
                case = Case(lib, device, n, nk, 40 + seed, hostile=False, positive=True, pt0=pt0)
                factor = table(nk, nk, seed)
                import torch

                from pace_amd.util import QuantityFactory, SubtileGridSizer

                qf = QuantityFactory(SubtileGridSizer(n, n, nk), device, torch.float32 if lib.real_bytes == 4 else torch.float64)
                ua, va = qf.zeros([X, Y, Z], ""), qf.zeros([X, Y, Z], "")
                cs = (slice(3, 3 + n), slice(3, 3 + n), slice(0, nk))

                def kinetic():
                    lib.call("pace_c2l_ord", C.byref(case.geom), C.byref(case.metrics), 2, case.q["u"].ptr, case.q["v"].ptr,
                             *[case.q[name].ptr for name in PLANES[2:]], ua.ptr, va.ptr, _stream(device))
                    _sync(device)
                    a, b, w = (np.array(x.numpy())[cs].astype(np.float64) for x in (ua, va, case.q["w"]))
                    return (a * a + b * b) + w * w

                ke_old = kinetic()
                pt_old = case.host["pt"][cs].astype(np.float64)
                case.call(factor)
                ke_new = kinetic()
                pt_new = case.raw("pt")[cs].astype(np.float64)
                d = (pt_new - pt_old) / ref.RCV + 0.5 * (ke_new - ke_old)
                bound = (19.0 * U64 + 4.0 * s) * ke_old
                if pt0 is None:
                    bound = bound + (s if s else U64) * np.abs(pt_new) / ref.RCV
                print(f"C{n} x {nk}, {lib.real_bytes}-byte reals, pt_old {'0' if pt0 == 0.0 else 'physical'}: |D| at most "
                      f"{np.abs(d).max():.3e}, {(np.abs(d) / bound).max():.3f} of the bound")
                assert (ke_new < ke_old).all() and (pt_new > pt_old).all()
                assert (np.abs(d) <= bound).all(), (n, nk, lib.real_bytes, pt0, float((np.abs(d) / bound).max()))


def check_refusals(device):
    from pace_amd import _lib

    lib = _libs(device)[0]
    n, nk = 12, 5
    case = Case(lib, device, n, nk, 30, hostile=False)
    good = table(nk, 3)
    q = case.q
    inf, nan = float("inf"), float("nan")

    def f(**over):
        a = good.copy()
        for k, value in over.items():
            a[int(k[1:])] = value
        return a

    bad = [dict(geom=False), dict(met=False), dict(factor=None)]
    bad += [{name: None} for name in PLANES[2:] + FIELDS]
    bad += [dict(conserve=2), dict(conserve=-1), dict(rcv=inf), dict(rcv=nan)]
    bad += [dict(factor=f(k0=nan)), dict(factor=f(k1=nan)), dict(factor=f(k4=nan)), dict(factor=f(k0=0.0)), dict(factor=f(k2=-0.5)),
            dict(factor=f(k1=1.0000001)), dict(factor=f(k4=inf)), dict(factor=f(k4=2.0))]
    bad += [dict(factor=f(k4=0.9)), dict(factor=f(k1=1.0)), dict(factor=f(k0=1.0))]  # a damped level after an undamped one
    bad += [{a: q[b].ptr} for a, b in itertools.permutations(FIELDS, 2)]
    for kw in bad:
        kw = dict(kw)
        factor = kw.pop("factor", good)
        with pytest.raises(_lib.PaceError, match="invalid argument"):
            case.call(factor, **kw)
    empty = _lib.Metrics()
    saved, case.metrics = case.metrics, empty
    with pytest.raises(_lib.PaceError, match="invalid argument"):
        case.call(good)
    case.metrics = saved
    assert case.changed() == []  # nothing is written on error
    # what is accepted: rcv not finite without conserve, every factor 1.0 (nothing launched), kmax = nk
    case.call(good, conserve=0, rcv=nan)
    assert case.changed() == ["u", "v", "w"]
    case.call(np.ones(nk))
    case.call(table(nk, nk))


@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_kernel_against_the_restatement_emulated(library):
    check_kernel("cpu", library)


@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_specials_emulated(library):
    check_specials("cpu", library)


@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_invariant_emulated(library):
    check_invariant("cpu", library)


def test_refusals_emulated():
    check_refusals("cpu")


def test_restatement_against_the_oracle():
    check_restatement_against_the_oracle()


def test_header_and_binding_agree_on_the_entry_point():
    from pace_amd import _lib

    text = open(os.path.join(ROOT, "include", "pace_hip.h")).read()
    declared = set(re.findall(r"\b(pace_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert set(_lib.EXPORTED_SYMBOLS) <= declared and "pace_rayleigh_super" in _lib.EXPORTED_SYMBOLS
    proto = re.search(r"\bint pace_rayleigh_super\s*\(([^;]*)\);", text).group(1)
    assert len(proto.split(",")) == len(_lib._PROTOS["pace_rayleigh_super"][1]) == 14


@pytest.mark.gpu
@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_kernel_against_the_restatement_on_the_gpu(library):
    check_kernel("cuda", library)


@pytest.mark.gpu
@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_specials_on_the_gpu(library):
    check_specials("cuda", library)


@pytest.mark.gpu
@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_invariant_on_the_gpu(library):
    check_invariant("cuda", library)


@pytest.mark.gpu
def test_refusals_on_the_gpu():
    check_refusals("cuda")
