"""pace_nudge (pace_amd/csrc/k_nudge.hip): one launch relaxes up to 32 windows of fields toward held or interpolated references.

* bit for bit against the numpy restatement of the contract (tests/nudge_reference.py) over the WHOLE raw storage of the field and
  of the tendency, row padding, halo and level nk included: every storage is filled with random values before the call, so an
  element written outside a window differs from the restatement, which leaves it as it was; the references are unchanged after.
  C12 x 1; C13 x 2 (odd rows, window start misaligned); C68 x 5 (rows of 68 / 69 points: more than 64 lanes); windows of
  (n, n + 1) and (n + 1, n); a window with k0 > 0; the whole storage as a window; planes of a 2-D field and of one level; row
  counts that are no multiple of the 16 rows of a workgroup; 1 item and 32 items of different sizes in one launch; ref1 NULL;
  weight 0, 1 and 0.3; ref0 == ref1; tendency NULL; apply == 0; both libraries;
* NaN, +-inf, -0.0 and a denormal planted in state and references: bits where the restatement is no NaN, NaN-ness where it is;
* every PACE_ERR_ARG of the header, 33 items among them; the header against the binding.

Every check is a function of the device: the CPU tier calls it with the emulation libraries, the GPU tier with the product's."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import ROOT, build_emu, build_emu_f32  # noqa: E402
import nudge_reference  # noqa: E402

X, Y, Z = "x", "y", "z"


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


class Storages:
    """Random-filled raw storages of one layout (n, nz) on the device."""

    def __init__(self, lib, device, n, nz, seed):
        import torch

        from pace_amd import _launch
        from pace_amd.util import QuantityFactory, SubtileGridSizer

        self.lib, self.device, self.n, self.nz = lib, device, n, nz
        self.real = torch.float32 if lib.real_bytes == 4 else torch.float64
        self.factory = QuantityFactory(SubtileGridSizer(n, n, nz), device, self.real)
        self.rng = np.random.default_rng(seed)
        self.geom = _launch.geometry([self.factory.zeros([X, Y, Z], "")], str, "")

    def new(self, dims=(X, Y, Z), specials=False):
        """A quantity whose WHOLE base (row padding included) holds random values of magnitude ~1 .. 300."""
        import torch

        q = self.factory.zeros(list(dims), "")
        values = self.rng.uniform(-300.0, 300.0, size=tuple(q._base.shape))
        if specials:
            flat = values.reshape(-1)
            where = self.rng.choice(flat.size, size=min(flat.size // 4, 400), replace=False)
            flat[where] = self.rng.choice([np.nan, np.inf, -np.inf, -0.0, 0.0, 5e-324, 1e-42, 3e38, -1.7e308], size=where.size)
        with np.errstate(over="ignore"):
            q._base.copy_(torch.as_tensor(values.astype(np.float32 if self.lib.real_bytes == 4 else np.float64)))
        return q

    @staticmethod
    def raw(q):
        """The base as a host array indexed [i, j, k] ([i, j]), i running over the padded row."""
        a = q._base.detach().cpu().numpy().copy()
        return a.transpose(2, 1, 0) if a.ndim == 3 else a.transpose(1, 0)


# an item of a case: window (i0, j0, k0, ni, nj, nk); plane: None, "2d" or a level; ref1: False, True or "same" (ref0 itself)
def spec(window, timescale=3600.0, ref1=True, tendency=True, plane=None):
    return dict(window=window, timescale=timescale, ref1=ref1, tendency=tendency, plane=plane)


def run_case(s, specs, weight, dt, apply, specials=False):
    """One launch over the items of `specs`; the field's and the tendency's whole raw storages against the restatement.
    -> per item (field after, tendency after) as the device left them."""
    import torch

    from pace_amd import _lib

    items = (_lib.NudgeItem * len(specs))()
    held = []
    for item, sp in zip(items, specs):
        dims = (X, Y) if sp["plane"] == "2d" else (X, Y, Z)
        field, ref0 = s.new(dims, specials), s.new(dims, specials)
        ref1 = ref0 if sp["ref1"] == "same" else (s.new(dims, specials) if sp["ref1"] else None)
        tendency = s.new(dims) if sp["tendency"] else None
        level = sp["plane"] if isinstance(sp["plane"], int) else None
        step = 0 if level is None else level * s.geom.sk * s.lib.real_bytes
        item.field, item.ref0 = field.ptr + step, ref0.ptr + step
        item.ref1 = None if ref1 is None else ref1.ptr + step
        item.tendency = None if tendency is None else tendency.ptr + step
        item.kind = _lib.DIAG_WINDOW3D if sp["plane"] is None else _lib.DIAG_PLANE
        item.i0, item.j0, item.k0, item.ni, item.nj, item.nk = sp["window"]
        item.timescale = sp["timescale"]
        held.append((field, ref0, ref1, tendency, level))
    before = [[None if q is None else s.raw(q) for q in row[:4]] for row in held]
    s.lib.call("pace_nudge", C.byref(s.geom), items, len(specs), float(weight), float(dt), int(apply), _stream(s.device))
    if s.device != "cpu":
        torch.cuda.synchronize()
    results = []
    for m, (sp, row, (f0, a0, e0, t0)) in enumerate(zip(specs, held, before)):
        level = row[4]

        def at(a):  # the plane of a level item
            return None if a is None else (a if level is None else a[:, :, level])

        want_f, want_t = nudge_reference.nudge(at(f0), at(a0), at(e0), sp["window"], sp["timescale"], weight, dt, apply, at(t0))
        got_f, got_t = s.raw(row[0]), None if row[3] is None else s.raw(row[3])
        full_f, full_t = f0.copy(), None if t0 is None else t0.copy()
        if level is None:
            full_f, full_t = want_f, want_t
        else:
            full_f[:, :, level] = want_f
            if full_t is not None:
                full_t[:, :, level] = want_t
        where = (s.n, s.nz, m, sp, weight, dt, apply)
        assert same(got_f, full_f), ("field",) + where + (int((_bits(got_f) != _bits(full_f)).sum()),)
        if full_t is not None:
            assert same(got_t, full_t), ("tendency",) + where + (int((_bits(got_t) != _bits(full_t)).sum()),)
        # the references are only read
        assert np.array_equal(_bits(s.raw(row[1])), _bits(a0))
        if row[2] is not None and row[2] is not row[1]:
            assert np.array_equal(_bits(s.raw(row[2])), _bits(e0))
        if not apply:
            assert np.array_equal(_bits(got_f), _bits(f0))
        results.append((got_f, got_t))
    return results


def many_items(n, nz, count):
    """`count` windows of different sizes inside the storage (n + 7, n + 7, nz + 1), different timescales, every third without a
    ref1, every fourth without a tendency."""
    out = []
    for m in range(count):
        i0, j0, k0 = m % 4, (m * 3) % 5, m % 2
        ni, nj, nk = 1 + (m * 7) % (n + 7 - i0), 1 + (m * 5) % (n + 7 - j0), 1 + m % (nz + 1 - k0)
        out.append(spec((i0, j0, k0, ni, nj, nk), timescale=600.0 * (m + 1), ref1=m % 3 != 0, tendency=m % 4 != 0))
    return out


def check_kernel(device, only=None):
    from pace_amd import _lib

    for which, lib in enumerate(_libs(device)):
        if only is not None and only != which:
            continue
        # C12 x 1: one item, the compute domain
        s = Storages(lib, device, 12, 1, 1)
        run_case(s, [spec((3, 3, 0, 12, 12, 1))], 0.3, 225.0, 1)
        # C13 x 2: odd rows; the staggered windows (n, n + 1) and (n + 1, n); ref1 NULL; ref0 == ref1; weights 0 and 1
        s = Storages(lib, device, 13, 2, 2)
        stagger = [spec((3, 3, 0, 13, 13, 2)), spec((3, 3, 0, 13, 14, 2), timescale=21600.0),
                   spec((3, 3, 0, 14, 13, 2), timescale=7200.0)]
        for weight in (0.0, 1.0, 0.3):
            run_case(s, stagger, weight, 450.0, 1)
        run_case(s, [dict(sp, ref1=False) for sp in stagger], 0.0, 450.0, 1)
        run_case(s, [dict(sp, ref1="same") for sp in stagger], 0.3, 450.0, 1)
        run_case(s, [dict(sp, tendency=False) for sp in stagger], 0.3, 450.0, 1)
        # C68 x 5: rows longer than a wave; 68 * 5 = 340 and 69 * 3 = 207 rows are no multiple of 16; k0 > 0; the whole storage;
        # planes of one level and of a 2-D field
        s = Storages(lib, device, 68, 5, 3)
        big = [spec((3, 3, 0, 68, 68, 5)), spec((3, 3, 0, 69, 68, 5), ref1=False), spec((3, 3, 2, 68, 69, 3)),
               spec((0, 0, 0, 75, 75, 6), timescale=1800.0), spec((3, 3, 0, 68, 69, 1), plane=4),
               spec((3, 3, 0, 68, 68, 1), plane="2d", ref1=False), spec((0, 0, 0, 75, 75, 1), plane="2d")]
        run_case(s, big, 0.3, 225.0, 1)
        # apply == 0: the field is only read, and the tendencies are those of the applying call on the same inputs
        for specs in (stagger, big):
            n, nz = (13, 2) if specs is stagger else (68, 5)
            applied = run_case(Storages(lib, device, n, nz, 7), specs, 0.3, 225.0, 1)
            only_tendencies = run_case(Storages(lib, device, n, nz, 7), specs, 0.3, 225.0, 0)
            for (_, t_applied), (_, t_only) in zip(applied, only_tendencies):
                assert np.array_equal(_bits(t_applied), _bits(t_only))
        # 32 items of different sizes in one launch, at both ends of the weight, stored or not
        s = Storages(lib, device, 12, 5, 4)
        run_case(s, many_items(12, 5, _lib.NUDGE_MAX_ITEMS), 0.7, 900.0, 1)
        run_case(s, [dict(sp, tendency=True) for sp in many_items(12, 5, _lib.NUDGE_MAX_ITEMS)], 1.0, 900.0, 0)
        # NaN, +-inf, -0.0, denormals and values near the largest in state and references
        s = Storages(lib, device, 13, 2, 5)
        for weight in (0.0, 0.3, 1.0):
            results = run_case(s, stagger + [dict(sp, ref1=False) for sp in stagger], weight, 450.0, 1, specials=True)
        assert any(np.isnan(f).any() and np.isinf(f).any() for f, _ in results)


def check_refusals(device):
    from pace_amd import _lib

    lib = _libs(device)[0]
    s = Storages(lib, device, 12, 5, 6)
    field, ref0, ref1, tendency = s.new(), s.new(), s.new(), s.new()
    before = [s.raw(q) for q in (field, ref0, ref1, tendency)]

    def item(**kw):
        x = _lib.NudgeItem(field.ptr, ref0.ptr, ref1.ptr, tendency.ptr, _lib.DIAG_WINDOW3D, 3, 3, 0, 12, 12, 5, 3600.0)
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    def call(items, weight=0.3, dt=225.0, apply=1, geom=s.geom, n=None):
        table = (_lib.NudgeItem * max(len(items), 1))(*items)
        lib.call("pace_nudge", None if geom is None else C.byref(geom), table, len(items) if n is None else n, weight, dt, apply,
                 _stream(device))

    plane = dict(kind=_lib.DIAG_PLANE, nk=1)
    bad_items = [
        item(kind=2), item(kind=-1),                                            # an unknown kind
        item(ni=0), item(nj=0), item(nk=0), item(i0=-1), item(j0=-1), item(k0=-1),  # an empty window, a negative origin
        item(ni=17), item(nj=17), item(nk=7), item(k0=2), item(i0=8),           # outside the storage (19, 19, 6)
        item(kind=_lib.DIAG_PLANE), item(k0=1, **plane),                         # a plane has k0 = 0 and nk = 1
        item(field=None), item(ref0=None),
        item(timescale=0.0), item(timescale=-1.0), item(timescale=float("inf")), item(timescale=float("nan")),
        item(ref0=field.ptr), item(ref1=field.ptr), item(tendency=field.ptr),   # the field is one of the item's other arrays
    ]
    for bad in bad_items:
        with pytest.raises(_lib.PaceError, match="invalid argument"):
            call([item(), bad])
    for kw in (dict(weight=-0.1), dict(weight=1.5), dict(weight=float("nan")), dict(dt=float("inf")), dict(dt=float("nan")),
               dict(geom=None), dict(n=0), dict(n=-1)):
        with pytest.raises(_lib.PaceError, match="invalid argument"):
            call([item()], **kw)
    with pytest.raises(_lib.PaceError, match="invalid argument"):  # nothing to do
        call([item(tendency=None)], apply=0)
    with pytest.raises(_lib.PaceError, match="invalid argument"):
        lib.call("pace_nudge", C.byref(s.geom), None, 1, 0.3, 225.0, 1, _stream(device))
    windows = many_items(12, 5, _lib.NUDGE_MAX_ITEMS + 1)
    with pytest.raises(_lib.PaceError, match="invalid argument"):  # 33 items
        call([item(i0=w["window"][0], ni=1, nj=1, nk=1) for w in windows])
    if device != "cpu":
        import torch

        torch.cuda.synchronize()
    # nothing is written on error
    assert all(np.array_equal(_bits(s.raw(q)), _bits(b)) for q, b in zip((field, ref0, ref1, tendency), before))
    # what is accepted: a plane, ref1 NULL, tendency NULL with apply
    second, third = s.new(), s.new()
    call([item(), item(field=second.ptr, tendency=None, **plane), item(field=third.ptr, ref1=None, tendency=None)])
    if device != "cpu":
        import torch

        torch.cuda.synchronize()


@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_kernel_against_numpy_emulated(library):
    check_kernel("cpu", library)


def test_refusals_emulated():
    check_refusals("cpu")


def test_header_and_binding_agree_on_the_entry_point():
    from pace_amd import _lib

    text = open(os.path.join(ROOT, "include", "pace_hip.h")).read()
    declared = set(re.findall(r"\b(pace_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert set(_lib.EXPORTED_SYMBOLS) <= declared and "pace_nudge" in _lib.EXPORTED_SYMBOLS
    proto = re.search(r"\bint pace_nudge\s*\(([^;]*)\);", text).group(1)
    assert len(proto.split(",")) == len(_lib._PROTOS["pace_nudge"][1]) == 7
    assert int(re.search(r"#define PACE_NUDGE_MAX_ITEMS (\d+)", text).group(1)) == _lib.NUDGE_MAX_ITEMS == 32
    body = re.search(r"typedef struct \{([^}]*)\} pace_nudge_item_t;", text).group(1)
    fields = re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", body))
    assert fields == [name for name, _ in _lib.NudgeItem._fields_]
    assert C.sizeof(_lib.NudgeItem) == 72 and _lib.NudgeItem.timescale.offset == 64
    # the by-value table stays inside the kernel-argument segment: 56 B a device-side item
    assert 32 * 56 + 33 * 4 + 4 < 4096


@pytest.mark.gpu
@pytest.mark.parametrize("library", [0, 1], ids=["f64lib", "f32lib"])
def test_kernel_against_numpy_on_the_gpu(library):
    check_kernel("cuda", library)


@pytest.mark.gpu
def test_refusals_on_the_gpu():
    check_refusals("cuda")
