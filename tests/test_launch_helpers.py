"""pace_amd/_launch.py: the one host-side home of the stream handle, the library-against-tensors check, the storage geometry
of a call, a window of a field as a table item, staging buffers and the cut into launches.

CPU tier, the emulation library, a C12 tile with 3 levels.  The expectations are written out from the strides and from what the
callers did before they shared these functions -- restart and diagnostics want one (nk, sk) of all 3-D fields, gather takes nk
from the first 3-D field and lets a later one have fewer levels, the safety check takes 3-D fields only -- never from the
functions under test.  One gpu test holds the stream handles of the three stream() methods to torch's, by device."""
import ctypes as C
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import build_emu  # noqa: E402

from pace_amd import _launch, _lib  # noqa: E402
from pace_amd.util import QuantityFactory, SubtileGridSizer  # noqa: E402

X, Y, Z, XI, YI, ZI = "x", "y", "z", "x_interface", "y_interface", "z_interface"
N, NZ = 12, 3
REFUSED, DIFFER = "refused: {}", "they differ"


@pytest.fixture(scope="module")
def emu():
    return _lib.Library(build_emu())


@pytest.fixture(scope="module")
def qf():
    return QuantityFactory(SubtileGridSizer(N, N, NZ), "cpu", torch.float64)


def geometry(fields, **options):
    g = _launch.geometry(fields, lambda f: REFUSED.format(tuple(getattr(f, "data", f).shape)), DIFFER, **options)
    return g.n, g.nk, g.sj, g.sk


def shorter(q, levels):
    """The quantity with fewer levels in the same storage: a view, the same strides."""
    data = q.data[:, :, :levels]
    return types.SimpleNamespace(data=data, dims=q.dims, shape=tuple(data.shape), ptr=q.ptr, origin=q.origin, extent=q.extent, units="")


# ---- geometry -----------------------------------------------------------------------------------------------------------------
def test_geometry_of_3d_2d_and_mixed_fields(qf):
    q3, qi, q2 = qf.zeros([X, Y, Z], ""), qf.zeros([XI, YI, ZI], ""), qf.zeros([X, Y], "")
    sj, sk = q3.data.stride(1), q3.data.stride(2)
    assert q3.data.shape == (N + 7, N + 7, NZ + 1) and q3.data.stride(0) == 1 and sj >= N + 7 and sk >= sj * (N + 7)
    assert geometry([q3, qi]) == (N, NZ, sj, sk)
    assert geometry([q2]) == (N, 1, sj, sj * (N + 7))  # no 3-D field: one level, a plane's worth of level stride
    assert geometry([q2, q3, q2]) == geometry([q3.data, q2.data]) == (N, NZ, sj, sk)  # Quantities or their tensors


def test_geometry_refusals(qf):
    q3, q2 = qf.zeros([X, Y, Z], ""), qf.zeros([X, Y], "")
    sj, sk = q3.data.stride(1), q3.data.stride(2)
    with pytest.raises(ValueError, match="refused"):  # stride 0 is not 1
        geometry([q3, q3.data.transpose(0, 1)])
    with pytest.raises(ValueError, match=r"refused: \(19, 19, 4, 2\)"):  # (the text is the caller's, about the offending field)
        geometry([q3, torch.zeros(2, NZ + 1, N + 7, N + 7).permute(3, 2, 1, 0)])
    with pytest.raises(ValueError, match="refused"):
        geometry([torch.zeros(N + 7)])
    other_tile = QuantityFactory(SubtileGridSizer(2 * N, 2 * N, NZ), "cpu", torch.float64).zeros([X, Y, Z], "")
    with pytest.raises(ValueError, match=DIFFER):  # two tile sizes
        geometry([q3, other_tile])
    with pytest.raises(ValueError, match=DIFFER):  # ... also where the other tile is 2-D
        geometry([q3, torch.empty_strided((2 * N + 7, 2 * N + 7), (1, sj))])
    with pytest.raises(ValueError, match=DIFFER):  # two row strides
        geometry([q2, torch.empty_strided((N + 7, N + 7), (1, sj + 8))])
    with pytest.raises(ValueError, match=DIFFER):  # two level strides
        geometry([q3, torch.empty_strided((N + 7, N + 7, NZ + 1), (1, sj, sk + sj))])
    with pytest.raises(ValueError, match=DIFFER):  # two level counts
        geometry([q3, shorter(q3, NZ)])
    with pytest.raises(ValueError, match="refused"):  # ndim: the safety check's 3-D fields only
        geometry([q3, q2], ndim=(3,))


def test_the_callers_keep_their_differences(qf, emu):
    """A second 3-D field with fewer levels in the same storage (the same sk): restart, diagnostics and the safety check refuse
    it, gather takes it -- but not a field with MORE levels than the first 3-D one; a 2-D field goes everywhere but into the
    safety check."""
    from pace_amd.driver.diagnostics import WindowPacker, _Request
    from pace_amd.driver.safety_checks import SafetyChecker
    from pace_amd.util import gather, restart

    q3, q2 = qf.zeros([X, Y, Z], ""), qf.zeros([X, Y], "")
    fewer = shorter(qf.zeros([X, Y, Z], ""), NZ)
    sj, sk = q3.data.stride(1), q3.data.stride(2)

    def request(q):
        return _Request("a", _lib.DIAG_PLANE, q, None, 0, (3, 3, 0, N, N, 1), (X, Y), "")

    def plan(*qs):
        geom = WindowPacker(emu)._plan([request(q) for q in qs], False)[0]
        return geom.n, geom.nk, geom.sj, geom.sk

    def safety(*qs):
        geom = SafetyChecker(emu)._plan([q.data for q in qs])[1][0]
        return geom.n, geom.nk, geom.sj, geom.sk

    def of(g):
        return g.n, g.nk, g.sj, g.sk

    whole = (N, NZ, sj, sk)
    assert of(restart._geometry([q3, q2])) == plan(q3, q2) == of(gather.geom_of([q3, q2])) == safety(q3, q3) == whole
    with pytest.raises(ValueError, match="do not share one storage layout"):
        restart._geometry([q3, fewer])
    with pytest.raises(ValueError, match="one layout and type on one device"):
        plan(q3, fewer)
    with pytest.raises(ValueError, match="one layout on one device"):
        safety(q3, fewer)
    assert of(gather.geom_of([q2, q3, fewer])) == whole  # gather: nk is the first 3-D field's
    with pytest.raises(ValueError, match="differ in geometry"):
        gather.geom_of([fewer, q3])  # ... and a later field may not have more levels
    with pytest.raises(ValueError, match="the safety check takes 3-D fields"):
        safety(q3, q2)
    four = types.SimpleNamespace(data=torch.zeros(2, NZ + 1, N + 7, N + 7).permute(3, 2, 1, 0), dims=(X, Y, Z, "tracer"))
    with pytest.raises(ValueError, match="cannot fill a quantity of dims"):
        restart._geometry([q3, four])
    with pytest.raises(ValueError, match="diagnostics take 2-D and 3-D fields"):
        plan(q3, four)
    with pytest.raises(ValueError, match="gather and scatter move"):
        gather.geom_of([q3, four])
    with pytest.raises(ValueError, match="gather and scatter move"):  # gather alone looks at the names of the axes
        gather.geom_of([types.SimpleNamespace(data=q3.data, dims=(Z, Y, X))])


# ---- windows ------------------------------------------------------------------------------------------------------------------
def test_window_of(qf):
    centre, corner, plane = qf.zeros([X, Y, Z], ""), qf.zeros([XI, YI, ZI], ""), qf.zeros([XI, Y], "")
    assert _launch.window_of(centre) == (centre.data.data_ptr(), _lib.DIAG_WINDOW3D, 3, 3, 0, N, N, NZ)
    assert _launch.window_of(corner) == (corner.data.data_ptr(), _lib.DIAG_WINDOW3D, 3, 3, 0, N + 1, N + 1, NZ + 1)
    assert _launch.window_of(plane) == (plane.data.data_ptr(), _lib.DIAG_PLANE, 3, 3, 0, N + 1, N, 1)
    for k in range(NZ + 1):  # (level 0 is a plane too, not the volume)
        assert _launch.window_of(corner, k) == (corner.data[..., k].data_ptr(), _lib.DIAG_PLANE, 3, 3, 0, N + 1, N + 1, 1)
    box = (0, 1, 2, N + 7, 5, 2)
    assert _launch.window_of(centre, window=box) == (centre.data.data_ptr(), _lib.DIAG_WINDOW3D) + box
    assert _launch.window_of(centre, 2, (0, 0, 0, N + 7, N + 7, 1)) == (centre.data[..., 2].data_ptr(), _lib.DIAG_PLANE, 0, 0, 0,
                                                                       N + 7, N + 7, 1)
    assert _launch.window_of(plane, window=(0, 0, 0, 4, 4, 1))[:2] == (plane.data.data_ptr(), _lib.DIAG_PLANE)


@pytest.mark.parametrize("struct", [_lib.DiagItem, _lib.UnpackItem, _lib.CubeItem, _lib.RestartItem])
def test_set_window_is_the_field_by_field_fill(struct):
    got, want = struct(), struct()
    _launch.set_window(got, (0x7f0012345678, _lib.DIAG_PLANE, 1, 2, 3, 4, 5, 6))
    want.field, want.kind = 0x7f0012345678, _lib.DIAG_PLANE
    want.i0, want.j0, want.k0 = 1, 2, 3
    want.ni, want.nj, want.nk = 4, 5, 6
    assert bytes(got) == bytes(want) and bytes(got) != bytes(struct())


def test_the_callers_windows(qf):
    """restart's windows, gather's items and gather.Window through the one function: what they were."""
    from pace_amd.util import gather, restart

    q3, q2 = qf.zeros([X, YI, Z], ""), qf.zeros([X, Y], "")
    assert restart._windows_of([(q3, None), (q2, None), (q3, 2)], 8) == [
        (q3.ptr, _lib.DIAG_WINDOW3D, 3, 3, 0, N, N + 1, NZ), (q2.ptr, _lib.DIAG_PLANE, 3, 3, 0, N, N, 1),
        (q3.data[..., 2].data_ptr(), _lib.DIAG_PLANE, 3, 3, 0, N, N + 1, 1)]
    x = gather.item_of(q3, 40)
    assert (x.field, x.kind, x.i0, x.j0, x.k0, x.ni, x.nj, x.nk, x.offset) == (q3.ptr, _lib.DIAG_WINDOW3D, 3, 3, 0, N, N + 1, NZ, 40)
    w = gather.Window(q3, _lib.DIAG_PLANE, 1, (3, 3, 0, N, N + 1, 1), (X, YI), "m")
    x = gather.item_of(w, 7)
    assert (x.field, x.kind, x.i0, x.j0, x.k0, x.ni, x.nj, x.nk, x.offset) == (q3.data[..., 1].data_ptr(), _lib.DIAG_PLANE, 3, 3, 0,
                                                                              N, N + 1, 1, 7)
    assert (w.origin, w.extent) == ((3, 3), (N, N + 1))
    assert gather.Window(q3, _lib.DIAG_WINDOW3D, 0, (0, 0, 0, 4, 4, 2), (X, YI, Z), "m").ptr == q3.ptr


# ---- chunks, streams, the library -----------------------------------------------------------------------------------------------
def test_chunks():
    n = 4
    assert list(_launch.chunks([], n)) == []
    assert list(_launch.chunks([7], n)) == [(0, [7])]
    assert list(_launch.chunks(list(range(n)), n)) == [(0, [0, 1, 2, 3])]
    assert list(_launch.chunks(list(range(n + 1)), n)) == [(0, [0, 1, 2, 3]), (n, [4])]


def test_cpu_has_no_stream_and_nothing_to_wait_for(monkeypatch):
    def no_device(*args, **kwargs):
        raise AssertionError("the CPU has no stream")

    monkeypatch.setattr(torch.cuda, "current_stream", no_device)
    for device in ("cpu", torch.device("cpu")):
        assert _launch.stream_of(device) is None
        assert _launch.wait_for(device) is None


def test_library_against_tensors(emu):
    assert _launch.default_device(emu) == torch.device("cpu")
    assert _launch.real_of(emu) == torch.float64 and emu.real_bytes == 8
    _launch.check_library(emu, "cpu")
    _launch.check_library(emu, torch.device("cpu"), torch.float64)
    with pytest.raises(_lib.PaceError, match="CPU tensors go with the emulation test library, device tensors with the product"):
        _launch.check_library(emu, torch.device("cuda", 0))
    with pytest.raises(ValueError, match="pt: field dtype torch.float32 does not match the library's storage type torch.float64"):
        _launch.check_library(emu, "cpu", torch.float32, name="pt")


# ---- staging --------------------------------------------------------------------------------------------------------------------
def test_staging_and_the_copies_on_the_cpu():
    dev, host = _launch.staging(5, torch.int64, "cpu")
    assert dev is not host and dev.data_ptr() != host.data_ptr() and not host.is_pinned()
    assert (dev.shape, dev.dtype, host.shape, host.dtype) == ((5,), torch.int64, (5,), torch.int64)
    one, same = _launch.staging(5, torch.float32, torch.device("cpu"), alias_on_cpu=True)
    assert one is same and one.dtype == torch.float32
    host.copy_(torch.arange(5))
    _launch.to_device(host, dev)
    assert dev.tolist() == [0, 1, 2, 3, 4]
    dev += 10
    _launch.to_host(dev, host)
    assert host.tolist() == [10, 11, 12, 13, 14]


def test_upload_table_on_the_cpu():
    table = (_lib.CubeItem * 3)()
    for m, item in enumerate(table):
        _launch.set_window(item, (1000 + m, _lib.DIAG_PLANE, m, m, 0, 4, 4, 1))
        item.offset = 16 * m
    keep = _launch.upload_table(table, torch.device("cpu"))
    assert keep[0].numel() * keep[0].element_size() == C.sizeof(table) and all(t.device.type == "cpu" for t in keep)
    assert C.string_at(keep[0].data_ptr(), C.sizeof(table)) == bytes(table)


# ---- the device -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_streams_by_device_and_a_table_on_the_device():
    from pace_amd.fv3core.stencils._common import Operator
    from pace_amd.tile import setup_factories
    from pace_amd.util import CubedSphereCommunicator, NullComm
    from pace_amd.util.checkpointer import ThresholdCalibrationCheckpointer

    lib = _lib.load()
    t = torch.zeros(4, device="cuda:0")
    _, factory, _, stencil_factory = setup_factories(lib, t.device, N, NZ)
    streams = (lambda: _launch.stream_of(t.device), Operator(stencil_factory, factory).stream,
               CubedSphereCommunicator(NullComm(0, 6), device=t.device, lib=lib).stream,
               ThresholdCalibrationCheckpointer(lib=lib, device=t.device).stream)
    side = torch.cuda.Stream(device=t.device)
    for stream in streams:
        # (ctypes reads a null handle -- the default stream's -- back as None)
        assert (stream().value or 0) == torch.cuda.current_stream(t.device).cuda_stream
        with torch.cuda.stream(side):
            assert stream().value == torch.cuda.current_stream(t.device).cuda_stream == side.cuda_stream
    assert _launch.default_device(lib) == t.device and _launch.real_of(lib) == torch.float64
    table = (C.c_uint8 * 24)(*range(24))
    dev, stage = _launch.upload_table(table, t.device)
    _launch.wait_for(t.device)
    assert dev.device == t.device and stage.is_pinned() and bytes(dev.cpu().numpy()) == bytes(stage.numpy()) == bytes(table)
