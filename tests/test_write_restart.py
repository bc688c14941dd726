"""pace_amd.util.write_restart and DycoreState.to_fortran_restart: the fixture restart (tests/golden/c12_restart, written by FMS)
read into six tiles' states and written back, and the files held against the fixture's with scipy -- version byte, dimensions,
variables, shapes, types, attributes (FMS's checksum among them: ours is formed on the device) and data bytes; the launch and
transfer counts of a call; round trips through the float32 library and float32 files; labels; a lone rank.
"""
import datetime
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import restart_helpers as rh  # noqa: E402
from helpers import build_emu, build_emu_f32  # noqa: E402
from restart_helpers import FIELDS, N, NZ, RESTART  # noqa: E402
from test_fortran_restart import CountingLib  # noqa: E402

TIME = datetime.datetime(2016, 8, 1, 0, 30)
START = datetime.datetime(2016, 8, 1, 0, 0)
KINDS = ("fv_core.res", "fv_tracer.res", "fv_srf_wnd.res")


@pytest.fixture(scope="module")
def emu_lib():
    from pace_amd import _lib

    return _lib.Library(build_emu())


@pytest.fixture(scope="module")
def emu_lib_f32():
    from pace_amd import _lib

    return _lib.Library(build_emu_f32())


def vertical_grid():
    path = os.path.join(RESTART, "fv_core.res.nc")
    return types.SimpleNamespace(ak=rh.file_array(path, "ak").astype(float), bk=rh.file_array(path, "bk").astype(float))


def read(path):
    """A NetCDF-3 file with scipy: (version byte, dimensions, global attributes, {variable: (dims, dtype, shape, attributes,
    the bytes of its data)})."""
    import scipy.io

    with scipy.io.netcdf_file(path, "r", mmap=False) as nc:
        variables = {name: (v.dimensions, v.data.dtype.str, v.shape, dict(v._attributes), np.array(v.data).tobytes())
                     for name, v in nc.variables.items()}
        return nc.version_byte, dict(nc.dimensions), dict(nc._attributes), variables


def write_six(lib, device, directory, **kwargs):
    """Six ranks: the fixture into a state, the state into `directory`."""
    from pace_amd.fv3core import DycoreState
    from pace_amd.util import run_tiles

    def program(comm):
        communicator = rh.communicator_of(comm, lib, device)
        state = DycoreState.from_fortran_restart(quantity_factory=rh.factory(lib, device, N, NZ), communicator=communicator, path=RESTART)
        state.to_fortran_restart(communicator=communicator, path=str(directory), time=TIME, start_time=START,
                                 grid_data=vertical_grid(), **kwargs)
        rh.sync(device)

    run_tiles(6, program)


def check_files_are_the_fixtures(lib, device, directory):
    write_six(lib, device, directory)
    assert sorted(os.listdir(directory)) == sorted(os.listdir(RESTART))
    for tile in range(6):
        for kind in KINDS:
            name = f"{kind}.tile{tile + 1}.nc"
            version, dims, attrs, got = read(os.path.join(str(directory), name))
            want_version, want_dims, want_attrs, want = read(os.path.join(RESTART, name))
            assert version == want_version == 2 and attrs == want_attrs == {"filename": ("RESTART/" + name).encode()}
            assert list(dims.items()) == list(want_dims.items()), (name, dims)
            extra = ["sgs_tke"] if kind == "fv_tracer.res" else []
            assert [v for v in got if v not in extra] == list(want), (name, list(got))
            for variable, (vdims, dtype, shape, vattrs, data) in got.items():
                tile_checksum = vattrs.pop("tile_checksum", None)
                if variable in want_dims or variable == "Time":  # the axes
                    assert tile_checksum is None and (vdims, dtype, shape, vattrs, data) == want[variable], (name, variable)
                    continue
                values = np.frombuffer(data, dtype=">f8")
                assert tile_checksum.decode() == "%16X" % values.astype("=f8").view(np.uint64).sum(dtype=np.uint64), (name, variable)
                if variable in extra:
                    assert (vdims, dtype, shape) == want["cld_amt"][:3] and set(vattrs) == {"long_name", "units", "checksum"}
                    assert not values.any()
                    continue
                assert list(vattrs) == list(want[variable][3]) == ["long_name", "units", "checksum"], (name, variable)
                assert (vdims, dtype, shape) == want[variable][:3], (name, variable)
                if kind == "fv_srf_wnd.res":
                    # (ua, va are zero after a Fortran restart; the fixture's surface winds are not)
                    assert not values.any() and vattrs == {**want[variable][3], "checksum": b"%16X" % 0}, (name, variable)
                else:
                    assert vattrs == want[variable][3], (name, variable, vattrs, want[variable][3])
                    assert data == want[variable][4], (name, variable)
    assert read(os.path.join(str(directory), "fv_core.res.nc")) == read(os.path.join(RESTART, "fv_core.res.nc"))
    with open(os.path.join(str(directory), "coupler.res")) as f, open(os.path.join(RESTART, "coupler.res")) as g:
        assert f.read() == g.read()


def test_written_files_are_the_fixtures_emulated(emu_lib, tmp_path):
    check_files_are_the_fixtures(emu_lib, "cpu", tmp_path)


def lone_state(lib, device, tile=2):
    from pace_amd.fv3core import DycoreState
    from pace_amd.util import NullComm

    counting = CountingLib(lib)
    communicator = rh.communicator_of(NullComm(rank=tile, total_ranks=6, fill_value=0.0), counting, device)
    qf = rh.factory(lib, device, N, NZ)
    state = DycoreState.from_fortran_restart(quantity_factory=qf, communicator=communicator, path=RESTART)
    # winds for the surface planes: distinct values over the whole storage, so that a wrong level or window shows
    rng = np.random.default_rng(5)
    for q in (state.ua, state.va, state.qsgs_tke):
        q.set(rng.uniform(-30.0, 30.0, q.shape))
    rh.sync(device)
    counting.calls.clear()
    return state, communicator, counting, qf


def check_counts_and_lone_rank(lib, device, directory, monkeypatch):
    """One launch, one device-to-host copy, no conversion of the values on the host; a lone NullComm leaves `checksum` out."""
    import torch

    from pace_amd.util import restart

    state, communicator, counting, _ = lone_state(lib, device)
    copies, writes, to_host = [], [], restart._to_host

    def counted_to_host(packed, host):
        copies.append((packed.numel() * packed.element_size(), packed.device.type, host.is_pinned() or device == "cpu",
                       host.data_ptr()))
        to_host(packed, host)

    class Recording:
        """A file whose writes are recorded: the address and the length of what each was given."""

        def __init__(self, file):
            self.file = file

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            self.file.close()

        def write(self, data):
            if not isinstance(data, str):
                view = np.frombuffer(data, dtype=np.uint8)
                writes.append((os.path.basename(self.file.name), view.ctypes.data, view.size))
            return self.file.write(data)

    monkeypatch.setattr(restart, "open", lambda *args, **kwargs: Recording(open(*args, **kwargs)), raising=False)
    monkeypatch.setattr(restart, "_to_host", counted_to_host)
    state.to_fortran_restart(communicator=communicator, path=str(directory), time=TIME, grid_data=None)
    monkeypatch.undo()
    assert counting.calls == ["pace_restart_pack"]
    elements = sum(rh.tile_array(2, field).size for field in FIELDS) + N * N * NZ + 2 * N * N  # (+ sgs_tke, u_srf, v_srf)
    assert [c[:3] for c in copies] == [(8 * elements + 8 * 18, torch.device(device).type, True)]
    # the values go to disk from the one pinned buffer itself: per file ONE write of a slice of it, which holds all the
    # file's data -- the host made no converted, swapped or gathered copy of them
    pinned, at = copies[0][3], 0
    for kind in restart.RESTART_NAMES:  # (the order of the files' sections in the buffer)
        size = 8 * sum(rh.tile_array(2, f).size for f, entry in FIELDS.items() if entry[1] == kind)
        size += {"fv_tracer.res": 8 * N * N * NZ, "fv_srf_wnd.res": 8 * 2 * N * N}.get(kind, 0)
        inside = [w for w in writes if w[0] == f"{kind}.tile3.nc" and pinned <= w[1] < pinned + 8 * elements]
        assert inside == [(f"{kind}.tile3.nc", pinned + at, size)], (kind, inside, writes)
        assert len([w for w in writes if w[0] == f"{kind}.tile3.nc"]) == 2  # (the header and the data)
        at += size
    # rank 2 is not rank 0: no coupler.res, no fv_core.res.nc
    assert sorted(os.listdir(directory)) == sorted(f"{kind}.tile3.nc" for kind in KINDS)
    for kind in KINDS:
        _, _, _, variables = read(os.path.join(str(directory), f"{kind}.tile3.nc"))
        for variable, (_, _, _, attrs, data) in variables.items():
            if "axis" in variable or variable == "Time":
                continue
            assert list(attrs) == ["long_name", "units", "tile_checksum"], (kind, variable, attrs)
            values = np.frombuffer(data, dtype=">f8")
            assert attrs["tile_checksum"].decode() == "%16X" % values.astype("=f8").view(np.uint64).sum(dtype=np.uint64)
    _, _, _, srf = read(os.path.join(str(directory), "fv_srf_wnd.res.tile3.nc"))
    _, _, _, tracer = read(os.path.join(str(directory), "fv_tracer.res.tile3.nc"))
    for variable, q in (("u_srf", state.ua), ("v_srf", state.va)):
        want = q.numpy()[3:3 + N, 3:3 + N, NZ - 1].T
        assert np.array_equal(np.frombuffer(srf[variable][4], dtype=">f8").reshape(N, N), want), variable
    assert np.array_equal(np.frombuffer(tracer["sgs_tke"][4], dtype=">f8").reshape(NZ, N, N),
                          state.qsgs_tke.numpy()[3:3 + N, 3:3 + N, :NZ].transpose(2, 1, 0))
    assert list(tracer)[-2:] == ["sgs_tke", "cld_amt"]
    return state, communicator


def test_counts_and_a_lone_rank_emulated(emu_lib, tmp_path, monkeypatch):
    check_counts_and_lone_rank(emu_lib, "cpu", tmp_path, monkeypatch)


def check_round_trips(lib, lib_f32, device, directory):
    """float32 library -> files -> float32 library is exact; float32 files read back as astype(float32); a label."""
    import dataclasses

    from pace_amd.fv3core import DycoreState
    from pace_amd.util import open_restart

    # 1. the float32 library: what it holds is written widened (exact) and read back narrowed (exact)
    state, communicator, _, qf = lone_state(lib_f32, device)
    first = str(directory / "f32")
    state.to_fortran_restart(communicator=communicator, path=first, time=TIME, label="later")
    assert sorted(os.listdir(first)) == sorted(f"later.{kind}.tile3.nc" for kind in KINDS)
    with pytest.raises(ValueError, match="no restart files found"):
        open_restart(first, communicator)
    back = DycoreState.init_zeros(qf)
    from pace_amd.fv3core.initialization.dycore_state import FORTRAN_RESTART_FIELDS

    to_state = {name: getattr(back, field) for field, name in FORTRAN_RESTART_FIELDS.items()}
    to_state["turbulent_kinetic_energy"] = back.qsgs_tke
    open_restart(first, communicator, label="later", to_state=to_state)
    rh.sync(device)
    for field in list(FORTRAN_RESTART_FIELDS) + ["qsgs_tke"]:
        got, want = getattr(back, field), getattr(state, field)
        window = tuple(slice(o, o + e) for o, e in zip(want.origin, want.extent))
        assert got.numpy().dtype == np.float32
        assert np.array_equal(got.numpy()[window].view(np.uint32), want.numpy()[window].view(np.uint32)), field
        assert np.abs(want.numpy()[window]).max() > 0 or field in ("qsgs_tke",), field
    assert len(dataclasses.fields(back)) == 32

    # 2. float32 files of the float64 library: astype(float32) of what it holds, tile_checksum of the 32-bit patterns only
    state, communicator, _, _ = lone_state(lib, device)
    second = str(directory / "files_f32")
    state.to_fortran_restart(communicator=communicator, path=second, time=TIME, file_dtype=np.float32)
    host = open_restart(second, communicator)
    for field, name in FORTRAN_RESTART_FIELDS.items():
        q = getattr(state, field)
        window = tuple(slice(o, o + e) for o, e in zip(q.origin, q.extent))
        want = q.numpy()[window].astype(np.float32).astype(np.float64)
        assert np.array_equal(host[name].data, want.transpose(*range(want.ndim)[::-1])), field
    for kind in KINDS:
        _, _, _, variables = read(os.path.join(second, f"{kind}.tile3.nc"))
        for variable, (_, dtype, _, attrs, data) in variables.items():
            if "axis" in variable or variable == "Time":
                assert dtype == ">f8"
                continue
            assert dtype == ">f4" and list(attrs) == ["long_name", "units", "tile_checksum"]
            patterns = np.frombuffer(data, dtype=">f4").astype("=f4").view(np.uint32)
            assert attrs["tile_checksum"].decode() == "%16X" % patterns.sum(dtype=np.uint64)


def test_round_trips_emulated(emu_lib, emu_lib_f32, tmp_path):
    check_round_trips(emu_lib, emu_lib_f32, "cpu", tmp_path)


def test_refusals(emu_lib, tmp_path):
    from pace_amd.util import LevelOf, write_restart

    state, communicator, _, _ = lone_state(emu_lib, "cpu")
    with pytest.raises(KeyError, match="no_such_name"):
        write_restart(str(tmp_path), communicator, {"no_such_name": state.pt}, time=TIME)
    with pytest.raises(ValueError, match="cannot give a variable of dims"):
        write_restart(str(tmp_path), communicator, {"x_wind": state.v}, time=TIME)
    with pytest.raises(ValueError, match="float64 or float32"):
        write_restart(str(tmp_path), communicator, {"x_wind": state.u}, time=TIME, file_dtype=np.int32)
    with pytest.raises(ValueError, match="LevelOf"):
        LevelOf(state.ua, NZ + 1)
    with pytest.raises(ValueError, match="LevelOf"):
        LevelOf(state.phis, 0)


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_written_files_are_the_fixtures_gpu(tmp_path):
    from pace_amd import _lib

    check_files_are_the_fixtures(_lib.load(), "cuda", tmp_path)


@pytest.mark.gpu
def test_counts_and_a_lone_rank_gpu(tmp_path, monkeypatch):
    from pace_amd import _lib

    check_counts_and_lone_rank(_lib.load(), "cuda", tmp_path, monkeypatch)


@pytest.mark.gpu
def test_round_trips_gpu(tmp_path):
    from pace_amd import _lib

    check_round_trips(_lib.load(), _lib.load(32), "cuda", tmp_path)
