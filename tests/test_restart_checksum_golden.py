"""pace_restart_pack's sums against FMS: the `checksum` attribute of the fixture restart (tests/golden/c12_restart, written by the
Fortran model, not by us) is, for each of its 17 variables, the wrapping sum over the six tiles of the kernel's sum of the
tile's window -- and open_restart(verify_checksums=True) holds a state against it.
"""
import os
import shutil
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import restart_helpers as rh  # noqa: E402
from helpers import build_emu, build_emu_f32  # noqa: E402
from restart_helpers import N, NZ, RESTART  # noqa: E402

SRF = {"eastward_wind_at_surface": "u_srf", "northward_wind_at_surface": "v_srf"}


@pytest.fixture(scope="module")
def emu_lib():
    from pace_amd import _lib

    return _lib.Library(build_emu())


@pytest.fixture(scope="module")
def emu_lib_f32():
    from pace_amd import _lib

    return _lib.Library(build_emu_f32())


def attributes():
    """restart variable -> (file kind, the checksum attribute), read here with scipy from tile 1's files; the other tiles' files
    carry the same text."""
    import scipy.io

    out = {}
    for kind in ("fv_core.res", "fv_tracer.res", "fv_srf_wnd.res"):
        per_tile = []
        for tile in range(6):
            with scipy.io.netcdf_file(os.path.join(RESTART, f"{kind}.tile{tile + 1}.nc"), "r", mmap=False) as nc:
                per_tile.append({name: v._attributes["checksum"].decode() for name, v in nc.variables.items()
                                 if "checksum" in v._attributes})
        assert all(p == per_tile[0] for p in per_tile)
        out.update({name: (kind, text) for name, text in per_tile[0].items()})
    assert len(out) == 17
    return out


def to_state_of(qf):
    """The seventeen variables' quantities: the DycoreState's fifteen and two 2-D ones for the surface winds."""
    from pace_amd.fv3core import DycoreState
    from pace_amd.fv3core.initialization.dycore_state import FORTRAN_RESTART_FIELDS

    state = DycoreState.init_zeros(qf)
    to_state = {name: getattr(state, field) for field, name in FORTRAN_RESTART_FIELDS.items()}
    for name in SRF:
        to_state[name] = qf.zeros(["x", "y"], "m/s")
    return to_state


def load_six(lib, device, directory=RESTART, **kwargs):
    """Six ranks read the restart; -> per tile {restart variable: the kernel's sum of the quantity's compute window}."""
    import ctypes as C

    import torch

    from pace_amd import _lib
    from pace_amd.util import open_restart, restart, run_tiles
    from pace_amd.util.grid import geom_struct

    def program(comm):
        communicator = rh.communicator_of(comm, lib, device)
        qf = rh.factory(lib, device, N, NZ)
        to_state = to_state_of(qf)
        open_restart(directory, communicator, to_state=to_state, **kwargs)
        names = [name for name in to_state if name != "time"]
        windows = restart._windows_of([(to_state[name], None) for name in names], lib.real_bytes)
        items = (_lib.RestartItem * len(windows))()
        for item, window in zip(items, windows):
            item.field, item.kind, item.i0, item.j0, item.k0, item.ni, item.nj, item.nk = window
        geom = geom_struct(qf)
        sums = torch.zeros(len(windows), dtype=torch.int64, device=device)
        need = lib.cdll.pace_restart_pack_workspace_bytes(C.byref(geom), items, len(windows))
        workspace = torch.zeros(need // 8, dtype=torch.int64, device=device)
        lib.call("pace_restart_pack", C.byref(geom), items, len(windows), _lib.RESTART_BE_F64, None, C.c_void_p(sums.data_ptr()),
                 C.c_void_p(workspace.data_ptr()), rh.stream_of(device))
        got = sums.cpu().numpy().view(np.uint64)
        return {restart.RESTART_PROPERTIES[name]["restart_name"]: got[m] for m, name in enumerate(names)}

    return run_tiles(6, program)


def check_sums_are_fms_checksums(lib, device):
    per_tile = load_six(lib, device, verify_checksums=True)  # (... and the verification passes on the fixture)
    want = attributes()
    assert sorted(per_tile[0]) == sorted(want)
    for variable, (kind, text) in want.items():
        assert len(text) == 16 and text == text.upper()
        globe = np.array([t[variable] for t in per_tile], dtype=np.uint64).sum(dtype=np.uint64)
        assert "%16X" % globe == text, (kind, variable)
        # the restatement of a tile's sum, from the file read with scipy
        for tile in (0, 5):
            a = rh.file_array(os.path.join(RESTART, f"{kind}.tile{tile + 1}.nc"), variable)
            assert per_tile[tile][variable] == a.astype("=f8").view(np.uint64).sum(dtype=np.uint64), (variable, tile)


def test_sums_are_fms_checksums_emulated(emu_lib):
    check_sums_are_fms_checksums(emu_lib, "cpu")


def offset_of(path, variable):
    """Where a variable's data begin in a NetCDF-3 file: where its bytes, read with scipy, are found."""
    with open(path, "rb") as f:
        raw = f.read()
    data = rh.file_array(path, variable).tobytes()
    begin = raw.find(data)
    assert begin > 0 and raw.find(data, begin + 1) < 0
    return begin


def flipped_copy(directory, tile=3):
    """The fixture with one mantissa bit of one value of delp flipped in one tile's file (a copy: the fixture is not touched)."""
    target = os.path.join(str(directory), "flipped")
    shutil.copytree(RESTART, target)
    path = os.path.join(target, f"fv_core.res.tile{tile + 1}.nc")
    begin = offset_of(path, "delp")
    with open(path, "r+b") as f:
        f.seek(begin + 8 * 1234 + 7)  # (big-endian: the last byte holds the lowest mantissa bits)
        byte = f.read(1)
        f.seek(-1, 1)
        f.write(bytes([byte[0] ^ 1]))
    rh.file_array.cache_clear()
    assert not np.array_equal(rh.file_array(path, "delp"), rh.tile_array(tile, "delp"))
    return target, path


def check_a_flipped_bit_is_found(lib, device, directory):
    target, path = flipped_copy(directory)
    load_six(lib, device, directory=target)  # (unverified, it reads)
    with pytest.raises(RuntimeError) as caught:
        load_six(lib, device, directory=target, verify_checksums=True)
    cause = caught.value.__cause__
    assert isinstance(cause, ValueError) and "delp of " in str(cause) and "fv_core.res.tile" in str(cause), cause


def test_a_flipped_bit_is_found_emulated(emu_lib, tmp_path):
    check_a_flipped_bit_is_found(emu_lib, "cpu", tmp_path)


def check_tile_checksum_and_lone_rank(lib, device, directory):
    """A lone NullComm: the fixture (no tile_checksum) cannot be verified -- one warning; files written here carry
    tile_checksum and are verified by the rank alone, and a flipped bit in them is named."""
    from pace_amd.util import NullComm, open_restart

    communicator = rh.communicator_of(NullComm(rank=3, total_ranks=6, fill_value=0.0), lib, device)
    qf = rh.factory(lib, device, N, NZ)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        to_state = to_state_of(qf)
        open_restart(RESTART, communicator, to_state=to_state, verify_checksums=True)
    assert len(caught) == 1 and "could not be verified" in str(caught[0].message), [str(w.message) for w in caught]
    from pace_amd.util import write_restart

    import datetime

    own = os.path.join(str(directory), "own")
    write_restart(own, communicator, to_state, time=datetime.datetime(2016, 8, 1))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        back = to_state_of(qf)
        open_restart(own, communicator, to_state=back, verify_checksums=True)
    rh.sync(device)
    for name in to_state:
        if name != "time":
            assert np.array_equal(back[name].numpy(), to_state[name].numpy()), name
    path = os.path.join(own, "fv_tracer.res.tile4.nc")
    begin = offset_of(path, "o3mr")
    with open(path, "r+b") as f:
        f.seek(begin + 8 * 77 + 6)
        byte = f.read(1)
        f.seek(-1, 1)
        f.write(bytes([byte[0] ^ 16]))
    with pytest.raises(ValueError, match=r"o3mr of .*fv_tracer\.res\.tile4\.nc.*tile_checksum"):
        open_restart(own, communicator, to_state=to_state_of(qf), verify_checksums=True)


def test_tile_checksum_and_a_lone_rank_emulated(emu_lib, tmp_path):
    check_tile_checksum_and_lone_rank(emu_lib, "cpu", tmp_path)


def test_the_float32_library_refuses_to_verify(emu_lib_f32):
    from pace_amd.util import NullComm, open_restart

    communicator = rh.communicator_of(NullComm(rank=0, total_ranks=6, fill_value=0.0), emu_lib_f32, "cpu")
    qf = rh.factory(emu_lib_f32, "cpu", N, NZ)
    with pytest.raises(ValueError, match="float32 library narrows"):
        open_restart(RESTART, communicator, to_state=to_state_of(qf), verify_checksums=True)
    open_restart(RESTART, communicator, to_state=to_state_of(qf))  # (the default is as before)


# ---- on the GPU: six tiles on one device ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sums_are_fms_checksums_gpu():
    from pace_amd import _lib

    check_sums_are_fms_checksums(_lib.load(), "cuda")


@pytest.mark.gpu
def test_a_flipped_bit_is_found_gpu(tmp_path):
    from pace_amd import _lib

    check_a_flipped_bit_is_found(_lib.load(), "cuda", tmp_path)


@pytest.mark.gpu
def test_tile_checksum_and_a_lone_rank_gpu(tmp_path):
    from pace_amd import _lib

    check_tile_checksum_and_lone_rank(_lib.load(), "cuda", tmp_path)
