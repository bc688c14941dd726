"""gather, gather_state, scatter and scatter_state of CubedSphereCommunicator (util/pace/util/communicator.py:111-329) for the
six tiles of a (1, 1) layout, against numpy stacking of the six compute-domain views:

* under run_cube (one launch for the whole cube), run_cube(snapshot=True) and run_tiles(6) (one launch per rank): every
  staggering, a 2-D field, a float32 field; None off the root; recv_quantity written in place; the reference's TypeError;
* gather_state with `time` and transfer_type=float32; scatter_state(gather_state(state)) equals the state;
* the launch structure under run_cube: exactly one pace_cube_gather per gather_state, no table upload the second time;
* six processes over torch.distributed (gloo, the emulation library);
* NullComm: the own slot holds the data, the other five the comm's fill value.

Every check is a function of the device; the GPU tier runs it in a child process with a time limit."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import ROOT, build_emu, build_emu_f32  # noqa: E402

X, Y, Z, XI, YI, ZI = "x", "y", "z", "x_interface", "y_interface", "z_interface"
ALL_DIMS = ([X, Y, Z], [XI, Y, Z], [X, YI, Z], [XI, YI, Z], [X, Y, ZI], [X, Y])
N, NZ = 12, 7


def _libs(device):
    from pace_amd import _lib

    if device == "cpu":
        return [_lib.Library(build_emu()), _lib.Library(build_emu_f32())]
    return [_lib.load(), _lib.load(32)]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def field_values(rank, which, dtype=np.float64, n=N, nz=NZ):
    """The whole storage [i, j, k] of field `which` on `rank`: every element different, on every rank."""
    rng = np.random.default_rng(1000 * rank + which)
    return (rng.random((n + 7, n + 7, nz + 1)) + rank).astype(dtype)


def make_quantity(qf, rank, which, dims, dtype=np.float64, n=N, nz=NZ):
    a = field_values(rank, which, dtype, n, nz)
    return qf.from_array(a if len(dims) == 3 else a[:, :, 0], dims, f"unit{which}")


def view_of(q):
    return q.data[tuple(slice(o, o + e) for o, e in zip(q.origin, q.extent))].detach().cpu().numpy()


def stacked(which, dims, extent, dtype=np.float64, n=N, nz=NZ):
    """numpy's answer: the six compute-domain views stacked."""
    out = []
    for r in range(6):
        a = field_values(r, which, dtype, n, nz)
        out.append(a[3:3 + extent[0], 3:3 + extent[1], :extent[2]] if len(dims) == 3 else a[3:3 + extent[0], 3:3 + extent[1], 0])
    return np.stack(out)


def tile_program(comm, libs, device, n=N, nz=NZ):
    """What every rank runs; returns what it saw, for the parent to check."""
    import torch

    from pace_amd.util import CubedSphereCommunicator, Quantity, QuantityFactory, SubtileGridSizer, TILE_DIM

    seen = {}
    for precision, lib in ((64, libs[0]), (32, libs[1])):
        tdtype, dtype = (torch.float64, np.float64) if precision == 64 else (torch.float32, np.float32)
        qf = QuantityFactory(SubtileGridSizer(n, n, nz), device, tdtype)
        cube = CubedSphereCommunicator(comm, device=device, lib=lib)
        r = cube.rank
        for which, dims in enumerate(ALL_DIMS if precision == 64 else ALL_DIMS[:1]):
            key = (precision, which)
            q = make_quantity(qf, r, which, dims, dtype, n, nz)
            g = cube.gather(q)
            if r != 0:
                assert g is None
            else:
                assert g.dims == (TILE_DIM,) + tuple(dims) and g.origin == (0,) * (len(dims) + 1) and g.extent == (6,) + q.extent
                assert g.units == q.units and g.data.dtype == tdtype and g.data.is_contiguous() and g.data.device.type == torch.device(device).type
                seen[key, "gather"] = g.data.cpu().numpy().copy()
                target = Quantity(torch.full((6,) + q.extent, -1.0, dtype=tdtype, device=device), (TILE_DIM,) + tuple(dims), q.units)
            again = cube.gather(q, recv_quantity=target if r == 0 else None)
            if r == 0:
                assert again is target
                seen[key, "gather_in_place"] = target.data.cpu().numpy().copy()
                with pytest.raises(TypeError, match="send_quantity is a required argument on the root rank"):
                    cube.scatter()
                g.data.mul_(2.0)  # what comes back is not what went out
            # scatter into a quantity of the rank's own (its halo must stay as it is) ...
            mine = qf.zeros(dims, "")
            mine._base[...] = -7.0
            back = cube.scatter(g if r == 0 else None, recv_quantity=mine)
            assert back is mine
            seen[key, "scatter"] = view_of(mine).copy()
            inside = torch.zeros(mine.data.shape, dtype=torch.bool)
            inside[tuple(slice(o, o + e) for o, e in zip(mine.origin, mine.extent))] = True
            assert (mine.data.cpu()[~inside] == -7.0).all()
            # ... and into one the communicator allocates
            fresh = cube.scatter(g if r == 0 else None)
            assert fresh.dims == tuple(dims) and fresh.extent == q.extent and fresh.units == q.units and fresh.data.dtype == tdtype
            seen[key, "scatter_fresh"] = view_of(fresh).copy()
        if precision == 32:
            continue
        # the states
        state = {"time": "2016-08-01 00:15:00", "a": make_quantity(qf, r, 0, [X, Y, Z], dtype, n, nz),
                 "b": make_quantity(qf, r, 5, [X, Y], dtype, n, nz), "c": make_quantity(qf, r, 4, [X, Y, ZI], dtype, n, nz),
                 "d": make_quantity(qf, r, 3, [XI, YI, Z], dtype, n, nz)}
        got = cube.gather_state(state, transfer_type=np.float32)
        if r != 0:
            assert got is None
        else:
            assert got["time"] == state["time"] and sorted(got) == sorted(state)
            assert all(isinstance(got[k].data, np.ndarray) and got[k].data.dtype == np.float32 for k in "abcd")
            assert got["a"].dims == (TILE_DIM, X, Y, Z) and got["a"].units == "unit0"
            seen["gather_state32"] = {k: got[k].data.copy() for k in "abcd"}
        whole = cube.gather_state(state)
        rank_state = cube.scatter_state(whole)  # (None off the root)
        assert rank_state["time"] == state["time"] and sorted(rank_state) == sorted(state)
        seen["round_trip"] = all(np.array_equal(_bits(view_of(rank_state[k])), _bits(view_of(state[k]))) for k in "abcd")
        mine = {k: qf.zeros(state[k].dims, "") for k in "ab"}
        rank_state = cube.scatter_state(whole, recv_state=dict(mine))
        assert rank_state["a"] is mine["a"] and rank_state["b"] is mine["b"]
        seen["round_trip_in_place"] = all(np.array_equal(_bits(view_of(rank_state[k])), _bits(view_of(state[k]))) for k in "abcd")
        if r == 0:
            with pytest.raises(TypeError, match="send_state is a required argument on the root rank"):
                cube.scatter_state()
    return seen


def check_results(results, n=N, nz=NZ):
    from pace_amd.util import SubtileGridSizer

    sizer = SubtileGridSizer(n, n, nz)
    for precision, dtype in ((64, np.float64), (32, np.float32)):
        for which, dims in enumerate(ALL_DIMS if precision == 64 else ALL_DIMS[:1]):
            key = (precision, which)
            want = stacked(which, dims, sizer.get_extent(dims) + ((1,) if len(dims) == 2 else ()), dtype, n, nz)
            root = results[0]
            assert np.array_equal(_bits(root[key, "gather"]), _bits(want)), key
            assert np.array_equal(_bits(root[key, "gather_in_place"]), _bits(want)), key
            for r in range(6):
                assert np.array_equal(_bits(results[r][key, "scatter"]), _bits(want[r] * dtype(2.0))), (key, r)
                assert np.array_equal(_bits(results[r][key, "scatter_fresh"]), _bits(want[r] * dtype(2.0))), (key, r)
    for name, which, dims in (("a", 0, [X, Y, Z]), ("b", 5, [X, Y]), ("c", 4, [X, Y, ZI]), ("d", 3, [XI, YI, Z])):
        want = stacked(which, dims, sizer.get_extent(dims) + ((1,) if len(dims) == 2 else ()), np.float64, n, nz).astype(np.float32)
        assert np.array_equal(_bits(results[0]["gather_state32"][name]), _bits(want)), name
    assert all(res["round_trip"] and res["round_trip_in_place"] for res in results)


def check_thread_transports(device):
    from pace_amd.util import run_cube, run_tiles

    libs = _libs(device)
    check_results(run_cube(lambda comm: tile_program(comm, libs, device)))
    check_results(run_cube(lambda comm: tile_program(comm, libs, device), snapshot=True))
    check_results(run_tiles(6, lambda comm: tile_program(comm, libs, device)))


class CountingLib:
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def call(self, name, *args):
        self.calls.append(name)
        return self._lib.call(name, *args)


def check_launch_structure(device):
    """Under run_cube a gather_state (four variables, six tiles: 24 items) is ONE pace_cube_gather for the whole cube, and the
    second call with the same fields uploads no table; gather and scatter are one launch each; with snapshot=True every rank
    launches for itself."""
    import torch

    from pace_amd import _launch
    from pace_amd.util import CubedSphereCommunicator, QuantityFactory, SubtileGridSizer, run_cube

    lib = CountingLib(_libs(device)[0])
    uploads = []
    real_upload = _launch.upload_table

    def counted_upload(arr, dev):
        uploads.append(len(arr))
        return real_upload(arr, dev)

    def program(comm):
        qf = QuantityFactory(SubtileGridSizer(N, N, NZ), device, torch.float64)
        cube = CubedSphereCommunicator(comm, device=device, lib=lib)
        r = cube.rank
        state = {"time": 0, "a": make_quantity(qf, r, 0, [X, Y, Z]), "b": make_quantity(qf, r, 5, [X, Y]),
                 "c": make_quantity(qf, r, 4, [X, Y, ZI]), "d": make_quantity(qf, r, 3, [XI, YI, Z])}
        counts = []

        def counted(fn):
            comm.barrier()
            if r == 0:
                lib.calls.clear()
                uploads.clear()
            comm.barrier()
            out = fn()
            comm.barrier()
            counts.append((collections.Counter(lib.calls), list(uploads)))
            return out

        counted(lambda: cube.gather_state(state))
        counted(lambda: cube.gather_state(state))
        g = counted(lambda: cube.gather(state["a"]))
        counted(lambda: cube.scatter(g, recv_quantity=state["a"]))
        whole = counted(lambda: cube.gather_state(state, transfer_type=np.float32))
        counted(lambda: cube.scatter_state(whole, recv_state=state))
        return counts

    _launch.upload_table = counted_upload
    try:
        fused = run_cube(program)
        snap = run_cube(program, snapshot=True)
    finally:
        _launch.upload_table = real_upload
    table = lambda items: (48 * items + 4 * (items + 1) + 7) // 8 * 8  # noqa: E731
    for counts in fused:
        assert counts[0] == ({"pace_cube_gather": 1}, [table(24)]), counts[0]
        assert counts[1] == ({"pace_cube_gather": 1}, []), counts[1]
        assert counts[2] == ({"pace_cube_gather": 1}, [table(6)]), counts[2]
        assert counts[3] == ({"pace_cube_scatter": 1}, [table(6)]), counts[3]
        assert counts[4] == ({"pace_cube_gather": 1}, []), counts[4]  # (the table does not depend on the dense type)
        assert counts[5] == ({"pace_cube_scatter": 1}, [table(24)]), counts[5]
    for counts in snap:
        assert counts[0] == ({"pace_cube_gather": 6}, [table(4)] * 6), counts[0]
        assert counts[1] == ({"pace_cube_gather": 6}, []), counts[1]
        assert counts[3] == ({"pace_cube_scatter": 6}, [table(1)] * 6), counts[3]


def check_null_comm(device):
    """NullComm: the rank's own slot holds its data, the other five the fill value; a rank is its own root."""
    import torch

    from pace_amd.util import CubedSphereCommunicator, NullComm, QuantityFactory, SubtileGridSizer

    lib = _libs(device)[0]
    qf = QuantityFactory(SubtileGridSizer(N, N, NZ), device, torch.float64)
    for rank, fill in ((0, 0.0), (4, -3.5)):
        cube = CubedSphereCommunicator(NullComm(rank, 6, fill_value=fill), device=device, lib=lib)
        q = make_quantity(qf, rank, 1, [XI, Y, Z])
        g = cube.gather(q)
        got = g.data.cpu().numpy()
        for slot in range(6):
            assert np.array_equal(got[slot], view_of(q) if slot == rank else np.full(q.extent, fill)), (rank, slot)
        state = cube.gather_state({"time": 3, "q": q, "p": make_quantity(qf, rank, 5, [X, Y])})
        assert state["time"] == 3 and np.array_equal(state["q"].data[rank], view_of(q))
        assert (np.delete(state["q"].data, rank, axis=0) == fill).all() and (np.delete(state["p"].data, rank, axis=0) == fill).all()
        back = cube.scatter(g)
        assert np.array_equal(_bits(view_of(back)), _bits(view_of(q)))


def test_thread_transports_emulated():
    check_thread_transports("cpu")


def test_launch_structure_emulated():
    check_launch_structure("cpu")


def test_null_comm_emulated():
    check_null_comm("cpu")


_WORKER = r"""
import os, sys, pickle
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import torch.distributed as dist
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:{port}", rank=int(sys.argv[1]), world_size=6)
from pace_amd import _lib
from pace_amd.util import TorchDistComm
import test_communicator_gather as t
libs = [_lib.Library(os.path.join({root!r}, "tests", "emu", name)) for name in ("libpace_emu.so", "libpace_emu_f32.so")]
out = t.tile_program(TorchDistComm(), libs, "cpu", 12, 2)
pickle.dump(out, open(sys.argv[2], "wb"))
dist.barrier(); dist.destroy_process_group()
"""


def test_six_processes_gloo(tmp_path):
    """One process per tile over torch.distributed (gloo and the emulation here; the same code path runs RCCL on the GPUs):
    every rank packs with one launch, the collective moves the dense tensors, the objects go through broadcast_object_list."""
    import pickle

    import test_halo

    build_emu()
    build_emu_f32()
    port = 31500 + os.getpid() % 2000
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, port=port))
    procs = [subprocess.Popen([sys.executable, str(script), str(r), str(tmp_path / f"out{r}.pkl")]) for r in range(6)]
    test_halo._wait_all(procs, 300)
    check_results([pickle.load(open(tmp_path / f"out{r}.pkl", "rb")) for r in range(6)], 12, 2)


# ---- the GPU tier: each check in a child process with a time limit --------------------------------------------------------------
def _in_child(what, timeout=300):
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); "
            f"import test_communicator_gather as t; t.check_{what}('cuda')")
    p = subprocess.run([sys.executable, "-X", "faulthandler", "-c", code], capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-6000:])


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["thread_transports", "launch_structure", "null_comm"])
def test_on_the_gpu(what):
    _in_child(what)
