"""The whole cubed sphere on one device: pace_halo_cube (one launch moves every strip of every field of every tile),
DeviceCubeComm / run_cube and the fused path of HaloUpdater / VectorInterfaceHaloUpdater.

* the kernel alone against a numpy restatement of its table, over the whole raw storage (sentinels everywhere outside the compute
  domains), both libraries, every staggering, and again under guard pages;
* run_cube against the reference run (tests/golden/halo_native_c12.npz) and against oracle/halo.py, with two updaters in flight;
* the launch structure of an update: one pace_halo_cube call for the whole cube, no pack, no unpack, no upload;
* one AcousticDynamics call (and, on the device, one DynamicalCore step) under run_cube equals the run under run_tiles bit for
  bit: the product's own call sequences keep the fused path's contract;
* the host checks of a table and of the streams.

Every check is a function of (library, device); the CPU tier calls it with the emulation library, the GPU tier in a child
process with a time limit, as tests/test_halo.py does."""
import collections
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers  # noqa: E402
import test_halo  # noqa: E402
from helpers import ROOT, build_emu, build_emu_f32  # noqa: E402

SENTINEL = -12345.0
X, Y, Z, XI, YI, ZI = "x", "y", "z", "x_interface", "y_interface", "z_interface"
# centre, corner, z-interface (nk + 1 levels), 2-D as scalars; the x- and y-interface staggerings as the components of a D-grid
# and of a C-grid vector (between rotated tiles one becomes the other: only a vector update can move them)
SCALAR_DIMS = ([X, Y, Z], [XI, YI, Z], [X, Y, ZI], [X, Y])
VECTOR_DIMS = ([X, YI, Z], [XI, Y, Z], [XI, Y, Z], [X, YI, Z])  # x of the D-grid pair, x of the C-grid pair, then their y


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


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------------
def _raw(q):
    """The raw storage [k][j][i] of a Quantity (row padding included) as a numpy array with three axes."""
    a = q._base.detach().cpu().numpy().copy()
    return a.reshape((1,) + a.shape) if a.ndim == 2 else a


def _filled(qf, dims, rng):
    """A field whose whole raw storage is the sentinel, with values in its compute domain."""
    q = qf.zeros(dims, "")
    q._base[...] = SENTINEL
    window = tuple(slice(o, o + e) for o, e in zip(q.origin, q.extent))
    q.data[window] = qf_tensor(qf, rng.random(q.extent) + 0.5)
    return q


def qf_tensor(qf, a):
    import torch

    return torch.as_tensor(np.asarray(a), dtype=qf.real, device=qf.device)


def kernel_case(lib, device, n, nz, n_points, seed):
    """Six tiles of C<n> x <nz> fields of every staggering, as a scalar group and as a vector group; the table is what the fused
    path builds; the expectation applies the table entry by entry with numpy.  Returns the number of entries."""
    import torch

    from pace_amd import _lib
    from pace_amd.util import CubedSphereCommunicator, NullComm, QuantityFactory, SubtileGridSizer
    from pace_amd.util import halo

    rng = np.random.default_rng(seed)
    sizer = SubtileGridSizer.from_tile_params(nx_tile=n, ny_tile=n, nz=nz, n_halo=3, extra_dim_lengths={}, layout=(1, 1))
    qf = QuantityFactory(sizer, device=device, dtype=torch.float32 if lib.real_bytes == 4 else torch.float64)
    cubes = [CubedSphereCommunicator(NullComm(r, 6), device=device, lib=lib) for r in range(6)]
    total = 0
    for vector in (False, True):
        if vector:
            dims = VECTOR_DIMS
            spec = [qf.get_quantity_halo_spec(d, n_halo=n_points) for d in dims]
            updaters = [halo.HaloUpdater(c, 1, spec[:2], spec[2:]) for c in cubes]
        else:
            dims = SCALAR_DIMS
            updaters = [halo.HaloUpdater(c, 1, [qf.get_quantity_halo_spec(d, n_halo=n_points) for d in dims]) for c in cubes]
        fields = [[_filled(qf, d, rng) for d in dims] for _ in range(6)]
        ptrs = tuple(tuple(q.ptr for q in fs) for fs in fields)
        arr, count = halo._build_cube_table(updaters, ptrs)
        assert count == 6 * 4 * len(dims)
        before = {q.ptr: _raw(q) for fs in fields for q in fs}
        expected = {p: a.copy() for p, a in before.items()}
        written = {p: np.zeros(a.shape, dtype=bool) for p, a in before.items()}
        real = np.float32 if lib.real_bytes == 4 else np.float64
        for x in arr[:count]:
            a, b, k = np.meshgrid(np.arange(x.na), np.arange(x.nb), np.arange(x.nk), indexing="ij")
            values = (x.sign * before[x.src][k, x.j0 + a * x.dj_a + b * x.dj_b, x.i0 + a * x.di_a + b * x.di_b].astype(np.float64)).astype(real)
            expected[x.dst][k, x.rj0 + b, x.ri0 + a] = values
            assert not written[x.dst][k, x.rj0 + b, x.ri0 + a].any()  # (no halo point is written twice)
            written[x.dst][k, x.rj0 + b, x.ri0 + a] = True
        keep = halo._upload_table(arr, qf.device)
        lib.call("pace_halo_cube", C.byref(updaters[0]._geom), C.c_void_p(keep[0].data_ptr()), count, _stream(device))
        if device != "cpu":
            torch.cuda.synchronize()
        for t, fs in enumerate(fields):
            for d, q in zip(dims, fs):
                got = _raw(q)
                assert got.dtype == real
                assert np.array_equal(got, expected[q.ptr]), (n, nz, n_points, vector, t, d)
                # what that means, spelled out: the compute domain is untouched, the edge halos within n_points hold values
                # (none of them the sentinel), and the corner blocks, the halo beyond n_points, the levels the field does not
                # have, the row padding and the spare row still hold the sentinel
                xi, yi = int(XI in d), int(YI in d)
                nk = (nz + 1 if ZI in d else nz) if len(d) == 3 else 1
                edge = np.zeros(got.shape, dtype=bool)
                edge[:nk, 3:3 + n + yi, 3 - n_points:3] = edge[:nk, 3:3 + n + yi, 3 + n + xi:3 + n + xi + n_points] = True
                edge[:nk, 3 - n_points:3, 3:3 + n + xi] = edge[:nk, 3 + n + yi:3 + n + yi + n_points, 3:3 + n + xi] = True
                assert np.array_equal(written[q.ptr], edge), (n, nz, n_points, vector, t, d)
                assert not (got[edge] == SENTINEL).any()
                own = np.zeros(got.shape, dtype=bool)
                own[:nk, 3:3 + n + yi, 3:3 + n + xi] = True
                assert np.array_equal(got[own], before[q.ptr][own])
                assert (got[~(edge | own)] == real(SENTINEL)).all()
        total += count
    return total


def check_kernel(device):
    """C12 and C13 (an odd size), 1 / 2 / 7 levels, 1 / 2 / 3 halo points, both libraries; the argument errors."""
    from pace_amd import _lib

    for lib in _libs(device):
        seed = 0
        for n in (12, 13):
            for nz in (1, 2, 7):
                for n_points in (1, 2, 3):
                    seed += 1
                    assert kernel_case(lib, device, n, nz, n_points, seed) == 6 * 4 * (len(SCALAR_DIMS) + len(VECTOR_DIMS))
        geom = _lib.Geom(12, 7, 32, 0, 32 * 19)
        lib.call("pace_halo_cube", C.byref(geom), None, 0, _stream(device))  # n == 0: nothing to do, no table needed
        with pytest.raises(_lib.PaceError, match="invalid argument"):
            lib.call("pace_halo_cube", C.byref(geom), None, 3, _stream(device))
        with pytest.raises(_lib.PaceError, match="invalid argument"):
            lib.call("pace_halo_cube", C.byref(geom), None, -1, _stream(device))
        with pytest.raises(_lib.PaceError, match="invalid argument"):
            lib.call("pace_halo_cube", None, None, 0, _stream(device))


def test_kernel_against_numpy_emulated():
    check_kernel("cpu")


@pytest.mark.parametrize("mode", ["over", "under"])
def test_kernel_under_guard_pages(mode):
    """The same cases in a child process in which every field and the table itself lie against an inaccessible page
    (tests/guard.py): a strip or a table row read or written one element outside its array ends the child."""
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
            f"import guard, test_halo_cube\nwith guard.guarded({mode!r}):\n    test_halo_cube.check_kernel('cpu')\n")
    p = subprocess.run([sys.executable, "-X", "faulthandler", "-c", code], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PACE_EMU_GUARD="1"))
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])


# ---- 2. against the reference run ---------------------------------------------------------------------------------------------
def check_reference_run(device):
    from pace_amd.util import run_cube

    lib = _libs(device)[0]
    n, nz, base, exp = test_halo.native_fixture()
    for snapshot in (False, True):
        results = run_cube(lambda comm: test_halo.native_tile_program(comm, lib, base, n, nz, device=device), snapshot=snapshot)
        test_halo.check_native(results, exp)
        base5 = test_halo._base()
        results = run_cube(lambda comm: test_halo.tile_program(comm, lib, base5, device=device), snapshot=snapshot)
        test_halo._check(results, base5)  # (two updaters in flight, waited out of order)


def test_run_cube_equals_the_reference_run_emulated():
    check_reference_run("cpu")


# ---- 3. launch structure ------------------------------------------------------------------------------------------------------
class CountingLib:
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def call(self, name, *args):
        self.calls.append(name)
        return self._lib.call(name, *args)


def check_launch_structure(device):
    """The nine-field group (216 strips): after the warm-up update one pace_halo_cube call per update for the WHOLE cube and
    nothing else, no upload; a storage swap costs one more table, once; with snapshot=True the counts are ThreadComm's."""
    from pace_amd.util import CubedSphereCommunicator, QuantityFactory, SubtileGridSizer, run_cube
    from pace_amd.util import halo

    lib = CountingLib(_libs(device)[0])
    uploads = []
    real_upload = halo._upload_table

    def counted_upload(arr, dev):
        uploads.append(len(arr))
        return real_upload(arr, dev)

    n, nz = 12, 5
    rng = np.random.default_rng(3)
    values = [[rng.random((n + 7, n + 7, nz + 1)) for _ in range(10)] for _ in range(6)]
    want = [[a.copy() for a in values[t][:9]] for t in range(6)]
    from oracle import halo as oh

    for f in range(9):
        oh.halo_update([want[t][f] for t in range(6)], n, nk=nz)

    def program(comm):
        sizer = SubtileGridSizer.from_tile_params(nx_tile=n, ny_tile=n, nz=nz, n_halo=3, extra_dim_lengths={}, layout=(1, 1))
        qf = QuantityFactory(sizer, device=device)
        cube = CubedSphereCommunicator(comm, device=device, lib=lib)
        r = cube.rank
        qs = [qf.from_array(values[r][f], [X, Y, Z], "") for f in range(10)]
        up = cube.get_scalar_halo_updater([qf.get_quantity_halo_spec([X, Y, Z])] * 9)
        counts = []

        def update():
            comm.barrier()
            if r == 0:
                lib.calls.clear()
                uploads.clear()
            comm.barrier()
            up.update(qs[:9])
            comm.barrier()
            counts.append((collections.Counter(lib.calls), list(uploads)))

        update()  # warm-up: the table is built and uploaded
        update()  # steady state
        got = [q.numpy() for q in qs[:9]]
        qs[0].swap_storage(qs[9])  # a ping-pong variant: another table, once
        update()
        qs[0].swap_storage(qs[9])
        update()
        return counts, got

    halo._upload_table = counted_upload
    try:
        fused = run_cube(program)
        snap = run_cube(program, snapshot=True)
    finally:
        halo._upload_table = real_upload
    for t in range(6):
        counts, got = fused[t]
        assert counts[0] == ({"pace_halo_cube": 1}, [216]), counts[0]
        assert counts[1] == ({"pace_halo_cube": 1}, []), counts[1]
        assert counts[2] == ({"pace_halo_cube": 1}, [216]), counts[2]
        assert counts[3] == ({"pace_halo_cube": 1}, []), counts[3]
        for f in range(9):
            assert np.array_equal(got[f], want[t][f]), (t, f)
        counts, got = snap[t]
        for c in counts:  # ThreadComm's: every rank packs once and unpacks once
            assert c == ({"pace_halo_pack": 6, "pace_halo_unpack": 6}, []), c
        for f in range(9):
            assert np.array_equal(got[f], want[t][f]), (t, f)


def test_launch_structure_emulated():
    check_launch_structure("cpu")


# ---- 4. the contract in the product's own sequences -----------------------------------------------------------------------------
def _same(a, b, what):
    for t in range(6):
        assert set(a[t]) == set(b[t])
        for k in a[t]:
            assert np.array_equal(a[t][k], b[t][k], equal_nan=True), (what, t, k)


def check_acoustic(device):
    """One AcousticDynamics call (the fixture's n_split >= 2) on six C12 tiles under run_cube and under run_tiles: every output
    field over its whole extent, bit for bit."""
    from pace_amd.util import run_cube, run_tiles

    lib = _libs(device)[0]
    fixes = [helpers.acoustic_fixture(t) for t in range(6)]
    assert int(fixes[0]["n_split"]) >= 2

    def program(comm):
        return helpers.run_acoustic_tile(comm, lib, device, fixes[comm.Get_rank()], 12, 79)

    _same(run_cube(program), run_tiles(6, program), "AcousticDynamics")


def check_dycore(device):
    """One DynamicalCore.step_dynamics (acoustic loop, tracer advection, remapping, c2l_ord) under both communicators."""
    from pace_amd.util import run_cube, run_tiles

    lib = _libs(device)[0]
    fa = [helpers.golden(f"acoustic_c12_tile{t}.npz") for t in range(6)]
    fd = [helpers.golden(f"dycore_c12_tile{t}.npz") for t in range(6)]

    def program(comm):
        return helpers.run_dycore_tile(comm, lib, device, fa[comm.Get_rank()], fd[comm.Get_rank()], 12, 79)

    _same(run_cube(program), run_tiles(6, program), "DynamicalCore.step_dynamics")


def test_acoustic_dynamics_under_both_communicators_emulated():
    check_acoustic("cpu")


# ---- 6. host checks -----------------------------------------------------------------------------------------------------------
def test_table_checks_refuse_before_any_launch():
    from pace_amd import _lib
    from pace_amd.util.halo import check_cube_table

    geom = _lib.Geom(12, 5, 32, 0, 32 * 19)

    def entry(**over):
        x = _lib.HaloXfer()
        x.dst, x.src, x.ri0, x.rj0, x.na, x.nb, x.nk = 0x1000, 0x2000, 0, 3, 3, 12, 5
        x.i0, x.j0, x.di_a, x.dj_a, x.di_b, x.dj_b, x.sign = 12, 3, 1, 0, 0, 1, 1.0
        for k, v in over.items():
            setattr(x, k, v)
        return x

    check_cube_table(geom, [entry()])
    check_cube_table(geom, [entry(), entry(dst=0x2000, src=0x1000)])  # two fields that feed each other's halos
    with pytest.raises(ValueError, match="outside"):
        check_cube_table(geom, [entry(ri0=17)])  # the destination ends one column past the 19 the storage has
    with pytest.raises(ValueError, match="outside"):
        check_cube_table(geom, [entry(i0=1, di_a=-1)])  # the source map runs below 0
    with pytest.raises(ValueError, match="outside"):
        check_cube_table(geom, [entry(j0=14, dj_b=1)])  # ... and past the last row
    with pytest.raises(ValueError, match="outside"):
        check_cube_table(geom, [entry(nk=7)])  # more levels than nk + 1
    with pytest.raises(ValueError, match="null"):
        check_cube_table(geom, [entry(src=0)])
    with pytest.raises(ValueError, match="reads"):
        check_cube_table(geom, [entry(), entry(dst=0x2000, src=0x3000, ri0=12)])  # writes the strip the first entry reads
    with pytest.raises(ValueError, match="reads"):
        check_cube_table(geom, [entry(dst=0x1000, src=0x1000, i0=2)])  # one entry, overlapping itself by one column


def check_refusals(device):
    """A table that fails the host checks is refused by the rank that would launch it, before any launch; so are tiles that
    started on different streams."""
    from pace_amd.util import CubedSphereCommunicator, QuantityFactory, SubtileGridSizer, run_cube
    from pace_amd.util import halo

    lib = CountingLib(_libs(device)[0])
    n, nz = 12, 3

    def program(bad):
        def run(comm):
            sizer = SubtileGridSizer.from_tile_params(nx_tile=n, ny_tile=n, nz=nz, n_halo=3, extra_dim_lengths={}, layout=(1, 1))
            qf = QuantityFactory(sizer, device=device)
            cube = CubedSphereCommunicator(comm, device=device, lib=lib)
            q = qf.zeros([X, Y, Z], "")
            up = cube.get_scalar_halo_updater([qf.get_quantity_halo_spec([X, Y, Z])])
            if cube.rank == 3:
                bad(cube, up)
            up.update([q])
        return run

    def other_stream(cube, up):
        if device == "cpu":
            cube.stream = lambda: C.c_void_p(4096)
        else:
            import torch

            side = torch.cuda.Stream()
            cube.stream = lambda: C.c_void_p(side.cuda_stream)

    def overlapping(cube, up):  # tile 3 would send what lies in its own west halo
        for strips in up._msgs.send.values():
            strips[0].i0 -= 3 if strips[0].di_a == 1 else 0
            strips[0].j0 -= 3 if strips[0].dj_a == 1 else 0

    def outside(cube, up):
        for strips in up._msgs.send.values():
            strips[0].i0 += 100

    for bad, message in ((other_stream, "different streams"), (outside, "outside the field's storage")):
        lib.calls.clear()
        with pytest.raises(RuntimeError, match=message):
            run_cube(program(bad))
        assert lib.calls == []
    # an overlap needs one field on both sides of an entry: all six tiles hand over the SAME storage
    shared = {}

    def shared_program(comm):
        sizer = SubtileGridSizer.from_tile_params(nx_tile=n, ny_tile=n, nz=nz, n_halo=3, extra_dim_lengths={}, layout=(1, 1))
        qf = QuantityFactory(sizer, device=device)
        cube = CubedSphereCommunicator(comm, device=device, lib=lib)
        q = shared.setdefault("q", qf.zeros([X, Y, Z], ""))
        up = cube.get_scalar_halo_updater([qf.get_quantity_halo_spec([X, Y, Z])])
        if cube.rank == 3:
            overlapping(cube, up)
        up.update([q])

    lib.calls.clear()
    with pytest.raises(RuntimeError, match="reads from the same field"):
        run_cube(shared_program)
    assert lib.calls == []
    assert halo.CUBE_TABLE_CACHE >= 2


def test_refusals_emulated():
    check_refusals("cpu")


def test_other_world_sizes_keep_the_error():
    from pace_amd import _lib
    from pace_amd.util import CubedSphereCommunicator, DeviceCubeComm, ThreadComm
    from pace_amd.util.comm import _World

    assert issubclass(DeviceCubeComm, ThreadComm)
    with pytest.raises(ValueError, match="ranks"):
        CubedSphereCommunicator(DeviceCubeComm(_World(4), 0), device="cpu", lib=_lib.Library(build_emu()))


# ---- the GPU tier: each check in a child process with a time limit --------------------------------------------------------------
def _in_child(what, timeout=300):
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); "
            f"import test_halo_cube; test_halo_cube.check_{what}('cuda')")
    p = subprocess.run([sys.executable, "-X", "faulthandler", "-c", code], capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-6000:])


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["kernel", "reference_run", "launch_structure", "acoustic", "dycore", "refusals"])
def test_on_the_gpu(what):
    _in_child(what)
