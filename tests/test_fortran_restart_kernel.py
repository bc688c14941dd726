"""pace_pe_peln_from_delp (pace_amd/csrc/k_state.hip): the interface pressures of a state read from a Fortran restart,
pe = ptop + the sum of delp above and peln = log(pe), on every column of the WHOLE storage (the reference writes .data:
driver/pace/driver/initialization.py:422-442).

One thread per column, the plane flattened over its padded rows in blocks of 64 lanes, so the shapes are

    C12 x 63    the fixture's delp of tile 2, random positive values planted in the halo, the stagger row and level nz
    C13 x 1     one layer: pe = (ptop, ptop + delp)
    C13 x 2
    C68 x 5     a row of 75 columns is more than one 64-lane block (row stride 80: blocks straddle rows)
    C12 x 130   past any 128-level assumption

What is asserted, over the whole raw storage, row padding included:

    pe     equal, bit for bit, to the sequential numpy restatement ptop + concatenate(0, cumsum(delp[..., :nz])); the float32
           library: to that float64 restatement (of the float32 delp it holds) cast to float32;
           a sentinel in the row padding unchanged;
           against the reference's own expression, ptop + np.sum(delp[:, :, :level], 2) (numpy sums the contiguous level axis
           pairwise), a relative difference of at most 2 (nz - 1) 2^-53: two summation orders of nz positive terms, each within
           (nz - 1) 2^-53 of the exact sum;
    peln   against np.log of the device's own pe: at most LOG_ULPS = 0.546 + 1 ulp -- the documented error of the device's log
           (lean_log, profiles/r06_transcendental_accuracy.txt) plus one ulp for numpy's; the float32 library: one float32 ulp
           (the logarithm is taken of the double before it is narrowed: half an ulp of float32 plus the 6e-8 that the rounding of
           pe moves its logarithm).

Under emulation the same cases also run with every allocation against an inaccessible page (tests/guard.py): a store past the
last row, into the row padding of the last row or before the first element ends the child.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import restart_helpers as rh  # noqa: E402
from helpers import build_emu, build_emu_f32  # noqa: E402

GUARDED = os.environ.get("PACE_GUARD_MODE")  # (a child run of test_pe_peln_with_guard_pages)
# (n, nz, ptop); the first takes the fixture's delp
SHAPES = [(12, 63, rh.PTOP), (13, 1, 300.0), (13, 2, 300.0), (68, 5, 1.0), (12, 130, 64.247)]
IDS = ["%dx%d" % s[:2] for s in SHAPES]


@pytest.fixture(scope="module")
def emu_lib():
    from pace_amd import _lib

    return _lib.Library(build_emu())


@pytest.fixture(scope="module")
def emu_lib_f32():
    from pace_amd import _lib

    return _lib.Library(build_emu_f32())


@pytest.fixture(scope="module")
def lib():
    from pace_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def lib_f32():
    from pace_amd import _lib

    return _lib.load(32)


def delp_of(n, nz):
    return rh.fixture_delp_storage() if (n, nz) == (rh.N, rh.NZ) else rh.synthetic_delp_storage(n, nz, seed=n * 1000 + nz)


def ulps(got, ref):
    """|got - ref| in units of the spacing at the larger of the two."""
    return np.abs(got - ref) / np.spacing(np.maximum(np.abs(got), np.abs(ref)))


def check_shape(lib, device, n, nz, ptop):
    """-> the figures that are printed and recorded."""
    ni = n + 7
    delp = delp_of(n, nz)
    assert delp.min() > 0
    pe, peln, stored = rh.run_pe_peln(lib, device, n, nz, delp, ptop)
    assert pe.shape == peln.shape and pe.shape[:2] == (nz + 1, ni) and pe.shape[2] >= ni and pe.shape[2] % 16 == 0
    # the row padding is neither written ...
    assert np.all(pe[:, :, ni:] == rh.SENTINEL) and np.all(peln[:, :, ni:] == rh.SENTINEL)
    # ... nor anything left unwritten inside the storage
    pe, peln = pe[:, :, :ni], peln[:, :, :ni]
    assert not np.any(pe == rh.SENTINEL) and not np.any(peln == rh.SENTINEL)
    want = rh.pe_restatement(stored, ptop, n, nz)
    figures = {}
    if lib.real_bytes == 8:
        assert np.array_equal(stored[:, :, :ni], delp)
        different = int(np.count_nonzero(pe != want))
        assert different == 0, different
        reference = rh.pe_reference_expression(stored, ptop, n, nz)
        figures["pe_vs_reference"] = float(np.max(np.abs(pe - reference) / reference))
        bound = 2 * (nz - 1) * 2.0 ** -53
        print(f"\nC{n} x {nz}: pe against the reference's expression {figures['pe_vs_reference']:.3e} (bound {bound:.3e})")
        assert figures["pe_vs_reference"] <= bound
        figures["peln_ulps"] = float(np.max(ulps(peln, np.log(pe))))
        print(f"C{n} x {nz}: peln against np.log(pe) {figures['peln_ulps']:.4f} ulp (bound {rh.LOG_ULPS})")
        assert figures["peln_ulps"] <= rh.LOG_ULPS
    else:
        assert pe.dtype == np.float32 and peln.dtype == np.float32
        different = int(np.count_nonzero(pe != want.astype(np.float32)))
        assert different == 0, different
        ref = np.log(pe.astype(np.float64))
        figures["peln_ulps32"] = float(np.max(np.abs(peln.astype(np.float64) - ref) / np.spacing(np.abs(ref).astype(np.float32))))
        print(f"\nC{n} x {nz} float32: peln against np.log(pe) {figures['peln_ulps32']:.4f} float32 ulp (bound 1)")
        assert figures["peln_ulps32"] <= 1.0
    return figures


@pytest.mark.parametrize("n,nz,ptop", SHAPES, ids=IDS)
def test_pe_peln_emulated(emu_lib, emu_lib_f32, n, nz, ptop):
    check_shape(emu_lib, "cpu", n, nz, ptop)
    check_shape(emu_lib_f32, "cpu", n, nz, ptop)


@pytest.mark.gpu
@pytest.mark.parametrize("n,nz,ptop", SHAPES, ids=IDS)
def test_pe_peln_gpu(lib, lib_f32, n, nz, ptop):
    check_shape(lib, "cuda", n, nz, ptop)
    check_shape(lib_f32, "cuda", n, nz, ptop)


@pytest.mark.parametrize("mode", ["over", "under"])
def test_pe_peln_with_guard_pages(mode):
    """The emulated cases of this file in a child pytest whose every allocation ends at (over) or starts right after (under) an
    inaccessible page (tests/guard.py, tests/test_guard_pages.py)."""
    if GUARDED:
        return  # (this IS the child)
    import test_guard_pages

    passed, tail = test_guard_pages._guarded_pytest(mode, ["test_fortran_restart_kernel.py"])
    for case in ["test_pe_peln_emulated[%s]" % i for i in IDS] + ["test_argument_errors_emulated"]:
        assert any(t.endswith("::" + case) for t in passed), (case, tail)


# ---- argument errors ------------------------------------------------------------------------------------------------------------
def check_argument_errors(lib, device):
    from pace_amd import _lib
    from pace_amd.util.grid import geom_struct

    n, nz = 12, 3
    qf = rh.factory(lib, device, n, nz)
    delp, pe, peln = (qf.zeros(["x", "y", "z"], "") for _ in range(3))
    geom = geom_struct(qf)

    def call(g=geom, a=delp.ptr, b=pe.ptr, c=peln.ptr):
        lib.call("pace_pe_peln_from_delp", C.byref(g) if g is not None else None, a, 100.0, b, c, rh.stream_of(device))

    call()  # the arguments themselves are fine
    for kwargs in (dict(a=None), dict(b=None), dict(c=None), dict(g=None),
                   dict(g=_lib.Geom(n, 0, geom.sj, 0, geom.sk)), dict(g=_lib.Geom(n, -1, geom.sj, 0, geom.sk)),
                   dict(g=_lib.Geom(0, nz, geom.sj, 0, geom.sk)), dict(g=_lib.Geom(n, nz, n + 6, 0, geom.sk))):
        with pytest.raises(_lib.PaceError, match="invalid argument"):
            call(**kwargs)
    rh.sync(device)
    assert float(pe.numpy()[0, 0, 0]) == 100.0 and float(pe.numpy()[n + 6, n + 6, nz]) == 100.0


def test_argument_errors_emulated(emu_lib, emu_lib_f32):
    check_argument_errors(emu_lib, "cpu")
    check_argument_errors(emu_lib_f32, "cpu")


@pytest.mark.gpu
def test_argument_errors_gpu(lib, lib_f32):
    check_argument_errors(lib, "cuda")
    check_argument_errors(lib_f32, "cuda")
