"""The argument tables of k_fvt_scalars and k_divdamp_fused (csrc/common.h PACE_KERNARG): each kernel takes ONE struct by value
and reads it in place from the kernel-argument segment.  A member read at a wrong offset is a wild pointer, and a table that
is stale, cached or misaligned gives wrong fields, so:

* CPU: the built library's metadata says what the device code assumes -- one explicit argument, by value, at offset 0;
* GPU: d_sw at sizes where every tile kind of the fused kernel runs (C96 x 13: 3 x 4 tiles of 32 x 24, corner, edge and interior;
  C48 x 8: the 16 x 24 tile shape), ONE operator called twice with another dt, the other output contract and the swapped
  buffers, against the oracle bit for bit; the fused kernel launched alone (the form that copies the winds' halo itself);
  the float32-storage build against the float64 one.
"""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import DSW_ARGS, DSW_CFG, ROOT, Env, compare, dsw_window, golden, oracle_grid

DSW_DEAD = ("delpc", "divgd", "uc", "vc")  # unspecified under skip_dead_outputs (include/pace_hip.h PACE_DSW_SKIP_DEAD_OUTPUTS)
DT2 = 0.75  # the second call's time step as a fraction of the first's


def live_window(name, n, nk):
    """What a call with skip_dead_outputs specifies (pace_amd/tile.py dsw_live_window): the transported scalars on the compute domain."""
    from pace_amd.tile import dsw_live_window

    return dsw_live_window(name, n, nk)


def column(nz):
    return {k: np.ascontiguousarray(v[:nz]) for k, v in golden("column_namelist_c12.npz").items()}


_state, _oracle = {}, {}


def state(n, nz):
    if (n, nz) not in _state:
        from pace_amd import synthetic

        m = synthetic.tile_metrics(n, nz)
        _state[(n, nz)] = (m, synthetic.acoustic_state(m, n, nz))
    return _state[(n, nz)]


def oracle_two_calls(n, nz):
    """The oracle's d_sw twice on the synthetic tile -- the full contract with dt, then (the divergence damping's work fields set
    back, as c_sw would) with DT2 * dt -- computed once per size and never modified: ({name: array} after call 1, after call 2)."""
    if (n, nz) not in _oracle:
        from oracle import dgrid_sw

        m, s = state(n, nz)
        g = oracle_grid(m, n, nz)
        st = dgrid_sw.DSWState(s["u"].shape)
        a = {k: s[k].copy() for k in DSW_ARGS}
        dgrid_sw.d_sw(g, column(nz), DSW_CFG, st, *[a[k] for k in DSW_ARGS], s["dt"])
        first = {k: v.copy() for k, v in a.items()}
        for k in DSW_DEAD:
            a[k][...] = s[k]
        dgrid_sw.d_sw(g, column(nz), DSW_CFG, st, *[a[k] for k in DSW_ARGS], DT2 * s["dt"])
        for d in (first, a):
            for v in d.values():
                v.setflags(write=False)
        _oracle[(n, nz)] = (first, a)
    return _oracle[(n, nz)]


def make_operator(lib, device, n, nz, **kw):
    from pace_amd.fv3core import DGridShallowWaterLagrangianDynamicsConfig
    from pace_amd.fv3core.stencils.d_sw import DGridShallowWaterLagrangianDynamics

    m, s = state(n, nz)
    env = Env(lib, device, m, n, nz)
    op = DGridShallowWaterLagrangianDynamics(env.stencil_factory, env.qf, env.grid_data, env.damping,
                                             {k: env.kq(v) for k, v in column(nz).items()}, False, False,
                                             DGridShallowWaterLagrangianDynamicsConfig(**DSW_CFG), **kw)
    return env, op, s


def synchronize(device):
    if device != "cpu":
        import torch

        torch.cuda.synchronize()


def device_two_calls(lib, device, n, nz, calls=2):
    """ONE operator with `swap_scalar_storage` called like oracle_two_calls: full contract, then skip_dead_outputs with the
    buffers the first call swapped in.  Returns the fields after each call."""
    env, op, s = make_operator(lib, device, n, nz, swap_scalar_storage=True)
    f = {k: env.q3(s[k]) for k in DSW_ARGS}
    res = []
    for call in range(calls):
        if call == 1:
            for k in DSW_DEAD:
                f[k].set(s[k])
        op(*[f[k] for k in DSW_ARGS], float(s["dt"]) * (DT2 if call else 1.0), skip_dead_outputs=bool(call))
        synchronize(device)
        res.append({k: f[k].numpy().copy() for k in DSW_ARGS})
    assert op._pingpong and op._wind_outputs, "the fused scalar + wind kernel is the one under test"
    return res


def check_two_calls(lib, device, n, nz):
    ref = oracle_two_calls(n, nz)
    got = device_two_calls(lib, device, n, nz)
    for k in DSW_ARGS:
        if k == "zh":
            continue
        W = dsw_window(k, n, nz)
        print(f"call 1 {k}: {compare(ref[0][k][W], got[0][k][W]):.3e}")
        assert np.array_equal(ref[0][k][W], got[0][k][W]), ("call 1", k, compare(ref[0][k][W], got[0][k][W]))
    for k in DSW_ARGS:
        if k == "zh" or k in DSW_DEAD:
            continue
        W = live_window(k, n, nz)
        print(f"call 2 {k}: {compare(ref[1][k][W], got[1][k][W]):.3e}")
        assert np.array_equal(ref[1][k][W], got[1][k][W]), ("call 2", k, compare(ref[1][k][W], got[1][k][W]))


@pytest.fixture(scope="module")
def lib():
    from pace_amd import _lib

    return _lib.load()  # raises if libpace_hip.so is missing: no fallback


@pytest.mark.gpu
@pytest.mark.parametrize("n,nz", [(96, 13), (48, 8)], ids=["c96-tile32x24", "c48-tile16x24"])
def test_d_sw_called_twice_with_swapped_buffers_matches_oracle(lib, n, nz):
    check_two_calls(lib, "cuda", n, nz)


def test_d_sw_called_twice_with_swapped_buffers_matches_oracle_emulated():
    """The same harness on the emulation (C48 x 2, the 16 x 24 tile shape): the emulation reads the by-value struct, so this checks
    the table's contents and the harness, not its place in the argument segment."""
    from helpers import build_emu
    from pace_amd import _lib

    check_two_calls(_lib.Library(build_emu()), "cpu", 48, 2)


def check_fused_kernel_alone(lib, device, n, nz):
    from pace_amd.fv3core.stencils._common import dptr

    ref = oracle_two_calls(n, nz)[0]
    env, op, s = make_operator(lib, device, n, nz)
    out6 = ("delp", "pt", "w", "q_con", "u", "v")

    def call(mask, f, outs):
        for k in out6:
            setattr(op._cfg, k + "_out", dptr(outs[k]))
        op._cfg.flags = 0
        return op.lib.cdll.pace_d_sw_phases(mask, C.byref(op._geom), *op._args([f[k] for k in DSW_ARGS], float(s["dt"])), op.stream())

    f = {k: env.q3(s[k]) for k in DSW_ARGS}
    whole, alone = ({k: env.q3(s[k]) for k in out6} for _ in range(2))
    assert call(15, f, whole) == 0
    assert call(256, f, alone) == 0
    synchronize(device)
    got = {k: v.numpy() for k, v in alone.items()}
    got["diss_est"] = f["diss_est"].numpy()
    for k, v in got.items():
        W = dsw_window(k, n, nz)
        print(f"{k}: {compare(ref[k][W], v[W]):.3e}")
        assert np.array_equal(ref[k][W], v[W]), (k, compare(ref[k][W], v[W]))
    for k in out6:  # ... and the inputs are left alone
        assert np.array_equal(f[k].numpy(), env.q3(s[k]).numpy(), equal_nan=True), k


@pytest.mark.gpu
def test_fused_kernel_alone_matches_oracle_c96(lib):
    """pace_d_sw_phases 256 -- the fused scalar + wind kernel alone, on what a whole call left in the workspace; the form that
    copies the winds' halo inside the kernel -- at C96 x 13: its six separate outputs and diss_est against the oracle's fields."""
    check_fused_kernel_alone(lib, "cuda", 96, 13)


@pytest.mark.gpu
def test_f32_library_c96_against_f64(lib):
    """The float32-storage build of the same kernels (its tables hold the same members at the same places) at C96 x 13, against
    the float64 library on the same state, within float32 storage accuracy (the bounds of tests/test_f32.py)."""
    from pace_amd import _lib

    n, nz = 96, 13
    a = device_two_calls(lib, "cuda", n, nz, calls=1)[0]
    b = device_two_calls(_lib.load(32), "cuda", n, nz, calls=1)[0]
    for k in DSW_ARGS:
        if k == "zh":
            continue
        W = dsw_window(k, n, nz)
        assert b[k].dtype == np.float32
        e = float(np.abs(a[k][W] - b[k][W]).max() / (np.abs(a[k][W]).max() + 1e-300))
        print(f"{k}: {e:.3e}")
        assert e < (5e-3 if k in ("heat_source", "diss_est") else 2e-5), (k, e)


# ---- the built library's metadata ---------------------------------------------------------------------------------------

def kernel_arguments(path, tmp_path):
    """{kernel symbol: [(offset, size, value_kind), ...]} of every gfx950 code object bundled in the shared library, from the
    AMDGPU metadata note (llvm-readelf --notes, as tools/regcheck.sh reads it)."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    objdump, readelf = (os.path.join(rocm, "lib", "llvm", "bin", t) for t in ("llvm-objdump", "llvm-readelf"))
    assert os.path.exists(objdump) and os.path.exists(readelf), f"the toolchain that built the library ({rocm}) is needed to read it"
    work = os.path.join(str(tmp_path), os.path.basename(path))
    shutil.copy(path, work)  # (the bundles are extracted next to the file)
    subprocess.run([objdump, "--offloading", work], check=True, capture_output=True)
    kernels = {}
    for obj in sorted(glob.glob(work + ".*gfx950")):
        notes = subprocess.run([readelf, "--notes", obj], check=True, capture_output=True, text=True).stdout
        args, cur = None, None
        for ln in notes.split("\n"):
            if re.match(r"\s+(- )?\.args:", ln):
                args, cur = [], None
                continue
            if args is None:
                continue
            m = re.match(r"\s+(- )?\.(offset|size|value_kind):\s+(\S+)", ln)
            if re.match(r"\s+- \.", ln) and not re.match(r"\s+- \.args:", ln) and len(ln) - len(ln.lstrip()) >= 6:
                cur = {}
                args.append(cur)
            if m and cur is not None and len(ln) - len(ln.lstrip()) >= 6:
                cur[m.group(2)] = m.group(3)
            m = re.match(r"\s+\.name:\s+(\S+)", ln)
            if m and len(ln) - len(ln.lstrip()) == 4:
                kernels[m.group(1)] = [(int(a["offset"]), int(a["size"]), a["value_kind"]) for a in args]
                args = None
    return kernels


@pytest.mark.parametrize("which", ["libpace_hip.so", "libpace_hip_f32.so"])
def test_argument_tables_are_one_by_value_argument_at_offset_zero(which, tmp_path):
    path = os.path.join(ROOT, "pace_amd", which)
    assert os.path.exists(path), "build the library first (make / __graft_entry__.build())"
    kernels = kernel_arguments(path, tmp_path)
    assert len(kernels) > 50  # (the parser saw the library's kernels)
    wanted = {"k_fvt_scalarsILi5E": 2, "k_fvt_scalarsILi6E": 2, "k_divdamp_fused": 1}  # (fvt:: and fvt16::)
    for stem, count in wanted.items():
        hits = {k: v for k, v in kernels.items() if stem in k}
        assert len(hits) == count, (stem, sorted(hits))
        for name, args in hits.items():
            explicit = [a for a in args if not a[2].startswith("hidden_")]
            assert len(explicit) == 1, (name, args)
            offset, size, kind = explicit[0]
            assert (offset, kind) == (0, "by_value") and size % 8 == 0 and size > 400, (name, explicit)
    # (a kernel with a plain argument list, parsed the same way: the parser tells the difference)
    plain = [v for k, v in kernels.items() if "k_copy_wind_halo" in k]
    assert plain and len([a for a in plain[0] if not a[2].startswith("hidden_")]) == 5
