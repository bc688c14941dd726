"""The device-only code of the dycore's hot path at the shapes its emulated twins are tested at.

What sits under `#ifdef PACE_EMU` / `#ifndef PACE_EMU` in pace_amd/csrc is code the CPU tier (tests/test_emu_kernels.py)
cannot see: the column solver's DPP lane moves, its reciprocal and its five instances by level count (k_riem3f.hip), the
atomic accumulate of the transport kernels, the padded launch of the flux preparation and c_sw's band on a side stream.
The workgroup maps themselves are shared text (csrc/wgmap.h) and checked exhaustively on the CPU (test_workgroup_maps...);
here the kernels that take them run on the device at small awkward shapes.  DESIGN.md section 6 has the rule and the
measured errors.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import (RIEM3_OPCHAIN_FLOORS, ROOT, Env, build_emu, build_wgmap_check, check_other_level_counts, check_riem_column_windows,
                     riem3_inputs, run_riem3)

CSRC = os.path.join(ROOT, "pace_amd", "csrc")


# ----------------------------------------------------------------------------------------------------------------------
# 1. the workgroup maps (CPU tier)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", ["plain", "asan_ubsan"])
def test_workgroup_maps_are_bijections_exhaustively(build):
    """tests/emu/wgmap_check.cpp, a stand-alone host program over the maps of csrc/wgmap.h -- the text the device build and the
    emulation build compile -- run as a child process, plain and under AddressSanitizer + UBSan: for every launch shape in its
    ranges the image of the launch's workgroups is exactly the set of (tile, level) / (block, chunk) pairs, each once (the flux
    preparation: the real ones, see below).  It prints the first offending shape.

    The ranges against the launchers, for every n in 12 .. 384 with up to 128 levels (tiles: FV_TI x FV_TJ = 32 x 24 and 16 x 24,
    FX_NT = 1024 points per block of the flux preparation, 256 per block of the kinetic energy).  The ranges gx, gy 1 .. 13,
    64 blocks and 16 chunks do NOT contain what the launchers produce, so the program's are wider:
      * transport (k_fvt.hip, k_fvtp2d.hip): the general kernel's grid is ceil(n / 32) x ceil(n / 24), at most 12 x 16 (gy = 14 ..
        16 from C313 on); the lean kernels launch n / 32 x n / 24 where 32 and 24 divide n, and n / 16 x n / 24 at the multiples
        of 48 that are no multiples of 32: C48 3 x 2, C144 9 x 6, C240 15 x 10, C336 21 x 14; the three-planes-high launch of
        d_sw's scalars (launch_transport_scalars3) is ceil(n / 32) x 3 ceil(n / 24), up to 12 x 48; nlev <= 129.  Checked: every
        triple in gx 1 .. 13, gy 1 .. 16, nlev 1 .. 130, and every grid outside that box that one of the four launch forms makes of
        some n in 12 .. 384 (the program derives them), with every nlev 1 .. 130.
      * kinetic energy + vorticity (k_dsw.hip): blocks x chunks of one or two levels, nlev <= 128; about (n + 7)^2 / 256 blocks
        + (n + 7)^2 / 220 vorticity patches: 11 at C12, about 360 at C192, about 1 300 at C384.  Checked: every block count 1 .. 64
        with every nlev 1 .. 130, and every block count 65 .. 1 400 with nlev 1, 7, 8, 9, 79, 127, 128 -- the map depends on the
        level count through nlev / 8 and nlev % 8 only; this part is a sweep, not an enumeration of all pairs.
      * flux preparation (k_fxadv.hip): blocks = ceil(row stride x rows / 1024): 1 at C12, 41 at C192, 153 at C384; chunks =
        ceil(nk / ch) with ch = 1 on small tiles, so up to 128 chunks (C12 x 79: 79).  Checked: every block count 1 .. 160 with
        every chunk count 1 .. 130.  What is proved there: every real (block, chunk) is taken once and the launch's other
        workgroups, (padded - blocks) per chunk, get block numbers past the last real one, which the kernel's box test returns.
      * the window tiles of the pack kernels (k_diag.hip, k_state.hip, k_gather.hip): 64 points in i by 32 (a column integral: 4)
        in the dense side's fastest axis s; a storage is at most 391 points wide and 129 levels deep, and the map depends on a
        width through ceil(ni / 64) and ni % 64 only.  Checked: every ni 1 .. 200 (three tiles and a partial fourth) with every
        ns 1 .. 100, as a plane and as a 3-D item of 1 .. 3 rows j (per j identical), with 32 and 4 rows per tile: the tiles
        0 .. window_tiles - 1 hold every point of the window once and none outside it.
      * table_find against a linear scan: tables of 1 .. 33 items (the by-value tables hold 32), eight each, every workgroup."""
    plain, sanitized = build_wgmap_check()
    p = subprocess.run([plain if build == "plain" else sanitized], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert "wgmap_check ok" in p.stdout, p.stdout[-2000:]


# ----------------------------------------------------------------------------------------------------------------------
# 3. the loop's operators at small awkward shapes: which (n, nz) reaches which branch, derived from the launchers' constants
# ----------------------------------------------------------------------------------------------------------------------
DEVICE_CHAIN_SHAPES = [(13, 33), (40, 3), (48, 8), (72, 8), (96, 13)]


def _define(source, name):
    """The default of `#define name <integer>` in a kernel source."""
    with open(os.path.join(CSRC, source)) as f:
        m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, f.read(), re.M)
    assert m, (source, name)
    return int(m.group(1))


LOG_NZ = 3  # levels of the logged runs: no launcher's grid depends on the level count but in the level axis itself


def _launch_log_child():
    """(child process) c_sw and d_sw of every size of DEVICE_CHAIN_SHAPES with LOG_NZ levels on the emulation build, which has the
    device build's tile constants and launchers; the emulation writes one line per kernel launch to stderr while
    PACE_EMU_LAUNCH_LOG is set (tests/emu/hip_emu.cpp)."""
    import sys

    from opchain import Chain, ProductOps
    from pace_amd import _lib

    lib = _lib.Library(build_emu())
    for n in sorted({n for n, _ in DEVICE_CHAIN_SHAPES}):
        chain = Chain(n, LOG_NZ)
        ops = ProductOps(lib, "cpu", chain)
        os.environ["PACE_EMU_LAUNCH_LOG"] = "1"
        print(f"[size] {n}", file=sys.stderr, flush=True)
        ops.run("c_sw", chain.S)
        ops.run("d_sw", chain.S)
        del os.environ["PACE_EMU_LAUNCH_LOG"]


def launcher_grids():
    """{n: {kernel name up to its template arguments: (grid x, y, z)}} of c_sw's and d_sw's launches, from the launchers themselves."""
    import sys

    code = (f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); "
            "import test_gpu_device_paths as t; t._launch_log_child()")
    env = {k: v for k, v in os.environ.items() if k != "PACE_EMU_LAUNCH_LOG"}
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    grids, n = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("[size] "):
            n = int(line.split()[1])
            grids[n] = {}
        elif line.startswith("[emu launch] "):
            kernel, dims = line[len("[emu launch] "):].split(" grid ")
            grids[n][kernel.split("<")[0].strip("() ")] = tuple(int(x) for x in dims.split(" block ")[0].split())
    return grids


def launch_facts(n, nz, grids):
    """What the launchers make of a C<n> tile with nz levels, read from the grids they launched (launcher_grids: a changed tile
    size or covers() changes these facts, and test_device_chain_shapes_reach_every_branch fails instead of its table lying):
    which kernel transports d_sw's scalars and on which tile grid (k_fvt.hip launch_scalars: k_fvt_scalars; k_fvtp2d.hip
    launch_transport_scalars3: k_fvtp2d_scalars3, three tile planes high), the branches of fv_tile_of_linear that grid takes
    with nz levels (csrc/wgmap.h), the flux preparation's block count (k_fxadv.hip launch_fxadv: one frame workgroup per level,
    then blocks x chunks of one level at these sizes), and whether c_sw launches its tile kernel (k_csw.hip CswTiles)."""
    g = grids[n]
    ti, tj = _define("fvt_core.h", "FV_TI"), _define("fvt_core.h", "FV_TJ")
    if "k_fvt_scalars" in g:
        gx, gy, gz = g["k_fvt_scalars"]
        assert n % gx == 0 and n // gy == tj, (n, g["k_fvt_scalars"])
        kernel, partial = {ti: "fvt32", _define("k_fvt16.hip", "FV_TI"): "fvt16"}[n // gx], False
    else:
        gx, gy3, gz = g["k_fvtp2d_scalars3"]
        assert gy3 % 3 == 0
        gy = gy3 // 3
        kernel, partial = "fvtp2d", gx * ti != n or gy * tj != n
    fx = g["k_fxadv_fused"][0]
    assert gz == LOG_NZ and (fx - LOG_NZ) % LOG_NZ == 0, (n, g)
    blocks = (fx - LOG_NZ) // LOG_NZ  # (the emulated launch is not padded: the real blocks)
    return dict(kernel=kernel, grid=(gx, gy, nz), partial_tiles=partial, reorder=gx >= 3 and gy >= 3,
                levels="full == 0" if nz < 8 else ("8k" if nz % 8 == 0 else "8k + r"),
                fx_blocks=blocks, fx_blocks_multiple_of_8=blocks % 8 == 0, csw_tiles="k_csw_tile" in g)


def test_device_chain_shapes_reach_every_branch():
    """The table of test_every_operator_at_device_shapes, derived from what the launchers launch (launcher_grids, launch_facts)
    and not only written down:

        (n, nz)    transport kernel, grid      fv_tile_of_linear                 fxadv blocks   c_sw interior tiles
        (13, 33)   k_fvtp2d, 1 x 1 x 33        8k + r, plain tile order          1  (pad 7)     none: the band alone
        (40,  3)   k_fvtp2d, 2 x 2 x 3         full == 0, plain order            3  (pad 5)     none
        (48,  8)   k_fvt 16 x 24, 3 x 2 x 8    8k, plain order (gy < 3)          4  (pad 4)     1 x 2: band on the side stream
        (72,  8)   k_fvtp2d, 3 x 3 x 8         8k, corner / edge / interior      7  (pad 1)     2 x 4
        (96, 13)   k_fvt 32 x 24, 3 x 4 x 13   8k + r, reorder with gx == 3      12 (pad 4)     2 x 6

    k_fvtp2d runs with partial tiles at all three of its sizes (13, 40 and 72 are no multiples of 32); d_sw's three scalars go
    through launch_transport_scalars3 there (grids 1 x 3, 2 x 6 and 3 x 9 -- the last one reordered).  Every shape has an fxadv
    block count that is no multiple of eight, so every launch has padding workgroups.  The kinetic-energy map sees the same level
    counts (one level per chunk at these sizes)."""
    grids = launcher_grids()
    facts = {shape: launch_facts(*shape, grids) for shape in DEVICE_CHAIN_SHAPES}
    expect = {(13, 33): ("fvtp2d", (1, 1, 33), True, False, "8k + r", 1, False),
              (40, 3): ("fvtp2d", (2, 2, 3), True, False, "full == 0", 3, False),
              (48, 8): ("fvt16", (3, 2, 8), False, False, "8k", 4, True),
              (72, 8): ("fvtp2d", (3, 3, 8), True, True, "8k", 7, True),
              (96, 13): ("fvt32", (3, 4, 13), False, True, "8k + r", 12, True)}
    for shape, f in facts.items():
        got = (f["kernel"], f["grid"], f["partial_tiles"], f["reorder"], f["levels"], f["fx_blocks"], f["csw_tiles"])
        assert got == expect[shape], (shape, got)
    # every branch the issue names is reached by at least one shape
    assert {f["levels"] for f in facts.values()} == {"full == 0", "8k", "8k + r"}
    assert {f["reorder"] for f in facts.values()} == {True, False}
    assert {f["kernel"] for f in facts.values()} == {"fvtp2d", "fvt16", "fvt32"}
    assert any(f["kernel"] == "fvtp2d" and f["partial_tiles"] for f in facts.values())
    assert any(not f["fx_blocks_multiple_of_8"] for f in facts.values())
    assert {f["csw_tiles"] for f in facts.values()} == {True, False}
    # the map itself (csrc/wgmap.h through the stand-alone program) takes the branches the table says: workgroup 8 is tile 1 of
    # level 0 where levels are dealt out eight at a time and workgroup 1 is where they are not -- the second CORNER with the
    # reorder, the second tile of the first row without --, and the first workgroup past the full levels starts level 8k
    plain, _ = build_wgmap_check()

    def tile_of(b, grid):
        out = subprocess.run([plain, "--fv", str(b)] + [str(x) for x in grid], capture_output=True, text=True, timeout=60, check=True)
        return tuple(int(x) for x in out.stdout.split())

    for (n, nz), f in facts.items():
        gx, gy, _ = f["grid"]
        if gx * gy > 1:
            second = tile_of(8 if nz >= 8 else 1, f["grid"])
            assert second == ((gx - 1, 0, 0) if f["reorder"] else (1 % gx, 1 // gx, 0)), (n, nz, second)
        if nz >= 8:
            assert tile_of(1, f["grid"]) == (0, 0, 1), (n, nz)
        if f["levels"] == "8k + r":
            full = nz // 8 * 8
            assert tile_of(full * gx * gy, f["grid"]) == (0, 0, full), (n, nz)


@pytest.mark.gpu
@pytest.mark.parametrize("n,nz", DEVICE_CHAIN_SHAPES)
def test_every_operator_at_device_shapes(n, nz):
    """All 15 operators of the acoustic loop body (tests/opchain.py), each on the oracle's inputs for it and at its Translate
    tolerance, on the device at the shapes of test_device_chain_shapes_reach_every_branch (see its table): every branch of the
    three workgroup maps, both transport families and both compiled shapes of the lean one, partial tiles, padded flux-preparation
    launches, c_sw with and without interior tiles beside its band.  Outputs that an operator only writes hold NaN before the call
    (opchain.WRITE_ONLY), so a workgroup that is skipped cannot pass."""
    import ctypes as C

    from opchain import Chain, ProductOps, check_case
    from pace_amd import _lib

    chain = Chain(n, nz)
    lib = _lib.load()
    ops = ProductOps(lib, "cuda", chain)
    # the device library takes the transport family the table says at this size (its own predicate: d_sw's winds ride on the lean
    # scalar kernel exactly where transport_lean_covers accepts the tile)
    lean = lib.cdll.pace_d_sw_wind_outputs_supported(C.byref(ops.dsw._geom), C.byref(ops.dsw._cfg)) == 1
    assert lean == (n in (48, 96)), (n, lean)
    seen = []
    for case in chain.cases():
        errs = check_case(ops, case, poison=True)
        print(f"OPCHAIN n={n} nz={nz} {case.name} " + " ".join(f"{k}={e:.2e}" for k, e in errs.items()))
        seen.append(case.name)
    assert len(seen) == 15


# ----------------------------------------------------------------------------------------------------------------------
# 2. the column solver on the device: every instance, every window shape
# ----------------------------------------------------------------------------------------------------------------------
# both ends of the range of every instance of k_riem_column<CG, L> (launch_column: L = 2 for 2 .. 32 levels, 4 up to 64, 5 up to
# 80, 6 up to 96, 8 up to 128): 16 L levels fill every lane, 16 L' + 1 is the sparsest case of the next instance, and the
# interface fields have one level more, which lands in the extra piece of the movers
RIEM_LEVEL_COUNTS = [2, 3, 32, 33, 64, 65, 80, 81, 96, 97, 127, 128]


def _report(tag, errs):
    print(f"RIEM {tag} " + " ".join(f"{k}={e:.2e}" for k, e in errs.items()))


@pytest.mark.gpu
@pytest.mark.parametrize("last_call", [False, True])
@pytest.mark.parametrize("nz", RIEM_LEVEL_COUNTS)
def test_riem_column_every_instance_on_device(nz, last_call):
    """riem_solver3 (both values of last_call) and riem_solver_c (compute + 1: other window bounds; once per level count, with
    last_call) on a C13 tile -- 169 columns, the head-only window shape -- at RIEM_LEVEL_COUNTS against the oracle, at the
    operators' own bounds (5e-6 and 5e-14), and nothing outside the compute domain is written.  The device builds of L = 2, 4 and 8
    run nowhere else; measured errors: DESIGN.md section 6.
    The near-zero floors are those of riem_solver3's check in tests/opchain.py (w, ppe: 1e-5 of the magnitude): the synthetic
    state's centre column has |w| = 2e-9 of the field's magnitude at some level counts, where the emulated tests' floor of 1e-9
    turns an absolute error of 7e-12 of the magnitude into a relative one of 2e-6 (96 levels) or 5.6e-6 (127) -- under emulation
    exactly as on the device."""
    from pace_amd import _lib

    errs = check_riem_column_windows(_lib.load(), "cuda", 13, nz=nz, last_call=last_call, solver_c=last_call, floors=RIEM3_OPCHAIN_FLOORS)
    _report(f"C13 nz={nz} last_call={int(last_call)}", errs)


@pytest.mark.gpu
@pytest.mark.parametrize("last_call", [False, True])
def test_riem_thread_per_column_fallback_129_levels_on_device(last_call):
    """129 levels: riem_column_supported is false and both solvers take the thread-per-column kernels of k_riem3.hip, which the
    device otherwise never runs; same checks, same bounds, last_call both ways (riem_solver_c once, with last_call)."""
    from pace_amd import _lib

    errs = check_riem_column_windows(_lib.load(), "cuda", 13, nz=129, last_call=last_call, solver_c=last_call, floors=RIEM3_OPCHAIN_FLOORS)
    _report(f"C13 nz=129 fallback last_call={int(last_call)}", errs)


@pytest.mark.gpu
@pytest.mark.parametrize("nz", [33, 97])
@pytest.mark.parametrize("n", [13, 16, 20, 40])
def test_riem_column_windows_on_device(n, nz):
    """ColumnWindows in each of its shapes, as test_riem_column_windows_emulated_vs_oracle (13: head only; 16: head and tail merged
    in one workgroup; 20: head and tail that do not fit together, no whole window; 40: head, a whole window and a tail), with the
    L = 4 and the L = 8 instance; riem_solver_c's compute + 1 gives each size other bounds."""
    from pace_amd import _lib

    errs = check_riem_column_windows(_lib.load(), "cuda", n, nz=nz, last_call=True, floors=RIEM3_OPCHAIN_FLOORS)
    _report(f"C{n} nz={nz}", errs)


@pytest.mark.gpu
@pytest.mark.parametrize("nz", [32, 91, 127])
def test_other_level_counts_on_device(nz):
    """test_other_level_counts_emulated_vs_oracle with the device library: d_sw (C12: the general transport kernel on one partial
    tile) within its Translate bound and riem_solver3 fed by it."""
    from pace_amd import _lib

    _report(f"C12 nz={nz} after d_sw", check_other_level_counts(_lib.load(), "cuda", nz, dsw_tol=3.2e-10))


@pytest.mark.gpu
@pytest.mark.parametrize("nz", [33, 97, 128])
def test_f32_riem_column_instances_against_f64_on_device(nz):
    """The float32-storage library's L = 4 and L = 8 instances (it has run L = 5 and 6 only) on C16 against the float64 device
    library on the same state, as test_f32_d_sw_and_riem3_c96_against_f64_gpu does and with its bounds."""
    from pace_amd import _lib, synthetic

    n = 16
    metrics = synthetic.tile_metrics(n, nz)
    s = synthetic.acoustic_state(metrics, n, nz)
    outs = {}
    for prec in (64, 32):
        env = Env(_lib.load(prec), "cuda", metrics, n, nz)
        outs[prec] = run_riem3(env, riem3_inputs(s), False, s["dt"], metrics["ptop"])
    errs = {}
    for k, nk in (("delz", nz), ("zh", nz + 1), ("pk3", nz + 1), ("w", nz), ("ppe", nz + 1)):
        a, b = outs[64][k][3:3 + n, 3:3 + n, :nk], outs[32][k][3:3 + n, 3:3 + n, :nk]
        errs[k] = float(np.abs(a - b).max() / (np.abs(a).max() + 1e-300))
    _report(f"f32 C16 nz={nz}", errs)
    for k, e in errs.items():
        assert e < (5e-3 if k in ("ppe", "w") else 2e-5), ("riem_solver3", k, e)
