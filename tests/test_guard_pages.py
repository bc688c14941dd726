"""Out-of-bounds accesses of the kernels, caught on the CPU: the emulated kernels run in a child process in which every array
the host layer allocates ends at (mode "over") or starts right after (mode "under") an inaccessible page (tests/guard.py).
A kernel that reads or writes outside an array it was handed dies there, and the emulator names it (PACE_EMU_GUARD=1).
Covered: the 15 operators of the acoustic loop, one DynamicalCore step, and the emulated tests of the moist side (both modes).
GPU sanitizers are not available on the pool; on the device such an access is a memory fault only when the array happens to
end at the end of an allocator segment (found that way in round 2: a metric row of a tile that sticks out of the storage)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_PRELUDE = f"""
import sys
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
import guard, helpers
from pace_amd import _lib
lib = _lib.Library(helpers.build_emu())
"""


PHYSICS_SIDE = ["test_microphysics.py", "test_physics.py", "test_physics_coupling.py", "test_fv_subgridz.py",
                "test_fv_update_phys.py", "test_sat_adjust.py", "test_column_tiling.py"]


def _run(body, mode):
    env = dict(os.environ, PACE_EMU_GUARD="1")
    code = _PRELUDE + f"with guard.guarded({mode!r}):\n" + "".join("    " + line + "\n" for line in body.strip().splitlines())
    p = subprocess.run([sys.executable, "-X", "faulthandler", "-c", code], capture_output=True, text=True, timeout=1200, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[:1500], p.stderr[-1500:])


@pytest.mark.parametrize("mode", ["over", "under"])
def test_operator_chain_with_guard_pages(mode):
    """All 15 operators of the acoustic loop + the stand-alone PPM / divergence-damping classes at C40 x 8: a size at which
    the 32 x 24 tiles of the transport family stick out of the domain by part of a tile (C12: by more than a tile, covered
    below; the 4 x 4-tile build covers tiles that divide the domain)."""
    _run("""
from opchain import Chain, ProductOps, check_case, check_standalone_operators
chain = Chain(40, 8)
ops = ProductOps(lib, "cpu", chain)
names = [case.name for case in chain.cases() if check_case(ops, case) is not None]
assert len(names) == 15
check_standalone_operators(lib, "cpu", 40, 8, exact=True)
""", mode)


def test_dynamical_core_step_with_guard_pages():
    """One whole DynamicalCore.step_dynamics on six C12 tiles (acoustic loop, tracer advection, remapping, c2l, all halo
    updates) with the grid from pace_amd.util.gridgen and the reference run's initial state: no access outside any array, and
    the reference run's output at the usual tolerances."""
    _run("""
fixes, outs = helpers.run_dycore_six_tiles(lib, "cpu", generated="metrics")
helpers.check_dycore(fixes, outs)
""", "over")


def test_allocations_are_guarded_when_asked():
    """PACE_GUARD_MODE set (the child runs below): the session fixture of tests/conftest.py has put tests/guard.py's wrappers in
    place of torch's four allocators, and a tensor from them lies against an inaccessible page.  Not set: torch's own."""
    import torch

    mode = os.environ.get("PACE_GUARD_MODE")
    wrapped = [f.__module__ == "guard" for f in (torch.full, torch.zeros, torch.empty, torch.as_tensor)]
    if not mode:
        assert not any(wrapped)
        return
    assert all(wrapped), wrapped
    import mmap

    for t in (torch.empty(5, dtype=torch.float64), torch.zeros(3, 2), torch.as_tensor([1.0, 2.0])):
        edge = t.data_ptr() + t.numel() * t.element_size() if mode == "over" else t.data_ptr()
        assert edge % mmap.PAGESIZE == 0, (mode, hex(edge))
    assert torch.isnan(torch.empty(5, dtype=torch.float64)).all()


def _guarded_pytest(mode, files):
    """The emulated tests of `files` in one child pytest without workers, whose session fixture (tests/conftest.py,
    PACE_GUARD_MODE) guards every allocation, after the sentinel test_allocations_are_guarded_when_asked.  The child has to end
    clean with nothing failed or skipped and the sentinel passed.  Returns (the ids that passed, the end of its output)."""
    env = dict(os.environ, PACE_GUARD_MODE=mode, PACE_EMU_GUARD="1")
    env.pop("PYTEST_XDIST_WORKER", None)  # (the child is a pytest of its own, not a worker of this one)
    env.pop("PYTEST_XDIST_WORKER_COUNT", None)
    env.pop("PYTEST_CURRENT_TEST", None)
    # (--capture=sys: what the emulator and the fault handler write to the process's own stderr when a kernel dies is not lost)
    here = os.path.join(ROOT, "tests")
    command = [sys.executable, "-X", "faulthandler", "-m", "pytest", "-n0", "-m", "not gpu", "-p", "no:cacheprovider", "-q", "-rp",
               "--capture=sys", "test_guard_pages.py::test_allocations_are_guarded_when_asked", *files]
    p = subprocess.run(command, cwd=here, capture_output=True, text=True, timeout=1200, env=env)
    tail = p.stdout[-3000:] + "\n" + p.stderr[-3000:]
    assert p.returncode == 0, f"the guarded run ({mode}) ended with {p.returncode}:\n{tail}"
    assert " passed" in p.stdout and "failed" not in p.stdout.splitlines()[-1] and "skipped" not in p.stdout.splitlines()[-1], tail
    # ... and it was a guarded run of what it is meant to be: the sentinel above passed in the child (the wrappers were in place),
    # every file contributed
    passed = set(re.findall(r"^PASSED (\S+)", p.stdout, flags=re.M))
    assert "test_guard_pages.py::test_allocations_are_guarded_when_asked" in passed, tail
    for name in files:
        assert any(t.startswith(name + "::") for t in passed), (name, tail)
    return passed, tail


@pytest.mark.parametrize("mode", ["over", "under"])
def test_physics_side_with_guard_pages(mode):
    """The moist side -- k_satadj.hip, k_subgridz.hip, k_updphys.hip, k_microphys.hip, k_physics.hip -- under guard pages: every
    emulated test of PHYSICS_SIDE (results as well as bounds; the C68 column-tiled cases, the saturation tables and
    LagrangianToEulerian(do_sat_adj=True) among them) in one child pytest without workers, whose session fixture
    (tests/conftest.py, PACE_GUARD_MODE) guards every allocation.  These kernels sweep to level nk of nk + 1-level storage, read
    delp[a - sk] from level 1 on, clamp their chunked loads and index 1-D edge vectors by the storage's i: an access one
    element outside ends the child, and the emulator names the kernel.  (Not seen: an overrun of exactly the one spare double
    every workspace has, and the padding of Quantity rows.)"""
    passed, tail = _guarded_pytest(mode, PHYSICS_SIDE)
    # the C68 cases of all five operators among them
    for case in ("test_microphysics_c68[emulated-base]", "test_microphysics_c68[emulated-sub2]", "test_microphysics_c68[emulated-mptime]",
                 "test_microphysics_c68[emulated-dry]", "test_microphysics_c68[emulated-accum]", "test_physics_c68[emulated]",
                 "test_physics_to_dycore_c68[emulated]", "test_dry_convective_adjust_c68[emulated-base]",
                 "test_sat_adjust_c68[emulated-mid]", "test_l2e_sat_adj_emulated[True]"):
        assert any(t.endswith("::" + case) for t in passed), (case, tail)
    assert len(passed) >= 100, len(passed)  # (81 before the C68 cases and the workspace tests, 109 with them)


VERTICAL_SIDE = ["test_vertical_edges.py"]


@pytest.mark.parametrize("mode", ["over", "under"])
def test_vertical_side_with_guard_pages(mode):
    """The remapping and column kernels -- k_remap.hip, k_l2e.hip, k_dycore.hip -- under guard pages: every emulated case of
    tests/test_vertical_edges.py in a guarded child pytest (_guarded_pytest).  k_remap_interfaces loads a chunk of eight levels
    ahead with clamps at both ends of the column (level -2 .. km), k_remap_layers reads pe1[L + 1] while it walks, the remap
    workspace has km + 1 levels per field and fillz prefetches two levels ahead: at 6 .. 128 levels, at C64 staggered in x (one
    live lane in a second block) and at C68 an access one element before ("under") or past ("over") an array ends the child.
    The module's float32-storage cases run with it, all of them (the guarded child takes 26 s with them, 16 s without): their rows
    are padded to 32 floats where the float64 rows are padded to 16 doubles, so the same sizes end elsewhere against the page."""
    passed, tail = _guarded_pytest(mode, VERTICAL_SIDE)
    for case in ("test_map_single_cross_product[emulated-64-9-xstag-9]", "test_map_single_cross_product[emulated-64-9-xstag-10]",
                 "test_map_single_cross_product[emulated-64-9-unstag-9]", "test_map_single_cross_product[emulated-64-9-ystag-10]",
                 "test_map_single_level_counts[emulated-68-12]", "test_map_single_level_counts[emulated-13-6]",
                 "test_map_single_level_counts[emulated-13-128]", "test_mapn_tracer_nine_tracers[emulated-68-7-10]",
                 "test_fillz_nine_patterns[emulated-68-7]", "test_fillz_nine_patterns[emulated-13-4]",
                 "test_neg_adj3_level_counts[emulated-68-7]", "test_lagrangian_to_eulerian_level_counts[emulated-68-9-False]",
                 "test_lagrangian_to_eulerian_level_counts[emulated-13-6-False]", "test_c2l_and_preamble_windows[emulated-64-2-2]",
                 "test_c2l_and_preamble_windows[emulated-68-5-4]", "test_ord8_transport_at_device_chain_shapes[emulated-40-3]",
                 "test_map_single_f32[emulated-64-9-xstag]", "test_map_single_f32[emulated-68-12-unstag]", "test_map_single_f32[emulated-13-6-unstag]",
                 "test_mapn_tracer_nine_tracers_f32[emulated-68-7-10]", "test_fillz_nine_patterns_f32[emulated-13-4]",
                 "test_neg_adj3_f32[emulated-68-7]", "test_lagrangian_to_eulerian_f32[emulated-68-9-False]",
                 "test_l2e_kernels_one_by_one[emulated-f32-64-6]", "test_l2e_kernels_one_by_one[emulated-f64-68-9]",
                 "test_c2l_and_preamble_windows_f32[emulated-64-2-2]", "test_ord8_transport_f32[emulated-13-5]"):
        assert any(t.endswith("::" + case) for t in passed), (case, tail)
    assert len(passed) >= 86, len(passed)  # (the sentinel + the 85 emulated cases of the module, test_column_makers among them)
