"""d_sw's kinetic energy + vorticity launch takes the interior region as register tiles (csrc/k_dsw.hip ke_vorticity_tile: a
thread owns 2 x R B-grid points and loads what they read once, as aligned pairs); PACE_KE_TILED=0 selects the point form for the
interior, PACE_KE_TILED=1 the tiles at any size.  Both forms evaluate the same expressions: they must
leave the same bits in every argument of d_sw over the whole storage (the separate-outputs contract: u, v and heat_source carry
the kinetic energy and the vorticity everywhere they are used), with one and with two levels per thread, and by itself (no
switch set) the launch must give those bits too.

Shapes: C12 x 3 -- the interior is 7 points wide (odd, less than one row of pairs of a wave) and the last chunk of two levels has
one; C24 x 4 on the canonical-tiling emulation; C48 x 5 -- width 43 is odd and no multiple of R divides the height for R in
2, 4, 8.  On the device C48 x 7 and C96 x 3, both libraries."""
import os

import numpy as np
import pytest

from helpers import DSW_ARGS, Env, build_emu, build_emu_canon, build_emu_f32, build_emu_small

# (PACE_KE_TILED, PACE_KE_LEVELS); the first is the reference: the point form
SWITCHES = (("0", "1"), ("1", "1"), ("0", "2"), ("1", "2"), (None, None))


def run_switches(lib, device, n, nz, separate_outputs=True):
    from pace_amd import synthetic
    from pace_amd.fv3core import DGridShallowWaterLagrangianDynamicsConfig
    from pace_amd.fv3core.stencils.d_sw import DGridShallowWaterLagrangianDynamics, get_column_namelist

    m = synthetic.tile_metrics(n, nz)
    s = synthetic.acoustic_state(m, n, nz)
    env = Env(lib, device, m, n, nz)
    cfg = DGridShallowWaterLagrangianDynamicsConfig()
    res = {}
    saved = {k: os.environ.pop(k, None) for k in ("PACE_KE_TILED", "PACE_KE_LEVELS")}
    try:
        for sw in SWITCHES:
            for k, val in zip(("PACE_KE_TILED", "PACE_KE_LEVELS"), sw):
                if val is not None:
                    os.environ[k] = val
            try:
                op = DGridShallowWaterLagrangianDynamics(env.stencil_factory, env.qf, env.grid_data, env.damping, get_column_namelist(cfg, env.qf),
                                                        False, False, cfg, swap_scalar_storage=True)
                f = {k: env.q3(s[k]) for k in DSW_ARGS}
                op(*[f[k] for k in DSW_ARGS], float(s["dt"]))
                op.join()
                if device == "cuda":
                    import torch

                    torch.cuda.synchronize()
                assert op._pingpong or not separate_outputs
                res[sw] = {k: f[k].numpy().copy() for k in DSW_ARGS}
            finally:
                os.environ.pop("PACE_KE_TILED", None)
                os.environ.pop("PACE_KE_LEVELS", None)
    finally:
        for k, val in saved.items():
            if val is not None:
                os.environ[k] = val
    return res


def check(res):
    ref = res[SWITCHES[0]]
    for sw, got in res.items():
        for k in ref:
            assert not (np.isnan(got[k]) & ~np.isnan(ref[k])).any(), (sw, k, "NaN where the point form left none")
            assert np.array_equal(ref[k], got[k], equal_nan=True), (sw, k, int((ref[k] != got[k]).sum()))


EMU = {"emu": build_emu, "small": build_emu_small, "canon": build_emu_canon, "f32": build_emu_f32}


# (the last column: the library takes separate outputs at this shape; where it does not, the in-place contract is compared)
@pytest.mark.parametrize("which,n,nz,separate", [("small", 12, 3, False), ("f32", 24, 3, False), ("canon", 24, 4, True), ("emu", 48, 5, True)])
def test_ke_tiles_equal_the_point_form_emulated(which, n, nz, separate):
    from pace_amd import _lib

    check(run_switches(_lib.Library(EMU[which]()), "cpu", n, nz, separate))


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("n,nz", [(48, 7), (96, 3)])
def test_ke_tiles_equal_the_point_form(bits, n, nz):
    from pace_amd import _lib

    lib = _lib.load(32) if bits == 32 else _lib.load()
    assert lib.real_bytes == bits // 8
    check(run_switches(lib, "cuda", n, nz))
