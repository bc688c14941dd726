"""tools/run_savepoints.py's FVSubgridZ entry (translate_fvsubgridz.py) on a pair of the serialised shapes written here from
the reference-run fixtures tests/golden/fvsubgridz_c12_*.npz: whole-domain fields of N + 6 points, `pe` on the compute domain
+ 1 and `peln` on the compute domain with the k axis in the middle, `pkz` on the compute domain, the scalar `dt`; leading
(savepoint, rank) axes.  CPU (emulated library)."""
import argparse
import os
import sys

import numpy as np

from helpers import ROOT, build_emu, golden
from test_fv_subgridz import IN3, NZ, OUT, case, expected, inputs

sys.path.insert(0, os.path.join(ROOT, "tools"))

N = 12
TAGS = ("base", "full")  # both with the runner's default namelist (nwat 6, fv_sg_adj 600, n_sponge 48); they differ in dt


def _write_pair(d):
    inp = inputs()
    full = np.s_[3:3 + N, 3:3 + N]

    def whole(a):  # the compute domain's values inside a whole-domain array of N + 6 points (zero halo)
        out = np.zeros((N + 6, N + 6, NZ))
        out[full] = a[:, :, :NZ]
        return out

    ins = {k: [] for k in IN3 + ["pe", "u_dt", "v_dt", "dt"]}
    outs = {k: [] for k in OUT}
    for tag in TAGS:
        c = case(tag)
        ks = int(c["k_sponge"])
        for k in IN3:
            if k == "peln":
                ins[k].append(np.moveaxis(inp[k], 2, 1))
            elif k == "pkz":
                ins[k].append(inp[k])
            else:
                ins[k].append(whole(inp[k]))
        pe = np.zeros((N + 2, N + 2, NZ + 1))
        pe[1, 1, 0] = float(c["pe00"])
        ins["pe"].append(np.moveaxis(pe, 2, 1))
        ins["u_dt"].append(np.zeros((N + 6, N + 6, NZ)))
        ins["v_dt"].append(np.zeros((N + 6, N + 6, NZ)))
        ins["dt"].append(np.array(float(c["timestep"])))
        for k in OUT:
            o = whole(inp[k]) if k in inp else np.zeros((N + 6, N + 6, NZ))
            o[full + (slice(0, ks),)] = expected(c, k, inp)
            outs[k].append(o)
    np.savez(os.path.join(d, "FVSubgridZ-In.npz"), **{k: np.stack(v)[:, None] for k, v in ins.items()})
    np.savez(os.path.join(d, "FVSubgridZ-Out.npz"), **{k: np.stack(v)[:, None] for k, v in outs.items()})
    np.savez(os.path.join(d, "metrics.npz"), **golden("grid_c12_tile0.npz"))


def test_fv_subgridz_pair_through_the_runner(tmp_path):
    import run_savepoints as rs
    from pace_amd import _lib

    d = str(tmp_path)
    _write_pair(d)
    lib = _lib.Library(build_emu())
    args = argparse.Namespace(device="cpu", metrics=os.path.join(d, "metrics.npz"), rank_tile=False, namelist={})
    ok, bound, worst = rs.run_one("FVSubgridZ", rs.read_pair(d, "FVSubgridZ"), args, lib)
    assert bound == 1e-14 and set(worst) == set(OUT)
    assert ok and max(worst.values()) == 0.0, worst  # (bit equality, as tests/test_fv_subgridz.py holds it)
    # ... and a wrong output is seen
    bad = dict(np.load(os.path.join(d, "FVSubgridZ-Out.npz")))
    bad["pt"] = bad["pt"] * (1 + 1e-12)
    np.savez(os.path.join(d, "FVSubgridZ-Out.npz"), **bad)
    ok, _, worst = rs.run_one("FVSubgridZ", rs.read_pair(d, "FVSubgridZ"), args, lib)
    assert not ok and worst["pt"] > 1e-14
    # ... and another namelist is another result
    args.namelist = {"fv_subgridz": {"n_sponge": 10}}
    ok, _, worst = rs.run_one("FVSubgridZ", rs.read_pair(d, "FVSubgridZ"), args, lib)
    assert not ok
