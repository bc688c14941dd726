"""tools/run_savepoints.py's entries FVUpdatePhys (six ranks, translate_fv_update_phys.py), UpdateDWindsPhys
(translate_update_dwind_phys.py) and FillGFS (translate_fillgfs.py) on pairs of the serialised shapes written here from the
reference-run fixtures tests/golden/fvupdatephys_c12_tile*.npz: whole-domain fields of N + 6 points, `u` / `v` with their staggered
row / column, `pe` on the compute domain + 1 and `peln` on the compute domain with the k axis in the middle, `pk` on the compute
domain; the "dwind" arrays from storage index 0; the physics' column arrays of FillGFS, levels from the surface up; leading
(savepoint, rank) axes.  Per-rank metric files hold the reference's grid terms.  CPU (emulated library)."""
import argparse
import os
import sys

import numpy as np

from helpers import ROOT, build_emu
from test_fv_update_phys import C, CASES, GRID_TERMS, N, NZ, ref_grids

sys.path.insert(0, os.path.join(ROOT, "tools"))
import fv_update_phys_np as npr  # noqa: E402

D, K = slice(0, N + 6), slice(0, NZ)
WATER = ("qvapor", "qliquid", "qice", "qrain", "qsnow", "qgraupel")


def _write_metrics(d):
    for t, g in enumerate(ref_grids()):
        np.savez(os.path.join(d, f"metrics{t}.npz"), **g["metrics"], **{k: g[k] for k in GRID_TERMS})
    return os.path.join(d, "metrics{rank}.npz")


def _stack(per_rank):
    return {k: np.stack([r[k] for r in per_rank])[None] for k in per_rank[0]}


def _write_fv_update_phys(d):
    inp, exp = CASES["apply"]()
    ins, outs = [], []
    for s, e in zip(inp, exp):
        one = {k: s[k][D, D, K] for k in ("u_dt", "v_dt", "t_dt", "ua", "va", "delp", "pt") + WATER}
        one.update(u=s["u"][D, 0:N + 7, K], v=s["v"][0:N + 7, D, K], ps=s["ps"][D, D], pk=s["pk"][C, C, :],
                   peln=np.moveaxis(s["peln"][C, C, :], 2, 1), pe=np.moveaxis(s["pe"][2:N + 4, 2:N + 4, :], 2, 1))
        ins.append(one)
        out = {k: e[k][D, D, K] for k in ("pt", "ua", "va") + WATER}
        out.update(u=e["u"][D, 0:N + 7, K], v=e["v"][0:N + 7, D, K])
        outs.append(out)
    np.savez(os.path.join(d, "FVUpdatePhys-In.npz"), **_stack(ins))
    np.savez(os.path.join(d, "FVUpdatePhys-Out.npz"), **_stack(outs))


def _write_update_dwinds_phys(d):
    inp, exp = CASES["winds"]()  # (NaN where the operator must not read: the serialised arrays start at storage index 0)
    ins = [{k: s[k][:, :, K] for k in ("u", "v", "u_dt", "v_dt")} for s in inp]
    outs = [{"u": e["u"][D, 0:N + 7, K], "v": e["v"][0:N + 7, D, K]} for e in exp]
    np.savez(os.path.join(d, "UpdateDWindsPhys-In.npz"), **_stack(ins))
    np.savez(os.path.join(d, "UpdateDWindsPhys-Out.npz"), **_stack(outs))


def _write_fillgfs(d):
    """The physics' arrays of the compute domain's columns.  delp is the difference of the serialised interface pressures
    there, so the expected vapour is the restatement's (which reproduced the reference's run) on exactly that delp."""
    inp, _ = CASES["update"]()
    ins, outs = {"IPD_prsi": [], "IPD_gq0": []}, {"IPD_qvapor": []}
    for s in inp:
        pe = np.zeros((N, N, NZ + 1))
        pe[:, :, 0] = s["pe"][C, C, 0]
        pe[:, :, 1:] = pe[:, :, :1] + np.cumsum(s["delp"][C, C, :NZ], axis=2)
        q = s["qvapor"][C, C, :NZ]
        ins["IPD_prsi"].append(np.reshape(pe[:, :, ::-1], (N * N, NZ + 1)))
        ins["IPD_gq0"].append(np.reshape(q[:, :, ::-1], (N * N, NZ))[:, :, None] * np.array([1.0, 0.5]))
        full_q, full_d = np.zeros((N + 7, N + 7, NZ + 1)), np.zeros((N + 7, N + 7, NZ + 1))
        full_q[C, C, :NZ] = q
        full_d[C, C, :NZ] = pe[:, :, 1:] - pe[:, :, :-1]
        npr.fill_gfs_delp(full_d, full_q, 1.0e-9)
        outs["IPD_qvapor"].append(np.reshape(full_q[C, C, :], (N * N, NZ + 1))[:, ::-1][:, 1:])
    np.savez(os.path.join(d, "FillGFS-In.npz"), **{k: np.stack(v)[None] for k, v in ins.items()})
    np.savez(os.path.join(d, "FillGFS-Out.npz"), **{k: np.stack(v)[None] for k, v in outs.items()})


def test_the_three_pairs_through_the_runner(tmp_path):
    import run_savepoints as rs
    from pace_amd import _lib

    d = str(tmp_path)
    lib = _lib.Library(build_emu())
    args = argparse.Namespace(device="cpu", metrics=_write_metrics(d), rank_tile=True, namelist={})

    _write_fv_update_phys(d)
    ok, bound, worst = rs.run_fv_update_phys(rs.read_pair(d, "FVUpdatePhys"), args, lib)
    assert bound == 1e-14 and set(worst) == {"pt", "u", "v", "ua", "va"} | set(WATER)
    assert ok and max(worst.values()) == 0.0, worst  # (bit equality, as tests/test_fv_update_phys.py holds it)
    bad = dict(np.load(os.path.join(d, "FVUpdatePhys-Out.npz")))
    bad["ua"] = bad["ua"] * (1 + 1e-12)
    np.savez(os.path.join(d, "FVUpdatePhys-Out.npz"), **bad)
    ok, _, worst = rs.run_fv_update_phys(rs.read_pair(d, "FVUpdatePhys"), args, lib)
    assert not ok and worst["ua"] > 1e-14 and worst["u"] == 0.0
    args.namelist = {"update_phys": {"dt_atmos": 450.0}}  # another namelist is another result
    ok, _, _ = rs.run_fv_update_phys(rs.read_pair(d, "FVUpdatePhys"), args, lib)
    assert not ok
    args.namelist = {}

    _write_update_dwinds_phys(d)
    ok, bound, worst = rs.run_one("UpdateDWindsPhys", rs.read_pair(d, "UpdateDWindsPhys"), args, lib)
    assert bound == 1e-14 and set(worst) == {"u", "v"}
    assert ok and max(worst.values()) == 0.0, worst

    _write_fillgfs(d)
    ok, bound, worst = rs.run_fillgfs(rs.read_pair(d, "FillGFS"), args, lib)
    assert bound == 1e-14 and ok and worst == {"IPD_qvapor": 0.0}, worst
    bad = dict(np.load(os.path.join(d, "FillGFS-Out.npz")))
    bad["IPD_qvapor"] = bad["IPD_qvapor"] + 1e-12
    np.savez(os.path.join(d, "FillGFS-Out.npz"), **bad)
    ok, _, _ = rs.run_fillgfs(rs.read_pair(d, "FillGFS"), args, lib)
    assert not ok
