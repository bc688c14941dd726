"""tools/run_savepoints.py's SatAdjust3d and QSInit entries (translate_satadjust3d.py, translate_qsinit.py) on pairs of the
serialised shapes written here from the reference-run fixtures tests/golden/satadj_c12.npz and qsinit.npz: the whole-domain
fields of N + 6 points, `peln` on the compute domain with the k axis in the middle, `pkz` on the compute domain, the Fortran's
1-based `kmp`, the five tables of length QS_LENGTH; leading (savepoint, rank) axes.  CPU (emulated library)."""
import argparse
import os
import sys

import numpy as np

from helpers import ROOT, build_emu, golden

sys.path.insert(0, os.path.join(ROOT, "tools"))

N = 12
SPECIES = ("qvapor", "qliquid", "qice", "qrain", "qsnow", "qgraupel")
CASES = (("mid", 0.0, 0.0), ("last", 1.0, 0.0), ("consv", 1.0, 1.0))  # (tag, last_step, fast_mp_consv)


def _write_sat_adjust_pair(d):
    from pace_amd.util import constants as c

    fix = golden("satadj_c12.npz")
    nk = len(fix["k_sel"])
    full = np.s_[3:3 + N, 3:3 + N]

    def whole(a):  # the compute domain's values inside a whole-domain array of N + 6 points (zero halo)
        out = np.zeros((N + 6, N + 6) + a.shape[2:])
        out[full] = a
        return out

    ins = {k: [] for k in SPECIES + ("te", "qcld", "hs", "peln", "delp", "delz", "q_con", "pt", "pkz", "cappa", "r_vir", "mdt",
                                      "fast_mp_consv", "last_step", "akap", "kmp")}
    outs = {k: [] for k in SPECIES + ("te", "qcld", "q_con", "pt", "pkz", "cappa")}
    for tag, last, consv in CASES:
        a = {k: fix["in_" + k] if "in_" + k in fix else np.zeros_like(fix["in_pt"]) for k in SPECIES + ("te", "qcld", "delp", "delz", "q_con",
                                                                                                        "pt", "pkz", "cappa")}
        for k in SPECIES + ("te", "qcld", "delp", "delz", "q_con", "pt", "cappa"):
            ins[k].append(whole(a[k]))
        ins["pkz"].append(a["pkz"])
        ins["peln"].append(np.moveaxis(np.full((N, N, nk + 1), 7.0), 2, 1))  # (unused by the non-hydrostatic adjustment)
        hs = np.zeros((N + 6, N + 6))
        hs[full] = fix["hs"]
        ins["hs"].append(hs)
        for k, v in (("r_vir", c.ZVIR), ("mdt", float(fix["mdt"])), ("fast_mp_consv", consv), ("last_step", last), ("akap", c.KAPPA),
                     ("kmp", float(fix["kmp"]) + 1)):
            ins[k].append(np.array(v))
        for k in outs:
            o = fix[f"out_{tag}_{k}"]
            outs[k].append(o if k == "pkz" else whole(o))
    np.savez(os.path.join(d, "SatAdjust3d-In.npz"), **{k: np.stack(v)[:, None] for k, v in ins.items()})
    np.savez(os.path.join(d, "SatAdjust3d-Out.npz"), **{k: np.stack(v)[:, None] for k, v in outs.items()})
    m = golden("grid_c12_tile0.npz")
    m["area"] = m["area"].copy()
    m["area"][full] = fix["area"]  # the area the reference run used
    np.savez(os.path.join(d, "metrics.npz"), **m)


def test_sat_adjust3d_pair_through_the_runner(tmp_path):
    import run_savepoints as rs
    from pace_amd import _lib

    d = str(tmp_path)
    _write_sat_adjust_pair(d)
    lib = _lib.Library(build_emu())
    args = argparse.Namespace(device="cpu", metrics=os.path.join(d, "metrics.npz"), rank_tile=False, namelist={})
    ok, bound, worst = rs.run_one("SatAdjust3d", rs.read_pair(d, "SatAdjust3d"), args, lib)
    assert bound == 2e-11 and set(worst) == set(SPECIES) | {"te", "qcld", "q_con", "pt", "pkz", "cappa"}
    assert ok, worst
    # ... and a wrong output is seen
    bad = dict(np.load(os.path.join(d, "SatAdjust3d-Out.npz")))
    bad["pt"] = bad["pt"] * (1 + 1e-9)
    np.savez(os.path.join(d, "SatAdjust3d-Out.npz"), **bad)
    ok, _, worst = rs.run_one("SatAdjust3d", rs.read_pair(d, "SatAdjust3d"), args, lib)
    assert not ok and worst["pt"] > 2e-11


def test_qsinit_pair_through_the_runner(tmp_path, capsys):
    import run_savepoints as rs
    from pace_amd import _lib

    d = str(tmp_path)
    q = golden("qsinit.npz")
    names = ("table", "table2", "tablew", "des2", "desw")
    assert q["index"][1] == 0  # the fixture starts at index -1; the savepoint at 0
    np.savez(os.path.join(d, "QSInit-In.npz"), **{k: np.zeros((1, 1, 1, 1, rs.QS_LENGTH)) for k in names})
    np.savez(os.path.join(d, "QSInit-Out.npz"), **{k: q[k][1:].reshape(1, 1, 1, 1, -1) for k in names})
    lib = _lib.Library(build_emu())
    args = argparse.Namespace(device="cpu", metrics=None, rank_tile=False, namelist={})
    ok, bound, worst = rs.run_qsinit(rs.read_pair(d, "QSInit"), args, lib)
    assert bound == 1e-12 and set(worst) == {"table2", "tablew", "des2", "desw"} and ok, worst
    # the command line reports it
    sys_argv = sys.argv
    sys.argv = ["run_savepoints.py", d, "--only", "QSInit", "--device", "cpu", "--lib", build_emu()]
    try:
        assert rs.main() == 0
    finally:
        sys.argv = sys_argv
    assert "QSInit: PASS" in capsys.readouterr().out
