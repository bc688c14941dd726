"""Generate the saturation adjustment's fixtures by RUNNING THE REFERENCE in this container (gtscript executed by
tools/gtinterp.py, 6 tile ranks on threads).  Data only.

* tests/golden/qsinit.npz: compute_q_tables (saturation_adjustment.py:540-558) over the indices -1 ... 2620 -- table, table2,
  tablew, des2, desw.
* tests/golden/satadj_c12.npz: SatAdjust3d (:947-1108) on tile 0.  The state going in is the one the reference's
  LagrangianToEulerian hands to the adjustment (captured at the call) on l2e_c12.npz's inputs, changed so that every branch
  is taken: deterministic condensates, some of them negative; a few columns shifted so that the temperatures span
  150 - 320 K; vapour raised above saturation in some points.  Cases (area and hs of tile 0, kmp = 2, mdt = 225 s):
    mid         last_step = False
    last        last_step = True
    consv       last_step = True, fast_mp_consv = True (te written)
    rad         last_step = True, rad_snow / rad_rain / rad_graupel = False, tintqs = True, icloud_f = 1
    icloud2     last_step = True, icloud_f = 2
  Level subset K_SEL of the compute domain (the operator is pointwise); "kmp" is the adjusted window's first level in the
  subset's numbering.  Points per branch (printed by this tool), of the 1152 in the window (T: 150 - 320 K):
    T < t_sub 96, t_sub <= T < T_WFR 395, T_WFR <= T < TICE 490, T >= TICE 171;
    negative input qice 88, qsnow 88, qliquid 84, qrain 83, qgraupel 88;
    last step: qvapor decreases 603, increases or stays 549;
    qa = 0 / 0 < qa < 1 / qa = 1: last 447 / 55 / 650, rad 358 / 119 / 675, icloud2 462 / 18 / 672;
    heavy cloud water (0.3 kg/kg at 239 - 242 K: the Bigg freezing limited by tc / icp2) and heavy rain (0.1 kg/kg at
    244 - 250 K: the freezing of rain limited by fac_r2g * dtmp / icp2) at every 17th point each: an emulated build without
    either limiter fails tests/test_sat_adjust.py on all five cases.
* tests/golden/l2e_satadj_c12.npz: LagrangianToEulerian (remapping.py:286-695) with do_sat_adj = True on l2e_c12.npz's inputs
  (read from that fixture), mid and last step.  Outputs only, and only those the adjustment changes (the others are
  l2e_c12.npz's), on the compute domain and the level subset L2E_K_SEL.
* tests/golden/dycore_satadj_k2_c12_tile{0..5}.npz: one whole DynamicalCore.step_dynamics with do_sat_adj = True, n_split = 1,
  k_split = 2 (the first remap's adjustment is a mid step, the second the last step) on the inputs of dycore_k2_c12_tile*.npz
  (make_golden_dycore.py 1 2; asserted equal here).  Outputs only, in that fixture's level-subset and column format.

    python tools/make_golden_satadj.py [qsinit] [satadj] [l2e] [dycore]     (all four by default)
"""
import dataclasses
import datetime
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
N, NZ = 12, 79
W = slice(2, 16)  # l2e_c12.npz's window of the 19 x 19 storage
C = slice(3, 15)  # the compute domain
K_SEL = [0, 1, 2, 3, 10, 25, 40, 55, 70, 78]
KMP = 2
L2E_K_SEL = [0, 1, 2, 3, 4, 10, 30, 50, 70, 76, 77, 78]
SPECIES = ["qvapor", "qliquid", "qrain", "qsnow", "qice", "qgraupel"]
SA_OUT = SPECIES + ["qcld", "te", "pt", "q_con", "pkz", "cappa"]
L2E_CHANGED = SPECIES + ["qcld", "pt", "q_con", "pkz", "cappa"]
WANT = set(sys.argv[1:]) or {"qsinit", "satadj", "l2e", "dycore"}


def perturb(a):
    """The adjustment's inputs changed so that every branch is taken (deterministic: a function of position only)."""
    i, j, k = np.meshgrid(np.arange(a["pt"].shape[0]), np.arange(a["pt"].shape[1]), np.arange(a["pt"].shape[2]), indexing="ij")
    out = {n: v.copy() for n, v in a.items()}
    base = 0.5 + 0.5 * np.sin(0.9 * i + 1.7 * j + 0.31 * k)
    for n, (name, scale) in enumerate((("qliquid", 1e-3), ("qrain", 4e-4), ("qice", 3e-4), ("qsnow", 2e-4), ("qgraupel", 1e-4))):
        f = scale * base * (0.5 + 0.5 * np.cos(1.1 * i - 0.6 * j + 0.13 * k + n))
        neg = ((5 * i + 3 * j + 11 * k + 2 * n) % 13) == 0
        out[name] = np.where(neg, -0.4 * f, f)
    # temperatures spanning 150 - 320 K: each column shifted by its own offset
    shift = -70.0 + 85.0 * ((3 * i + 7 * j) % 11) / 10.0
    out["pt"] = np.clip(a["pt"] + shift, 150.0, 320.0)
    # vapour above saturation in some points, well below it in others
    fac = np.where(((i + 2 * j + k) % 4) == 0, 3.0, np.where(((i + j) % 3) == 0, 0.2, 1.0))
    out["qvapor"] = a["qvapor"] * fac
    # heavy cloud water at 239 - 242 K, where the Bigg freezing's limiter tc / icp2 is the smaller side of its min(), and heavy
    # rain at 244 - 250 K, where the freezing of rain to graupel is limited by fac_r2g * dtmp / icp2
    bigg = ((7 * i + 5 * j + 3 * k) % 17) == 0
    r2g = ((7 * i + 5 * j + 3 * k) % 17) == 8
    out["qliquid"] = np.where(bigg, 0.3, out["qliquid"])
    out["qrain"] = np.where(r2g, 0.1, out["qrain"])
    qc = sum(out[n] for n in ("qliquid", "qrain", "qice", "qsnow", "qgraupel"))
    t = np.where(bigg, 239.0 + 3.0 * ((i + j + k) % 5) / 4.0, 244.0 + 6.0 * ((i + j + k) % 5) / 4.0)
    out["pt"] = np.where(bigg | r2g, t * (1.0 + (461.50 / 287.05 - 1) * out["qvapor"]) * (1.0 - qc), out["pt"])
    return out


def main():
    import capture
    import pace.fv3core as fv3core
    import pace.util.constants as constants
    import refenv
    from pace.fv3core.stencils import saturation_adjustment as sa
    from pace.fv3core.stencils.remapping import LagrangianToEulerian
    from threadcomm import run_ranks

    argv, sys.argv = sys.argv, sys.argv[:1]  # make_golden_dycore reads its own command line at import
    import make_golden_dycore  # noqa: F401
    sys.argv = argv
    l2e = np.load(os.path.join(GOLDEN, "l2e_c12.npz"))

    def rank(comm):
        tile = comm.Get_rank()
        env = refenv.build_rank(comm, N, NZ, with_state="dycore" in WANT)
        out = {}
        if "dycore" in WANT:
            out["dycore"] = run_dycore(env, tile)
        if tile != 0:
            return out
        qf, sf = env.qf, env.stencil_factory
        if "qsinit" in WANT:
            index = np.arange(-1, sa.QS_LENGTH, dtype=np.float64)
            shp = (1, 1, len(index))
            fields = {n: np.zeros(shp) for n in ("tablew", "table2", "table", "desw", "des2")}
            st = sf.from_origin_domain(sa.compute_q_tables, origin=(0, 0, 0), domain=shp)
            st(index.reshape(shp).copy(), fields["tablew"], fields["table2"], fields["table"], fields["desw"], fields["des2"])
            out["qsinit"] = {"index": index, **{n: v.reshape(-1) for n, v in fields.items()}}
        if not ({"satadj", "l2e"} & WANT):
            return out
        config = capture.dycore_config(n_split=2, npx=N + 1, npz=NZ)
        rcfg = config.remapping

        def q3(a=None):
            q = qf.zeros(["x", "y", "z"], units="")
            if a is not None:
                q.data[W, W, :] = a
            return q

        def q2(a):
            q = qf.zeros(["x", "y"], units="")
            q.data[W, W] = a
            return q

        captured = {}
        real_call = sa.SatAdjust3d.__call__

        def spy(self, te, qvapor, qliquid, qice, qrain, qsnow, qgraupel, qcld, hs, peln, delp, delz, q_con, pt, pkz, cappa, *rest):
            if not captured:
                for name, q in (("qvapor", qvapor), ("qliquid", qliquid), ("qice", qice), ("qrain", qrain), ("qsnow", qsnow),
                                ("qgraupel", qgraupel), ("qcld", qcld), ("delp", delp), ("delz", delz), ("q_con", q_con),
                                ("pt", pt), ("pkz", pkz), ("cappa", cappa)):
                    captured[name] = np.array(q.data)
            return real_call(self, te, qvapor, qliquid, qice, qrain, qsnow, qgraupel, qcld, hs, peln, delp, delz, q_con, pt, pkz,
                             cappa, *rest)

        sa.SatAdjust3d.__call__ = spy
        l2e_out = {}
        for tag, last in (("mid", False), ("last", True)):
            f = {n: q3(l2e["in_" + n]) for n in ("pt", "delp", "delz", "peln", "u", "v", "w", "q_con", "pkz", "pk", "pe", "cappa", "qcld")}
            tracers = {str(n): q3(l2e["in_tr_" + str(n)]) for n in l2e["tracer_names"]}
            ps, wsd, phis = q2(l2e["in_ps"]), q2(l2e["in_wsd"]), q2(l2e["in_phis"])
            ak, bk = qf.zeros(["z_interface"], units=""), qf.zeros(["z_interface"], units="")
            ak.data[:], bk.data[:] = l2e["ak"], l2e["bk"]
            pfull = qf.zeros(["z"], units="")
            pfull.data[:NZ] = l2e["pfull"]
            dp1 = q3()
            op = LagrangianToEulerian(sf, qf, rcfg, env.grid_data.area_64, fv3core.stencils.fv_dynamics.NQ, pfull, tracers)
            assert op.kmp == KMP, op.kmp
            op(tracers, f["pt"], f["delp"], f["delz"], f["peln"], f["u"], f["v"], f["w"], f["cappa"], f["q_con"], f["qcld"], f["pkz"],
               f["pk"], f["pe"], phis, ps, wsd, ak, bk, dp1, float(l2e["ptop"]), constants.KAPPA, constants.ZVIR, last, config.consv_te,
               config.dt_atmos / config.k_split)
            allf = {**f, **tracers}
            for n in L2E_CHANGED:
                l2e_out[f"{tag}_{n}"] = np.ascontiguousarray(np.array(allf[n].data)[C, C][:, :, L2E_K_SEL])
            if tag == "mid":  # the fields the adjustment leaves alone must be l2e_c12.npz's outputs, bit for bit
                for n in ("u", "v", "w", "delp", "delz", "pe", "peln", "pk"):
                    assert np.array_equal(np.array(f[n].data)[3:15, 3:15], l2e["out_" + n][1:13, 1:13]), n
        sa.SatAdjust3d.__call__ = real_call
        l2e_out["k_sel"] = np.array(L2E_K_SEL)
        out["l2e"] = l2e_out

        # ---- SatAdjust3d alone, on the captured state made to take every branch
        base = {n: captured[n][C, C][:, :, K_SEL] for n in captured}
        inp = perturb(base)
        area = np.array(env.grid_data.area_64.data)[C, C]
        hs = l2e["in_phis"][1:13, 1:13]
        sub = dict(out=dict(k_sel=np.array(K_SEL), kmp=np.int64(K_SEL.index(KMP)), mdt=np.float64(225.0), area=area, hs=hs,
                            **{"in_" + n: v for n, v in inp.items()}))
        sz = len(K_SEL)
        cases = {
            "mid": (rcfg.sat_adjust, False, False),
            "last": (rcfg.sat_adjust, True, False),
            "consv": (rcfg.sat_adjust, True, True),
            "rad": (dataclasses.replace(rcfg.sat_adjust, rad_snow=False, rad_rain=False, rad_graupel=False, tintqs=True, icloud_f=1),
                    True, False),
            "icloud2": (dataclasses.replace(rcfg.sat_adjust, icloud_f=2), True, False),
        }
        # a grid of sz levels: the operator is pointwise, so the level subset is a state of its own
        from pace.dsl.stencil import GridIndexing, StencilFactory
        from pace.util import QuantityFactory, SubtileGridSizer

        sizer = SubtileGridSizer(nx=N, ny=N, nz=sz, n_halo=3, extra_dim_lengths={})
        qfs = QuantityFactory.from_backend(sizer, "numpy")
        gis = GridIndexing.from_sizer_and_communicator(sizer, env.cube)
        sfs = StencilFactory(sf.config, gis)
        area_q = qfs.zeros(["x", "y"], units="m^2")
        area_q.data[:] = np.array(env.grid_data.area_64.data)
        hs_q = qfs.zeros(["x", "y"], units="")
        hs_q.data[W, W] = l2e["in_phis"]
        for tag, (scfg, last, consv) in cases.items():
            fields = {}
            for n in SA_OUT + ["delp", "delz"]:
                q = qfs.zeros(["x", "y", "z"], units="")
                q.data[:] = np.nan
                q.data[C, C, :sz] = inp[n] if n in inp else 0.0
                fields[n] = q
            op = sa.SatAdjust3d(sfs, scfg, area_q, K_SEL.index(KMP))
            op(fields["te"], fields["qvapor"], fields["qliquid"], fields["qice"], fields["qrain"], fields["qsnow"], fields["qgraupel"],
               fields["qcld"], hs_q, qfs.zeros(["x", "y", "z_interface"], units=""), fields["delp"], fields["delz"], fields["q_con"], fields["pt"], fields["pkz"], fields["cappa"],
               constants.ZVIR, 225.0, consv, last, constants.KAPPA, K_SEL.index(KMP))
            for n in SA_OUT:
                sub["out"][f"out_{tag}_{n}"] = np.ascontiguousarray(np.array(fields[n].data)[C, C, :sz])
        out["satadj"] = sub["out"]
        return out

    res = run_ranks(6, rank)
    os.makedirs(GOLDEN, exist_ok=True)
    r0 = res[0]
    if "qsinit" in r0:
        np.savez_compressed(os.path.join(GOLDEN, "qsinit.npz"), **r0["qsinit"])
    if "satadj" in r0:
        d = r0["satadj"]
        np.savez_compressed(os.path.join(GOLDEN, "satadj_c12.npz"), **d)
        branch_counts(d)
    if "l2e" in r0:
        np.savez_compressed(os.path.join(GOLDEN, "l2e_satadj_c12.npz"), **r0["l2e"])
    if "dycore" in r0:
        for t, r in enumerate(res):
            np.savez_compressed(os.path.join(GOLDEN, f"dycore_satadj_k2_c12_tile{t}.npz"), **r["dycore"])
    for name in ("qsinit.npz", "satadj_c12.npz", "l2e_satadj_c12.npz", "dycore_satadj_k2_c12_tile0.npz"):
        p = os.path.join(GOLDEN, name)
        if os.path.exists(p):
            print(name, os.path.getsize(p) // 1024, "KB")


def run_dycore(env, tile):
    """make_golden_dycore.py's k_split = 2 run (n_split = 1) with do_sat_adj = True; outputs in its format."""
    import capture
    import pace.fv3core as fv3core
    from make_golden_dycore import COLS, K_SEL as DK_SEL, STATE_OUT, condensates  # (imported by main with its own argv)

    config = capture.dycore_config(n_split=1, k_split=2, npx=N + 1, npz=NZ, do_sat_adj=True)
    state = env.state
    for name, f in condensates(tile, state.qvapor.data.shape).items():
        getattr(state, name).data[:] = f * (np.asarray(state.delp.data) > 0)
    ref = np.load(os.path.join(GOLDEN, f"dycore_k2_c12_tile{tile}.npz"))
    for k in ("pt", "qvapor"):
        assert np.array_equal(np.array(getattr(state, k).data)[3:15, 3:15, :], ref["in_" + k]), k
    assert np.array_equal(np.array(state.ps.data), ref["in_ps"])
    dycore = fv3core.DynamicalCore(
        comm=env.cube, grid_data=env.grid_data, stencil_factory=env.stencil_factory, quantity_factory=env.qf,
        damping_coefficients=env.damping, config=config, timestep=datetime.timedelta(seconds=config.dt_atmos),
        phis=env.state.phis, state=env.state)
    dycore.step_dynamics(state)
    out = {}
    for name in STATE_OUT:
        a = np.array(getattr(state, name).data)
        out["out_" + name] = np.ascontiguousarray(a[3:16, 3:16][:, :, DK_SEL])
        out["col_" + name] = np.stack([a[i, j, :] for (i, j) in COLS])
    out["out_ps"] = np.array(state.ps.data)[3:16, 3:16]
    return out


def branch_counts(d):
    """Points per branch of the "last" case (inputs and outputs; the window is the levels from kmp on)."""
    kmp = int(d["kmp"])
    win = (slice(None), slice(None), slice(kmp, None))
    qv, ql, qr, qi, qs, qg = (d["in_" + n][win] for n in ("qvapor", "qliquid", "qrain", "qice", "qsnow", "qgraupel"))
    qpz = ql + qr + qi + qs + qg
    t = d["in_pt"][win] / ((1.0 + (461.50 / 287.05 - 1) * qv) * (1.0 - qpz))
    tice, t_wfr = 273.16, 273.16 - 40.0
    print("points", t.size, "T < t_sub", int((t < 184.0).sum()), "t_sub <= T < T_WFR", int(((t >= 184.0) & (t < t_wfr)).sum()),
          "T_WFR <= T < TICE", int(((t >= t_wfr) & (t < tice)).sum()), "T >= TICE", int((t >= tice).sum()))
    print("negative input", {n: int((d["in_" + n][win] < 0).sum()) for n in ("qice", "qsnow", "qliquid", "qrain", "qgraupel")})
    dv = d["out_last_qvapor"][win] - qv
    print("last step: qvapor decreases", int((dv < 0).sum()), "increases or stays", int((dv >= 0).sum()))
    for tag in ("last", "rad", "icloud2"):
        qa = d[f"out_{tag}_qcld"][win]
        print(tag, "qa = 0:", int((qa == 0).sum()), "0 < qa < 1:", int(((qa > 0) & (qa < 1)).sum()), "qa = 1:", int((qa == 1).sum()))


if __name__ == "__main__":
    main()
