"""Generate the dry convective adjustment's fixtures by RUNNING THE REFERENCE in this container (gtscript executed by
tools/gtinterp.py, 6 tile ranks on threads).  Data only.

tests/golden/fvsubgridz_c12_in{0,1,2}.npz and fvsubgridz_c12_<case>.npz: DryConvectiveAdjustment
(fv3core/pace/fv3core/stencils/fv_subgridz.py:740-964) on tile 0 of the C12 x 79 baroclinic initial state, whole columns.  What the
test case leaves unset or zero (ua, va, w, the condensates, qo3mr, qsgs_tke, qcld) is filled deterministically, and pt and the
winds are changed so that every branch is taken (perturb() below).  Cases:

    tag       n_sponge  fv_sg_adj  timestep
    base      48        600        225       fra < 1, t_max = 325
    full      48        600        900       fra >= 1: no blending
    top       10        600        225       k_sponge < 24: t_max = 315
    all       None      600        225       every level, gz from the surface
    pe1       48        600        225       pe[isc, jsc, 0] = 1.0: t_min = 160
    nwat0     48        600        225       nwat = 0: xvir = 0
    base_r32  48        600        225       base with the inputs rounded to float32 and widened again

Inputs are stored once (in_<name>, compute domain, 79 levels; peln 80; of pe only pe00 = pe[isc, jsc, 0], all the operator
reads).  Outputs per case on (compute domain, levels < k_sponge; a case too large for one file continues in <case>_b.npz),
packed against the case's inputs: a field of which fewer
than half of the points change is stored as the flat indices of the changed points and their values (unpack() below; u_dt and
v_dt against zeros).  base_r32's inputs are not stored: they are base's, rounded.

The coverage conditions are counted with restate(), a numpy restatement of the operator kept here, after asserting that it
reproduces every output of every case of the reference's run bit for bit.  A fixture that misses a condition is not written;
the counts are stored in fvsubgridz_c12_base.npz (cov_*) and printed.

    python tools/make_golden_fvsubgridz.py
"""
import os
import sys
import types
import warnings

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
N, NZ = 12, 79
C = slice(3, 15)  # the compute domain
TRACERS = ["qvapor", "qliquid", "qrain", "qice", "qsnow", "qgraupel", "qo3mr", "qsgs_tke", "qcld"]
MIXED = TRACERS + ["ua", "va", "w"]
IN3 = ["delp", "delz", "pkz", "peln", "pt"] + MIXED[9:] + TRACERS
OUT = ["pt", "ua", "va", "w"] + TRACERS + ["u_dt", "v_dt"]
# tag: (n_sponge, fv_sg_adj, timestep, nwat, pe00 override, inputs rounded to float32)
CASES = {
    "base": (48, 600, 225.0, 6, None, False),
    "full": (48, 600, 900.0, 6, None, False),
    "top": (10, 600, 225.0, 6, None, False),
    "all": (None, 600, 225.0, 6, None, False),
    "pe1": (48, 600, 225.0, 6, 1.0, False),
    "nwat0": (48, 600, 225.0, 0, None, False),
    "base_r32": (48, 600, 225.0, 6, None, True),
}
IN_FILES = (IN3[:6], IN3[6:12], IN3[12:])
MAX_BYTES = 630787  # tests/golden/satadj_c12.npz

# util/pace/util/constants.py (GFS_PHYS), as pace_amd/util/constants.py has them
GRAV, RDGAS, RVGAS, CP_AIR = 9.80665, 287.05, 461.50, 1004.6
CV_AIR, ZVIR, CP_VAP, CV_VAP = CP_AIR - RDGAS, RVGAS / RDGAS - 1, 4.0 * RVGAS, 3.0 * RVGAS
C_ICE, C_LIQ = 1972.0, 4.1855e3


# ---- the operator restated in numpy: columns vectorised, levels and sweeps as loops ----------------------------------------
def restate(f, pe00, n_sponge, fv_sg_adj, timestep, nwat, t_max=None, t_min=None):
    """f: name -> (nx, ny, >= nk [+ 1 for peln]) arrays.  Returns (outputs on levels < k_sponge, statistics): per (sweep, level)
    ri, ri_ref before and after the level's factor, tv1, tv2, and whether the level was done (level 0 forms no ri)."""
    nk = NZ
    ks = nk if n_sponge is None else n_sponge
    if t_max is None:
        t_max = 315.0 if ks < min(nk, 24) else 325.0
    if t_min is None:
        t_min = 160.0 if pe00 < 2.0 else 165.0
    xvir = 0.0 if nwat == 0 else ZVIR
    q = {n: f[n][:, :, :ks].copy() for n in MIXED}
    t0 = f["pt"][:, :, :ks].copy()
    delp, pkz, delz, peln = f["delp"], f["pkz"], f["delz"], f["peln"]
    shp = t0.shape

    def cm(k):
        q_liq = q["qliquid"][:, :, k] + q["qrain"][:, :, k]
        q_sol = q["qice"][:, :, k] + q["qsnow"][:, :, k] + q["qgraupel"][:, :, k]
        qv = q["qvapor"][:, :, k]
        cpm = (1.0 - (qv + q_liq + q_sol)) * CP_AIR + qv * CP_VAP + q_liq * C_LIQ + q_sol * C_ICE
        cvm = (1.0 - (qv + q_liq + q_sol)) * CV_AIR + qv * CV_VAP + q_liq * C_LIQ + q_sol * C_ICE
        return cpm, cvm

    def tvol(k):
        u, v, w = q["ua"][:, :, k], q["va"][:, :, k], q["w"][:, :, k]
        return gz[:, :, k] + 0.5 * (u * u + v * v + w * w)

    def qcon(k):
        return q["qliquid"][:, :, k] + q["qice"][:, :, k] + q["qsnow"][:, :, k] + q["qrain"][:, :, k] + q["qgraupel"][:, :, k]

    def adjust_cvm(k):
        cpm, cvm = cm(k)
        tv = tvol(k)
        t0[:, :, k] = (te[:, :, k] - tv) / cvm
        se[:, :, k] = cpm * t0[:, :, k] + tv

    gz, se, te = np.zeros(shp), np.zeros(shp), np.zeros(shp)
    gzh = np.zeros(shp[:2])
    for k in range(ks - 1, -1, -1):
        cpm, cvm = cm(k)
        gz[:, :, k] = gzh - 0.5 * GRAV * delz[:, :, k]
        tmp = tvol(k)
        se[:, :, k] = cpm * t0[:, :, k] + tmp
        te[:, :, k] = cvm * t0[:, :, k] + tmp
        gzh = gzh - GRAV * delz[:, :, k]

    st = {n: np.full((3,) + shp, np.nan) for n in ("ri", "ref0", "ref", "tv1", "tv2")}
    st["mixed"] = np.zeros((3,) + shp, dtype=bool)
    for s, ratio in enumerate((0.25, 0.5, 0.999)):
        h0 = {n: np.zeros(shp[:2]) for n in MIXED + ["te"]}
        below = np.zeros(shp[:2], dtype=bool)
        for k in range(ks - 1, -1, -1):
            dp = delp[:, :, k]
            if k < ks - 1:
                for n in MIXED:
                    q[n][:, :, k] = np.where(below, q[n][:, :, k] + h0[n] / dp, q[n][:, :, k])
                te[:, :, k] = np.where(below, te[:, :, k] + h0["te"] / dp, te[:, :, k])
                adjust_cvm(k)
            if k == 0:
                break
            tv1 = t0[:, :, k - 1] * (1.0 + xvir * q["qvapor"][:, :, k - 1] - qcon(k - 1))
            tv2 = t0[:, :, k] * (1.0 + xvir * q["qvapor"][:, :, k] - qcon(k))
            pt1 = tv1 / pkz[:, :, k - 1]
            pt2 = tv2 / pkz[:, :, k]
            du, dv = q["ua"][:, :, k - 1] - q["ua"][:, :, k], q["va"][:, :, k - 1] - q["va"][:, :, k]
            ri = (gz[:, :, k - 1] - gz[:, :, k]) * (pt1 - pt2) / (0.5 * (pt1 + pt2) * (du * du + dv * dv + 1.0e-4))
            hot = (tv1 > t_max) & (tv1 > tv2)
            ri = np.where(hot, 0.0, np.where(tv2 < t_min, np.where(ri < 0.1, ri, 0.1), ri))
            d = 400.0e2 - dp / (peln[:, :, k + 1] - peln[:, :, k])
            ref0 = 0.25 + (1.0 - 0.25) * np.where(d > 0, d, 0.0) / 200.0e2
            ref0 = np.where(1.0 < ref0, 1.0, ref0)
            ref = ref0 * {3: 1.5, 2: 2.0, 1: 4.0}.get(k, 1.0)
            mixed = ri < ref
            r = ri / ref
            r = np.where(r < 0.0, 0.0, r)
            dm = delp[:, :, k - 1]
            mc = ratio * dm * dp / (dm + dp) * ((1.0 - r) * (1.0 - r))
            h_te = mc * (se[:, :, k] - se[:, :, k - 1])
            for n in MIXED:
                h = mc * (q[n][:, :, k] - q[n][:, :, k - 1])
                q[n][:, :, k] = np.where(mixed, q[n][:, :, k] - h / dp, q[n][:, :, k])
                h0[n] = h
            te[:, :, k] = np.where(mixed, te[:, :, k] - h_te / dp, te[:, :, k])
            h0["te"] = h_te
            adjust_cvm(k)
            below = mixed
            for n, v in (("ri", ri), ("ref0", ref0), ("ref", ref), ("tv1", tv1), ("tv2", tv2), ("mixed", mixed)):
                st[n][s, :, :, k] = v
    fra = timestep / fv_sg_adj
    out = {}
    orig = {n: f[n][:, :, :ks] for n in MIXED}
    ta = f["pt"][:, :, :ks]
    if fra < 1.0:
        t0 = ta + (t0 - ta) * fra
        for n in MIXED:
            q[n] = orig[n] + (q[n] - orig[n]) * fra
    rdt = 1.0 / timestep
    out["u_dt"] = rdt * (q["ua"] - orig["ua"])
    out["v_dt"] = rdt * (q["va"] - orig["va"])
    out["pt"] = t0
    out.update(q)
    return out, st


# ---- the inputs -------------------------------------------------------------------------------------------------------------
def perturb(a):
    """The operator's inputs on the compute domain (name -> (12, 12, 79 or 80)), every one a function of the baroclinic state
    and of position only."""
    shape = a["pt"].shape
    i, j, k = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), np.arange(shape[2]), indexing="ij")
    col = i * shape[1] + j
    out = {n: a[n].copy() for n in ("delp", "delz", "pkz", "peln", "qvapor")}
    base = 0.5 + 0.5 * np.sin(0.7 * i + 1.3 * j + 0.37 * k)
    for n, (name, scale) in enumerate((("qliquid", 2e-4), ("qrain", 1e-4), ("qice", 5e-5), ("qsnow", 3e-5), ("qgraupel", 2e-5),
                                       ("qo3mr", 1e-6), ("qsgs_tke", 1e-2), ("qcld", 0.3))):
        f = scale * (0.2 + base * (0.5 + 0.5 * np.cos(0.9 * i - 0.4 * j + 0.11 * k + n)))
        if n < 5:
            f = np.where(((3 * i + 5 * j + 7 * k + n) % 23) == 0, -0.3 * f, f)
        out[name] = f
    out["ua"] = 15.0 * np.sin(0.4 * i + 0.2 * j) + 0.25 * (NZ - k) + 2.0 * np.sin(0.8 * k + 0.3 * i)
    out["va"] = 5.0 * np.cos(0.3 * i - 0.5 * j) + 1.5 * np.cos(0.6 * k + 0.2 * j)
    out["w"] = 0.3 * np.sin(0.5 * i + 0.7 * j + 0.9 * k)
    # +-4 K from level to level in every third column: the bulk of the mixing
    pt = a["pt"].copy()
    pt = pt + np.where(col % 3 == 0, 4.0 * np.where(k % 2 == 0, 1.0, -1.0) * (0.5 + 0.5 * np.sin(1.1 * i + 0.7 * j + 0.5 * k)), 0.0)
    # hot points (above t_max = 325 K, and between 315 and 325 K for the case "top") over a cooler level, and cold points
    # (below t_min = 160 K, and between 160 and 165 K for the case "pe1") under a warmer one: stable pairs, so that only the
    # t_max / t_min branch makes them mix
    hot = (col % 7 == 1) & ((k % 6) == 2)
    pt = np.where(hot, np.where((i + j + k) % 2 == 0, 331.0, 320.0) + 0.01 * k, pt)
    cold = (col % 7 == 4) & ((k % 6) == 5)
    pt = np.where(cold, np.where((i + j + k) % 2 == 0, 150.0, 162.5) + 0.01 * k, pt)
    out["pt"] = pt
    # the wind shear over levels 0 ... 3 chosen so that, on the state as it is before any mixing, ri of levels 3, 2, 1 equals a
    # target that cycles through values below and above the unscaled ri_ref (1.0 there), inside and outside the factors 1.5, 2, 4
    targets = np.array([0.4, 1.2, 1.4, 1.7, 1.9, 2.6, 3.6, 5.0])
    qc = out["qliquid"] + out["qice"] + out["qsnow"] + out["qrain"] + out["qgraupel"]
    theta = pt * (1.0 + ZVIR * out["qvapor"] - qc) / out["pkz"]
    zmid = np.zeros(shape)
    zh = np.zeros(shape[:2])
    for kk in range(47, -1, -1):
        zmid[:, :, kk] = zh - 0.5 * GRAV * out["delz"][:, :, kk]
        zh = zh - GRAV * out["delz"][:, :, kk]
    for kk in (3, 2, 1):
        out["va"][:, :, kk - 1] = out["va"][:, :, kk]
        x = (zmid[:, :, kk - 1] - zmid[:, :, kk]) * (theta[:, :, kk - 1] - theta[:, :, kk]) / (0.5 * (theta[:, :, kk - 1] + theta[:, :, kk]))
        t = targets[(col[:, :, 0] + 3 * kk) % len(targets)]
        du2 = x / t - 1.0e-4
        out["ua"][:, :, kk - 1] = out["ua"][:, :, kk] + np.sqrt(np.where(du2 > 0, du2, 0.0))
    return out


# ---- packing ------------------------------------------------------------------------------------------------------------------
def pack(d, key, out, inp):
    """A field of which fewer than half of the points differ from `inp` in their bits: indices and values of those points."""
    out = np.ascontiguousarray(out)
    changed = np.flatnonzero(out.view(np.int64).ravel() != np.ascontiguousarray(inp).view(np.int64).ravel())
    if 2 * len(changed) < out.size:
        d[key + "__idx"] = changed.astype(np.int32)
        d[key + "__val"] = out.ravel()[changed]
    else:
        d[key] = out


def unpack(d, key, inp):
    if key in d:
        return d[key]
    out = np.ascontiguousarray(inp).copy()
    out.ravel()[d[key + "__idx"]] = d[key + "__val"]
    return out


def case_inputs(inp, tag):
    pe00 = float(inp["pe00"]) if CASES[tag][4] is None else CASES[tag][4]
    f = {n: inp[n] for n in IN3}
    if CASES[tag][5]:
        f = {n: v.astype(np.float32).astype(np.float64) for n, v in f.items()}
    return f, pe00


def coverage(inp, outs, stats, stats_top325_out):
    """The counts the fixture has to reach (name -> (count, at least))."""
    st = stats["base"]
    done = ~np.isnan(st["ri"])
    mixed = st["mixed"]
    cov = {"mixing": (int(mixed.sum()), 500), "not_mixing": (int((done & ~mixed).sum()), 500)}
    for k in (1, 2, 3):
        cov[f"mixing_level{k}"] = (int(mixed[:, :, :, k].sum()), 10)
        cov[f"factor_decides_level{k}"] = (int((mixed & (st["ri"] >= st["ref0"]))[:, :, :, k].sum()), 5)
    cov["t_max_branch"] = (int((done & (st["tv1"] > 325.0) & (st["tv1"] > st["tv2"])).sum()), 10)
    # (ri as stored is after the clamp: a clamped point holds exactly 0.1)
    cold = done & ~((st["tv1"] > 325.0) & (st["tv1"] > st["tv2"])) & (st["tv2"] < 165.0)
    cov["t_min_branch_clamped"] = (int((cold & (st["ri"] == 0.1)).sum()), 10)
    diff = lambda a, b: np.zeros(a["pt"].shape, dtype=bool) | np.logical_or.reduce([a[n] != b[n] for n in OUT])  # noqa: E731
    cov["t_min_decides_pe1"] = (int(diff(outs["pe1"], outs["base"]).sum()), 10)
    cov["t_max_decides_top"] = (int(diff(outs["top"], stats_top325_out).sum()), 10)
    cov["ri_ref_capped"] = (int((done & (st["ref0"] == 1.0)).sum()), 10)
    cov["ri_ref_uncapped"] = (int((done & (st["ref0"] < 1.0)).sum()), 10)
    mixed_col = mixed.any(axis=(0, 3))
    nonzero = all((inp[n][:, :, :48][mixed_col] != 0).all() for n in TRACERS[1:])
    cov["tracers_nonzero_in_mixed_columns"] = (int(nonzero), 1)
    cov["negative_condensate"] = (int(sum((inp[n][:, :, :48][mixed_col] < 0).sum() for n in TRACERS[1:6])), 1)
    cov["mixed_columns"] = (int(mixed_col.sum()), 1)
    return cov


def main():
    import refenv
    from pace.fv3core.stencils.fv_subgridz import DryConvectiveAdjustment
    from threadcomm import run_ranks

    def rank(comm):
        env = refenv.build_rank(comm, N, NZ, with_state=True)
        if comm.Get_rank() != 0:
            return None
        state = env.state
        raw = {n: np.array(getattr(state, n).data)[C, C, :NZ + (n == "peln")] for n in ("delp", "delz", "pkz", "peln", "pt", "qvapor")}
        inp = perturb(raw)
        inp["pe00"] = np.float64(np.array(state.pe.data)[3, 3, 0])
        outs = {}
        for tag, (n_sponge, fv_sg_adj, timestep, nwat, _, _) in CASES.items():
            f, pe00 = case_inputs(inp, tag)
            ns = types.SimpleNamespace()
            for n in IN3 + ["pe"]:
                full = np.zeros((N + 7, N + 7, NZ + 1))
                if n == "pe":
                    full[:] = np.array(state.pe.data)
                    full[3, 3, 0] = pe00
                else:
                    full[C, C, :f[n].shape[2]] = f[n]
                setattr(ns, n, full)
            u_dt, v_dt = np.zeros((N + 7, N + 7, NZ + 1)), np.zeros((N + 7, N + 7, NZ + 1))
            op = DryConvectiveAdjustment(env.stencil_factory, env.qf, nwat, fv_sg_adj, n_sponge, False)
            op(ns, u_dt, v_dt, timestep)
            ks = NZ if n_sponge is None else n_sponge
            o = {n: np.ascontiguousarray(getattr(ns, n)[C, C, :ks]) for n in OUT[:-2]}
            o["u_dt"], o["v_dt"] = np.ascontiguousarray(u_dt[C, C, :ks]), np.ascontiguousarray(v_dt[C, C, :ks])
            # nothing outside the window is written
            for n in OUT[:-2]:
                assert np.array_equal(getattr(ns, n)[C, C, ks:f[n].shape[2]], f[n][:, :, ks:]), (tag, n)
            outs[tag] = o
        return inp, outs

    inp, outs = run_ranks(6, rank)[0]

    # the restatement reproduces the reference's run bit for bit, every case and output
    stats = {}
    for tag, (n_sponge, fv_sg_adj, timestep, nwat, _, _) in CASES.items():
        f, pe00 = case_inputs(inp, tag)
        mine, stats[tag] = restate(f, pe00, n_sponge, fv_sg_adj, timestep, nwat)
        for n in OUT:
            assert np.array_equal(mine[n].view(np.int64), outs[tag][n].view(np.int64)), (tag, n, "restatement differs from the reference")
    print("restate() equals the reference's run bit for bit:", ", ".join(CASES))
    f, pe00 = case_inputs(inp, "top")
    top325, _ = restate(f, pe00, 10, 600, 225.0, 6, t_max=325.0)
    cov = coverage(inp, outs, stats, top325)
    for name, (count, least) in cov.items():
        print(f"  {name:36s} {count:6d}  (at least {least})")
    missed = [name for name, (count, least) in cov.items() if count < least]
    if missed:
        raise SystemExit(f"coverage conditions missed, nothing written: {missed}")

    os.makedirs(GOLDEN, exist_ok=True)
    written = []
    for m, names in enumerate(IN_FILES):
        d = {"in_" + n: inp[n] for n in names}
        if m == 0:
            d["pe00"] = inp["pe00"]
        written.append((f"fvsubgridz_c12_in{m}.npz", d))
    for tag, (n_sponge, fv_sg_adj, timestep, nwat, pe00_over, r32) in CASES.items():
        f, pe00 = case_inputs(inp, tag)
        ks = NZ if n_sponge is None else n_sponge
        d = dict(k_sponge=np.int64(ks), n_sponge=np.int64(-1 if n_sponge is None else n_sponge), fv_sg_adj=np.int64(fv_sg_adj),
                 timestep=np.float64(timestep), nwat=np.int64(nwat), pe00=np.float64(pe00), r32=np.int64(r32))
        for n in OUT:
            pack(d, "out_" + n, outs[tag][n], f[n][:, :, :ks] if n in f else np.zeros_like(outs[tag][n]))
        if tag == "base":
            for name, (count, least) in cov.items():
                d["cov_" + name] = np.array([count, least])
        written.append((f"fvsubgridz_c12_{tag}.npz", d))
    for name, d in written:
        p = os.path.join(GOLDEN, name)
        np.savez_compressed(p, **d)
        if os.path.getsize(p) > MAX_BYTES:  # the second half of the outputs goes to <case>_b.npz
            late = [k for k in d if k.startswith("out_") and k.split("__")[0][4:] in OUT[len(OUT) // 2:]]
            np.savez_compressed(p, **{k: v for k, v in d.items() if k not in late})
            name_b = name[:-4] + "_b.npz"
            np.savez_compressed(os.path.join(GOLDEN, name_b), **{k: d[k] for k in late})
            print(name_b, os.path.getsize(os.path.join(GOLDEN, name_b)) // 1024, "KB")
            assert os.path.getsize(os.path.join(GOLDEN, name_b)) <= MAX_BYTES, name_b
        size = os.path.getsize(p)
        print(name, size // 1024, "KB")
        assert size <= MAX_BYTES, (name, size)


if __name__ == "__main__":
    main()
