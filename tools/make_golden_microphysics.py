"""Generate the cloud microphysics' fixtures by RUNNING THE REFERENCE in this container (gtscript executed by
tools/gtinterp.py, 6 tile ranks on threads).  Data only.

tests/golden/microphysics_c12_in_p*.npz and microphysics_c12_<case>_p*.npz: Microphysics
(physics/pace/physics/stencils/microphysics.py:1897-2533) on tile 0 of the C12 x 79 baroclinic initial state, compute domain, all
levels.  Of the baroclinic state the temperature, the layer mass and the layer depth are taken; everything else it leaves unset
or zero is pace_amd.synthetic.microphysics_state(): layered condensates about the freezing level, humidity scaled both ways about
saturation, a mixed land mask, winds, omga and the wmp prepare_microphysics makes of it.  Cases:

    tag      timestep  mp_time   ntimes
    base     225       225       1
    sub2     450       225       2        (the namelist's dt_atmos stays 225: _update_timestep_if_needed acts)
    mptime   225       112.5     2        another dts
    dry      225       225       1        no condensate anywhere: every no_fall path
    accum    225       225       1        the tendencies non-zero on entry (pace_amd.synthetic.microphysics_tendencies)

Stored: every field of MicrophysicsState plus area at entry (in_*; the tendencies are zero, or the formula above), every tendency,
wmp and the four precipitation fields after the call (out_*; precipitation as 2-D fields, the generator asserts that all levels
hold the column's value), and that no other state field changed.  Files are split at 630 787 bytes (<prefix>_p0.npz, _p1.npz ...).

Conditioning: every input of each case is perturbed by a relative 1e-15 N(0, 1) and the reference run again; for every compared
variable the reference's metric between the two runs has to stay below a quarter of the test's bound (2.2e-8, the reference's
own `Microph` device line), or nothing is written.

Coverage: the branch counts are taken by the emulated library built with -DPACE_MP_COVERAGE (make emu-mpcov: the product kernel
with counters, k_microphys.hip MP_COV), after that library has reproduced every output of every case of the reference's run
within the bound.  A fixture that misses a count is not written; the counts are stored in the base case (cov_*) and printed.
The reference's sedimentation switches the melting of FALLING ice, snow and graupel off (microphysics.py:861-868, stop_k = 0), so
there is nothing to count there: what melts is cloud ice before the fall (sedi_ice_melt) and snow / graupel in icloud (psmlt, pgmlt).

    python tools/make_golden_microphysics.py [--check]      (--check: compare and count, write nothing)
"""
import glob
import os
import subprocess
import sys
import types
import warnings

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
N, NZ = 12, 79
C = slice(3, 3 + N)
MAX_BYTES = 630787  # tests/golden/satadj_c12.npz
STATE3 = ["pt", "qvapor", "qliquid", "qrain", "qice", "qsnow", "qgraupel", "qcld", "ua", "va", "delp", "delz", "omga", "delprsi",
          "wmp", "dz"]
TEND = ["qv_dt", "ql_dt", "qr_dt", "qi_dt", "qs_dt", "qg_dt", "qa_dt", "udt", "vdt", "pt_dt"]
PRECIP = ["rain", "snow", "ice", "graupel"]
OUT = TEND + ["wmp"] + PRECIP
CASES = {
    "base": dict(timestep=225.0, mp_time=225.0, dry=False, accum=False),
    "sub2": dict(timestep=450.0, mp_time=225.0, dry=False, accum=False),
    "mptime": dict(timestep=225.0, mp_time=112.5, dry=False, accum=False),
    "dry": dict(timestep=225.0, mp_time=225.0, dry=True, accum=False),
    "accum": dict(timestep=225.0, mp_time=225.0, dry=False, accum=True),
}
MAX_ERROR = 2.2e-8
NEAR_ZERO = {"ql_dt": 1e-8, "qr_dt": 1e-9, "qg_dt": 1e-18, "udt": 1e-8, "vdt": 1e-8}
# the counts the fixture has to reach, per sub-step where the kernel takes them (k_microphys.hip MP_COV)
COVERAGE = ["rain_falls", "rain_no_fall", "ice_falls", "ice_no_fall", "snow_falls", "snow_no_fall", "graupel_falls",
            "graupel_no_fall", "sedi_ice_melt", "rain_evaporation", "rain_accretion", "autoconv_land", "autoconv_ocean",
            "icloud_ice_melt", "icloud_water_freeze", "psaci", "psacw", "pracs", "psmlt", "pgmlt", "pgfr", "pgacs",
            "instant_evaporation", "condensation", "ice_deposition", "ice_sublimation", "snow_sublimation", "graupel_sublimation",
            "graupel_deposition", "fix_negative"]


def compare(a, b, near_zero=0.0):
    from pace_amd.tile import compare as cmp

    return cmp(a, b, near_zero=near_zero)


def case_inputs(thermo, tag):
    """name -> array on the compute domain: the state at entry, the tendencies at entry, area."""
    from pace_amd import synthetic

    cfg = CASES[tag]
    s = synthetic.microphysics_state(thermo["pt"], thermo["delp"], thermo["delz"], dry=cfg["dry"])
    for m, name in enumerate(TEND):
        s[name] = synthetic.microphysics_tendencies(thermo["pt"].shape, m) if cfg["accum"] else np.zeros(thermo["pt"].shape)
    s["area"] = thermo["area"].copy()
    return s


def embed(a, fill=0.0):
    full = np.full((N + 7, N + 7, NZ + 1) if a.ndim == 3 else (N + 7, N + 7), fill)
    if a.ndim == 3:
        full[C, C, :NZ] = a
    else:
        full[C, C] = a
    return full


def run_reference(env, inp, tag):
    """The reference's Microphysics on the case's inputs; returns the outputs on the compute domain."""
    from pace.physics import PhysicsConfig
    from pace.physics.stencils.microphysics import Microphysics

    cfg = CASES[tag]
    nml = PhysicsConfig(dt_atmos=225, hydrostatic=False, npx=N + 1, npy=N + 1, npz=NZ, nwat=6, do_qa=True, mp_time=cfg["mp_time"])
    mp = Microphysics(env.stencil_factory, env.qf, env.grid_data, nml)
    mp._area = embed(inp["area"], 1.0)
    state = types.SimpleNamespace(**{n: embed(inp[n]) for n in STATE3 + TEND + ["land"]})
    # (the halo of the divisors must not be zero: the interpreter evaluates whole arrays)
    for n in ("pt", "delp", "delprsi"):
        getattr(state, n)[getattr(state, n) == 0.0] = 1.0
    for n in ("delz", "dz"):
        getattr(state, n)[getattr(state, n) == 0.0] = -1.0
    mp(state, cfg["timestep"])
    out = {n: np.ascontiguousarray(getattr(state, n)[C, C, :NZ]) for n in TEND + ["wmp"]}
    for n in PRECIP:
        f = np.array(getattr(mp, "_" + n).data)[C, C, :NZ]
        assert (f == f[:, :, :1]).all(), (tag, n, "differs between levels")
        out[n] = np.ascontiguousarray(f[:, :, 0])
    for n in STATE3:
        if n != "wmp":
            assert np.array_equal(getattr(state, n)[C, C, :NZ], inp[n]), (tag, n, "changed by the reference")
    assert np.array_equal(state.land[C, C], inp["land"])
    return out


def run_emulated(lib, inp, tag, workspace_tail=0):
    """pace_amd's Microphysics on the emulated library; returns (outputs, the operator)."""
    from pace_amd.physics import Microphysics, MicrophysicsState, PhysicsConfig
    from pace_amd.tile import Env

    cfg = CASES[tag]
    metrics = {"area": embed(inp["area"], 1.0), "da_min": 1.0, "da_min_c": 1.0,
               **{k: np.zeros((N + 7, N + 7)) for k in ("del6_u", "del6_v", "divg_u", "divg_v")}}
    env = Env(lib, "cpu", metrics, N, NZ)
    nml = PhysicsConfig(dt_atmos=225, hydrostatic=False, npx=N + 1, npy=N + 1, npz=NZ, nwat=6, do_qa=True, mp_time=cfg["mp_time"])
    mp = Microphysics(env.stencil_factory, env.qf, env.grid_data, nml)
    q = {n: env.q3(embed(inp[n], np.nan)) for n in STATE3}
    state = MicrophysicsState(*[q[n] for n in STATE3[:13]], q["delprsi"], q["wmp"], q["dz"], env.q3(), env.q2(embed(inp["land"], np.nan)))
    for n in TEND:
        getattr(state, n).set(embed(inp[n], np.nan))
    mp(state, cfg["timestep"])
    out = {n: getattr(state, n).numpy()[C, C, :NZ] for n in TEND + ["wmp"]}
    for n in PRECIP:
        out[n] = getattr(mp, "_" + n).numpy()[C, C, 0]
    return out, mp


def errors(ref, got):
    return {n: compare(ref[n], got[n], near_zero=NEAR_ZERO.get(n, 1e-18)) for n in OUT}


def save_split(prefix, d):
    """d in files of at most MAX_BYTES: <prefix>_p0.npz, _p1.npz, ...; returns their names."""
    for old in glob.glob(os.path.join(GOLDEN, prefix + "_p*.npz")):
        os.remove(old)
    parts, cur = [], {}

    def write(content, idx):
        p = os.path.join(GOLDEN, f"{prefix}_p{idx}.npz")
        np.savez_compressed(p, **content)
        return p

    for key, val in d.items():
        trial = dict(cur, **{key: val})
        p = write(trial, len(parts))
        if os.path.getsize(p) > MAX_BYTES and cur:
            write(cur, len(parts))
            parts.append(dict(cur))
            cur = {key: val}
            p = write(cur, len(parts))
            assert os.path.getsize(p) <= MAX_BYTES, (prefix, key)
        else:
            cur = trial
    parts.append(cur)
    names = [f"{prefix}_p{m}.npz" for m in range(len(parts))]
    for nm in names:
        size = os.path.getsize(os.path.join(GOLDEN, nm))
        print(nm, size // 1024, "KB")
        assert size <= MAX_BYTES, (nm, size)
    return names


def load_split(prefix):
    d = {}
    for p in sorted(glob.glob(os.path.join(GOLDEN, prefix + "_p*.npz"))):
        d.update(np.load(p, allow_pickle=False))
    return d


def main():
    check_only = "--check" in sys.argv
    import refenv
    from threadcomm import run_ranks

    def rank(comm):
        env = refenv.build_rank(comm, N, NZ, with_state=True)
        if comm.Get_rank() != 0:
            return None
        st = env.state
        thermo = {n: np.array(getattr(st, n).data)[C, C, :NZ].copy() for n in ("pt", "delp", "delz")}
        thermo["area"] = np.array(env.grid_data.area.data)[C, C].copy()
        rng = np.random.default_rng(7)
        inputs, outs, cond = {}, {}, {}
        for tag in CASES:
            inp = case_inputs(thermo, tag)
            inputs[tag] = inp
            outs[tag] = run_reference(env, inp, tag)
            pert = {n: v * (1.0 + 1e-15 * rng.standard_normal(v.shape)) for n, v in inp.items()}
            again = run_reference(env, pert, tag)
            cond[tag] = errors(outs[tag], again)
            if os.environ.get("MP_GOLDEN_DEBUG"):
                for n in OUT:
                    a, b = outs[tag][n], again[n]
                    m = 2 * np.abs(a - b) / (np.abs(a) + np.abs(b) + 1e-300)
                    m = np.where((np.abs(a) < NEAR_ZERO.get(n, 1e-18)) & (np.abs(b) < NEAR_ZERO.get(n, 1e-18)), 0, m)
                    w = np.unravel_index(np.argmax(m), m.shape)
                    if m[w] > MAX_ERROR / 4:
                        print("   debug", tag, n, w, a[w], b[w], inp["pt"][w] if a.ndim == 3 else "", w[0] * N + w[1])
        return thermo, inputs, outs, cond

    thermo, inputs, outs, cond = run_ranks(6, rank)[0]

    print("conditioning: the reference against itself on inputs perturbed by 1e-15 (at most", MAX_ERROR / 4, ")")
    failed = []
    for tag in CASES:
        worst = max(cond[tag], key=cond[tag].get)
        print(f"  {tag:7s} worst {worst} {cond[tag][worst]:.2e}   " + " ".join(f"{n} {e:.1e}" for n, e in cond[tag].items() if e > 0))
        failed += [(tag, n, e) for n, e in cond[tag].items() if not e <= MAX_ERROR / 4]
    for tag in CASES:
        for n in OUT:
            assert np.isfinite(outs[tag][n]).all(), (tag, n)

    # the emulated library, with counters, against the reference's run
    subprocess.run(["make", "-s", "-j8", "emu-mpcov"], cwd=ROOT, check=True)
    from pace_amd import _lib

    lib = _lib.Library(os.path.join(ROOT, "tests", "emu", "libpace_emu_mpcov.so"))
    print("the emulated library against the reference's run (at most", MAX_ERROR, ")")
    cov = None
    for tag in CASES:
        got, mp = run_emulated(lib, inputs[tag], tag)
        e = errors(outs[tag], got)
        worst = max(e, key=e.get)
        print(f"  {tag:7s} worst {worst} {e[worst]:.2e}   " + " ".join(f"{n} {x:.1e}" for n, x in e.items() if x > 0))
        failed += [(tag, "emulated " + n, x) for n, x in e.items() if not x <= MAX_ERROR]
        if tag == "base":
            tail = mp._workspace[-(len(COVERAGE) + 1):-1].numpy().view(np.int64)
            cov = dict(zip(COVERAGE, (int(x) for x in tail)))
    print("coverage of case base (counts over points or columns):")
    for name, count in cov.items():
        print(f"  {name:24s} {count:7d}")
    missed = [name for name, count in cov.items() if count == 0]
    if failed or missed:
        raise SystemExit(f"nothing written: conditioning / parity failed {failed}, coverage missed {missed}")
    if check_only:
        return

    os.makedirs(GOLDEN, exist_ok=True)
    base_in = inputs["base"]
    d = {"in_" + n: base_in[n] for n in STATE3 + ["land", "area"]}
    save_split("microphysics_c12_in", d)
    for tag, cfg in CASES.items():
        d = dict(timestep=np.float64(cfg["timestep"]), mp_time=np.float64(cfg["mp_time"]), dry=np.int64(cfg["dry"]),
                 accum=np.int64(cfg["accum"]))
        d.update({"out_" + n: outs[tag][n] for n in OUT})
        d.update({"cond_" + n: np.float64(cond[tag][n]) for n in OUT})
        if tag == "base":
            d.update({"cov_" + n: np.int64(v) for n, v in cov.items()})
        save_split(f"microphysics_c12_{tag}", d)


if __name__ == "__main__":
    main()
