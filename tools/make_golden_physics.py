"""Generate the fixtures of the Physics shell and of the physics-to-dycore coupling by RUNNING THE REFERENCE in this container
(gtscript executed by tools/gtinterp.py, 6 tile ranks on threads).  Data only.

tests/golden/physics_c12_<part>_p*.npz: Physics (physics/pace/physics/stencils/physics.py:204-369) with the microphysics on tile
0 of the C12 x 79 baroclinic case, then fill_gfs_delp and prepare_tendencies_and_update_tracers
(stencils/pace/stencils/update_atmos_state.py:19-92, the `else` branch of UpdateAtmosphereState.__call__).  The dycore state is
the fields of tests/golden/microphysics_c12_in_p*.npz plus pace_amd.synthetic.physics_extras(); land comes from that fixture;
namelist dt_atmos = 225, do_qa = True, the rest default; ptop is the reference grid's.  Parts:

    pre      after everything before the microphysics: the eight tracers, delp, prsi, phii, phil, delprsi, dz, wmp (and ptop)
    post     after the whole call: the ten tendencies, wmp, the ten physics_updated_* fields
    coupled  the physics side is the state after the call, the dycore side the original one, u_dt / v_dt / pt_dt on entry are
             pace_amd.synthetic.microphysics_tendencies(shape, 10 .. 12): u_dt, v_dt, pt_dt, delp, the six tracers and
             physics_updated_specific_humidity (fill_gfs_delp works on it) after the two stencils

all on the compute domain; interface fields have nk + 1 levels.  Files are split at 630 787 bytes.

Nothing is written unless every stored value is finite, both clamps of the mid-layer pressure act, qvapor is below 1e-10 and
below 0 somewhere, physics_updated_specific_humidity is below 1e-9 somewhere (fill_gfs_delp has work), tools/physics_np.py
reproduces `pre` and `coupled` bit for bit, and the emulated library reproduces the run under the tests' bounds: `pre`, the
forward Euler and `coupled` bit for bit, the tendencies and wmp within the reference's `Microph` line.

    python tools/make_golden_physics.py [--check]      (--check: compare, write nothing)
"""
import os
import sys
import warnings

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402

import physics_np as npr  # noqa: E402
from make_golden_microphysics import MAX_ERROR, NEAR_ZERO, TEND, load_split, save_split  # noqa: E402

N, NZ = 12, 79
DT = 225.0
TRACERS = ["qvapor", "qliquid", "qrain", "qice", "qsnow", "qgraupel", "qo3mr", "qsgs_tke"]
LAYER_IN = npr.COPIED  # what the dycore hands over (sixteen fields)
PRE = TRACERS + ["delp", "prsi", "phii", "phil", "delprsi", "dz", "wmp"]
UPDATED = [out for _, _, out in npr.UPDATED]
POST = TEND + ["wmp"] + UPDATED
DYCORE_TEND = ["u_dt", "v_dt", "pt_dt"]
COUPLED = DYCORE_TEND + ["delp"] + npr.SUM_ORDER + ["physics_updated_specific_humidity"]
INTERFACE = ("prsi", "phii", "prsik")
STATE3 = LAYER_IN + UPDATED + ["delprsi", "phii", "phil", "dz", "wmp", "prsi", "prsik"]


def dycore_inputs(n=N, nk=NZ, thermo=None):
    """name -> array on the compute domain: the sixteen fields CopyDycoreToPhysics carries, plus land and area.  C12 x 79: the
    microphysics fixture's fields; any other size (or `thermo` = (pt, delp, delz)): pace_amd.synthetic's columns."""
    from pace_amd import synthetic

    if thermo is None and (n, nk) == (N, NZ):
        inp = {k[3:]: v for k, v in load_split("microphysics_c12_in").items()}
    else:
        inp = synthetic.microphysics_state(*(thermo or synthetic.microphysics_columns(n, nk)))
        i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        inp["area"] = 2.0e10 * (1.0 + 0.3 * np.sin(0.3 * i + 0.2 * j))
    inp.update(synthetic.physics_extras(inp["pt"].shape))
    return {name: inp[name] for name in LAYER_IN + ["land", "area"]}


def coupling_tendencies(shape):
    from pace_amd import synthetic

    return {name: synthetic.microphysics_tendencies(shape, 10 + m) for m, name in enumerate(DYCORE_TEND)}


def embed(a, n, fill=np.nan, levels=None):
    """A compute-domain array in the library's full storage (n + 7, n + 7, nk + 1); a layer field leaves level nk at `fill`."""
    if a.ndim == 2:
        full = np.full((n + 7, n + 7), fill)
        full[3:3 + n, 3:3 + n] = a
        return full
    nk1 = levels if levels is not None else a.shape[2] + 1
    full = np.full((n + 7, n + 7, nk1), fill)
    full[3:3 + n, 3:3 + n, :a.shape[2]] = a
    return full


def window(full, name, n, nk):
    return full[3:3 + n, 3:3 + n, :nk + 1 if name in INTERFACE else nk]


# ---- pace_amd's operators (the emulated library here, the device in the tests) ------------------------------------------------

def make_env(lib, device, area, n, nk, ptop):
    from pace_amd.tile import Env

    # (the dictionary of tests/helpers.py minimal_metrics plus ptop; tools/ imports nothing from tests/: keep the two alike)
    metrics = {"area": embed(area, n, 1.0), "da_min": 1.0, "da_min_c": 1.0, "ptop": ptop,
               **{k: np.zeros((n + 7, n + 7)) for k in ("del6_u", "del6_v", "divg_u", "divg_v")}}
    return Env(lib, device, metrics, n, nk)


def namelist(n=N, nk=NZ, **kw):
    from pace_amd.physics import PhysicsConfig

    values = dict(dt_atmos=225, hydrostatic=False, npx=n + 1, npy=n + 1, npz=nk, nwat=6, do_qa=True)
    values.update(kw)
    return PhysicsConfig(**values)


def physics_state(env, fields, n, nk, packages=("microphysics",), tensors=False, fill=np.nan):
    """A PhysicsState on `fill`-filled storage (whatever is read or written outside the compute domain shows) holding `fields`
    (name -> compute-domain array; missing ones stay at `fill`)."""
    from pace_amd.physics import PhysicsState

    storages = {}
    for name in STATE3 + ["land"]:
        q = env.q2() if name == "land" else env.q3()
        q.set(embed(fields[name], n, fill, nk + 1) if name in fields else np.full(q.shape, fill))
        storages[name] = q.data
    if tensors:
        state = PhysicsState(**storages, quantity_factory=env.qf, active_packages=list(packages))
    else:
        state = PhysicsState.init_from_storages(storages, env.sizer, env.qf, list(packages))
    if state.microphysics is not None:
        for name in TEND:
            f = getattr(state.microphysics, name)
            (f.data if hasattr(f, "dims") else f)[...] = float(fill)
            if name in fields:
                set_field(f, embed(fields[name], n, fill, nk + 1))
    return state


def set_field(f, full):
    import torch

    t = f.data if hasattr(f, "dims") else f
    t[...] = torch.as_tensor(full, dtype=t.dtype).to(t.device)


def to_numpy(f):
    """A copy: on the CPU Quantity.numpy() and Tensor.numpy() are views of the storage."""
    return np.array(f.numpy() if hasattr(f, "dims") else f.detach().cpu().numpy())


def state_arrays(state):
    """Every field of a PhysicsState (its tendencies included) as full numpy arrays."""
    out = {name: to_numpy(getattr(state, name)) for name in STATE3 + ["land"]}
    if state.microphysics is not None:
        out.update({name: to_numpy(getattr(state.microphysics, name)) for name in TEND})
    return out


def sync(device):
    if device != "cpu":
        import torch

        torch.cuda.synchronize()


# ---- the reference ------------------------------------------------------------------------------------------------------------

def run_reference(env, inp):
    """Physics, then the coupling stencils; returns (pre, post, coupled, ptop) on the compute domain."""
    import types

    from pace.physics import PhysicsConfig
    from pace.physics.physics_state import PhysicsState
    from pace.physics.stencils.physics import Physics
    from pace.stencils.update_atmos_state import fill_gfs_delp, prepare_tendencies_and_update_tracers

    nml = PhysicsConfig(dt_atmos=225, hydrostatic=False, npx=N + 1, npy=N + 1, npz=NZ, nwat=6, do_qa=True)
    physics = Physics(env.stencil_factory, env.qf, env.grid_data, nml, ["microphysics"])
    physics._microphysics._area = embed(inp["area"], N, 1.0)
    state = PhysicsState.init_zeros(env.qf, ["microphysics"])
    C = slice(3, 3 + N)
    for name in LAYER_IN:
        getattr(state, name)[C, C, :NZ] = inp[name]
    state.land[C, C] = inp["land"]
    # (the halo of the divisors must not be zero: the interpreter evaluates whole arrays)
    for name, value in (("pt", 1.0), ("delp", 1.0), ("delz", -1.0)):
        f = getattr(state, name)
        f[f == 0.0] = value
    pre = {}
    microphysics = physics._microphysics

    def arr(f):  # the state's fields are bare arrays, the tendencies Quantities
        return f if isinstance(f, np.ndarray) else np.asarray(f.data)

    def snapshot(mp_state, timestep):
        pre.update({name: np.array(window(arr(getattr(state, name)), name, N, NZ)) for name in PRE})
        for name in TEND:
            assert (arr(getattr(mp_state, name))[C, C, :NZ] == 0.0).all(), name
        microphysics(mp_state, timestep=timestep)

    physics._microphysics = snapshot
    physics(state, DT)
    post = {name: np.array(arr(getattr(state.microphysics, name))[C, C, :NZ]) for name in TEND}
    post.update({name: np.array(getattr(state, name)[C, C, :NZ]) for name in ["wmp"] + UPDATED})

    gi = env.grid_indexing
    fill = env.stencil_factory.from_origin_domain(fill_gfs_delp, origin=gi.origin_full(), domain=gi.domain_full(add=(0, 0, 1)))
    couple = env.stencil_factory.from_origin_domain(prepare_tendencies_and_update_tracers, origin=gi.origin_compute(),
                                                    domain=gi.domain_compute(add=(0, 0, 1)))
    dycore = types.SimpleNamespace(**{name: embed(inp[name], N, 0.0) for name in ["delp"] + npr.SUM_ORDER})
    dycore.delp[dycore.delp == 0.0] = 1.0
    tend = {name: embed(v, N, 0.0) for name, v in coupling_tendencies(inp["pt"].shape).items()}
    fill(dycore.delp, state.physics_updated_specific_humidity, 1.0e-9)
    couple(tend["u_dt"], tend["v_dt"], tend["pt_dt"], state.physics_updated_ua, state.physics_updated_va, state.physics_updated_pt,
           state.physics_updated_specific_humidity, state.physics_updated_qliquid, state.physics_updated_qrain,
           state.physics_updated_qsnow, state.physics_updated_qice, state.physics_updated_qgraupel, state.ua, state.va, state.pt,
           dycore.qvapor, dycore.qliquid, dycore.qrain, dycore.qsnow, dycore.qice, dycore.qgraupel, state.prsi, dycore.delp,
           1.0 / float(nml.dt_atmos))
    coupled = {name: np.array(tend[name][C, C, :NZ]) for name in DYCORE_TEND}
    coupled.update({name: np.array(getattr(dycore, name)[C, C, :NZ]) for name in ["delp"] + npr.SUM_ORDER})
    coupled["physics_updated_specific_humidity"] = np.array(state.physics_updated_specific_humidity[C, C, :NZ])
    # what the coupling read of the physics state besides `post`: pt, ua, va are not changed by Physics
    for name in ("pt", "ua", "va"):
        assert np.array_equal(getattr(state, name)[C, C, :NZ], inp[name]), name
    return pre, post, coupled, float(env.grid_data.ptop)


# ---- checks -------------------------------------------------------------------------------------------------------------------

def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def coupling_inputs(inp, post, pre):
    """The physics side of the coupling from the fixtures: name -> compute-domain array."""
    phy = {name: post[name] for name in UPDATED}
    phy.update(ua=inp["ua"], va=inp["va"], pt=inp["pt"], prsi=pre["prsi"])
    return phy


def numpy_pre(inp, ptop):
    s = {name: inp[name].copy() for name in LAYER_IN}
    clamps = npr.prepare(s, ptop)
    return s, clamps


def numpy_coupled(inp, phy, tend_in, rdt=1.0 / 225.0):
    """tools/physics_np.py's coupling with tools/fv_update_phys_np.py's fill_gfs_delp on full arrays; returns compute-domain
    arrays under COUPLED's names."""
    import fv_update_phys_np as fnp

    n, nk = inp["pt"].shape[0], inp["pt"].shape[2]
    delp_full = embed(inp["delp"], n, 1.0)
    q_full = embed(phy["physics_updated_specific_humidity"], n, 1.0)
    fnp.fill_gfs_delp(delp_full, q_full, 1.0e-9)
    phy = dict(phy, physics_updated_specific_humidity=q_full[3:3 + n, 3:3 + n, :nk].copy())
    tend = {name: v.copy() for name, v in tend_in.items()}
    dycore = {name: inp[name].copy() for name in ["delp"] + npr.SUM_ORDER}
    npr.prepare_tendencies_and_update_tracers(tend, phy, dycore, rdt)
    out = dict(tend)
    out.update(dycore)
    out["physics_updated_specific_humidity"] = phy["physics_updated_specific_humidity"]
    return out


def run_operators(lib, device, inp, ptop, n=N, nk=NZ, phy_fields=None, whole=False):
    """CopyDycoreToPhysics -> Physics -> PhysicsToDycore on pace_amd's operators.  With `phy_fields` the coupling is fed those
    (the fixture's physics side) instead of the operator's own result.  whole: Physics.__call__ instead of its three parts
    (`pre` is then None; only wmp and the tendencies of it change afterwards).  Returns (pre, post, coupled) as full arrays."""
    import types

    from pace_amd.physics import Physics
    from pace_amd.stencils import CopyDycoreToPhysics

    env = make_env(lib, device, inp["area"], n, nk, ptop)
    nml = namelist(n, nk)
    dycore = types.SimpleNamespace(**{name: env.q3(embed(inp[name], n)) for name in LAYER_IN})
    state = physics_state(env, {"land": inp["land"]}, n, nk)
    CopyDycoreToPhysics(env.stencil_factory, env.qf)(dycore, state)
    physics = Physics(env.stencil_factory, env.qf, env.grid_data, nml, ["microphysics"])
    if whole:
        pre = None
        physics(state, DT)
    else:
        physics.prepare(state)
        sync(device)
        pre = state_arrays(state)
        physics._microphysics(state.microphysics, timestep=DT)
        physics.update(state, DT)
    sync(device)
    post = state_arrays(state)
    if phy_fields is not None:
        for name, v in phy_fields.items():
            set_field(getattr(state, name), embed(v, n, np.nan, nk + 1))
    coupled = couple(env, nml, dycore, state, coupling_tendencies(inp["pt"].shape), n, device)
    return pre, post, coupled


def couple(env, nml, dycore, state, tend_in, n, device):
    """PhysicsToDycore on a dycore namespace and a physics state; returns COUPLED's fields as full arrays."""
    from pace_amd.stencils import PhysicsToDycore

    tend = {name: env.q3(embed(v, n)) for name, v in tend_in.items()}
    PhysicsToDycore(env.stencil_factory, env.qf, nml)(dycore, state, tend["u_dt"], tend["v_dt"], tend["pt_dt"])
    sync(device)
    coupled = {name: to_numpy(tend[name]) for name in DYCORE_TEND}
    coupled.update({name: to_numpy(getattr(dycore, name)) for name in ["delp"] + npr.SUM_ORDER})
    coupled["physics_updated_specific_humidity"] = to_numpy(state.physics_updated_specific_humidity)
    return coupled


def run_coupling(lib, device, inp, phy, tend_in, n=N, nk=NZ, dt_atmos=225, tensors=False):
    """PhysicsToDycore alone: the dycore side is `inp`, the physics side `phy` (coupling_inputs)."""
    import types

    env = make_env(lib, device, inp["area"], n, nk, 300.0)
    pick = (lambda q: q.data) if tensors else (lambda q: q)
    dycore = types.SimpleNamespace(**{name: pick(env.q3(embed(inp[name], n))) for name in ["delp"] + npr.SUM_ORDER})
    state = physics_state(env, phy, n, nk, tensors=tensors)
    return couple(env, namelist(n, nk, dt_atmos=dt_atmos), dycore, state, tend_in, n, device)


def tendency_errors(ref, got_full, n=N, nk=NZ):
    from pace_amd.tile import compare

    return {name: compare(ref[name], window(got_full[name], name, n, nk), near_zero=NEAR_ZERO.get(name, 1e-18)) for name in TEND + ["wmp"]}


def main():
    check_only = "--check" in sys.argv
    import subprocess

    import refenv
    from threadcomm import run_ranks

    inp = dycore_inputs()

    def rank(comm):
        env = refenv.build_rank(comm, N, NZ, with_state=False)
        return run_reference(env, inp) if comm.Get_rank() == 0 else None

    pre, post, coupled, ptop = run_ranks(6, rank)[0]
    failed = []
    for part, d in (("pre", pre), ("post", post), ("coupled", coupled)):
        failed += [(part, name, "not finite") for name, v in d.items() if not np.isfinite(v).all()]

    # the restatement: bit for bit, and the conditions on the state
    s, (hi, lo) = numpy_pre(inp, ptop)
    print(f"ptop {ptop!r}; pressure clamps: upper {int(hi.sum())} cells, lower {int(lo.sum())}; qvapor < 1e-10: "
          f"{int((pre['qvapor'] < 1e-10).sum())}, < 0: {int((pre['qvapor'] < 0).sum())}; physics_updated_specific_humidity < 1e-9: "
          f"{int((post['physics_updated_specific_humidity'] < 1e-9).sum())}")
    if not (hi.any() and lo.any()):
        failed.append(("pre", "clamps", (int(hi.sum()), int(lo.sum()))))
    if not ((pre["qvapor"] < 1e-10).any() and (pre["qvapor"] < 0).any()):
        failed.append(("pre", "qvapor", "no small or negative value"))
    if not (post["physics_updated_specific_humidity"] < 1e-9).any():
        failed.append(("post", "physics_updated_specific_humidity", "fill_gfs_delp has no work"))
    failed += [("numpy pre", name, "bits") for name in PRE if not same_bits(s[name], pre[name])]
    phy = coupling_inputs(inp, post, pre)
    want = numpy_coupled(inp, phy, coupling_tendencies(inp["pt"].shape))
    failed += [("numpy coupled", name, "bits") for name in COUPLED if not same_bits(want[name], coupled[name])]
    euler = {out: post[out] for out in UPDATED}
    for x, x_dt, out in npr.UPDATED:
        x0 = pre[x] if x in pre else inp[x]
        if not same_bits(x0 + post[x_dt] * DT, euler[out]):
            failed.append(("numpy euler", out, "bits"))

    # the emulated library
    subprocess.run(["make", "-s", "-j8", "emu"], cwd=ROOT, check=True)
    from pace_amd import _lib

    lib = _lib.Library(os.path.join(ROOT, "tests", "emu", "libpace_emu.so"))
    e_pre, e_post, e_coupled = run_operators(lib, "cpu", inp, ptop, phy_fields=phy)
    failed += [("emulated pre", name, "bits") for name in PRE if not same_bits(window(e_pre[name], name, N, NZ), pre[name])]
    errs = tendency_errors(post, e_post)
    print("the emulated library's tendencies against the reference's (at most", MAX_ERROR, "):",
          " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    failed += [("emulated post", name, e) for name, e in errs.items() if not e <= MAX_ERROR]
    for x, x_dt, out in npr.UPDATED:
        w = lambda name: window(e_post[name], name, N, NZ)  # noqa: E731
        if not same_bits(w(x) + w(x_dt) * DT, w(out)):
            failed.append(("emulated euler", out, "bits"))
    failed += [("emulated coupled", name, "bits") for name in COUPLED
               if not same_bits(window(e_coupled[name], name, N, NZ), coupled[name])]
    if failed:
        raise SystemExit(f"nothing written: {failed}")
    print("numpy and the emulated library reproduce the run")
    if check_only:
        return
    save_split("physics_c12_pre", dict({name: pre[name] for name in PRE}, ptop=np.float64(ptop)))
    save_split("physics_c12_post", {name: post[name] for name in POST})
    save_split("physics_c12_coupled", {name: coupled[name] for name in COUPLED})


if __name__ == "__main__":
    main()
