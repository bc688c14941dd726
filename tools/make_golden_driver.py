"""Generate tests/golden/driver_c12_tile<t>_p*.npz by RUNNING THE REFERENCE in this container (6 tile ranks on threads, real halo
exchanges, gtscript executed by tools/gtinterp.py): ONE step of the reference driver's loop (driver/pace/driver/driver.py:618-640)
with the reference's own classes,

    DynamicalCore.step_dynamics -> DycoreToPhysics -> Physics -> UpdateAtmosphereState

under the namelist of tests/golden/driver_baroclinic_c12.yaml (C12 x 79, dt_atmos 225, n_split 1, k_split 1, do_sat_adj true,
nwat 6, do_qa true, dycore_only false, fv_sg_adj 0: no dry convective adjustment).

INPUTS ARE NOT STORED: they are what tests/helpers.py:run_dycore_tile builds -- the fields of acoustic_c12_tile<t>.npz, in_pt /
in_qvapor / in_ps of dycore_c12_tile<t>.npz and helpers.dycore_condensates -- which this tool asserts of the reference's own
initial state.  The driver grid terms are those of drivergrid_c12.npz (asserted), handed over with the TRUE vlat
(tools/make_golden_fvupdatephys.py).

OUTPUTS per tile, on the level subset K_SEL of the compute window + the staggered row / column (out_<v>) and on the full columns
COLS (col_<v>), as the dycore fixtures: the dycore state (DYCORE_OUT of tests/helpers.py) and ps, the three tendencies u_dt, v_dt,
pt_dt, and the ten physics_updated_* fields of the physics state.

sens_<v>: the chain is run a second time with the initial winds perturbed by 1e-13 m/s exactly as tools/wind_noise_sensitivity.py
perturbs them (default_rng(0), tiles in order, u then v, standard normal over the whole storage); sens_<v> is the distance of the
two runs in the tests' metric -- max |a - b| / max |a| over a tile's stored points, the largest of the six tiles: the reference's
own sensitivity to the smallest perturbation that flips its branch decisions.

Nothing is written unless every stored value is finite and the microphysics changed at least one condensate species on every tile.

    python tools/make_golden_driver.py            writes the fixtures
    python tools/make_golden_driver.py --check    runs the same and compares with the committed fixtures, bit for bit

Data only.
"""
import datetime
import os
import sys
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402

from make_golden_microphysics import load_split, save_split  # noqa: E402

sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
from helpers import DYCORE_OUT as STATE_OUT, dycore_condensates as condensates  # noqa: E402

# the level subset and the columns of the dycore fixtures (tools/make_golden_dycore.py)
N, NZ = 12, 79
K_SEL = [0, 1, 2, 3, 4, 40, 77, 78, 79]
COLS = [(3, 3), (8, 9), (14, 14), (3, 14)]

GOLDEN = os.path.join(HERE, "..", "tests", "golden")
DT = 225.0
TENDENCIES = ["u_dt", "v_dt", "pt_dt"]
UPDATED = ["physics_updated_specific_humidity", "physics_updated_qliquid", "physics_updated_qrain", "physics_updated_qice",
           "physics_updated_qsnow", "physics_updated_qgraupel", "physics_updated_cloud_fraction", "physics_updated_pt",
           "physics_updated_ua", "physics_updated_va"]
CONDENSATE_TENDENCIES = ["ql_dt", "qr_dt", "qi_dt", "qs_dt", "qg_dt"]
STORED = STATE_OUT + TENDENCIES + UPDATED


def arr(f):
    """The physics state's fields are bare arrays under the interpreter, the rest Quantities."""
    return f if isinstance(f, np.ndarray) else np.asarray(f.data)


def wind_noise():
    """tools/wind_noise_sensitivity.py:18-21."""
    rng = np.random.default_rng(0)
    shape = (N + 7, N + 7, NZ + 1)
    out = []
    for _ in range(6):
        out.append({k: 1e-13 * rng.standard_normal(shape) for k in ("u", "v")})
    return out


def settings():
    import yaml

    with open(os.path.join(GOLDEN, "driver_baroclinic_c12.yaml")) as f:
        d = yaml.safe_load(f)
    assert d["nx_tile"] == N and d["nz"] == NZ and d["dt_atmos"] == DT and not d.get("dycore_only", False)
    derived = dict(layout=(1, 1), npx=N + 1, npy=N + 1, npz=NZ, dt_atmos=d["dt_atmos"])
    return dict(d["dycore_config"], ntiles=6, **derived), dict(d["physics_config"], **derived)


def run_chain(noise=None):
    import refenv  # (first: it installs the shim under which the reference imports)

    import pace.fv3core as fv3core
    from pace.physics import PhysicsConfig
    from pace.physics.physics_state import PhysicsState
    from pace.physics.stencils.physics import Physics
    from pace.stencils.update_atmos_state import DycoreToPhysics, UpdateAtmosphereState
    from pace.util.grid import DriverGridData
    from threadcomm import run_ranks

    dycore_values, physics_values = settings()
    config = fv3core.DynamicalCoreConfig(**dycore_values)
    physics_config = PhysicsConfig(**physics_values)
    assert config.n_split == 1 and config.k_split == 1 and config.do_sat_adj and config.nwat == 6 and config.fv_sg_adj == 0
    assert not config.do_dry_convective_adjustment
    driver_grid = np.load(os.path.join(GOLDEN, "drivergrid_c12.npz"))

    def rank(comm):
        env = refenv.build_rank(comm, N, NZ)
        state, mt, tile = env.state, env.mt, comm.Get_rank()
        for name, f in condensates(tile, state.qvapor.data.shape).items():
            getattr(state, name).data[:] = f * (np.asarray(state.delp.data) > 0)
        if noise is None:  # the inputs are the ones the tests rebuild
            ac = np.load(os.path.join(GOLDEN, f"acoustic_c12_tile{tile}.npz"))
            dy = np.load(os.path.join(GOLDEN, f"dycore_c12_tile{tile}.npz"))
            for k in "u v w delz delp pe pk peln phis uc vc ua va".split():
                assert np.array_equal(ac["in_" + k], np.asarray(getattr(state, k).data)), (tile, k)
            for k in ("pt", "qvapor"):
                assert np.array_equal(dy["in_" + k], np.asarray(getattr(state, k).data)[3:15, 3:15, :]), (tile, k)
            assert np.array_equal(dy["in_ps"], np.asarray(state.ps.data)), tile
            for k in ("vlon", "vlat", "es1", "ew2", "edge_vect_s", "edge_vect_n"):
                assert np.array_equal(driver_grid[f"{k}_tile{tile}"], np.asarray(getattr(mt, k).data), equal_nan=True), (tile, k)
            assert np.array_equal(driver_grid[f"edge_vect_w_tile{tile}"], np.asarray(mt.edge_vect_w_1d.data)), tile
            assert np.array_equal(driver_grid[f"edge_vect_e_tile{tile}"], np.asarray(mt.edge_vect_e_1d.data)), tile
        else:
            for k in ("u", "v"):
                getattr(state, k).data[:] = np.asarray(getattr(state, k).data) + noise[tile][k]
        grid_info = DriverGridData.new_from_grid_variables(vlon=mt.vlon, vlat=mt.vlat, edge_vect_n=mt.edge_vect_n,
                                                           edge_vect_s=mt.edge_vect_s, edge_vect_e=mt.edge_vect_e,
                                                           edge_vect_w=mt.edge_vect_w, es1=mt.es1, ew2=mt.ew2)
        tend = types.SimpleNamespace(**{k: env.qf.zeros(["x", "y", "z"], units="") for k in TENDENCIES})
        physics_state = PhysicsState.init_zeros(env.qf, ["microphysics"])
        dycore = fv3core.DynamicalCore(comm=env.cube, grid_data=env.grid_data, stencil_factory=env.stencil_factory,
                                       quantity_factory=env.qf, damping_coefficients=env.damping, config=config,
                                       timestep=datetime.timedelta(seconds=DT), phis=state.phis, state=state)
        physics = Physics(env.stencil_factory, env.qf, env.grid_data, physics_config, ["microphysics"])
        dycore_to_physics = DycoreToPhysics(env.stencil_factory, env.qf, config, config.do_dry_convective_adjustment, False)
        end_of_step_update = UpdateAtmosphereState(env.stencil_factory, env.grid_data, physics_config, env.cube, grid_info, state,
                                                   env.qf, False, True, tend)
        # driver.py:618-640
        dycore.step_dynamics(state)
        dycore_to_physics(dycore_state=state, physics_state=physics_state, tendency_state=tend, timestep=DT)
        # (the halo of the physics' divisors must not be zero: the interpreter evaluates whole arrays -- tools/make_golden_physics.py)
        for name, value in (("pt", 1.0), ("delp", 1.0), ("delz", -1.0)):
            f = arr(getattr(physics_state, name))
            f[f == 0.0] = value
        physics(physics_state, timestep=DT)
        end_of_step_update(dycore_state=state, phy_state=physics_state, u_dt=tend.u_dt, v_dt=tend.v_dt, pt_dt=tend.pt_dt, dt=DT)
        fields = {name: np.array(arr(getattr(state, name))) for name in STATE_OUT}
        fields.update({name: np.array(arr(getattr(tend, name))) for name in TENDENCIES})
        fields.update({name: np.array(arr(getattr(physics_state, name))) for name in UPDATED})
        out = {"timestep": np.float64(DT), "n_split": np.int64(config.n_split), "k_split": np.int64(config.k_split),
               "k_sel": np.array(K_SEL), "cols": np.array(COLS)}
        for name, a in fields.items():
            out["out_" + name] = np.ascontiguousarray(a[3:16, 3:16][:, :, K_SEL])
            out["col_" + name] = np.stack([a[i, j, :] for (i, j) in COLS])
        out["out_ps"] = np.array(state.ps.data)[3:16, 3:16]
        acted = max(float(np.abs(arr(getattr(physics_state.microphysics, name))[3:15, 3:15, :NZ]).max())
                    for name in CONDENSATE_TENDENCIES)
        return out, acted

    return run_ranks(6, rank)


def stored_points(out, name):
    if name == "ps":
        return out["out_ps"][:N, :N].ravel()
    di = 1 if name in ("v", "mfxd", "cxd") else 0
    dj = 1 if name in ("u", "mfyd", "cyd") else 0
    nk = NZ + 1 if name in ("pe", "pk", "peln") else NZ
    idx = [m for m, k in enumerate(K_SEL) if k < nk]
    return np.concatenate([out["out_" + name][:N + di, :N + dj][:, :, idx].ravel(), out["col_" + name][:, :nk].ravel()])


def scaled_distance(refs, others):
    """The tests' metric between two runs: per variable, max |a - b| / max |a| over a tile's stored points, the worst tile."""
    worst = {}
    for ref, other in zip(refs, others):
        for name in STORED + ["ps"]:
            a, b = stored_points(ref, name), stored_points(other, name)
            worst[name] = max(worst.get(name, 0.0), float(np.abs(a - b).max() / (np.abs(a).max() + 1e-300)))
    return worst


def main():
    check_only = "--check" in sys.argv
    base = run_chain()
    outs, acted = [r[0] for r in base], [r[1] for r in base]
    failed = []
    for t, out in enumerate(outs):
        failed += [(t, name, "not finite") for name in STORED + ["ps"] if not np.isfinite(stored_points(out, name)).all()]
        if not acted[t] > 0.0:
            failed.append((t, "microphysics", "changed no condensate species"))
    print("largest condensate tendency per tile:", " ".join(f"{a:.2e}" for a in acted))
    perturbed = [r[0] for r in run_chain(wind_noise())]
    sens = scaled_distance(outs, perturbed)
    print("sens:", " ".join(f"{k} {v:.1e}" for k, v in sens.items()))
    failed += [("sens", name, v) for name, v in sens.items() if not np.isfinite(v)]
    if failed:
        raise SystemExit(f"nothing written: {failed}")
    for out in outs:
        out.update({"sens_" + name: np.float64(v) for name, v in sens.items()})
    if check_only:
        for t, out in enumerate(outs):
            old = load_split(f"driver_c12_tile{t}")
            assert sorted(old) == sorted(out), (t, sorted(set(old) ^ set(out)))
            for k in old:
                assert np.array_equal(old[k], out[k]), (t, k)
            print("tile", t, "reproduces the committed fixture")
        return
    for t, out in enumerate(outs):
        save_split(f"driver_c12_tile{t}", out)


if __name__ == "__main__":
    main()
