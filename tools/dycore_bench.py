"""Timing of whole DynamicalCore steps on the GPU box: the six tiles of a cubed sphere resident on ONE device (one host
thread per tile, halo exchanges through ThreadComm), synthetic balanced state, fp64.

    python tools/dycore_bench.py [--n 192] [--nz 79] [--n-split 4] [--steps 2] [--single] [--sat-adj] [--sg-adj]
                                 [--tracer-subcycling {fixed,courant}]

Prints the wall time per step for all six tiles (the device is shared, so per tile = / 6) and the split between the
acoustic loop, the tracer advection, the remapping and the rest, from synchronising timers.
"""
import argparse
import datetime
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


class SyncTimer:
    def __init__(self):
        self.t = {}

    def clock(self, name):
        timer = self

        class Ctx:
            def __enter__(self):
                torch.cuda.synchronize()
                self.t0 = time.perf_counter()

            def __exit__(self, *a):
                torch.cuda.synchronize()
                timer.t[name] = timer.t.get(name, 0.0) + time.perf_counter() - self.t0
                return False

        return Ctx()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=192)
    ap.add_argument("--nz", type=int, default=79)
    ap.add_argument("--n-split", type=int, default=4)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--precision", type=int, default=64, choices=(64, 32), help="storage type of the fields: libpace_hip.so or libpace_hip_f32.so")
    ap.add_argument("--single", action="store_true",
                    help="one tile only, behind a lone-rank LoopbackComm (each halo receives what the tile sent to that neighbour): the "
                         "device time of one tile's step without the thread rendezvous of the six-tile mode")
    ap.add_argument("--sat-adj", action="store_true", help="do_sat_adj = True: the saturation adjustment runs in the remapping")
    ap.add_argument("--sg-adj", action="store_true",
                    help="fv_sg_adj = 600: the reference driver's end of a dycore-only step runs after each step -- DycoreToPhysics (the "
                         "dry convective adjustment, reported as dry_conv_adjust), then UpdateAtmosphereState (fill_gfs_delp and "
                         "ApplyPhysicsToDycore with its halo updates, reported as update_atmos_state)")
    ap.add_argument("--comm", default="thread", choices=("thread", "cube"),
                    help="six tiles: ThreadComm (pack, device-side copies, unpack per tile) or DeviceCubeComm (run_cube: one "
                         "pace_halo_cube launch per halo update for the whole cube)")
    ap.add_argument("--tracer-subcycling", default="fixed", choices=("fixed", "courant"),
                    help="the tracer advection's sub-cycles: the reference's three on every level, or int(1 + cmax(k)) on level k from "
                         "the level's largest Courant number over the globe (DynamicalCoreConfig.tracer_courant_subcycling); the "
                         "counts of the last step are printed")
    args = ap.parse_args()
    if os.environ.get("PACE_BENCH_TRACE"):
        import faulthandler

        faulthandler.dump_traceback_later(float(os.environ["PACE_BENCH_TRACE"]), exit=True)
    from helpers import Env, acoustic_config, dycore_condensates

    from pace_amd import _lib, synthetic
    from pace_amd.fv3core import DynamicalCoreConfig
    from pace_amd.fv3core.initialization.dycore_state import DycoreState
    from pace_amd.fv3core.stencils.fv_dynamics import DynamicalCore
    from pace_amd.util import CubedSphereCommunicator, LoopbackComm, constants as c, run_cube, run_tiles

    lib = _lib.load(args.precision)
    n, nz = args.n, args.nz
    metrics = synthetic.tile_metrics(n, nz)
    courant = args.tracer_subcycling == "courant"
    if courant:  # the synthetic tile has no cell-centre sine: the mean of its four face sines stands in
        metrics = dict(metrics, sin_sg5=np.minimum(0.25 * sum(metrics[f"sin_sg{m}"] for m in (1, 2, 3, 4)), 1.0))
    s = synthetic.acoustic_state(metrics, n, nz)
    dt_atmos = float(s["dt"]) * args.n_split
    results = {}
    lock = threading.Lock()
    driver_terms = None
    if args.sg_adj:  # the driver grid terms of the six tiles, generated once for all tile threads
        from pace_amd.util import gridgen

        driver_terms = gridgen.tiles(n, nz)

    def program(comm):
        tile = comm.Get_rank()
        env = Env(lib, "cuda", metrics, n, nz)
        cube = CubedSphereCommunicator(comm, device="cuda", lib=lib)
        arrays = {k: s[k] for k in "u v w delz delp pt pe uc vc ua va q_con".split()}
        arrays["peln"] = np.log(s["pe"])
        arrays["pk"] = np.exp(c.KAPPA * arrays["peln"])
        arrays["phis"] = c.GRAV * s["zs"]
        arrays["ps"] = s["pe"][:, :, nz]
        arrays["pt"] = s["pt"] * np.exp(c.KAPPA * np.log(1.0e5))  # a temperature-like magnitude
        arrays["qvapor"] = 0.01 * np.exp(-6.0 * (1.0 - s["pe"] / s["pe"][:, :, nz:])) * (s["delp"] > 0)
        for name, f in dycore_condensates(tile, s["delp"].shape).items():
            arrays[name] = np.abs(f)
        state = DycoreState.init_from_numpy_arrays(arrays, env.qf)
        config = DynamicalCoreConfig(npx=n + 1, npy=n + 1, npz=nz, dt_atmos=dt_atmos, k_split=1, n_split=args.n_split,
                                     acoustic_dynamics=acoustic_config(args.n_split), do_sat_adj=args.sat_adj,
                                     fv_sg_adj=600 if args.sg_adj else -1, tracer_courant_subcycling=courant)
        core = DynamicalCore(cube, env.grid_data, env.stencil_factory, env.qf, env.damping, config, state.phis, state,
                             datetime.timedelta(seconds=dt_atmos))
        to_physics = None
        if config.do_dry_convective_adjustment:  # (driver: driver/pace/driver/driver.py:618-640)
            import types

            from pace_amd.stencils import DycoreToPhysics, UpdateAtmosphereState
            from pace_amd.util.grid import DriverGridData

            terms = driver_terms[tile]
            info = DriverGridData.new_from_grid_variables(**{k: terms[k] for k in ("vlon", "vlat", "es1", "ew2", "edge_vect_w", "edge_vect_e",
                                                                                    "edge_vect_s", "edge_vect_n")}, quantity_factory=env.qf)
            tend = types.SimpleNamespace(u_dt=env.q3(), v_dt=env.q3(), pt_dt=env.q3())
            adj = types.SimpleNamespace(nwat=config.nwat, fv_sg_adj=config.fv_sg_adj, n_sponge=min(config.n_sponge, nz),
                                        hydrostatic=config.hydrostatic, layout=config.layout)
            to_physics = DycoreToPhysics(env.stencil_factory, env.qf, adj, True, True)
            update = UpdateAtmosphereState(env.stencil_factory, env.grid_data, config, cube, info, state, env.qf, True, True, tend)
        core.step_dynamics(state)  # warm-up
        torch.cuda.synchronize()
        comm.barrier()
        timer = SyncTimer()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            core.step_dynamics(state, timer)
            if to_physics is not None:
                with timer.clock("dry_conv_adjust"):
                    to_physics(state, None, tend, dt_atmos)
                with timer.clock("update_atmos_state"):
                    update(state, None, tend.u_dt, tend.v_dt, tend.pt_dt, dt_atmos)
        torch.cuda.synchronize()
        comm.barrier()
        wall = time.perf_counter() - t0
        with lock:
            results[tile] = (wall, dict(timer.t), float(np.isnan(state.w.numpy()).mean()), float(np.isnan(state.pt.numpy()).mean()),
                             core.tracer_subcycles() if courant else None)

    if args.single:
        program(LoopbackComm(rank=0, total_ranks=6))
        wall = results[0][0] / args.steps
        cells = n * n * nz
        print(f"C{n} x {nz}L, ONE tile (lone-rank LoopbackComm), n_split = {args.n_split}, k_split = 1, do_sat_adj = {args.sat_adj}, "
              f"{args.steps} steps")
        print(f"wall per step: {1e3 * wall:9.2f} ms   ({cells * args.n_split / wall / 1e9:5.2f} G cell-updates/s counting the "
              f"acoustic substeps; the timers synchronise the device at every section boundary)")
    else:
        run_cube(program) if args.comm == "cube" else run_tiles(6, program)
        wall = max(r[0] for r in results.values()) / args.steps
        cells = 6 * n * n * nz
        print(f"C{n} x {nz}L, six tiles on one device (--comm {args.comm}), n_split = {args.n_split}, k_split = 1, do_sat_adj = {args.sat_adj}, "
              f"{args.steps} steps")
        print(f"wall per step (six tiles): {1e3 * wall:9.2f} ms   = {1e3 * wall / 6:7.2f} ms per tile   "
              f"({cells * args.n_split / wall / 1e9:5.2f} G cell-updates/s counting the acoustic substeps)")
    t = results[0][1]
    tot = sum(t.values())
    for k, v in t.items():
        print(f"  {k:18s} {1e3 * v / args.steps:9.2f} ms of tile 0's wall time (threads interleave on the device) {100 * v / tot:5.1f} %")
    print(f"  NaN fraction after the run: w {results[0][2]:.2e}, pt {results[0][3]:.2e}")
    if courant:
        counts = results[0][4]
        print(f"  tracer sub-cycles of the last step (--tracer-subcycling courant): " +
              ", ".join(f"{int((counts == v).sum())} levels x {int(v)}" for v in np.unique(counts)) + "; fixed: every level x 3")
    else:
        print("  tracer sub-cycles (--tracer-subcycling fixed): every level x 3")


if __name__ == "__main__":
    main()
