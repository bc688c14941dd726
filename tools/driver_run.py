"""Run the model from one of the reference's driver configuration files: pace_amd.driver.Driver, its step_all, one JSON line.

    python tools/driver_run.py CONFIG.yaml [--steps N] [--device D] [--cpu-emulation] [--diagnostics DIR]
                               [--diagnostics-format npz|netcdf] [--write-fortran-restart DIR] [--cube]

runs ONE rank (tile 0) with the `null` communicator -- its halos receive zeros, so this exercises the loop, not the weather --
and, launched under torch.distributed.run as tools/dycore_run.py is,

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 6 --master-addr 127.0.0.1 --master-port 29511 \\
        tools/driver_run.py CONFIG.yaml [--steps N] [--cpu-emulation]

the six tiles of the cubed sphere, one process per tile (RCCL on GPUs, gloo with --cpu-emulation).  A lone process whose file
says `comm_config: {type: cube}`, or which is given --cube, runs the six tiles itself on ONE device
(pace_amd.driver.run_cube_driver: every halo update is one kernel launch for the whole cube) and prints the same line.
--steps replaces the
file's run length.  --diagnostics DIR writes the file's diagnostics into DIR as per-tile numpy archives (it replaces
diagnostics_config.path and sets output_format: npz; pace_amd.driver.NpzMonitor describes the files).  With --cube the globe is
gathered (one pace_cube_gather launch per store) and rank 0 writes one file per time chunk with a tile axis of 6, as npz or,
with --diagnostics-format netcdf, as NetCDF-3 (pace_amd.util.NetCDFMonitor).
--write-fortran-restart DIR writes the final state into DIR as restart files of the Fortran model (Driver.write_fortran_restart)
with a restart.yaml, from which `python tools/driver_run.py DIR/restart.yaml` resumes.  Rank 0 prints: workload, steps, ms per step (mean of the main loop's clock, the slowest rank), SYPD
(Driver.sypd()), and the time of the safety check per call with its verdict: the checks the file asks for inside the loop
(safety_check_frequency) and, after the run, three timed calls on the final state whose verdict is reported, not raised (a lone
tile behind zero halos need not stay within the bounds).
"""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--steps", type=int, default=None, help="run this many steps instead of the file's days / hours / minutes / seconds")
    ap.add_argument("--device", default=None, help="one-rank runs: the device (default cuda:0)")
    ap.add_argument("--cpu-emulation", action="store_true", help="the CPU emulation library (and gloo): a logic check, not a timing")
    ap.add_argument("--diagnostics", metavar="DIR", default=None,
                    help="write the file's diagnostics into DIR (diagnostics_config.path = DIR, output_format = npz)")
    ap.add_argument("--write-fortran-restart", metavar="DIR", default=None,
                    help="write the final state into DIR in the Fortran model's restart format, with a restart.yaml that resumes from it")
    ap.add_argument("--diagnostics-format", choices=("npz", "netcdf"), default="npz",
                    help="with --diagnostics: numpy archives, or (with --cube) NetCDF-3 files of the whole globe")
    ap.add_argument("--cube", action="store_true", help="a lone process: run all six tiles on the one device (comm_config.type: cube)")
    args = ap.parse_args()
    import yaml

    from pace_amd import _lib
    from pace_amd.driver import Driver, DriverConfig

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    with open(args.config) as f:
        settings = yaml.safe_load(f)
    cube = world == 1 and (args.cube or (settings.get("comm_config") or {}).get("type") == "cube")
    if args.cube and world != 1:
        raise SystemExit("--cube runs the six tiles in ONE process: start it without a launcher")
    if cube:
        settings["comm_config"] = {"type": "cube"}
        device = "cpu" if args.cpu_emulation else (args.device or "cuda:0")
    elif world == 1:
        settings["comm_config"] = {"type": "null", "config": {"rank": 0, "total_ranks": 6}}
        device = "cpu" if args.cpu_emulation else (args.device or "cuda:0")
    elif world == 6:
        import torch.distributed as dist

        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if args.cpu_emulation:
            dist.init_process_group(backend="gloo")
            device = "cpu"
        else:
            dist.init_process_group(backend="nccl", device_id=torch.device(f"cuda:{local_rank}"))
            device = f"cuda:{local_rank}"
        settings["comm_config"] = {"type": "torch"}
    else:
        raise SystemExit("a cubed sphere has six tiles: launch six ranks, or one for a lone tile")
    if device != "cpu":
        torch.cuda.set_device(torch.device(device))
    if args.steps is not None:
        settings.update(days=0, hours=0, minutes=0, seconds=0)
    if args.diagnostics is not None:
        if args.diagnostics_format == "netcdf" and not cube:
            raise SystemExit("--diagnostics-format netcdf is written for the whole cube only: add --cube")
        settings["diagnostics_config"] = dict(settings.get("diagnostics_config") or {}, path=args.diagnostics,
                                              output_format=args.diagnostics_format)
    config = DriverConfig.from_dict(settings)
    if args.steps is not None:
        config.seconds = int(round(args.steps * config.dt_atmos))
        if config.n_timesteps() != args.steps:
            raise SystemExit(f"--steps {args.steps} is no whole number of seconds at dt_atmos {config.dt_atmos}")
        config.source["seconds"] = config.seconds  # (a restart.yaml of this run runs as long as this run)
    lib = _lib.Library(os.path.join(ROOT, "tests", "emu", "libpace_emu.so")) if args.cpu_emulation else _lib.load()
    if cube:
        from pace_amd.util import run_cube

        def tile(comm):  # (run_cube_driver's program, with the restart written before the clean-up)
            d = Driver(copy.deepcopy(config), comm=comm, lib=lib, device=device)
            d.step_all()
            if args.write_fortran_restart is not None:
                d.write_fortran_restart(args.write_fortran_restart)
            d.cleanup()
            return d

        drivers = run_cube(tile)
        driver = drivers[0]
    else:
        drivers = [Driver(config, lib=lib, device=device)]
        driver = drivers[0]
        driver.step_all()
        if args.write_fortran_restart is not None:
            driver.write_fortran_restart(args.write_fortran_restart)
    if device != "cpu":
        torch.cuda.synchronize()
    steps = config.n_timesteps()
    loop, total = driver.performance_collector.timestep_timer, driver.performance_collector.total_timer
    ms_per_step = max(1e3 * d.performance_collector.timestep_timer.times.get("mainloop", 0.0)
                      / max(1, d.performance_collector.timestep_timer.hits.get("mainloop", 0)) for d in drivers)
    checks = total.hits.get("safety_check", 0)
    verdict, check_times = "within bounds", []
    for _ in range(3):
        t0 = time.perf_counter()
        try:
            driver.safety_checker.check_state(driver.state.dycore_state)  # (ends in its own transfer: the host clock sees all of it)
        except RuntimeError as e:
            verdict = " ".join(str(e).split())
        check_times.append(1e3 * (time.perf_counter() - t0))
    check_ms = sorted(check_times)[1]
    sypd = driver.sypd()
    if cube:
        sypd = config.dt_atmos / (ms_per_step * 1e-3) / 365.0 if ms_per_step > 0 else sypd
    if world == 6:
        t = torch.tensor([ms_per_step], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        ms_per_step = float(t.item())
        sypd = config.dt_atmos / (ms_per_step * 1e-3) / 365.0 if ms_per_step > 0 else sypd
    pt = driver.state.dycore_state.pt.numpy()
    if rank == 0:
        what = "dycore only" if config.dycore_only else ("dycore, no physics coupling" if config.disable_step_physics else "dycore + microphysics")
        print(json.dumps({
            "workload": f"Driver.step_all, C{config.nx_tile}x{config.nz}L, {what}, n_split={config.dycore_config.n_split}, "
                        f"k_split={config.dycore_config.k_split}, dt_atmos={config.dt_atmos:g} s, "
                        + ("six tiles, one process per tile" if world == 6 else
                           "six tiles in one process on one device" if cube else "ONE tile, null communicator (zero halos)"),
            "n_gpus": 0 if args.cpu_emulation else world, "steps": steps, "ms_per_step": ms_per_step, "sypd": sypd,
            "safety_checks_in_loop": checks, "safety_check_ms_per_call": check_ms, "safety_check": verdict,
            "nan_fraction_pt": float((pt != pt).mean()),
            "transport": "CPU emulation" if args.cpu_emulation else ("RCCL" if world == 6 else "pace_halo_cube" if cube else "none")}))
    if not cube:
        driver.cleanup()
    if world == 6:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
