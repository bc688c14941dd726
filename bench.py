"""Benchmark of the hot path named in BASELINE.json: one acoustic substep = d_sw + riem_solver3 on one
cubed-sphere tile per GPU, fp64, C192 x 79 levels, synthetic (baroclinic-like) state.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--n 192] [--nz 79] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A "step" is one d_sw call followed by one riem_solver3 call on one pristine, HBM-resident copy of the
model state (K + W copies are staged before the timed region, up to STATE_POOL_BYTES of them: more steps are
timed in rounds, and the copies are restored between rounds; nothing is re-used between steps, so no step
benefits from cached data of the previous one).  Prints ONE JSON line on rank 0.

A plain run does only what the headline needs: set-up, warm-up, the K timed steps, the line.  --full adds
what else the benchmark measures and checks after the timed region: the dominant kernel alone and its
roofline (HBM traffic from two rocprofv3 --pmc child passes, stream bandwidths), the substep under d_sw's
other output contract, the CPU baseline and the verification of the last timed step against the oracle,
and the per-phase diagnosis of a multi-rank step.  --dump-outputs DIR writes what the last timed step
computed (rank 0's tile) as DIR/<field>.npy: see dump_outputs.

Multi-GPU: one tile per GPU, weak scaling.  With exactly 6 ranks the ranks ARE the six faces of the cube and the
delp / pt / q_con halo exchange that sits between d_sw and riem_solver3 in the acoustic loop (dyn_core.py:854) runs
inside the timed region: HIP pack -> one grouped RCCL send/recv per rank -> HIP unpack.  With any other rank count
there is no cubed-sphere topology to exchange over; the tiles are independent replicas (no data-path collective).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md)
BYTES_PER_CELL_UPDATE = 360.0  # d_sw 32 fields + riem_solver3 13 fields, fp64
TRANSPORT_FIELDS = 9  # fused transport kernel: q, crx, cry, xfx, yfx, x/y mass flux, delp in; updated scalar out
STATE_POOL_BYTES = 64 << 30  # device memory for the staged state copies (~90 copies at C192 x 79, fp64): a bound set by the arguments
DUMP_VALUES_PER_FIELD = 1 << 18  # --dump-outputs: at most this many values per field (at most 29 fields x 2 MiB in fp64: < 64 MB in all)


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=None)  # (None: one, or what a launcher's WORLD_SIZE says)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--n", "--tile-size", dest="n", type=int, default=192)  # (--n alone is ambiguous to torch.distributed.run)
    p.add_argument("--nz", type=int, default=79)
    p.add_argument("--precision", type=int, default=64, choices=(64, 32),
                   help="storage type of the fields (the headline metric is fp64; 32 runs libpace_hip_f32.so: float32 fields, "
                        "float64 arithmetic in registers)")
    p.add_argument("--state", choices=("baroclinic", "synthetic"), default="baroclinic",
                   help="baroclinic: the operands of the second acoustic substep of the Jablonowski-Williamson case on the gnomonic "
                        "cubed sphere (grid and initial state from pace_amd's own generators, six tiles stepped together on the "
                        "device once, this rank's tile captured at the reference's D_SW-In checkpoint; cached in the temp dir); "
                        "synthetic: pace_amd/synthetic.py's single-tile balanced state (no set-up cost)")
    p.add_argument("--full-outputs", action="store_true",
                   help="d_sw also brings its dead work fields (delpc, divgd, uc, vc) to the state the reference leaves them in, as "
                        "the last substep of a remapping step does (default: skipped, as in every other substep of AcousticDynamics)")
    p.add_argument("--full", action="store_true",
                   help="after the timed region, also measure and check what the headline does not need: the dominant kernel's roofline, "
                        "the other output contract, the CPU baseline + verification against the oracle, the multi-rank phase diagnosis "
                        "(each of them can be left out again by its --no-* option)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the output fields of the last timed step as DIR/<field>.npy (a fixed sample of each larger field)")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-traffic", action="store_true", help="skip the two rocprofv3 --pmc child passes that measure roofline.traffic")
    p.add_argument("--no-other-contract", action="store_true",
                   help="skip the timing of the substep under d_sw's other output contract (profiled runs: its launches would be averaged "
                        "into the step's kernels)")
    p.add_argument("--watchdog", type=float, default=900.0, help="multi-rank runs: seconds after which a stuck run exits")
    p.add_argument("--exchange", choices=("on", "off"), default="on",
                   help="multi-rank runs: keep the delp/pt/q_con halo exchange inside the measured step (default) or run the tiles independently")
    p.add_argument("--graph", choices=("on", "off"), default="off",
                   help="replay each step from a captured HIP graph (measured: no gain at C48 ... C192 -- the launches are "
                        "already queued ahead of the GPU; kept as an option)")
    p.add_argument("--overlap", choices=("on", "off", "auto"), default="auto",
                   help="the wind half of d_sw on a side stream next to the scalar phase / the column solver (on), or the whole step "
                        "on one stream (off).  auto: off on one GPU -- measured in round 4 at C48 / C96 / C192: 0.224 / 0.345 / 0.966 ms "
                        "on one stream against 0.248 / 0.373 / 0.978 with the side stream (the sum of the kernels' isolated times is "
                        "the step: nothing is left to overlap) --, on when a halo exchange is in flight (more than one rank)")
    p.add_argument("--full-loop", action="store_true",
                   help="multi-rank runs: after the timed region, run the WHOLE acoustic loop body (AcousticDynamics: c_sw ... nh_p_grad, "
                        "all seven halo exchanges of a substep over the transport of the run) and report ms per substep and the host time "
                        "of every halo updater under comm.full_loop -- a diagnosis, never part of `value`")
    p.add_argument("--emulate", action="store_true",
                   help="TEST ONLY (tests/test_halo.py): run the multi-rank code path -- partitioner, pack / exchange / unpack, barrier, "
                        "max-over-ranks reduction, the JSON line -- on the CPU over gloo with the emulation build of the kernels; no "
                        "performance meaning, the line says so")
    return p.parse_args()


def column_namelist(nz, qf):
    from pace_amd.fv3core import DGridShallowWaterLagrangianDynamicsConfig
    from pace_amd.fv3core.stencils.d_sw import get_column_namelist

    return get_column_namelist(DGridShallowWaterLagrangianDynamicsConfig(), qf)


_CPU = {}  # per worker process: the operands of the measured substep, loaded once


def _cpu_load(path):
    if _CPU.get("path") != path:
        d = np.load(path)
        _CPU.clear()
        _CPU.update(path=path, metrics={k[2:]: d[k] for k in d.files if k.startswith("m_")},
                    s={k[2:]: d[k] for k in d.files if k.startswith("f_")}, dt=float(d["dt"]), ptop=float(d["ptop"]))
    return _CPU


def _cpu_dsw_slab(args):
    """One worker, phase 1: the numpy oracle's d_sw on a slab of levels (levels are independent in d_sw).  Returns (seconds,
    {name: output slab})."""
    path, n, nz, k0, k1 = args
    import time as _t

    from oracle import dgrid_sw
    from oracle._np import Grid
    from pace_amd.fv3core import DGridShallowWaterLagrangianDynamicsConfig
    from pace_amd.fv3core.stencils.d_sw import column_namelist_arrays
    from pace_amd.tile import DSW_ARGS, DSW_CFG

    c = _cpu_load(path)
    s = c["s"]
    col = column_namelist_arrays(DGridShallowWaterLagrangianDynamicsConfig(), nz)
    nk = k1 - k0
    sl = lambda a_: np.ascontiguousarray(np.concatenate([a_[:, :, k0:k1], a_[:, :, k1 - 1:k1]], axis=2))  # noqa: E731
    colk = {k: np.ascontiguousarray(np.concatenate([v[k0:k1], v[k1 - 1:k1]])) for k, v in col.items()}
    g = Grid(n, nk, c["metrics"])
    a = {k: sl(s[k]) for k in DSW_ARGS}
    st = dgrid_sw.DSWState(a["u"].shape)
    t0 = _t.perf_counter()
    dgrid_sw.d_sw(g, colk, DSW_CFG, st, *[a[k] for k in DSW_ARGS], c["dt"])
    sec = _t.perf_counter() - t0
    return sec, {k: a[k][:, :, :nk] for k in DSW_ARGS if k != "zh"}


def _cpu_riem_strip(args):
    """One worker, phase 2: the oracle's riem_solver3 on all levels of a strip of rows (columns are independent), on the fields
    d_sw left (file `upd`).  Returns (seconds, {name: output strip})."""
    path, upd, n, nz, j0, j1 = args
    import time as _t

    from oracle import vertical
    from oracle._np import Grid

    c = _cpu_load(path)
    s = c["s"]
    u = np.load(upd)
    rows = slice(3 + j0, 3 + j1)
    b = {k: np.ascontiguousarray((u[k] if k in u.files else s[k])[:, rows])
         for k in ("cappa", "delz", "q_con", "delp", "pt", "zh", "pe", "ppe", "pk3", "pk", "peln", "w")}
    zs, ws = np.ascontiguousarray(s["zs"][:, rows]), np.ascontiguousarray(s["ws"][:, rows])
    gr = Grid(n, nz, c["metrics"])
    gr.js, gr.je, gr.nj = 0, (j1 - j0) - 1, j1 - j0
    t0 = _t.perf_counter()
    vertical.riem_solver3(gr, False, c["dt"], b["cappa"], c["ptop"], zs, ws, b["delz"], b["q_con"], b["delp"], b["pt"], b["zh"], b["pe"],
                          b["ppe"], b["pk3"], b["pk"], b["peln"], b["w"], p_fac=0.05)
    sec = _t.perf_counter() - t0
    return sec, {k: b[k] for k in ("delz", "zh", "ppe", "pk3", "w")}


def _cpu_omp_job(args):
    """One child process: the C++ / OpenMP restatement (oracle/omp/dsw_riem3.cpp: one parallel loop nest per reference stencil, i
    first, whole-field temporaries) of d_sw + riem_solver3 on the operands the GPU was timed on, all host cores.  1 warm-up,
    `reps` timed substeps (operands restored outside the timed region).  Returns (list of seconds, threads, outputs of the warm-up
    run in the oracle's layout)."""
    path, n, nz, reps, threads, bind = args
    import time as _t

    # bind: threads pinned to cores, next to each other (set before the OpenMP runtime starts in this fresh process).  Either way the
    # operands and the workspace are first touched BY THE TEAM, level by level as the loop nests walk them (oracle/omp_port.py team_copy)
    if bind:
        os.environ["OMP_PROC_BIND"] = "close"
        os.environ["OMP_PLACES"] = "cores"
    from oracle import omp_port
    from oracle._np import Grid
    from pace_amd.fv3core import DGridShallowWaterLagrangianDynamicsConfig
    from pace_amd.fv3core.stencils.d_sw import column_namelist_arrays
    from pace_amd.tile import DSW_CFG

    c = _cpu_load(path)
    s = c["s"]
    omp_port.load()
    col = column_namelist_arrays(DGridShallowWaterLagrangianDynamicsConfig(), nz)
    tile = omp_port.Tile(Grid(n, nz, c["metrics"]))
    zero = np.zeros_like(s["u"])
    dsw = omp_port.DswCall(tile, col, DSW_CFG, zero, zero, {k: s[k] for k in omp_port.DSW_FIELDS}, c["dt"])
    omp_port.set_threads(min(threads, 8))
    dsw.run()  # warm-up (page faults, the workspace) -- and the operands of the column solver
    o = dsw.outputs()
    riem = omp_port.RiemCall(tile, {k: (o[k] if k in ("q_con", "delp", "pt", "w") else s[k]) for k in omp_port.RIEM_FIELDS},
                             False, c["dt"], c["ptop"], 0.05)
    riem.run()
    r = riem.outputs()
    out = {k: np.ascontiguousarray(o[k]) for k in omp_port.DSW_FIELDS}
    out.update({"riem." + k: np.ascontiguousarray(r[k]) for k in ("delz", "zh", "ppe", "pk3", "w")})
    # The thread count: the box reports more logical cores than this (ordinary-user, containerised) process is given time on,
    # and an OpenMP team larger than that collapses (measured: 256 threads on the 256 reported cores, 21.8 s per substep; 8 threads
    # on 8 real cores, 0.2 s).  So the team size is chosen by measurement: doubling from 8 up to the reported count while one
    # d_sw gets faster; the timed repetitions then use the best one -- `cores` reports it.
    tried, best_t, best = {}, min(threads, 8), None
    t = min(threads, 8)
    while True:
        omp_port.set_threads(t)
        dsw.reset()
        riem.reset()
        t0 = _t.perf_counter()
        dsw.run()
        riem.run()  # (both operators: on a shared host the column solver's best team is not d_sw's)
        tried[t] = _t.perf_counter() - t0
        if best is None or tried[t] < best:
            best, best_t = tried[t], t
        if tried[t] > 1.5 * best or t >= threads:
            break
        t = min(2 * t, threads)
        dsw.work = omp_port._fresh(dsw.src)  # (first touch by the NEW team)
        dsw.fp = omp_port._ptrs(dsw.work)
        riem.work = omp_port._fresh(riem.src)
        riem.fp = omp_port._ptrs(riem.work)
    omp_port.set_threads(best_t)
    secs = []
    for _ in range(reps):
        dsw.reset()
        riem.reset()
        t0 = _t.perf_counter()
        dsw.run()
        riem.run()
        secs.append(_t.perf_counter() - t0)
    return secs, best_t, out, {str(k): round(v, 4) for k, v in tried.items()}


def cpu_baseline(n, nz, metrics, s, dt, ptop, reps=10, numpy_reps=3):
    """The CPU baseline of SURVEY.md section 8(d): the C++ / OpenMP restatement at the reference's granularity (one parallel loop
    nest per reference stencil, i first, every intermediate a whole field in memory -- what the reference's gt:cpu_ifirst
    backend generates; oracle/omp/dsw_riem3.cpp, bit-identical to the numpy oracle in d_sw, tests/test_oracle_omp.py) on ALL
    host cores and on the SAME operands the GPU was timed on.  Protocol of BASELINE.md section 4.1: one warm-up, `reps` timed
    substeps, the MEDIAN.  kind = 'port' (the reference's own CPU backend needs GT4Py + GridTools and cannot be built here).
    Beside it, as in rounds 1-2, the numpy oracle in one process per core (`numpy_*` keys; `numpy_reps` timed substeps): phase 1 =
    d_sw on a slab of levels per process, phase 2 = riem_solver3 on a strip of rows per process.
    Returns (record, outputs): the NUMPY oracle's output fields of the substep, for bench.py's `verified`."""
    import multiprocessing as mp
    import tempfile

    cores = max(1, min(os.cpu_count() or 1, nz, 32))  # (every worker maps the operands: bounded)
    # level slabs: the first one holds the three sponge levels AND a level below them -- the oracle, like the reference, derives
    # where the high-order divergence damping starts from the first level with nord > 0 of the column it is given
    first = min(nz, max(4, round(nz / cores)))
    rest = max(1, cores - 1)
    kb = [0] + [first + round(i * (nz - first) / rest) for i in range(rest + 1)] if nz > first else [0, nz]
    jb = [round(i * n / cores) for i in range(cores + 1)]
    tmp = tempfile.mkdtemp(prefix="pace_cpu_", dir=os.environ.get("PACE_BENCH_CACHE", tempfile.gettempdir()))
    path, upd = os.path.join(tmp, "operands.npz"), os.path.join(tmp, "after_dsw.npz")
    np.savez(path, dt=dt, ptop=ptop, **{"m_" + k: np.asarray(v) for k, v in metrics.items()},
             **{"f_" + k: v for k, v in s.items() if isinstance(v, np.ndarray)})
    jobs1 = [(path, n, nz, kb[i], kb[i + 1]) for i in range(len(kb) - 1) if kb[i + 1] > kb[i]]
    jobs2 = [(path, upd, n, nz, jb[i], jb[i + 1]) for i in range(cores) if jb[i + 1] > jb[i]]
    ctx = mp.get_context("spawn")  # no fork from a process that has initialised the GPU
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    walls, out = [], {}
    try:
        with ctx.Pool(len(jobs1)) as pool:
            for rep in range(numpy_reps + 1):  # rep 0: warm-up (imports, page faults, the operands file)
                r1 = pool.map(_cpu_dsw_slab, jobs1)
                if rep == 0:
                    for k in r1[0][1]:
                        full = np.array(s[k], dtype=np.float64)
                        for (p_, n_, nz_, k0, k1), (_, o) in zip(jobs1, r1):
                            full[:, :, k0:k1] = o[k]
                        out[k] = full
                    np.savez(upd, **{k: out[k] for k in ("q_con", "delp", "pt", "w")})
                r2 = pool.map(_cpu_riem_strip, jobs2)
                if rep == 0:
                    for k in r2[0][1]:
                        full = np.array(out[k] if k in out else s[{"ppe": "ppe"}.get(k, k)], dtype=np.float64)
                        for (p_, u_, n_, nz_, j0, j1), (_, o) in zip(jobs2, r2):
                            full[:, 3 + j0:3 + j1] = o[k]
                        out["riem." + k] = full
                    continue
                walls.append(max(x[0] for x in r1) + max(x[0] for x in r2))
            one = pool.map(_cpu_dsw_slab, jobs1[:1])[0][0] + pool.map(_cpu_riem_strip, jobs2[:1])[0][0]  # one share, the other cores idle
        ncpu = os.cpu_count() or 1
        omp_err = None
        try:
            # twice, each in a process of its own (no other OpenMP runtime, no GPU context): threads left to the scheduler, and
            # pinned (OMP_PROC_BIND=close OMP_PLACES=cores) -- on a containerised host whose process may run on fewer cores than it is
            # shown, pinning was measured 3 x SLOWER (round 6: 105 against 30 ms); the faster of the two is the baseline
            # (bounded: a worker that dies -- a library built for another CPU -- must not hang the bench line)
            runs = []
            for bind in (False, True):
                with ctx.Pool(1) as pool:
                    runs.append(pool.map_async(_cpu_omp_job, [(path, n, nz, reps, ncpu, bind)]).get(timeout=300)[0] + (bind,))
            runs.sort(key=lambda r_: float(np.median(r_[0])))
            omp_secs, omp_threads, omp_out, omp_tried, omp_bound = runs[0]
            omp_other = {"pinned" if runs[1][4] else "not pinned": f"{float(np.median(runs[1][0])) * 1e3:.1f} ms on {runs[1][1]} threads"}
        except Exception as e:  # noqa: BLE001 -- the numpy figure below still stands
            omp_err = f"{type(e).__name__}: {str(e)[:200]}"
            sys.stderr.write(f"[bench] the C++ / OpenMP baseline failed ({omp_err}); reporting the numpy oracle's figure\n")
    finally:
        import shutil

        shutil.rmtree(tmp, ignore_errors=True)
    wall = float(np.median(walls))
    numpy_rec = {"numpy_value": n * n * nz / wall, "numpy_cores": len(jobs1),
                 "numpy_sample": f"{numpy_reps} substeps after 1 warm-up, numpy oracle, {len(jobs1)} processes (levels / rows split), median "
                                 f"{wall:.2f} s (min {min(walls):.2f}, max {max(walls):.2f})",
                 "numpy_one_core_value": n * n * nz / (one * len(jobs1))}
    if omp_err is not None:
        rec = {"value": numpy_rec["numpy_value"], "unit": "cell-updates/s", "cores": len(jobs1), "kind": "port",
               "detail": f"numpy oracle (the C++ / OpenMP restatement could not be run here: {omp_err})", "sample": numpy_rec["numpy_sample"], **numpy_rec}
        return rec, out
    owall = float(np.median(omp_secs))
    # the restatement against the numpy oracle on these operands (d_sw: the same operations in the same order; the column solver
    # through another libm): worst error relative to each field's magnitude
    port_err = 0.0
    for k, v in omp_out.items():
        if k in out and k != "zh":
            a_, b_ = np.asarray(out[k], dtype=np.float64)[3:3 + n, 3:3 + n, :nz], v[3:3 + n, 3:3 + n, :nz]
            port_err = max(port_err, float(np.abs(a_ - b_).max() / max(np.abs(a_).max(), 1e-300)))
    rec = {"value": n * n * nz / owall, "unit": "cell-updates/s", "cores": omp_threads, "kind": "port",
           "detail": "restatement, reference granularity: C++ / OpenMP, one parallel loop nest per reference stencil, i first, "
                     f"OMP_NUM_THREADS = {omp_threads}, the fastest team size on this host (seconds of one substep per team size: {omp_tried}; "
                     f"{ncpu} logical cores reported), threads {'pinned to cores (OMP_PROC_BIND=close)' if omp_bound else 'not pinned'} "
                     f"(the other way: {omp_other}), operands and workspace first touched by the team (oracle/omp/dsw_riem3.cpp)",
           "sample": f"{reps} substeps (d_sw + riem_solver3) at C{n}x{nz}L after 1 warm-up, the operands the GPU was timed on, median "
                     f"{owall * 1e3:.1f} ms (min {min(omp_secs) * 1e3:.1f}, max {max(omp_secs) * 1e3:.1f})",
           "max_error_vs_numpy_oracle": port_err, **numpy_rec}
    return rec, out


DEAD_AFTER_DSW = ("delpc", "divgd", "uc", "vc")  # work fields of the divergence damping (d_sw.py:1032-1033)


def verify_against_oracle(got, ref, n, nz, skip=()):
    """One timed batch's device outputs against the oracle's outputs on the same operands, in the reference's metric with the
    bounds of its Translate tests: d_sw 3.2e-10 (translate_d_sw.py:19), riem_solver3 5e-6 (overrides/standard.yaml:49-61).
    `skip`: outputs the run did not ask for (DEAD_AFTER_DSW unless --full-outputs).  Returns (ok, {variable: error})."""
    from pace_amd.tile import DSW_ARGS, compare, dsw_live_window, dsw_window, window

    errs, ok = {}, True
    for k in DSW_ARGS:
        if k in ("zh", "delp", "pt", "w", "q_con") and ("riem." + k) in ref:
            pass
        if k == "zh" or k not in ref or k in skip:
            continue
        if k == "w":  # overwritten by riem_solver3 afterwards: compared below
            continue
        # --full-outputs: TranslateD_SW's own windows (the whole storage for the centred fields, translate_d_sw.py:36-65); with the
        # dead work fields skipped the scalars' corner blocks are not specified either (pace_amd/tile.py dsw_live_window)
        W = dsw_live_window(k, n, nz) if skip else dsw_window(k, n, nz)
        scale = float(np.abs(ref[k][W]).max())
        e = compare(ref[k][W], got[k][W], near_zero=1e-12 * max(scale, 1e-300))
        errs["d_sw." + k] = e
        ok = ok and e < 3.2e-10
    for k in ("delz", "zh", "ppe", "pk3", "w"):
        nk = nz if k in ("delz", "w") else nz + 1
        W = window(n, 0, 0, nk)
        r = ref["riem." + k][W]
        scale = float(np.abs(r).max())
        e = compare(r, got[k][W], near_zero=(1e-5 if k in ("ppe", "w") else 1e-9) * scale)
        errs["riem_solver3." + k] = e
        ok = ok and e < 5e-6
    return ok, errs


def dump_outputs(out_dir, b, n, nz, skip=()):
    """--dump-outputs: the fields one step hands back to its caller, as the device left them in the state copy `b`, written as
    out_dir/<field>.npy in the storage type (float64, or float32 for --precision 32).  d_sw's arguments over the windows its
    contract specifies (those of verify_against_oracle; `skip`: the dead work fields a run did not ask for), riem_solver3's outputs
    over the compute domain.  A window of more than DUMP_VALUES_PER_FIELD values is sampled: that many flat indices, drawn by a
    generator seeded with the field's name and sorted, so the same arguments sample the same points in every run and build."""
    import zlib

    import torch

    from pace_amd.tile import DSW_ARGS, dsw_live_window, dsw_window, window

    fields = {}
    for k in DSW_ARGS:
        if k in ("zh", "w") or k in skip:  # (zh, w: riem_solver3 writes them last)
            continue
        fields[k] = dsw_live_window(k, n, nz) if skip else dsw_window(k, n, nz)
    for k in ("delz", "zh", "pe", "ppe", "pk3", "pk", "peln", "w"):
        fields[k] = window(n, 0, 0, nz if k in ("delz", "w") else nz + 1)
    os.makedirs(out_dir, exist_ok=True)
    for k, W in fields.items():
        a = b[k].data[W]
        if a.numel() > DUMP_VALUES_PER_FIELD:
            rng = np.random.default_rng(zlib.crc32(k.encode()))
            idx = np.sort(rng.choice(a.numel(), DUMP_VALUES_PER_FIELD, replace=False))
            a = a.reshape(-1)[torch.as_tensor(idx, device=a.device)]
        np.save(os.path.join(out_dir, k + ".npy"), a.detach().cpu().numpy())


def measure_traffic(kernel_substring, n, nz, precision=64):
    """HBM bytes per launch of the dominant kernel, measured NOW: this script is run twice more as a child under
    `rocprofv3 --kernel-trace --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` (separate passes, as MI355X_MICROARCH.md prescribes; no
    tracing domains beyond the kernel trace) for three steps, and the counters of the kernel are averaged.
    bytes = FETCH_SIZE x 1024 x 2 (the gfx950 correction; calibrated for this code's 8 B-per-lane loads in
    profiles/r02_pmc_calibration.json) + WRITE_SIZE x 1024.  Returns (bytes, detail) or (None, reason)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile

    exe = shutil.which("rocprofv3")
    if exe is None:
        return None, "rocprofv3 not found"
    vals = {}
    tmp = tempfile.mkdtemp(prefix="pace_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp", PACE_BENCH_CACHE=os.environ.get("PACE_BENCH_CACHE", tempfile.gettempdir()))
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(tmp, counter)
            cmd = [exe, "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__), "--steps", "3",
                   "--warmup", "1", "--n", str(n), "--nz", str(nz), "--precision", str(precision), "--full", "--no-cpu-baseline", "--no-traffic",
                   "--no-other-contract"]
            p = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=240)
            if p.returncode != 0:
                return None, f"rocprofv3 --pmc {counter} failed (rc {p.returncode}): {p.stderr[-300:]}"
            got = []
            for f in glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True):
                for r in csv.DictReader(open(f)):
                    if any(k in r["Kernel_Name"] for k in kernel_substring) and r["Counter_Name"] == counter:
                        got.append(float(r["Counter_Value"]))
            if not got:
                return None, f"no {counter} rows for {kernel_substring}"
            vals[counter] = sum(got) / len(got)
    except (subprocess.TimeoutExpired, OSError) as e:
        return None, f"{type(e).__name__}: {e}"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    read_b, write_b = 2.0 * vals["FETCH_SIZE"] * 1024.0, vals["WRITE_SIZE"] * 1024.0
    return read_b + write_b, {"read_bytes": read_b, "write_bytes": write_b, "method": "rocprofv3 --pmc, two child passes of this command"}


def full_loop_diagnosis(lib, dev, n, nz, rank, world, emulate, n_split=4):
    """The whole acoustic loop body (reference: fv3core/pace/fv3core/stencils/dyn_core.py:686-945) on this rank's tile over the run's
    transport: the baroclinic case on the generated cubed sphere at 6 ranks, the synthetic tile on a ring of tiles otherwise (the
    stand-in topology of the timed step).  Returns ms per substep (max over ranks) and, per halo updater, calls per substep and the
    mean HOST time of start (pack launch + grouped send / receive post) and wait (+ unpack launch) on this rank."""
    import collections
    import time

    import torch
    import torch.distributed as dist

    from pace_amd import synthetic
    from pace_amd.fv3core import AcousticDynamicsConfig, DGridShallowWaterLagrangianDynamicsConfig, RiemannConfig
    from pace_amd.fv3core.initialization.dycore_state import DycoreState
    from pace_amd.fv3core.stencils.dyn_core import AcousticDynamics
    from pace_amd.tile import Env
    from pace_amd.util import CubedSphereCommunicator, CubedSpherePartitioner, RingPartitioner, TorchDistComm
    from pace_amd.util import halo as halo_mod

    if world == 6:
        from pace_amd.fv3core.initialization.baroclinic import baroclinic_state_six_tiles
        from pace_amd.util import gridgen

        tiles = gridgen.tiles(n, nz)
        st = baroclinic_state_six_tiles(tiles, n, nz)[rank]
        metrics = {k: v for k, v in tiles[rank].items() if k not in ("ee1", "ee2", "es1", "ew2")}
        arrays = {k: st[k] for k in "u v w delz delp pe pk peln phis uc vc ua va pt qvapor ps".split()}
        timestep = 2 * 225.0 * 48.0 / n / 2.0 / 2.0 * n_split
        part = CubedSpherePartitioner()
    else:
        metrics = synthetic.tile_metrics(n, nz)
        sy = synthetic.acoustic_state(metrics, n, nz)
        arrays = {k: sy[k] for k in "u v w delz delp pt pe pk peln q_con ua va uc vc".split()}
        arrays["phis"] = sy["zs"] * 9.80665
        timestep = float(sy["dt"]) * n_split
        part = RingPartitioner(world)
    env = Env(lib, dev, metrics, n, nz)
    cube = CubedSphereCommunicator(TorchDistComm(), part, device=dev, lib=lib)
    state = DycoreState.init_from_numpy_arrays(arrays, env.qf)
    ac = AcousticDynamicsConfig(n_split=n_split, k_split=1, nord=3, d_con=1.0, rf_fast=True, rf_cutoff=3000.0, tau=10.0, p_fac=0.05,
                                hord_tm=6, delt_max=0.002, d_grid_shallow_water=DGridShallowWaterLagrangianDynamicsConfig(),
                                riemann=RiemannConfig(p_fac=0.05))
    dyn = AcousticDynamics(cube, env.stencil_factory, env.qf, env.grid_data, env.damping, 0, False, False, ac, state.phis, env.q2(), state)
    names = {id(getattr(w, "_updater", None)): k for k, w in vars(dyn._halo_updaters).items() if getattr(w, "_updater", None) is not None}
    acc = collections.defaultdict(lambda: [0.0, 0])
    on = {"v": False}
    saved = {}
    for method in ("start", "wait"):
        orig = getattr(halo_mod.HaloUpdater, method)
        saved[method] = orig

        def timed(self, *a, _orig=orig, _m=method, **kw):
            t0 = time.perf_counter()
            r = _orig(self, *a, **kw)
            if on["v"]:
                e = acc[(names.get(id(self), f"updater {self._tag}"), _m)]
                e[0] += time.perf_counter() - t0
                e[1] += 1
            return r

        setattr(halo_mod.HaloUpdater, method, timed)
    try:
        sync = (lambda: None) if emulate else torch.cuda.synchronize
        dyn(state, timestep=timestep, n_map=1)  # warm-up
        sync()
        dist.barrier()
        on["v"] = True
        t0 = time.perf_counter()
        dyn(state, timestep=timestep, n_map=1)
        sync()
        wall = time.perf_counter() - t0
    finally:
        for method, orig in saved.items():
            setattr(halo_mod.HaloUpdater, method, orig)
    t = torch.tensor([wall], device=dev, dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    finite = bool(torch.isfinite(state.delp.data).all().item())
    per = {}
    for (k, m), (sec, cnt) in sorted(acc.items()):
        per.setdefault(k, {})[m + "_host_us"] = round(1e6 * sec / max(1, cnt), 1)
        per[k]["calls_per_substep"] = round(cnt / n_split, 2)
    host_us = 1e6 * sum(v[0] for v in acc.values()) / n_split
    return {"what": "AcousticDynamics, whole loop body, not part of the timed region", "n_split": n_split,
            "topology": "cubed sphere" if world == 6 else f"ring of {world} tiles (stand-in)",
            "ms_per_substep_max_over_ranks": float(t.item()) * 1e3 / n_split, "halo_host_us_per_substep_this_rank": round(host_us, 1),
            "updaters": per, "finite": finite}


def launch_ranks(args):
    """`python bench.py --gpus N` without a launcher around it: start the N ranks ourselves, as a CHILD process
    (`python -m torch.distributed.run --nproc-per-node N bench.py <the same arguments>`), relay what it prints and return its
    exit code.  Called before anything in this process has touched a GPU (no torch import yet): the parent only waits.  The rank
    count of a run comes from its launcher (fv3core/examples/standalone/runfile/acoustics.py:125-220 takes it from mpirun)."""
    import socket
    import subprocess

    with socket.socket() as s:  # a free rendezvous port on the loopback interface
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stderr.write(f"[bench] --gpus {args.gpus} without WORLD_SIZE: starting the ranks: {' '.join(cmd)}\n")
    sys.stderr.flush()
    return subprocess.call(cmd)


def main():
    args = parse()
    env_world = os.environ.get("WORLD_SIZE")
    if args.gpus is None:  # left at its default: a launcher's world is adopted; only an EXPLICIT mismatch is refused
        args.gpus = int(env_world) if env_world is not None else 1
    if env_world is None and args.gpus > 1:
        sys.exit(launch_ranks(args))
    if env_world is not None and int(env_world) != args.gpus:
        sys.stderr.write(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={env_world} ranks; pass the same "
                         f"number to both (or run `python bench.py --gpus N` and let it start the ranks)\n")
        sys.exit(2)
    import torch

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        import threading

        import torch.distributed as dist

        # A multi-rank run that stops making progress (a peer died, a transport problem) must end by itself: exit with an
        # error after a generous bound instead of occupying the node.
        phase = {"name": "init_process_group", "timer": None}

        def _give_up():
            sys.stderr.write(f"bench.py: rank {rank} spent more than {args.watchdog} s in phase '{phase['name']}', giving up\n")
            sys.stderr.flush()
            os._exit(124)

        def arm(name):
            """The limit applies per phase (rendezvous, preflight, staging, warm-up, timed loop, reduction): it is re-armed
            at every phase boundary, so a long run is not killed for being long, only a phase that stops."""
            if phase["timer"] is not None:
                phase["timer"].cancel()
            phase["name"] = name
            t = threading.Timer(args.watchdog, _give_up)
            t.daemon = True
            t.start()
            phase["timer"] = t

        arm("init_process_group")
        if args.emulate:
            dist.init_process_group(backend="gloo")
        else:
            dist.init_process_group(backend="nccl", device_id=torch.device(f"cuda:{local_rank}"))
            torch.cuda.set_device(local_rank)
        if args.exchange != "off":
            # preflight: the point-to-point pattern of the halo exchange (one grouped send/recv with both ring neighbours)
            # on a few bytes, under a short watchdog of its own -- a transport that cannot do this should fail here, fast
            arm("preflight exchange")
            pre = threading.Timer(min(120.0, args.watchdog), _give_up)
            pre.daemon = True
            pre.start()
            dev0 = torch.device("cpu" if args.emulate else f"cuda:{local_rank}")
            peers = sorted({(rank - 1) % world, (rank + 1) % world})
            sb = {p_: torch.full((8,), float(rank), dtype=torch.float64, device=dev0) for p_ in peers}
            rb = {p_: torch.zeros(8, dtype=torch.float64, device=dev0) for p_ in peers}
            ops = [dist.P2POp(dist.irecv, rb[p_], p_) for p_ in peers] + [dist.P2POp(dist.isend, sb[p_], p_) for p_ in peers]
            for w_ in dist.batch_isend_irecv(ops):
                w_.wait()
            if not args.emulate:
                torch.cuda.synchronize()
            for p_ in peers:
                if float(rb[p_][0].item()) != float(p_):
                    sys.stderr.write(f"bench.py: preflight exchange returned wrong data on rank {rank}\n")
                    os._exit(125)
            pre.cancel()
    else:
        def arm(name):
            return None
    if args.emulate:
        dev = "cpu"
        torch.cuda.synchronize = lambda *a, **k: None  # nothing below touches a GPU in this mode
    else:
        torch.cuda.set_device(local_rank)
        dev = f"cuda:{local_rank}"
    arm("staging")

    from pace_amd.tile import DSW_ARGS, Env

    from pace_amd import _lib, synthetic
    from pace_amd.fv3core import DGridShallowWaterLagrangianDynamicsConfig, RiemannConfig
    from pace_amd.fv3core.stencils.d_sw import DGridShallowWaterLagrangianDynamics
    from pace_amd.fv3core.stencils.riem_solver3 import NonhydrostaticVerticalSolver

    lib = _lib.Library(os.path.join(ROOT, "tests", "emu", "libpace_emu.so")) if args.emulate else _lib.load(args.precision)
    item = float(lib.real_bytes)
    n, nz = args.n, args.nz
    state_kind = "synthetic" if args.emulate else args.state
    state_note = ""
    if state_kind == "baroclinic":
        import tempfile

        from pace_amd.tile import baroclinic_substep_inputs

        try:
            metrics, s, sc = baroclinic_substep_inputs(lib, dev, n, nz, rank % 6,
                                                       cache_dir=os.environ.get("PACE_BENCH_CACHE", tempfile.gettempdir()))
            s["dt"] = sc["dt"]
            if lib.real_bytes == 4:  # the reference's fill values of unused entries (1e30 ... 1e40) do not fit float32
                big = float(np.finfo(np.float32).max)
                s = {k: (np.clip(v, -big, big) if isinstance(v, np.ndarray) else v) for k, v in s.items()}
        except Exception as e:  # noqa: BLE001 -- the measurement must not be lost to its set-up: say so and use the synthetic state
            state_kind = "synthetic"
            state_note = f" (the baroclinic set-up failed: {type(e).__name__}: {str(e)[:160]})"
            sys.stderr.write(f"[bench] baroclinic state set-up failed, falling back to the synthetic state: {e!r}\n")
        torch.cuda.empty_cache()
    if state_kind != "baroclinic":
        metrics = synthetic.tile_metrics(n, nz)
        s = synthetic.acoustic_state(metrics, n, nz)
    env = Env(lib, dev, metrics, n, nz)
    col = column_namelist(nz, env.qf)
    # as AcousticDynamics constructs it; under --graph the in-place path (a captured graph is bound to the buffers it was captured
    # on, and the swap rebinds them at every call)
    dsw = DGridShallowWaterLagrangianDynamics(env.stencil_factory, env.qf, env.grid_data, env.damping, col, nested=False,
                                              stretched_grid=False, config=DGridShallowWaterLagrangianDynamicsConfig(),
                                              swap_scalar_storage=args.graph != "on")
    riem = NonhydrostaticVerticalSolver(env.stencil_factory, env.qf, RiemannConfig())
    ptop = float(metrics["ptop"])
    dt = float(s["dt"])

    RIEM_ONLY = ("cappa", "delz", "pe", "ppe", "pk3", "pk", "peln")
    base = {k: env.q3(s[k]) for k in list(DSW_ARGS) + list(RIEM_ONLY)}
    zs, ws = env.q2(s["zs"]), env.q2(s["ws"])
    nbatch = args.steps + args.warmup

    def clone_state():
        out = {}
        for k, q in base.items():
            c = env.q3()
            c._base.copy_(q._base)
            out[k] = c
        return out

    # at most STATE_POOL_BYTES of copies: step i runs on copy i % len(batches); a run with more steps than copies times them in
    # rounds of len(batches) steps and gives the copies their pristine state back between two rounds (outside the timed region)
    batches = [clone_state()]
    copy_bytes = sum(q._base.numel() * q._base.element_size() for q in batches[0].values())
    batches += [clone_state() for _ in range(min(nbatch, max(1, STATE_POOL_BYTES // copy_bytes)) - 1)]
    torch.cuda.synchronize()

    # The halo exchange of the acoustic loop stays inside the measured step whenever there is more than one rank: on the
    # cubed-sphere topology at 6 ranks, and at rank counts that cannot form a cube (the driver's 2 / 4 / 8) on a periodic
    # ring of tiles with the same four edge strips per tile (same message sizes and pack / exchange / unpack path; a
    # stand-in topology, named as such in the output).
    exchange, topology = None, "none"
    if world > 1 and args.exchange != "off":
        from pace_amd.util import CubedSphereCommunicator, CubedSpherePartitioner, RingPartitioner, TorchDistComm
        from pace_amd.util.constants import X_DIM, Y_DIM, Z_DIM

        part = CubedSpherePartitioner() if world == 6 else RingPartitioner(world)
        cube = CubedSphereCommunicator(TorchDistComm(), part, device=dev, lib=lib)
        exchange = cube.get_scalar_halo_updater([env.qf.get_quantity_halo_spec([X_DIM, Y_DIM, Z_DIM])] * 3)
        from pace_amd.util.constants import X_INTERFACE_DIM, Y_INTERFACE_DIM

        # the exchange in front of d_sw (dyn_core.py:817-820): the C-grid winds, as a vector update
        exchange_winds = cube.get_vector_halo_updater([env.qf.get_quantity_halo_spec([X_INTERFACE_DIM, Y_DIM, Z_DIM])],
                                                      [env.qf.get_quantity_halo_spec([X_DIM, Y_INTERFACE_DIM, Z_DIM])])
        topology = "uc,vc before and delp,pt,q_con after d_sw over RCCL (cubed sphere)" if world == 6 else \
            f"uc,vc before and delp,pt,q_con after d_sw over RCCL (ring of {world} tiles: stand-in topology, cubed-sphere strip sizes)"

    overlap = args.overlap == "on" or (args.overlap == "auto" and world > 1)
    skip_dead = not args.full_outputs

    def step(b):
        args = [b[k] for k in DSW_ARGS]
        if exchange is not None:
            # the uc / vc strips travel while the interior of d_sw's flux preparation runs (it reads no halo value of them)
            exchange_winds.start([b["uc"]], [b["vc"]])
            dsw.start_flux_preparation(*args, dt)
            exchange_winds.wait()
        # the wind half of d_sw runs on a side stream, concurrently with the (latency-bound) column solver
        # (a substep that is not the last of its remapping step, 7 of 8 at C192: the divergence damping's work fields delpc, divgd,
        # uc, vc are dead after it -- SURVEY.md 8(d) counts no bytes for them --, AcousticDynamics does not ask for them)
        dsw(*args, dt, overlap_winds=overlap, skip_dead_outputs=skip_dead)
        if exchange is not None:
            # delp / pt / q_con travel while the column solver runs: it works on the compute domain's columns only (the halos are
            # needed by what follows it -- pk3_halo, nh_p_grad, the next substep's c_sw; dyn_core.py:854 updates them right here)
            exchange.start([b["delp"], b["pt"], b["q_con"]])
        riem(False, dt, b["cappa"], ptop, zs, ws, b["delz"], b["q_con"], b["delp"], b["pt"], b["zh"], b["pe"], b["ppe"], b["pk3"],
             b["pk"], b["peln"], b["w"])
        if exchange is not None:
            exchange.wait()
        dsw.join()

    def barrier():
        if world > 1:
            import torch.distributed as dist

            dist.barrier()
        torch.cuda.synchronize()

    use_graph = args.graph == "on"
    stepped = set()  # copies that are no longer pristine

    def refresh(slots):
        again = [j for j in slots if j in stepped]
        for j in again:
            for k, q in base.items():
                batches[j][k]._base.copy_(q._base)
            stepped.discard(j)
        if again:
            torch.cuda.synchronize()

    arm("warm-up")
    for i in range(args.warmup):
        refresh([i % len(batches)])
        step(batches[i % len(batches)])
        stepped.add(i % len(batches))
    timed = [i % len(batches) for i in range(args.warmup, nbatch)]  # the state copy of every timed step
    graphs = None
    if use_graph:
        # one graph per state copy (a graph is bound to the buffers it was captured on); both streams of the step are
        # captured through the fork/join events.  Capturing launches nothing, so the copies stay pristine.
        torch.cuda.synchronize()
        graphs = {}
        for j in timed:
            if j not in graphs:
                graphs[j] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[j]):
                    step(batches[j])
    arm("timed loop")
    elapsed = 0.0
    for r in range(0, len(timed), len(batches)):  # (one round unless the steps outnumber the copies)
        rnd = timed[r:r + len(batches)]
        refresh(rnd)
        barrier()
        t0 = time.perf_counter()
        if graphs is not None:
            for j in rnd:
                graphs[j].replay()
        else:
            for j in rnd:
                step(batches[j])
        barrier()
        elapsed += time.perf_counter() - t0
        stepped.update(rnd)
    last = batches[timed[-1]]  # what the last timed step computed
    arm("reduction + report")
    if world > 1:
        import torch.distributed as dist

        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    ms_per_step = 1e3 * elapsed / args.steps
    if args.dump_outputs and rank == 0:  # before anything below steps the copies again
        dump_outputs(args.dump_outputs, last, n, nz, skip=DEAD_AFTER_DSW if skip_dead else ())
    # Multi-rank diagnosis (--full; NOT part of the timed region): the same step again with the device synchronised after every
    # phase, max over ranks per phase -- where a 6-GPU step spends its time (pack + post, interior compute under the exchange, wait +
    # unpack, the rest of d_sw, the scalar exchange, the column solver).  The phases overlap in the timed loop, so they sum to
    # more than ms_per_step.
    phase_ms = None
    if exchange is not None and args.full:
        arm("phase diagnosis")
        names = ["uc_vc_start(pack+post)", "flux_prep_interior", "uc_vc_wait(+unpack)", "d_sw_rest", "delp_pt_qcon_start(pack+post)",
                 "riem_solver3", "delp_pt_qcon_wait(+unpack)"]
        acc = np.zeros(len(names))
        nd = min(3, len(batches))
        for i in range(nd):
            b = batches[i]
            a_ = [b[k] for k in DSW_ARGS]
            marks = []

            def mark():
                torch.cuda.synchronize()
                marks.append(time.perf_counter())

            mark()
            exchange_winds.start([b["uc"]], [b["vc"]]); mark()
            dsw.start_flux_preparation(*a_, dt); mark()
            exchange_winds.wait(); mark()
            dsw(*a_, dt, overlap_winds=True); dsw.join(); mark()
            exchange.start([b["delp"], b["pt"], b["q_con"]]); mark()
            riem(False, dt, b["cappa"], ptop, zs, ws, b["delz"], b["q_con"], b["delp"], b["pt"], b["zh"], b["pe"], b["ppe"], b["pk3"],
                 b["pk"], b["peln"], b["w"]); mark()
            exchange.wait(); mark()
            acc += np.diff(marks)
        import torch.distributed as dist

        t = torch.tensor(acc / nd * 1e3, device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        phase_ms = {k: float(v) for k, v in zip(names, t.tolist())}
    # The whole loop body over the run's transport (--full-loop; NOT part of the timed region, and never fatal): AcousticDynamics on
    # this rank's tile of the baroclinic case, four substeps, every HaloUpdater.start / wait timed on the host.
    full_loop = None
    if world > 1 and args.full_loop:
        arm("full loop diagnosis")
        try:
            full_loop = full_loop_diagnosis(lib, dev, n, nz, rank, world, args.emulate)
        except Exception as e:  # noqa: BLE001 -- a diagnosis must not cost the measured line
            full_loop = {"error": f"{type(e).__name__}: {str(e)[:300]}"}
    cells = n * n * nz
    value = world * cells * args.steps / elapsed
    # the last TIMED batch's fields as the device left them (taken now: the roofline loop below accumulates into mfx / mfy)
    got_last = None
    if args.full and rank == 0 and not args.no_cpu_baseline and world == 1:
        torch.cuda.synchronize()
        got_last = {k: last[k].numpy().astype(np.float64) for k in list(DSW_ARGS) + ["delz", "ppe", "pk3"]}

    # The OTHER output contract of d_sw, timed right here in the same way (not part of `value`): the line quotes the substep that
    # skips the divergence damping's dead work fields (7 of 8 substeps of a remapping step); the reference's full contract --
    # every argument as TranslateD_SW compares it, the halo of the work fields and the scalars' corner blocks included -- is the
    # eighth.  (--full-outputs swaps the two.)  The state copies have been stepped once already: a second step of the same
    # arithmetic, same bytes.
    other_contract = None
    if args.full and world == 1 and not use_graph and not args.no_other_contract:
        nb = min(10, len(batches))

        def step_other(b):
            dsw(*[b[k] for k in DSW_ARGS], dt, overlap_winds=overlap, skip_dead_outputs=not skip_dead)
            riem(False, dt, b["cappa"], ptop, zs, ws, b["delz"], b["q_con"], b["delp"], b["pt"], b["zh"], b["pe"], b["ppe"], b["pk3"],
                 b["pk"], b["peln"], b["w"])
            dsw.join()

        for i in range(min(3, nb)):
            step_other(batches[i])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for i in range(nb):
            step_other(batches[-1 - i])
        torch.cuda.synchronize()
        other_contract = {"ms_per_step": 1e3 * (time.perf_counter() - t1) / nb, "steps": nb,
                          "d_sw_outputs": "dead work fields skipped" if args.full_outputs else
                          "the reference's full contract (flags = 0): all 21 arguments over TranslateD_SW's windows"}

    # The dominant kernel OF THE STEP, timed live with events on the launch stream, alone, on HBM-resident operands that change
    # from launch to launch.  Production tilings: k_fvt_scalars -- the scalar phase of d_sw (delp, w, q_con, pt transported, damped
    # and updated in one kernel; pace_amd/csrc/fvt_core.h), launched exactly as the step launches it (pace_d_sw_phases, mask 2,
    # separate outputs).  Other tilings: the single-scalar transport kernel k_fvtp2d<6, 2, 1> through pace_fvtp2d_update (three of
    # the step's launches are instances of it).
    roof = None
    if args.full and rank == 0 and not args.emulate:
        import ctypes as C

        from pace_amd.fv3core.stencils._common import dptr, host_column

        geom = dsw._geom
        fused = bool(getattr(dsw, "_pingpong", False))
        winds_fused = fused and bool(getattr(dsw, "_wind_outputs", False))
        if fused:
            roof_names = ("k_fvt_scalars",)
            if winds_fused:
                roof_kernel = ("k_fvt_scalars<6> with the winds (d_sw: delp, w, q_con, pt transported and updated, the vorticity transport, "
                               "the wind update and the dissipative heating in one kernel)")
                # distinct 3-D fields once per direction: delp, w, q_con, pt, crx, cry, xfx, yfx, mfx, mfy,
                # relative vorticity, u, v, kinetic energy, damped vorticity, heat_source in; delp, w, q_con, pt, mfx, mfy,
                # diss_est, u, v, heat_source out
                algo_fields = 26
            else:
                roof_kernel = "k_fvt_scalars<6> (d_sw scalar phase: delp, w, q_con, pt in one kernel)"
                # ... delp, w, q_con, pt, crx, cry, xfx, yfx, mfx, mfy in; delp, w, q_con, pt, mfx, mfy, diss_est, w's heating term out
                algo_fields = 18
            spare_sets = [[env.q3() for _ in range(6)] for _ in range(2)]

            def kernel(r):
                b = batches[r % len(batches)]  # a different state copy every launch: operands come from HBM, as inside a step
                sp = spare_sets[r % 2]
                c_ = dsw._cfg
                c_.delp_out, c_.pt_out, c_.w_out, c_.q_con_out = (dptr(x) for x in sp[:4])
                c_.u_out, c_.v_out = (dptr(sp[4]), dptr(sp[5])) if winds_fused else (None, None)
                # (256: the fused kernel alone, on the kinetic energy / vorticity / damped vorticity the last step left in the workspace)
                lib.call("pace_d_sw_phases", 256 if winds_fused else 2, C.byref(geom), *dsw._args([b[k] for k in DSW_ARGS], dt), dsw.stream())
        else:
            roof_kernel = "k_fvtp2d<6, 2, 1> (transport + damping + flux-form update of one scalar)"
            roof_names = ("k_fvtp2d<6, 2, 1", "k_fvtp2dILi6ELi2ELi1E", "k_fvt<6, 2, 1", "k_fvtILi6ELi2ELi1E")
            algo_fields = TRANSPORT_FIELDS
            da_min = env.damping.da_min
            nord_t, damp_t = host_column(col["nord_t"], nz), host_column(col["damp_t"], nz)
            kdev = torch.as_tensor(np.concatenate([(damp_t * da_min) ** (nord_t + 1), nord_t]), dtype=env.qf.real, device=dev)
            out = env.q3()

            def kernel(r):
                b = batches[r % len(batches)]
                lib.call("pace_fvtp2d_update", C.byref(geom), C.byref(env.grid_data.c_struct()), b["pt"].ptr, b["crx"].ptr, b["cry"].ptr,
                         b["xfx"].ptr, b["yfx"].ptr, b["mfx"].ptr, b["mfy"].ptr, b["delp"].ptr, kdev.data_ptr(),
                         kdev.data_ptr() + lib.real_bytes * nz, int(nord_t.max()), out.ptr, 6, nz, dsw.stream())

        reps = max(10, args.steps)
        for r in range(3):
            kernel(r)
        # a pair of events around EVERY launch, the median of them: one stall of the host thread between two launches (a shared
        # host: 50 ms were seen once) would otherwise be averaged into every launch of the batch
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for r, (e0, e1) in enumerate(evs):
            e0.record()
            kernel(3 + r)
            e1.record()
        torch.cuda.synchronize()
        per_launch = sorted(e0.elapsed_time(e1) * 1e-3 for e0, e1 in evs)
        t_kernel = float(np.median(per_launch))
        algo = algo_fields * item * n * n * nz
        # HBM bytes per launch: measured live by two child passes under rocprofv3 --pmc (see measure_traffic), null otherwise
        traffic, traffic_detail = (None, "skipped (--no-traffic)")
        if not args.no_traffic and world == 1:
            torch.cuda.synchronize()
            traffic, traffic_detail = measure_traffic(roof_names, n, nz, args.precision)
        # what this memory system sustains on plain streams, next to the spec peak the fractions are priced against (SURVEY.md
        # section 8d): this repo's own read / write / copy kernels at 16 bytes per lane over 1 GiB buffers (tools/ubench/streams.hip,
        # built by __graft_entry__.build() into build/ubench_streams and run here as a child process), and torch's copy_
        streams = None
        try:
            import subprocess

            exe = os.path.join(ROOT, "build", "ubench_streams")
            # (not under --no-traffic: that is what the profiled children of measure_traffic / collect_*.sh run with, and a
            # child process would inherit the profiler's preload and stream 1 GiB buffers under counter collection)
            if os.path.exists(exe) and not args.no_traffic:
                torch.cuda.synchronize()
                txt = subprocess.run([exe], capture_output=True, text=True, timeout=120).stdout
                rows = {ln[:28].strip(): ln[28:].split() for ln in txt.splitlines() if ln[:5] in ("read ", "write", "copy ")}
                streams = {"read_16B_per_lane": 1e3 * float(rows["read  16 B/lane"][0]), "write_16B_per_lane": 1e3 * float(rows["write 16 B/lane"][0]),
                           "copy_16B_per_lane": 1e3 * float(rows["copy  16 B/lane"][0]), "read_8B_per_lane": 1e3 * float(rows["read   8 B/lane"][0]),
                           "copy_8B_per_lane": 1e3 * float(rows["copy   8 B/lane"][0]), "unit": "GB/s, plain grid, median of 5"}
        except Exception as e:  # noqa: BLE001
            sys.stderr.write(f"[bench] stream micro-benchmark failed: {e!r}\n")
        try:
            if args.no_traffic:
                raise RuntimeError("skipped")
            src = torch.empty(1 << 27, dtype=torch.float64, device=dev).normal_()
            dst = torch.empty_like(src)
            for _ in range(2):
                dst.copy_(src)
            c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            c0.record()
            for _ in range(10):
                dst.copy_(src)
            c1.record()
            torch.cuda.synchronize()
            torch_copy_gbs = 10 * 2 * src.numel() * 8 / (c0.elapsed_time(c1) * 1e-3) / 1e9
            del src, dst
        except Exception:  # noqa: BLE001
            torch_copy_gbs = None
        copy_gbs = streams["copy_16B_per_lane"] if streams else torch_copy_gbs
        roof = {"kernel": roof_kernel, "bound": "hbm", "achieved": algo / t_kernel / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "measured_copy_GBs": copy_gbs, "measured_streams": streams, "torch_copy_GBs": torch_copy_gbs,
                "frac": algo / t_kernel / 1e9 / HBM_PEAK_GBS, "traffic": traffic, "traffic_detail": traffic_detail,
                "us_per_launch": t_kernel * 1e6, "us_per_launch_min_max": [per_launch[0] * 1e6, per_launch[-1] * 1e6],
                "launches_timed": reps, "algorithmic_bytes_per_launch": algo, "algorithmic_fields": algo_fields,
                "where_in_the_step": ("the step's longest launch (more than half of it); timed here alone, exactly as the step launches it "
                                      "(pace_d_sw_phases 256: on the kinetic energy / vorticities the last step left in the workspace)" if winds_fused else
                                      "the step's longest launch; timed here exactly as the step launches it, alone" if fused else
                                      "three of the step's launches are instances of this kernel; timed here alone, one scalar"),
                "limited_by": ("its instruction stream and the waits in it: five transports + the wind update per tile are ~5 400 instructions "
                               "per wave (4 077 vector, 45 % of them fp64; no FMA contraction: the results are bit-identical to the numpy "
                               "oracle) on sixteen waves per CU (128 registers, 77.5 KB of LDS per workgroup); hardware counters "
                               "(profiles/r06_sq_counters.json): vector issue alone is ~200 us of the kernel's ~390, a wave waits on its "
                               "memory / LDS counters 54 % of its cycles (31 barriers per tile, two workgroups per CU to interleave); its L2 "
                               "misses (~1.9 x the algorithmic bytes: halo rows of neighbouring tiles and the operands of the five passes) "
                               "move at 2.9 TB/s -- DESIGN.md section 4" if fused else
                               "the bytes it really moves (L2 misses ~1.5 x algorithmic at ~3.5 TB/s) -- DESIGN.md section 4")}

    if rank == 0:
        line = {
            "metric": f"cell-updates/s per acoustic substep (d_sw+riem3), C{n}x{nz}L; % HBM roofline",
            "value": value,
            "unit": "cell-updates/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f64" if lib.real_bytes == 8 else "f32 storage, f64 arithmetic in registers",
            "data": ("synthetic (CPU EMULATION DRY RUN: no performance meaning)" if args.emulate else
                     "synthetic: Jablonowski-Williamson baroclinic case on the generated cubed sphere, this rank's tile at the D_SW-In "
                     "checkpoint of the second acoustic substep" if state_kind == "baroclinic" else "synthetic (pace_amd/synthetic.py)" + state_note),
            "config": {"workload": f"C{n}x{nz}L one tile per GPU, d_sw + riem_solver3 acoustic substep, " + ("fp64" if lib.real_bytes == 8 else "fp32 fields"),
                       "cells_per_tile": cells, "tiles": world, "parallelism": f"tile-per-gpu x{world}",
                       "halo_exchange": topology,
                       "launch": "hip graph replay" if use_graph else "eager",
                       "streams": "wind half of d_sw on a side stream" if overlap else "one stream",
                       "d_sw_outputs": ("all 21 arguments as the reference leaves them (the last substep of a remapping step)" if args.full_outputs
                                        else "every argument but the divergence damping's work fields delpc, divgd, uc, vc, which c_sw recomputes before "
                                             "anything reads them (a substep that is not the last of its remapping step: 7 of 8 at C192; "
                                             "--full-outputs measures the other)")},
            "step_hbm_frac": BYTES_PER_CELL_UPDATE * (item / 8.0) * cells / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBS,
            "roofline": roof,
            "other_contract": other_contract,
        }
        if world > 1:
            import torch.distributed as dist

            # what the collective library saw (RCCL is reached through torch.distributed's "nccl" backend)
            line["comm"] = {"backend": dist.get_backend(), "world_size": dist.get_world_size(),
                            "exchanges_per_step": {"uc,vc (vector, before d_sw)": exchange_winds.message_bytes(),
                                                   "delp,pt,q_con (after d_sw, under riem_solver3)": exchange.message_bytes()},
                            "exchanges_note": "bytes of the one message per neighbour and update, rank 0; AcousticDynamics has seven such "
                                              "groups per substep (dyn_core.py:720-942), this step the two that surround d_sw",
                            "phase_ms_max_over_ranks_synchronised": phase_ms,
                            "phase_note": "the step once more with the device synchronised after every phase (diagnosis, not the timed "
                                          "region): what overlaps in the timed loop -- the interior of the flux preparation with the uc / vc "
                                          "exchange, riem_solver3 with the delp / pt / q_con exchange -- is serial here, so "
                                          "sum(phases) - ms_per_step is what the overlap hides"}
            if full_loop is not None:
                line["comm"]["full_loop"] = full_loop
        if args.full and not args.no_cpu_baseline and world == 1:  # rank 0 at N = 1 only
            try:
                rec, ref = cpu_baseline(n, nz, metrics, s, dt, ptop)
            except Exception as e:  # noqa: BLE001 -- the measured line must not be lost to its CPU leg: say so
                sys.stderr.write(f"[bench] cpu_baseline failed: {e!r}\n")
                line["cpu_baseline"] = {"value": None, "unit": "cell-updates/s", "cores": 0, "kind": "port",
                                        "sample": f"failed: {type(e).__name__}: {str(e)[:200]}"}
                line["verified"] = None
                print(json.dumps(line))
                return
            line["cpu_baseline"] = rec
            # the last TIMED batch's fields as the device left them, against the oracle on the same operands
            skipped = () if args.full_outputs else DEAD_AFTER_DSW
            ok, errs = verify_against_oracle(got_last, ref, n, nz, skip=skipped)
            line["verified"] = bool(ok)
            line["verified_detail"] = {"what": "the last timed batch's outputs vs the numpy oracle on the same operands: d_sw at 3.2e-10 "
                                               "(translate_d_sw.py:19), riem_solver3 at 5e-6 (overrides/standard.yaml:49-61)"
                                               + (f"; not asked for and not compared: {', '.join(skipped)} (dead after d_sw)" if skipped else ""),
                                       "max_error": max(errs.values()), "worst": max(errs, key=errs.get), "errors": errs}
        print(json.dumps(line))
    if world > 1:
        import torch.distributed as dist

        dist.destroy_process_group()


if __name__ == "__main__":
    main()
