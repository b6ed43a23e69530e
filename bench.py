#!/usr/bin/env python3
"""bench.py — BASELINE.json metric on MI355X: "Mphotons/s traced +
Mgather-samples/s, Cornell box 1M photons @1080p" (configs[1] = C2).

A step is one photon-mapping pass over the C2 workload from the initial PPM
state (the reference's default single pass), inputs (scene, BVH, eye-pass
records) already resident in HBM:
    reset PPM state (deferred: the gather starts from the initial state) ->
    emit + trace 262,144 paths (1,048,576 photon slots) per GPU, counting the
    bucket cells of the deposits -> scan + fill the photon buckets -> range
    query + PPM update over the 2,073,600 gather points (+ the reduce-scatter
    of (M, L) and all-gather of radii for N > 1).
`value` = emitted photon paths over all ranks / step time (whole job,
Mphotons/s); `mgather_samples_per_s` = gather points / step time.

Single GPU: `python bench.py`. N GPUs (one process per GPU): either
`python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N`
or plain `python bench.py --gpus N`, which starts that launcher itself as a
child process (before torch is imported) and relays rank 0's JSON line
(weak scaling: the config's paths per GPU). At N > 1 the line also carries the
other exchange (`alt_exchange`: the slot all-gather when the headline ran the
reduce exchange), timed the same way after the headline steps. Strong scaling: `--total-paths T`
splits T paths per pass over the N ranks (`--config c4 --total-paths 4194304`
is BASELINE C4's 16,777,216 photon slots at any N) and reports "scaling":
"strong". At N > 1 `stages_ms.exchange` is the per-pass exchange (RCCL
all-reduce + reduce-scatter, or the slot all-gather) timed to completion in
the stage-timed passes after the timed region.

A plain run sets up, warms up, times the steps and prints the headline line.
`--full` adds everything else the line can carry, each from runs of its own
after the timed steps: the per-stage split (`stages_ms`, `kernel_rates`), the
counting launches behind `roofline` / `trace_roofline`, the exchange timing
and the other exchange at N > 1, and the CPU baseline.

`--dump-outputs DIR` writes what the last timed step computed, as float32
`DIR/<name>.npy`: `radiance` (PassRunner.final_gather over all records, record
order) and, on one GPU, the PPM state the pass left in the records (`flux`,
`radius2`, `photon_count`). Above 60 MB in all, the per-record arrays keep the
same fixed, seeded sample of records, listed in `record_index` (float64).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "cuda-raytrace_amd"))

METRIC = "Mphotons/s traced + Mgather-samples/s, Cornell box 1M photons @1080p"
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
VALU_FP32_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: peak FP32 (vector)


# BASELINE.json configs: scene, resolution, photon paths
# per GPU per pass (slots = 4 x paths), progressive passes
CONFIGS = {
    "c1": dict(scene="cornell", W=256, H=256, paths=25_000, progressive=False,
               desc="C1: Cornell box, 100,000 photon slots (25,000 paths), 256x256 gather points"),
    "c2": dict(scene="cornell", W=1920, H=1080, paths=262_144, progressive=False,
               desc="C2: Cornell box, 1,048,576 photon slots (262,144 paths) per GPU, 1920x1080 gather points"),
    "c3": dict(scene="soup", W=1920, H=1080, paths=1_048_576, progressive=False,
               desc="C3: Cornell enclosure + 1M-triangle soup, 4,194,304 photon slots (1,048,576 paths) per GPU, "
                    "1920x1080 gather points"),
    "c4": dict(scene="cornell", W=3840, H=2160, paths=524_288, progressive=False,
               desc="C4 per-GPU share: Cornell box, 2,097,152 photon slots (524,288 paths) per GPU, 3840x2160 "
                    "gather points (the 8-GPU config's photon shard; every rank gathers the whole 4K view)"),
    "c5": dict(scene="caustic", W=1920, H=1080, paths=1_048_576, progressive=True,
               desc="C5: caustic scene (Cornell + glass and mirror spheres), 4,194,304 photon slots (1,048,576 "
                    "paths) per GPU per progressive pass, 1920x1080 gather points; a step = one progressive pass"),
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="c2", choices=sorted(CONFIGS))
    ap.add_argument("--structure", default="grid", choices=["grid", "kd"])
    ap.add_argument("--exchange", default="reduce", choices=["reduce", "allgather"])
    ap.add_argument("--paths", type=int, default=None, help="photon paths per GPU per pass (default: the config's)")
    ap.add_argument("--total-paths", type=int, default=None,
                    help="strong scaling: photon paths per pass over ALL ranks, split evenly (e.g. --config c4 "
                         "--total-paths 4194304: BASELINE C4's 16,777,216 slots at any N); reported as scaling "
                         "'strong'. Default: weak scaling, --paths per GPU")
    ap.add_argument("--estimator", default="ppm", choices=["ppm", "knn"],
                    help="ppm: the reference's fixed-radius PPM gather (headline); knn: pbrt-v2 LPhoton kNN")
    ap.add_argument("--knn-k", type=int, default=50, help="kNN photons per lookup (pbrt 'nused')")
    ap.add_argument("--radius2", type=float, default=None,
                    help="initial / maximum search radius^2 (default: 4 for ppm = raytracing.cu:123, 100 for knn)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-threads", type=int, default=None,
                    help="oracle threads (default: this process's CPU share: OMP_NUM_THREADS, else its affinity set)")
    ap.add_argument("--no-census", action="store_true")
    ap.add_argument("--gather-event-every", type=int, default=4,
                    help="HIP events on the gather of every N-th timed step (the roofline's launch time; 1 = every step)")
    ap.add_argument("--no-alt-exchange", action="store_true",
                    help="N > 1: skip timing the other exchange (reduce <-> allgather) after the headline steps")
    ap.add_argument("--pipeline", type=int, default=int(os.environ.get("PM_BENCH_PIPELINE", "0")),
                    help="1: each timed pass's gather overlaps the next pass's trace (second stream; one GPU)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run what the headline figure does not need: per-stage split "
                         "passes, counting launches (roofline), exchange timing and the other exchange (N > 1), "
                         "the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the arrays the last timed step computed as DIR/<name>.npy (float32; a fixed, seeded "
                         "sample of the records above 60 MB in all)")
    return ap.parse_args()


def build_scene(cfg):
    from pmrender import scenes
    c = CONFIGS[cfg]
    if c["scene"] == "cornell":
        return scenes.cornell_box(c["W"], c["H"])
    if c["scene"] == "soup":
        return scenes.triangle_soup(1_000_000, c["W"], c["H"])
    return scenes.caustic_scene(c["W"], c["H"])


def kernel_src_sha():
    """Hash of the HIP sources and their build flags: a committed PMC profile is this build's only if it matches."""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "cuda-raytrace_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h", ".cpp")):
            with open(os.path.join(csrc, f), "rb") as fh:
                h.update(f.encode() + fh.read())
    with open(os.path.join(ROOT, "cuda-raytrace_amd", "Makefile"), "rb") as fh:  # compile flags
        h.update(b"Makefile" + fh.read())
    return h.hexdigest()[:16]


def load_pmc_traffic(kernel_prefix, config, field="hbm_bytes_per_launch"):
    """Per-launch HBM bytes (rocprofv3 FETCH_SIZE/WRITE_SIZE passes, gfx950
    FETCH x2 correction; tools/pmc_traffic.py) of this kernel from the
    committed profile — only if it was measured on these exact HIP sources
    and this config; else (None, reason)."""
    sha = kernel_src_sha()
    path, d = None, None
    for rnd in ("r06", "r05", "r04", "r03", "r02"):      # the newest committed profile of these sources
        cand = os.path.join(ROOT, "profiles", rnd, "pmc_traffic_%s.json" % config)
        if os.path.exists(cand):
            with open(cand) as f:
                dd = json.load(f)
            if path is None:
                path, d = cand, dd
            if dd.get("kernel_src_sha") == sha:
                path, d = cand, dd
                break
    if path is None:
        return None, "no committed PMC profile for this config"
    if d.get("kernel_src_sha") != sha:
        return None, "committed PMC profile is from other HIP sources (%s)" % d.get("kernel_src_sha")
    k = d.get("kernels", {}).get(kernel_prefix)
    if not k:
        return None, "kernel not in the committed PMC profile"
    return k.get(field), os.path.relpath(path, ROOT)


def cpu_model():
    try:
        out = subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout
        for line in out.splitlines():
            if line.startswith("Model name:"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return None


def default_cpu_threads():
    """This process's CPU share: OMP_NUM_THREADS (16 per GPU on the GPU box,
    where os.cpu_count() reports the whole machine), else the affinity set."""
    env = os.environ.get("OMP_NUM_THREADS")
    if env and env.isdigit() and int(env) > 0:
        return int(env)
    try:
        return len(os.sched_getaffinity(0))
    except Exception:
        return os.cpu_count() or 1


def cpu_baseline(scene, params, threads, cfg):
    """Oracle (CPU restatement of the reference, test infrastructure) timed on
    this host: whole passes of the same workload (trace the config's paths +
    pbrt kd-tree build + range query/PPM update over all gather points)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle
    orc = scene.load_into(oracle.Oracle(nthreads=threads))
    recs0 = orc.eye_pass(params)                     # setup (the GPU eye pass is outside the step too)
    # repeat whole passes (fresh PPM state each, like the GPU step) until the
    # sample holds >= 12 s of CPU work (wall x threads), at most 20 passes
    passes, dt, nodes = 0, 0.0, []
    while passes < 20 and (passes == 0 or dt * threads < 12.0):
        recs = recs0.copy()
        t0 = time.perf_counter()
        slots = orc.trace_photons(params, passes, 0, params.paths_per_pass)
        nodes = orc.build_kdtree(slots)
        orc.gather(nodes, recs, params)
        dt += time.perf_counter() - t0
        passes += 1
    return {
        "value": round(params.paths_per_pass * passes / dt / 1e6, 4),
        "unit": "Mphotons/s",
        "cores": threads,
        "kind": "port",
        "host_cpus": os.cpu_count(),
        "threads_note": "the oracle runs std::thread over this process's CPU share (OMP_NUM_THREADS: 16 per GPU "
                        "on the MI355X box), not hardware_concurrency(): the box's other CPUs belong to the other "
                        "GPUs' jobs, so host_cpus threads would not be a clean measurement",
        "cpu_model": cpu_model(),
        "sample": f"{passes} full {cfg.upper()} passes on the host with {threads} threads (this process's CPU share; "
                  f"the host has {os.cpu_count()}) — each: trace {params.paths_per_pass} paths + pbrt kd-tree "
                  f"build over ~{len(nodes)} photons + gather/PPM over {len(recs0)} records; {dt:.2f} s wall, "
                  f"{dt * threads:.1f} thread-s",
        "mgather_samples_per_s": round(len(recs0) * passes / dt / 1e6, 4),
    }


DUMP_BUDGET_BYTES = 60_000_000
DUMP_SEED = 20240607


def dump_outputs(path, arrays):
    """Write per-record arrays (all of one length) as path/<name>.npy, float32.
    Over DUMP_BUDGET_BYTES in all, every array keeps the same seeded sample of
    records, whose indices go to record_index.npy (float64: exact below 2^53)."""
    os.makedirs(path, exist_ok=True)
    n = len(next(iter(arrays.values())))
    row_bytes = sum(a[:1].astype(np.float32).nbytes for a in arrays.values())
    keep = None
    if n * row_bytes > DUMP_BUDGET_BYTES:
        m = DUMP_BUDGET_BYTES // (row_bytes + 8)
        keep = np.sort(np.random.default_rng(DUMP_SEED).choice(n, size=m, replace=False))
        np.save(os.path.join(path, "record_index.npy"), keep.astype(np.float64))
    for name, a in arrays.items():
        a = a if keep is None else a[keep]
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a, dtype=np.float32))


def self_launch(n):
    """`bench.py --gpus N` (N > 1) started as a plain process: start
    torch.distributed.run with N ranks on this node as a CHILD process (this
    process has not imported torch or touched the GPU), relay rank 0's JSON
    line on stdout (everything else the ranks print goes to stderr) and exit
    with the launcher's code."""
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env["PM_BENCH_LAUNCHED"] = "1"
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env)
    for line in proc.stdout:
        s = line.strip()
        if s.startswith("{"):
            try:
                json.loads(s)
                print(s, flush=True)
                continue
            except ValueError:
                pass
        sys.stderr.write(line)
    return proc.wait()


def main():
    args = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        if world == 1 and args.gpus > 1:
            if os.environ.get("PM_BENCH_LAUNCHED") == "1":
                sys.exit("bench.py: the self-launched ranks have no WORLD_SIZE")
            sys.exit(self_launch(args.gpus))
        args.gpus = world

    import torch  # first: the renderer then shares torch's HIP runtime (one runtime per process)
    import torch.distributed as dist
    # rehearsal knobs for the N > 1 path on a 1-GPU box (not for measurement):
    # PM_BENCH_ONE_DEVICE=1 puts every rank on device 0, PM_BENCH_BACKEND=gloo
    # replaces RCCL (which needs one GPU per rank)
    if os.environ.get("PM_BENCH_ONE_DEVICE") == "1":
        local = 0
    torch.cuda.set_device(local)
    if world > 1:
        backend = os.environ.get("PM_BENCH_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)

    from pmrender import hip
    from pmrender.abi import PM_ESTIMATOR_KNN, PM_ESTIMATOR_PPM, PM_GATHER_GRID, PM_GATHER_KDTREE, \
        PM_REC_EXCEPTION, PM_REC_INVALID, PM_REC_MISS, RenderParams
    from pmrender.dist import HipEngine, PassRunner

    cfg = CONFIGS[args.config]
    if args.total_paths is not None:
        args.paths = -(-args.total_paths // world)      # this rank's chunk (PassRunner's split)
    if args.paths is None:
        args.paths = cfg["paths"]
    scene, workload = build_scene(args.config), cfg["desc"]
    if args.total_paths is not None:
        workload = (f"{args.config.upper()} strong scaling: {args.total_paths:,} photon paths "
                    f"({args.total_paths * 4:,} slots) per pass over all {world} GPU(s), "
                    f"{scene.width}x{scene.height} gather points; scene of: " + cfg["desc"])
    progressive = cfg["progressive"]
    t_setup = time.perf_counter()
    ctx = scene.load_into(hip.Context(local))
    structure = PM_GATHER_KDTREE if args.structure == "kd" else PM_GATHER_GRID
    knn = args.estimator == "knn"
    if knn and world > 1:
        args.exchange = "allgather"        # the kNN estimate is not a sum over photon shards
    radius2 = args.radius2 if args.radius2 is not None else (100.0 if knn else 4.0)
    est = dict(estimator=PM_ESTIMATOR_KNN if knn else PM_ESTIMATOR_PPM, knn_lookup=args.knn_k, initial_radius2=radius2)
    p = RenderParams.defaults(paths_per_pass=args.paths, gather_structure=structure, **est)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        eng = HipEngine(ctx)
        ctx.eye_pass(p, eng._s())
        runner = PassRunner(eng, p, rank, world, args.exchange, total_paths=args.total_paths)
        # a step is one pass over the config's workload: from the initial PPM
        # state (the reference's single pass), or for progressive configs the
        # next pass of one render (Halton permutation of pass k, radii shrink)
        pass_no = [0]

        def step(ahead=False):
            # ahead: with --pipeline, issue the next step's trace during this one's gather
            if progressive:
                runner.step(pass_no[0], reset=pass_no[0] == 0, next_pass=pass_no[0] + 1 if ahead else None)
                pass_no[0] += 1
            else:
                runner.step(0, reset=True, next_pass=0 if ahead else None)

        runner.pipeline = bool(args.pipeline) and world == 1
        # the pipeline never reaches across the timed region's edges: the first
        # timed step traces its own pass, the last issues no trace ahead
        for i in range(args.warmup):
            step(ahead=i < args.warmup - 1)
        runner.flush()
        torch.cuda.synchronize()
        setup_s = time.perf_counter() - t_setup
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        ctx.timing_reset()
        # events only on the roofline kernel's stage inside the timed region,
        # and only on every --gather-event-every-th step: a timed dispatch's
        # events leave ~4.5 us idle before and ~5 us after it (rocprofv3
        # kernel trace, profiles/r06/event_gaps), 6 % of a C2 step
        ev_every = max(1, args.gather_event_every)
        sampled = 0
        t0 = time.perf_counter()
        for i in range(args.steps):
            timed = i % ev_every == 0
            sampled += timed
            ctx.set_stage_timing("gather" if timed else "")
            step(ahead=i < args.steps - 1)
        runner.flush()                 # the last pass's exchange is part of the timed work
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        if world > 1:
            dist.barrier()
            t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        gather_launches, gather_ms_total = ctx.timing_total("gather")
        if args.dump_outputs:
            # the state the last timed step left, before any later pass touches it
            passes_run = args.warmup + args.steps if progressive else 1     # since the last reset
            radiance = torch.empty((ctx.num_records(), 3), dtype=torch.float32, device="cuda")
            runner.final_gather(float(runner.emitted_per_pass * passes_run), radiance)
            torch.cuda.synchronize()
            dump = {"radiance": radiance.cpu().numpy()}
            if world == 1:
                state = ctx.download_records()
                dump.update(flux=state["flux"], radius2=state["radius2"], photon_count=state["photon_count"])
            if rank == 0:
                dump_outputs(args.dump_outputs, dump)
            del radiance, dump
        gather_ms = gather_ms_total / max(gather_launches, 1)
        # per-stage split: a few more passes after the timed region, every stage timed
        ctx.set_stage_timing("all")
        ctx.timing_reset()
        # N > 1: each pass's exchange also timed here, run to completion at
        # once (in the timed steps it overlaps the next pass's trace + build)
        runner.time_exchange = world > 1
        runner.pipeline = False            # stage times of passes run one after another
        split_passes = min(args.steps, 10) if args.full else 0
        for _ in range(split_passes):
            step()
        runner.flush()
        torch.cuda.synchronize()
        runner.time_exchange = False
        # ms per pass (a stage may launch several times per pass: the
        # all-gather mode gathers each of the rank's bands; a reset runs only
        # on the passes that start from the initial state)
        stages = {}
        for name in ("reset", "trace", "build", "gather", "update"):
            n, ms = ctx.timing_total(name)
            if n:
                stages[name] = round(ms / (n if name == "reset" else split_passes), 5)
        if runner.exchange_ms:
            stages["exchange"] = round(sum(runner.exchange_ms) / len(runner.exchange_ms), 5)

        census = canonical = tcensus = None
        n_valid = None
        if args.full and not args.no_census:
            # untimed counting launch of the same step: algorithmic-byte units
            ctx.set_counting(True)
            step()
            runner.flush()
            torch.cuda.synchronize()
            census = ctx.gather_counters(full=True)
            tcensus = ctx.trace_counters()
            ctx.set_counting(False)
            n_valid = ctx.map_info()["valid"]
            if rank == 0 and world == 1 and structure == PM_GATHER_GRID and not knn:
                # SURVEY.md §8d's per-unit figure counts V on the canonical pbrt kd-tree
                pk = RenderParams.defaults(paths_per_pass=args.paths, gather_structure=PM_GATHER_KDTREE)
                ctx.set_counting(True)
                ctx.reset_records(pk, eng._s())
                ctx.trace_photons(pk, 0, 0, args.paths, 0, eng._s())
                ctx.build_photon_map(pk, args.paths * 4, eng._s())
                ctx.gather(pk, eng._s())
                torch.cuda.synchronize()
                canonical = ctx.gather_counters(full=True)
                ctx.set_counting(False)

        # N > 1: the other exchange timed the same way (K steps between barriers,
        # max over ranks), so the line carries both designs: reduce (default)
        # and the all-gather of photon slots that north_star names
        alt = None
        if args.full and world > 1 and not args.no_alt_exchange and not knn:
            alt_x = "allgather" if args.exchange == "reduce" else "reduce"
            if args.exchange == "reduce":
                ctx.set_record_view(False)             # band gathers address records, not the active view
            runner2 = PassRunner(eng, p, rank, world, alt_x, total_paths=args.total_paths)
            pass2 = [0]

            def step2():
                if progressive:
                    runner2.step(pass2[0], reset=pass2[0] == 0)
                    pass2[0] += 1
                else:
                    runner2.step(0, reset=True)

            for _ in range(max(1, args.warmup)):
                step2()
            runner2.flush()
            torch.cuda.synchronize()
            dist.barrier()
            torch.cuda.synchronize()
            ctx.set_stage_timing("")
            t1 = time.perf_counter()
            for _ in range(args.steps):
                step2()
            runner2.flush()
            torch.cuda.synchronize()
            el2 = time.perf_counter() - t1
            dist.barrier()
            t = torch.tensor([el2], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el2 = float(t.item())
            xb2 = (40 * runner2.slots_per_rank * world if alt_x == "allgather"
                   else 28 * runner2.v_per * world)
            alt = {"exchange": alt_x,
                   "value": round(runner2.total * args.steps / el2 / 1e6, 3),
                   "unit": "Mphotons/s",
                   "ms_per_step": round(el2 / args.steps * 1e3, 5),
                   "mgather_samples_per_s": round(scene.width * scene.height * args.steps / el2 / 1e6, 3),
                   "exchange_bytes_per_pass_per_rank": int(xb2),
                   "note": ("40-B photon slots all-gathered into a replicated map, each rank gathers its 8-row "
                            "bands (north_star's design)" if alt_x == "allgather" else
                            "photon-count all-reduce + flux reduce-scatter, every rank gathers every active record "
                            "against its own photon shard") + "; timed like the headline steps, after them"}
            if args.exchange == "reduce":
                ctx.set_record_view(True)              # the census / record reads below use the full set

    n_rec = ctx.num_records()
    recs = ctx.download_records()
    live = (recs["flags"] & (PM_REC_MISS | PM_REC_EXCEPTION | PM_REC_INVALID)) == 0
    active = int(live.sum())
    g_points = scene.width * scene.height
    paths_total = runner.total             # all ranks' paths per pass (strong: --total-paths)
    ms_per_step = elapsed / args.steps * 1e3
    value = paths_total * args.steps / elapsed / 1e6

    # the records THIS rank gathers per pass: all of them (one GPU; the reduce
    # exchange replicates the gather), or its 8-row bands (all-gather exchange)
    bands_mode = world > 1 and args.exchange == "allgather"
    ranges = runner.bands[rank] if bands_mode else [(0, n_rec)]
    n_mine = sum(c for _, c in ranges)
    act_mine = int(sum(live[b:b + c].sum() for b, c in ranges))
    if bands_mode:
        # band gathers launch every tile of their ranges: inactive records are read (16 B: the flags)
        inactive_read = n_mine - act_mine
    else:
        # full-range gathers launch only the tiles holding an active record
        # (records are stored in 8x8 tiles of 64, one wave each)
        pad = (-len(live)) % 64
        tiles = np.concatenate([live, np.zeros(pad, bool)]).reshape(-1, 64)
        inactive_read = int((~tiles[tiles.any(axis=1)]).sum()) - pad * int(tiles[-1].any())
    # per-pass gather time of this rank (the all-gather mode launches once per band)
    gather_pass_ms = gather_ms_total / sampled if sampled else 0.0     # the event-timed steps
    split = world > 1 and args.exchange == "reduce"

    roofline = None
    kernel_name = ("k_gather_knn_ss" if knn else "k_gather_tile" if structure == PM_GATHER_GRID else "k_gather_kd")
    if n_valid is None:
        n_valid = ctx.map_info()["valid"]
    if args.full and gather_pass_ms > 0:
        # The timed step starts from the initial PPM state (a deferred reset):
        # the gather reads only each active record's position and normal
        # (32 B; flux, N and r^2 are the initial constants, pm_gather.hip
        # GatherRec::load) and writes its PPM state (20 B: flux + r^2, N) —
        # or, in the split gather of the reduce exchange, its partial sums
        # (28 B: int32 M + three int64 flux words); the flags of the inactive
        # records of each launched tile (16 B); every valid photon once (40 B)
        wr = 28 if split else 20
        fresh_floor = (32 + wr) * act_mine + 16 * inactive_read + 40 * n_valid
        # SURVEY.md §8d compulsory bytes (92 B per active record: the PPM
        # state read as well — what a pass that continues a render moves)
        compulsory = 92 * act_mine + 40 * n_valid
        achieved = fresh_floor / (gather_pass_ms * 1e-3) / 1e9
        traffic, traffic_src = (load_pmc_traffic(kernel_name, args.config + ("_knn" if knn else ""))
                                if world == 1 else (None, "PMC traffic profiles are single-GPU runs"))
        roofline = {
            # what bounds the kernel (see "limiter"); the roofline it is priced
            # against is HBM ("peak", "unit"): the path moves bytes, no MFMA work
            "bound": "valu" if knn else "latency",
            "priced_against": "hbm",
            "kernel": "k_knn_pack + k_gather_knn_ss (pbrt LPhoton kNN: photon pairs through the scalar cache, "
                      "bit-pattern histograms for r_k^2, fused record update; + k_gather_knn_tile for handed-back "
                      "tiles)" if knn
            else ("k_gather_tile<1,0> (split partial sums for the reduce exchange)" if split else
                  "k_gather_tile<0,1> (LDS-staged range query + fused PPM update)") if structure == PM_GATHER_GRID
            else "k_gather_kd<0,0>",
            "achieved": round(achieved, 1),
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4),
            "traffic": traffic,
            "algorithmic_bytes_per_launch": int(fresh_floor),
            "formula": ("(32 + %d)*G_act + 16*G_inactive_launched + 40*N_valid: the bytes the timed (fresh-state) "
                        "gather must move — position + normal read, %s written per active record, flags of the "
                        "inactive records of launched tiles, each valid photon once" %
                        (wr, "partial sums (M, flux)" if split else "PPM state (flux, r^2, N)")),
            "units": {"G_act": act_mine, "G_inactive_launched": inactive_read, "N_valid": n_valid,
                      "records_gathered": n_mine},
            "survey_8d_compulsory": {
                "formula": "92*G_act + 40*N_valid (SURVEY.md §8d: 72 B read incl. the PPM state + 20 B written)",
                "bytes_per_launch": int(compulsory),
                "GBs_at_measured_time": round(compulsory / (gather_pass_ms * 1e-3) / 1e9, 1),
                "frac": round(compulsory / (gather_pass_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "note": "prices the PPM-state reads of a pass that continues a render; the timed pass starts "
                        "from the initial state and does not perform them (graded figure: algorithmic_bytes_per_launch)"},
            "avg_launch_ms": round(gather_ms, 5),
            "gather_ms_per_pass": round(gather_pass_ms, 5),
            "launches_timed": gather_launches,
            "launches_timed_note": "HIP events on the gather of every %d-th timed step (%d of %d), on its stream" % (
                ev_every, sampled, args.steps),
            "achieved_basis": "since round 5 the fresh-pass floor over the per-pass gather time (rounds 2-4 graded "
                              "SURVEY.md §8d's 92-B compulsory bytes, which include PPM-state reads the timed pass "
                              "does not make; round 1 priced the per-lane algorithmic bytes)",
            "limiter": ("VALU issue + scalar-cache misses (profiles/r04): ~3.7 passes over each tile's union "
                        "(histogram, collect, sum), every lane testing every streamed photon pair" if knn else
                        "VALU issue + per-wave latency (profiles/r02 counters): the kernel reads each record "
                        "once and each tile's photons once, so HBM is not what bounds it"),
        }
        if world > 1:
            roofline["rank"] = rank
            roofline["per_rank"] = "rank 0's gather; every rank gathers %s" % (
                "its own interleaved 8-row bands against the replicated map" if bands_mode else
                "every active record against its own photon shard (the reduce exchange)")
        if census is not None and not bands_mode:
            vis, hits, rows, act = census
            inactive = n_rec - act
            if knn:
                l1_bytes = 72 * act + 16 * inactive + 8 * rows + 16 * vis + 28 * hits
                l1_formula = "72*G_act + 16*G_inactive + 8*bucket_rows + 16*photons_tested + 28*photons_found"
            elif structure == PM_GATHER_GRID:
                l1_bytes = 72 * act + 16 * inactive + 8 * rows + 16 * vis + 20 * hits
                l1_formula = "72*G_act + 16*G_inactive + 8*bucket_rows + 16*photons_tested + 20*photons_in_radius"
            else:
                l1_bytes = 72 * act + 16 * inactive + 16 * vis + 24 * hits
                l1_formula = "72*G_act + 16*G_inactive + 16*kd_nodes_visited + 24*photons_in_radius"
            roofline["units"].update({"bucket_rows": rows, "photons_tested": vis,
                                      "photons_found" if knn else "photons_in_radius": hits})
            # the per-lane kernel's operand bytes (16 B per photon each lane
            # tests): what the L1 / LDS deliver, not HBM traffic
            roofline["l1_delivered"] = {"bytes_per_launch": int(l1_bytes), "formula": l1_formula,
                                        "GBs": round(l1_bytes / (gather_pass_ms * 1e-3) / 1e9, 1)}
        if traffic is not None:
            raw = load_pmc_traffic(kernel_name, args.config + ("_knn" if knn else ""), "hbm_bytes_uncorrected")[0]
            roofline["traffic_uncorrected"] = raw
            roofline["traffic_correction"] = ("traffic = 2 x FETCH_SIZE + WRITE_SIZE (the guide's gfx950 halving of "
                                              "FETCH_SIZE, stated for wide coalesced streaming reads; this kernel's "
                                              "reads are 16-B records and photon rows, so the true bytes lie between "
                                              "traffic_uncorrected and traffic)")
            roofline["traffic_GBs"] = round(traffic / (gather_ms * 1e-3) / 1e9, 1)
            roofline["traffic_frac"] = round(traffic / (gather_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
            roofline["traffic_over_floor"] = round(traffic / fresh_floor, 3)
            roofline["traffic_source"] = traffic_src
        else:
            roofline["traffic_note"] = traffic_src
        if canonical is not None:
            cv, ch, _, cact = canonical
            survey_bytes = 92 * cact + 16 * cv + 24 * ch
            roofline["survey_8d_graded"] = {
                "formula": "92*G_act + 16*V_kd + 24*H (SURVEY.md §8d, V on the canonical pbrt kd-tree)",
                "bytes_per_launch": int(survey_bytes), "V_kd": cv, "H": ch,
                "GBs_at_measured_time": round(survey_bytes / (gather_ms * 1e-3) / 1e9, 1),
                "note": "V counts kd-tree nodes a tree walk would fetch; the bucket kernel fetches none of them, "
                        "so this exceeds what the kernel moves"}

    exchange = None
    if args.full and world > 1:
        # bytes this rank sends into the collectives per pass
        if args.exchange == "reduce":
            xb = 4 * runner.v_per * world + 24 * runner.v_per * world
            xf = "4 B count all-reduce + 24 B flux reduce-scatter per active record (view rows padded to the world)"
        else:
            xb = 40 * runner.slots_per_rank * world
            xf = "40-B photon slots all-gathered: every rank's chunk"
        exchange = {"bytes_per_pass": int(xb), "formula": xf, "backend": dist.get_backend(),
                    "ms_per_pass": stages.get("exchange"),
                    "GBs": round(xb / (stages["exchange"] * 1e-3) / 1e9, 2) if stages.get("exchange") else None,
                    "note": "timed to completion in the stage-timed passes after the timed region; in the timed "
                            "steps the reduce exchange overlaps the next pass's trace + build"}

    trace_roofline = None
    if tcensus is not None and "trace" in stages and ctx.scene_info()["mode"] == "brute":
        # brute-force scene (C2's Cornell box: 30 triangles + 1 disk, no BVH):
        # the triangles are read through the scalar cache, so the kernel's
        # algorithmic work is arithmetic — ~41 FP32 operations per primitive
        # test (OptiX test: dot 5, exact reciprocal 5, e2 6, cross 9, three
        # dots 15, beta+gamma 1) against the VALU FP32 peak
        rays, nodes, prims, deposits = tcensus
        tflop = 41.0 * prims / (stages["trace"] * 1e-3) / 1e12
        trace_roofline = {
            "bound": "valu", "kernel": "k_trace_lane<0,MODE_BRUTE>", "achieved": round(tflop, 2),
            "peak": VALU_FP32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(tflop / VALU_FP32_PEAK_TFLOPS, 4),
            "flops_per_launch": int(41 * prims), "formula": "41 * prim_tests",
            "units": {"rays": rays, "prim_tests": prims, "deposits": deposits},
            "avg_launch_ms": stages["trace"],
            "note": "one occupancy round of 4,096 waves, each as long as its longest path (~5 rays against 3.46 on "
                    "average); ~64 % VALU busy, ~60 % of the VALU work in the packed triangle-pair test "
                    "(profiles/r05/trace_c2)"}
    elif tcensus is not None and "trace" in stages:
        rays, nodes, prims, deposits = tcensus
        # SURVEY.md §8d (reported, not graded): 40 B per deposit + 32 B per BVH
        # node entered + 36 B per primitive test (RNG is inline Philox: 0 B)
        tbytes = 40 * deposits + 32 * nodes + 36 * prims
        tach = tbytes / (stages["trace"] * 1e-3) / 1e9
        trace_roofline = {
            "bound": "hbm",
            "kernel": {"bvh-hbm": "k_trace_pool (4-wide BVH in HBM / MALL, pooled paths)",
                       "bvh-instanced": "k_trace_lane<0,MODE_INST> (top tree + one tree per object mesh)"}.get(
                           ctx.scene_info()["mode"], "k_trace_lane<0,MODE_LDS>"),
            "achieved": round(tach, 1), "peak": HBM_PEAK_GBS,
            "unit": "GB/s", "frac": round(tach / HBM_PEAK_GBS, 4), "algorithmic_bytes_per_launch": int(tbytes),
            "formula": "40*deposits + 32*bvh_nodes + 36*prim_tests (SURVEY.md §8d B_trace)",
            "units": {"rays": rays, "bvh_nodes": nodes, "prim_tests": prims, "deposits": deposits},
            "per_ray": {"bvh_nodes": round(nodes / max(rays, 1), 2), "prim_tests": round(prims / max(rays, 1), 2)},
            "avg_launch_ms": stages["trace"],
            "note": "latency-bound traversal: the BVH reads hit L2 / the 256 MiB MALL, so B_trace is mostly "
                    "cache traffic, not HBM"}

    out = {
        "metric": METRIC,
        "value": round(value, 3),
        "unit": "Mphotons/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 5),
        "higher_is_better": True,
        "scaling": "strong" if args.total_paths else "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic: scene built in code (pmrender/scenes.py), BASELINE.json config " + args.config.upper(),
        "config": {
            "workload": workload,
            "photon_slots_per_gpu": runner.per * int(p.max_photon_count),
            "paths_per_gpu": runner.per,
            "paths_per_pass_all_gpus": runner.total,
            "gather_points": g_points,
            "active_gather_points": active,
            "structure": args.structure,
            "estimator": args.estimator + (f" (k={args.knn_k})" if knn else ""),
            "radius2": radius2,
            "exchange": args.exchange if world > 1 else "none",
            "parallelism": f"photon-shard x{world}" if world > 1 else "single",
            "pass_pipeline": bool(args.pipeline) and world == 1,
        },
        "mgather_samples_per_s": round(g_points * args.steps / elapsed / 1e6, 3),
        # the reference's "Total photons" convention (4 slots per path): value x 4
        "mphoton_slots_per_s": round(paths_total * int(p.max_photon_count) * args.steps / elapsed / 1e6, 3),
        "kernel_rates": {
            "trace_mphotons_per_s": round(runner.paths / (stages["trace"] * 1e-3) / 1e6, 2) if "trace" in stages else None,
            # records this rank gathered per pass over its per-pass gather time
            "gather_msamples_per_s": round(n_mine / (gather_pass_ms * 1e-3) / 1e6, 2) if gather_pass_ms > 0 else None,
        },
        "stages_ms": stages,
        "setup_s": round(setup_s, 3),
        "roofline": roofline,
        "trace_roofline": trace_roofline,
    }
    if exchange is not None:
        out["exchange"] = exchange
    if alt is not None:
        out["alt_exchange"] = alt
    if rank == 0 and args.full and not args.no_cpu_baseline:
        try:
            out["cpu_baseline"] = cpu_baseline(scene, RenderParams.defaults(paths_per_pass=args.paths, **est),
                                               args.cpu_threads or default_cpu_threads(), args.config)
        except Exception as exc:  # the baseline is reported, never required for the GPU number
            out["cpu_baseline"] = {"error": repr(exc)}
    if rank == 0:
        print(json.dumps(out), flush=True)
    ctx.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
