#!/usr/bin/env python
"""bench.py -- MPC steps/sec of the Avoid-MPC hot path on MI355X (BASELINE.json's metric).

  python bench.py --gpus N --steps K --warmup W
      N > 1: one process per GPU.  Under torch.distributed.run (RANK / WORLD_SIZE in the environment) this process IS a rank;
      started plainly it re-launches itself as `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr
      127.0.0.1 --master-port <free port> bench.py <same arguments>` and rank 0 prints the one JSON line.
  python bench.py --workload flight ...                 closed-loop flights (warm-started control periods), see flight_main()
  python bench.py ... --full                            the default workload plus everything beyond its headline (below)
  python bench.py ... --dump-outputs DIR                also writes what the last timed step returned, DIR/<name>.npy

One "step" = one pass of the hot path over one batch of synthetic scenes resident in HBM: for every scene a fresh
depth frame (build the obstacle + edge KD indices) and one control step (<= 3 outer passes of {dual KD queries, pack P,
interior-point solve run to tol 1e-4}, zero warm start), SURVEY.md section 8(d).  value = scenes
processed by all ranks / wall time (max over ranks).
Workload: BASELINE.json configs[1] (50k-point cloud, N = 20, K = 8) batched as configs[2] (256 scenes per GPU); scenes
are independent, so N GPUs run N x 256 scenes (weak scaling) and the only collective is the gather of the sweep's controls
(one ncclAllGather of 4 doubles per scene-step at the end of the timed region, issued through the library's own RCCL binding
amk_shard_gather).  The steps are kept in flight by the C ABI's amk_pipeline_* (what a C++ host calls; tests/cpp/sweep_driver.cpp
is that host).  Every in-flight step owns its own frames (distinct clouds: the working set
is `streams` x 169 MB, far beyond the 256 MiB Infinity Cache).

A plain run sets up, warms up, times --steps steps and prints the contract's fields and the configuration.  With --full the
JSON line of the default workload also carries what takes runs or checks of its own:
  parity      |u - u*|_inf and (J - J*)/J* of the GPU solve on the committed fixtures of the three BASELINE sizes
              (tests/golden/mpc_parity_golden.npz: converged optima, SURVEY.md section 8(d) gate) and the check of one
              in-flight slot's controls / flags of the timed workload against the CPU oracle (same scenes);
  roofline    SURVEY 8(d)'s ruler: frac = frac_hbm_8d = steps/s x algorithmic bytes per scene-step / 8 TB/s (the whole step), and beside
              it frac_valu_issue + dominant_kernel: what the dominant kernel (mpc_solve_kernel, a serial interior-point solve per
              wavefront, not HBM-bound) fills of the chip's VALU issue slots; roofline_hbm = that kernel's own bytes / launch duration;
  roofline_kd_build   the HBM-bound kernel of the step;
  cpu_baseline, kernels_single_stream, hbm_peak_measured_gbs, value_steady_state (when --steps < --steady-steps).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E, /opt/skills/guides/MI355X_MICROARCH.md
# amk_common.h KernelClass: what the library's HIP-event timing (amk__timing_*) can bracket
KCLASS = [None, "step_knn_grid_kernel", "step_scan_kernel (cross-check mode only)", "step_plan_pack_kernel", None,
          "mpc_solve_kernel", "step_begin_kernel", "kd_build_kernel"]
PROFILE_TAG = "r06"
N_CU, N_SIMD, CLOCK_GHZ = 256, 4, 2.4   # MI355X: /opt/skills/guides/MI355X_MICROARCH.md


def measured_hbm_peak(torch, lib, gib=1.0, reps=10):
    """SURVEY.md 8(d) / BASELINE.md 3: the ACHIEVABLE HBM rate beside the vendor peak -- a float4 device copy of `gib` GiB
    (amk__hbm_copy_probe, csrc/probe.hip; far beyond the 256 MiB Infinity Cache), bytes read + bytes written over the time of
    the copy.  Runs before the pipeline's buffers exist; returns GB/s."""
    import ctypes as C
    nb = int(gib * (1 << 30)) // 16 * 16
    src = torch.empty(nb, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
    src.fill_(1)
    torch.cuda.synchronize()
    ms = C.c_double()
    lib.amk__hbm_copy_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    lib.amk__hbm_copy_probe.restype = C.c_int
    rc = lib.amk__hbm_copy_probe(src.data_ptr(), dst.data_ptr(), nb, reps, None, C.byref(ms), None)
    assert rc == 0, rc
    del src, dst
    torch.cuda.empty_cache()
    return 2.0 * nb / (ms.value * 1e-3) / 1e9


def alg_bytes_per_step(n, ne, N, K):
    """every input read once, every output written once, per scene-step."""
    nx = 10 + 14 * N
    plen = 54 + 10 * N + 3 * K * N
    return 12 * n + 12 * ne + 8 * plen + 8 * nx + 8 * nx + 32


def solve_alg_bytes(N, K):
    """Algorithmic HBM bytes of ONE launch of the dominant kernel (mpc_solve_kernel) per scene:
    reads vecRefStates (20+10N+3KN doubles), the 192-double parameter block and the warm start
    (nx); writes the solution (nx), u (4), x0Array (14N) and the refilled reference path (10N)."""
    nx = 10 + 14 * N
    return 8 * ((20 + 10 * N + 3 * K * N) + 192 + nx + nx + 4 + 14 * N + 10 * N)


# ------------------------------------------------------------------------------------------------
# CPU baseline (rank 0, N = 1 only) = the checker of the timed workload: the oracle's restatement of the same step on
# the SAME scenes one in-flight slot processed, one scene per core at a time.  KD builds are timed on the reference's
# own nanoflann (oracle/_ref, compiled from /root/reference in place with the reference's flags) when it was built.
# ------------------------------------------------------------------------------------------------
def _cpu_scene(args):
    cloud, edge, sq, posx, ref, T, K, use_ref = args
    import numpy as np  # noqa: F401
    from avoid_mpc_amd import synth
    from tests import _oracle
    prm = synth.MpcParams(T=T, K=K)
    t_ref = None
    t_begin = time.time()
    if use_ref:   # FrameKDMap::AddVertex's two InitializeNew calls on the reference's nanoflann (reference flags)
        t0 = time.perf_counter()
        ko, ke = _oracle.kd_ref(cloud, strict=False), _oracle.kd_ref(edge, strict=False)
        t_ref = time.perf_counter() - t0
        ko.close(); ke.close()
    t0 = time.perf_counter()
    kd, ke = _oracle.kd_oracle(cloud), _oracle.kd_oracle(edge)
    t1 = time.perf_counter()
    mpc = _oracle.MpcOracle(prm.T, prm.dt, prm.K); mpc.configure(prm)
    r = _oracle.step_oracle(kd, ke, mpc, prm, sq, posx, ref.copy())
    t2 = time.perf_counter()
    kd.close(); ke.close(); mpc.close()
    return r["u"], r["flags"], t1 - t0, t2 - t1, t_ref, t_begin, time.time()


def cpu_baseline_and_check(scenes, T, K, gpu_u, gpu_flags):
    """scenes: list of (cloud, edge, sq, posx, ref) numpy tuples of one slot.  -> (cpu_baseline dict, check dict)"""
    import multiprocessing as mp
    import numpy as np
    from tests import _oracle
    _oracle.build_oracle()
    use_ref = _oracle.load_ref(strict=False) is not None
    cores = os.cpu_count() or 1
    try:
        cores = len(os.sched_getaffinity(0))
    except Exception:
        pass
    quota, quota_cores = None, None
    try:   # a container may see every core of the host and still be limited to a CPU-time quota (cgroup v2)
        quota = open("/sys/fs/cgroup/cpu.max").read().strip()
        q, per = quota.split()
        if q != "max":
            quota_cores = max(1, int(float(q) / float(per)))
    except Exception:
        pass
    workers = max(1, min(cores, quota_cores or cores, 128, len(scenes)))
    jobs = [(c, e, sq, px, rf, T, K, use_ref) for (c, e, sq, px, rf) in scenes]
    # true single-process latency: two scenes alone on the machine, before the pool starts
    lone = [_cpu_scene(j) for j in jobs[:2]]
    lone_build = float(np.mean([(r[4] if use_ref else r[2]) for r in lone])); lone_step = float(np.mean([r[3] for r in lone]))
    # bounded sample of ~10-20 s of CPU work: the slot's scenes, repeated until that much single-process time is queued
    reps = int(max(1, min(8, round(12.0 / max(1e-3, len(jobs) * (lone_build + lone_step))))))
    ctx = mp.get_context("spawn")
    t0 = time.perf_counter()
    with ctx.Pool(workers) as pool:
        res_all = pool.map(_cpu_scene, jobs * reps, chunksize=1)
    wall = time.perf_counter() - t0
    span_all = max(r[6] for r in res_all) - min(r[5] for r in res_all)
    n_all = len(res_all)
    res = res_all[:len(jobs)]
    build = np.array([(r[4] if use_ref else r[2]) for r in res]); step = np.array([r[3] for r in res])
    busy = float((build + step).sum())
    span = span_all                                           # first scene started .. last scene finished (no startup)
    value = n_all / span
    base = {"value": round(value, 2), "unit": "MPC steps/s", "cores": workers, "kind": "port",
            "sample": f"the {len(res)} scenes of one in-flight slot of the timed workload, one per process at a time on "
                      f"{workers} processes (= usable host cores: min of the affinity mask and the cgroup CPU quota); value = scene-steps / (last finish - first start) = {n_all} / {span:.2f} s "
                      f"(the slot {reps} x; {wall:.1f} s wall incl. process startup); KD builds "
                      + ("on the reference's own nanoflann compiled in place with the reference's flags (oracle/_ref), "
                         if use_ref else "on the oracle's restatement of nanoflann, ")
                      + "queries / step logic / interior-point solve on the oracle's restatement (CasADi + IPOPT are absent)",
            "kd_build_kind": "reference" if use_ref else "port", "span_s": round(span, 3), "cgroup_cpu_max": quota, "cores_visible": cores,
            "if_every_core_ran_at_single_process_speed": round(workers / (lone_build + lone_step), 1),
            "all_core_ms_per_step_per_core": round(1e3 * busy / len(res), 3),
            "all_core_kd_build_ms": round(1e3 * float(build.mean()), 3),
            "single_process_ms_per_step": round(1e3 * (lone_build + lone_step), 3),
            "single_process_kd_build_ms": round(1e3 * lone_build, 3),
            "single_process_queries_and_solves_ms": round(1e3 * lone_step, 3)}
    cu = np.stack([r[0] for r in res]); cf = np.stack([r[1] for r in res])
    same = np.all(cf == gpu_flags, axis=1)          # isSafety, solves, status, interior-point iterations
    du = np.abs(cu - gpu_u).max(axis=1)
    other = int(np.sum(~same & (du > 1e-3)))
    check = {"scenes": len(res), "flags_identical": int(same.sum()),
             "du_max_where_flags_identical": float(du[same].max()) if same.any() else None,
             "du_max_all": float(du.max()), "scenes_in_another_local_minimum": other,
             "ok": bool(int((~same).sum()) <= max(1, len(res) // 100) and (not same.any() or du[same].max() <= 1e-6)
                        and other <= max(1, len(res) // 200)),
             "note": "same scenes, GPU step vs CPU oracle; a scene whose iteration counts differ took a different branch "
                     "at a rounding-level tie: it normally ends at the same optimum (1e-3, the parity gate); allowed: "
                     "<= 1 % such scenes, <= 0.5 % in another local minimum of the non-convex NLP (census over 2048 scenes: "
                     "0.2 % / 0.15 %)"}
    return base, check


def fixture_parity(torch, precision):
    """The GPU solve with the shipped options on the committed fixtures -> the SURVEY section 8(d) gate numbers."""
    import numpy as np
    from avoid_mpc_amd import synth
    from avoid_mpc_amd.host import MpcBatch
    path = os.path.join(ROOT, "tests", "golden", "mpc_parity_golden.npz")
    if not os.path.exists(path):
        return None
    G = np.load(path)
    out = {}
    for cfg in ("C1", "C2", "C5"):
        c = synth.CONFIGS[cfg]
        prm = synth.MpcParams(T=c["T"], K=c["K"])
        refs = torch.from_numpy(G[cfg + ".ref"]).cuda()
        m = MpcBatch(prm.T, prm.dt, prm.K, refs.shape[0]); m.configure(prm); m.set_precision(precision)
        u, _, info = m.Solve(refs, faster=True)
        w = m.get_warm_start()
        J = m.eval(w, refs, want=("f",))["f"]
        torch.cuda.synchronize()
        u, w, J, info = u.cpu().numpy(), w.cpu().numpy(), J.cpu().numpy(), info.cpu().numpy()
        ws, Js = G[cfg + ".wstar"], G[cfg + ".Jstar"]
        du = np.abs(u - ws[:, 10:14]).max(axis=1); dx = np.abs(w - ws).max(axis=1); dJ = (J - Js) / Js
        out[cfg] = {"scenes": int(len(du)), "frac_u_within_1e-3": round(float(np.mean(du <= 1e-3)), 4),
                    "frac_x_within_1e-3": round(float(np.mean(dx <= 1e-3)), 4), "du_median": float(np.median(du)),
                    "du_p90": float(np.quantile(du, 0.9)), "du_max": float(du.max()),
                    "dJ_rel_median": float(np.median(dJ)), "dJ_rel_max": float(dJ.max()),
                    "ipm_iters_mean": round(float(info[:, 1].mean()), 2), "converged": int((info[:, 0] == 0).sum())}
        m.close()
    out["gate"] = ("SURVEY.md 8(d): every fixture scene converged (status 0) with |u - u*|_inf <= 1e-3, |x - x*|_inf <= 1e-3 on "
                   ">= 98 %; u* = converged local optimum of this project's method (fixture); what independent solvers reach "
                   "from the same start: tests/test_mpc_independent.py")
    out["ok"] = bool(all(out[c]["converged"] == out[c]["scenes"] and out[c]["du_max"] <= 1e-3 and
                         out[c]["frac_x_within_1e-3"] >= 0.98 for c in ("C1", "C2", "C5")))
    return out


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(d, outputs):
    """--dump-outputs: one step's results (dict of arrays with the scene as the leading axis) as DIR/<name>.npy in float64
    (flags are small integers: exact).  Above DUMP_MAX_BYTES in all, a fixed seeded sample of scenes is written, and its
    scene indices as scene_index.npy."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    out = {k: np.asarray(v, dtype=np.float64) for k, v in outputs.items()}
    S = len(next(iter(out.values())))
    per_scene = sum(a.nbytes for a in out.values()) // S
    keep = min(S, (DUMP_MAX_BYTES - 8 * S) // per_scene)
    if keep < S:
        idx = np.sort(np.random.default_rng(0).choice(S, keep, replace=False))
        out = {k: a[idx] for k, a in out.items()}
        out["scene_index"] = idx.astype(np.float64)
    for k, a in out.items():
        np.save(os.path.join(d, k + ".npy"), np.ascontiguousarray(a))


# ------------------------------------------------------------------------------------------------
def self_launch(n):
    """`python bench.py --gpus N` without a launcher: re-run this script as N ranks of ONE node under torch.distributed.run
    (the driver's own command line), stream rank 0's JSON line through, return the launcher's exit code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL across processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def rccl_report(torch):
    """Which RCCL the process carries (make the first multi-GPU run debuggable): the file amk_shard bound its
    collectives from (dladdr of ncclAllGather; the copy already in the process when there is one), its version, PyTorch's RCCL
    version, and every librccl the process has mapped -- more than one distinct file means two RCCL instances in one process."""
    from avoid_mpc_amd.host import Shard
    info = Shard.rccl_info()
    try:
        mapped = sorted({l.split()[-1] for l in open("/proc/self/maps") if "librccl" in l})
    except OSError:
        mapped = None
    try:
        tv = torch.cuda.nccl.version()
        tv = ".".join(str(v) for v in tv) if isinstance(tv, tuple) else str(tv)
    except Exception as e:   # (a CPU-only dry run)
        tv = f"unavailable ({type(e).__name__})"
    return {"amk_shard_bound": info, "torch_nccl_version": tv, "librccl_files_mapped": mapped,
            "single_rccl_instance": None if mapped is None else len(mapped) <= 1}


def write_rank_file(rank, payload):
    """One small JSON file per rank, written BEFORE the exchange step: if a collective hangs, what every rank measured and which
    RCCL it bound is still on disk (gpurun_out/bench_ranks/rank<r>.json; AMK_BENCH_RANK_DIR overrides the directory)."""
    d = os.environ.get("AMK_BENCH_RANK_DIR", os.path.join(ROOT, "gpurun_out", "bench_ranks"))
    try:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, f"rank{rank}.json"), "w") as f:
            json.dump(payload, f)
    except OSError as e:
        print(f"bench.py: rank {rank}: cannot write the per-rank file: {e}", file=sys.stderr)


def dry_run(args):
    """The launch path without a GPU: rendezvous over gloo, the library's own partition (amk_shard_scene_range /
    amk_shard_padded_count), an all-gather shaped like the sweep's, max-over-ranks of a wall time, one JSON line from rank 0."""
    import numpy as np
    import torch
    import torch.distributed as dist
    from avoid_mpc_amd import capi
    world = int(os.environ.get("WORLD_SIZE", "1")); rank = int(os.environ.get("RANK", "0"))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29511")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lib = capi.load()
    total = args.scenes * world
    first, count = C.c_int(), C.c_int()
    capi.check(lib.amk_shard_scene_range(rank, world, total, C.byref(first), C.byref(count)), "amk_shard_scene_range")
    padded = lib.amk_shard_padded_count(world, total)
    t0 = time.perf_counter()
    local = torch.full((args.steps, padded, 4), float(rank), dtype=torch.float64)
    local[:, :, 0] = torch.arange(first.value, first.value + padded, dtype=torch.float64)[None, :]
    out = [torch.empty_like(local) for _ in range(world)]
    rccl = rccl_report(torch)
    write_rank_file(rank, {"rank": rank, "world": world, "device": "cpu (dry run)", "first_scene": first.value, "scenes": count.value,
                           "rccl": rccl, "stage": "before the gather"})
    dist.all_gather(out, local)
    dt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    dist.all_reduce(dt, op=dist.ReduceOp.MAX)
    ok = all(int(out[r][0, 0, 1]) == r for r in range(world)) and \
        [int(out[r][0, 0, 0]) for r in range(world)] == [r * args.scenes for r in range(world)]
    dist.barrier()
    if rank == 0:
        print(json.dumps({"metric": "dry run (launch path only)", "value": None, "unit": "MPC steps/s", "n_gpus": world,
                          "steps": args.steps, "warmup": args.warmup, "dry_run": True, "ranks_seen": world, "gather_ok": bool(ok),
                          "scenes_per_rank": count.value, "padded_scenes_per_rank": padded, "max_over_ranks_s": float(dt.item()),
                          "rccl": rccl, "rank_files": os.environ.get("AMK_BENCH_RANK_DIR", os.path.join(ROOT, "gpurun_out", "bench_ranks"))}), flush=True)
    dist.destroy_process_group()
    return 0


def flight_main(args):
    """--workload flight: the reference's regime.  Every step is one control period of a batch of S flights: a fresh frame
    (both index builds), GetInitPath on the slot's own mRefPath, GetCurStateQuad per pass, the re-plan loop from the previous
    period's solution (mNlpW0), PubCmd / PubSlowDownCmd -- all inside amk_pipeline's TASK mode -- and the vehicle (the MPC's own
    model driven by the command: two torch kernels per batch and period, part of the workload, not of the product).  The loop
    never synchronises with the host: the vehicle's kernels are queued on the slot's own stream behind the step (a host with its
    own streams would use amk_pipeline_frame.input_ready / amk_pipeline_wait_stream: tests/test_pipeline_gpu.py).
    value = flight-periods per second = MPC steps/s of warm-started steps; the cold-start headline is the default workload."""
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "32")
    import numpy as np
    import torch
    from avoid_mpc_amd import capi, flight, synth
    from avoid_mpc_amd.host import Pipeline
    lib = capi.load()
    assert int(os.environ.get("WORLD_SIZE", "1")) == 1, "the flight workload is a single-GPU secondary measurement"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    prm = synth.MpcParams(T=args.T, K=args.K)
    S, n, ne, N = args.scenes, args.points, args.points // 10, prm.N
    nslots, gang = max(1, args.streams), args.gang if args.gang > 0 else 8
    B = nslots * gang                                        # batches of flights = (slot, gang position) pairs
    # periods per flight: 52 unless asked otherwise (17 m at 10 m/s: the corridor's first 8 m are free of obstacles, shorter flights
    # would measure mostly those); an explicit --steps gives ceil(steps / batches)
    P = args.periods if args.periods > 0 else (52 if args.steps == 2048 else max(2, -(-args.steps // B)))
    W = min(B, 4)                                            # distinct world sets (frames of W x P x 169 MB stay resident)
    # the corridor outlasts the flights (80 m holds the default 52 periods; beyond its last cylinder a frame degenerates)
    world_len = max(80.0, 8.0 + prm.speed * prm.dt * P + 30.0 + 10.0)
    # with the keyframe map the frames are what a forward-looking sensor returns: nothing behind the vehicle (points from 1 m ahead
    # of the nominal position on).  A 360-degree cloud makes DroneBehindPts (FrameKDMap.cpp:233-252) pop every keyframe the period
    # after its insertion -- its nearest points are beside and behind the drone at once -- and the map would stand empty half the time
    back = (-1.0 if args.frames_behind is None else args.frames_behind) if args.keyframes > 0 else (6.0 if args.frames_behind is None else args.frames_behind)
    worlds = [flight.FlightWorldsTorch(S, n, prm, 9000 + w, dev, length=world_len, back=back) for w in range(W)]
    t_gen = time.perf_counter()
    frames = [[worlds[w].frame(t) for t in range(P)] for w in range(W)]
    torch.cuda.synchronize()
    t_gen = time.perf_counter() - t_gen
    A, Bm, c = flight.affine_plant(prm.tau, prm.dt)
    ABt = torch.from_numpy(np.concatenate([A, Bm], axis=1).T.copy()).to(dev)      # [14, 10]: x' = [x, a_cmd, 0] @ ABt + c
    cvec = torch.from_numpy(c).to(dev)
    kf = dict(max_frame_count=args.keyframes, th_dist=0.1, th_count=10, depth_min=0.1) if args.keyframes > 0 else None   # yaml :71-73,66
    # PtIsInFrame's camera for cloud frames: the yaml's 640 x 480 / 10 sensor (mpc_parameters.yaml:59-66) with the yaml's extrinsic
    # T_b_c (:67-71: 5 cm ahead of the body's origin, looking along its +x); mCurFrame.Twc = Twb * T_b_c, Twb = [I | odometry position]
    kf_cam = capi.FrameCamera(32.0, 32.0, 32.0, 24.0, 100.0, 64, 48) if kf else None
    pl = Pipeline(nslots, S, n, ne, prm, queue_depth=args.queue_depth if args.queue_depth > 0 else 2, gang=gang,
                  keyframes=dict(kf, Tbc=flight.TBC_YAML) if kf else None)
    tbc = torch.from_numpy(flight.TBC_YAML).to(dev)
    Twc = [tbc.repeat(S, 1, 1).contiguous() for _ in range(B)] if kf else None
    for i in range(nslots):
        pl.kd(i, 0).set_tie_order(args.tie_order); pl.kd(i, 1).set_tie_order(args.tie_order)
        pl.mpc(i).set_precision(args.precision)
        if args.ipm_max_iter is not None:
            pl.mpc(i).set_solver_options(1e-4, args.ipm_max_iter)
        if args.solve_budget is not None:
            pl.mpc(i).set_solve_budget(args.solve_budget, args.budget_rounds)
    x0 = np.zeros((B, S, 10)); ref0 = np.zeros((B, S, N, 10))
    for b in range(B):
        for s_ in range(S):
            x0[b, s_], ref0[b, s_] = flight.initial_state(77000 + b * S + s_, prm)
    ref0_d = torch.from_numpy(ref0).to(dev)
    # the vehicle's kernels run on the slot's own stream, right behind the step that produced the command: no second set of
    # streams (2 B streams oversubscribe the 32 hardware queues), no events; batch b lives on slot b // gang, position b % gang
    slot_stream = [torch.cuda.ExternalStream(lib.amk_pipeline_stream(pl.h, i), device=dev) for i in range(nslots)]

    def fly(periods, log=None):
        """All B batches for `periods` periods from the start state; returns (seconds, host seconds in submit)."""
        x = [torch.from_numpy(x0[b]).to(dev) for b in range(B)]
        xu = [torch.zeros((S, 14), dtype=torch.float64, device=dev) for _ in range(B)]   # [x, a_cmd, yaw_dot = 0]
        cmd = [torch.zeros((S, 3), dtype=torch.float64, device=dev) for _ in range(B)]   # Command.acceleration of the period
        torch.cuda.synchronize()
        t0 = time.perf_counter(); t_sub = 0.0
        for t in range(periods):
            for si in range(nslots):
                ts = time.perf_counter()
                tickets = []
                for g in range(gang):
                    b = si * gang + g
                    cl, ed = frames[b % W][t]
                    if kf:   # mCurFrame.Twc of the frame, written on the slot's stream behind the vehicle
                        with torch.cuda.stream(slot_stream[si]):
                            torch.add(x[b][:, 0:3], tbc[0:3, 3], out=Twc[b][:, 0:3, 3])
                    tickets.append(pl.submit(cl, ed, ref_path_init=ref0_d[b] if t == 0 else None, odom=x[b], cmd_out=cmd[b],
                                             keep_warm_start=t > 0, order_after_current_stream=False,
                                             Twc_cur=Twc[b] if kf else None, cam=kf_cam))
                    assert tickets[-1] % nslots == si
                t_sub += time.perf_counter() - ts
                with torch.cuda.stream(slot_stream[si]):      # queued behind the gang's launches on the same stream
                    for g in range(gang):
                        b = si * gang + g
                        xu[b][:, 0:10] = x[b]
                        xu[b][:, 10:13] = cmd[b]
                        torch.addmm(cvec, xu[b], ABt, out=x[b])                           # the vehicle over one control period
                        if log is not None:
                            log["pos"][b, t + 1] = x[b][:, 0:3]
                            o = pl.output_tensors(tickets[g])
                            log["flags"][b, t] = o["flags"]; log["u"][b, t] = o["u"]
        pl.drain()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, t_sub

    fly(min(P, max(2, args.warmup)))                          # untimed: workspaces, first-touch, clocks
    dt, t_sub = fly(P)
    log = dict(pos=torch.zeros((B, P + 1, S, 3), dtype=torch.float64, device=dev), flags=torch.zeros((B, P, S, 4), dtype=torch.int32, device=dev),
               u=torch.zeros((B, P, S, 4), dtype=torch.float64, device=dev))
    log["pos"][:, 0] = torch.from_numpy(x0[:, :, 0:3]).to(dev)
    fly(P, log)                                               # the same flights once more, logged (untimed)
    pos = log["pos"].cpu().numpy().transpose(0, 2, 1, 3); fl = log["flags"].cpu().numpy().transpose(0, 2, 1, 3)
    ug = log["u"].cpu().numpy().transpose(0, 2, 1, 3)                                     # [B, S, P(+1), .]
    clear = np.stack([worlds[b % W].clearance(pos[b]) for b in range(B)])                 # [B, S, P + 1]
    cmin = clear.min(axis=2)
    stats = {"flights": int(B * S), "periods": P, "solves_per_step": round(float(fl[..., 1].mean()), 3),
             "ipm_iters_per_step": round(float(fl[..., 3].mean()), 2), "ipm_iters_first_period": round(float(fl[:, :, 0, 3].mean()), 2),
             "unsafe_periods": int((fl[..., 0] == 0).sum()), "capped_solves": int((fl[..., 2] > 0).sum()),
             "min_clearance_median_m": round(float(np.median(cmin)), 3), "flights_inside_drone_radius": int((cmin < prm.radius).sum()),
             "flights_through_a_cylinder": int((cmin < 0).sum()), "x_final_mean_m": round(float(pos[:, :, -1, 0].mean()), 2)}
    if kf:   # what the maps hold at the end of the flights (a map that stands empty would make the sweep and the merges free)
        ms = [pl.kfmap_state(i) for i in range(nslots)]
        nk = np.concatenate([m["n_keyframes"] for m in ms]); nq = np.concatenate([m["n_query_frames"] for m in ms])
        stats["keyframes_at_end_mean_max"] = [round(float(nk.mean()), 2), int(nk.max())]
        stats["query_frames_at_end_mean_max"] = [round(float(nq.mean()), 2), int(nq.max())]
        stats["outliers_of_the_last_sweep_mean"] = round(float(np.concatenate([m["last_outliers"] for m in ms]).mean()), 1)
    parity = None
    if not args.no_cpu_baseline and not args.no_parity:
        # the same flights on the CPU oracle: a sample of batch 0, on the frames the GPU saw
        from tests import _flight
        nf = min(S, 16)
        cl = np.stack([frames[0][t][0][:nf].cpu().numpy() for t in range(P)], axis=1)     # [nf, P, n, 3]
        ed = np.stack([frames[0][t][1][:nf].cpu().numpy() for t in range(P)], axis=1)
        t0 = time.perf_counter()
        o = _flight.oracle_flights_on_frames(cl, ed, x0[0, :nf], ref0[0, :nf], args.T, args.K,
                                             keyframes=dict(kf, cam=(32.0, 32.0, 32.0, 24.0, 100.0, 64, 48)) if kf else None)
        t_cpu = time.perf_counter() - t0
        g = dict(x=np.concatenate([pos[0, :nf], np.zeros((nf, P + 1, 7))], axis=2), flags=fl[0, :nf], u=ug[0, :nf])
        cmp = _flight.compare(g, o, pos_tol=1e-6)
        parity = {"flights_vs_cpu_oracle": {"flights": nf, "periods": P, "separated": cmp["separated"],
                                            "dpos_max_while_flags_agree_m": cmp["dpos_max_while_together"],
                                            "dpos_final_max_of_separated_m": cmp["dpos_final_max_separated"],
                                            "ok": bool(cmp["dpos_max_while_together"] <= 1e-6 and cmp["separated"] <= 1 and cmp["dpos_final_max_separated"] <= 0.05),   # census: 1.2 % of flights separate over 150 periods and end within 1.3 cm of the oracle's (was nf // 8, unbounded)
                                            "cpu_oracle_steps_per_s_all_cores": round(nf * P / t_cpu, 1), "cores": _flight.usable_cores(),
                                            "note": "same frames, same start; a flight separates when its flags differ in some period "
                                                    "(another branch at a rounding-level tie); tests/test_flight_gpu.py is the "
                                                    "64-flight x 100-period version of this check"}}
    steps = B * P
    value = S * steps / dt
    step_bytes = alg_bytes_per_step(n, ne, N, prm.K)
    line = {"metric": f"MPC steps/sec ({n // 1000}k-pt cloud, N={N}, {prm.K} obstacle constraints) -- closed-loop flights, warm-started",
            "value": round(value, 1), "unit": "MPC steps/s", "n_gpus": 1, "steps": steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * dt / steps, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64" if args.precision == 64 else "f32", "data": "synthetic",
            "config": {"workload": f"closed-loop flights: {B} batches x {S} flights x {P} control periods; per period and flight a fresh "
                                   f"{n}-pt frame + {ne}-pt edge cloud (both index builds), GetInitPath, warm start kept "
                                   f"(mNlpW0), <= {prm.max_iter} re-plan passes, PubCmd / PubSlowDownCmd, vehicle = the MPC's model; "
                                   "SECONDARY to the cold-start headline (default workload)",
                       "scenes_per_gpu": S, "points": n, "horizon": N, "K": prm.K, "batches": B, "periods": P, "streams_in_flight": nslots,
                       "steps_per_launch": gang, "queue_depth_per_slot": args.queue_depth if args.queue_depth > 0 else 2,
                       "distinct_world_sets": W, "world_length_m": world_len, "distinct_frames_bytes": int(W * P * S * 12 * (n + ne)),
                       "frame_generation_s_untimed": round(t_gen, 2), "host_submit_ms_per_step": round(1e3 * t_sub / steps, 4),
                       "orchestration": "amk_pipeline TASK mode (prologue / epilogue kernels); the vehicle's kernels are queued on the "
                                        "slot's own stream behind the step: no host synchronisation inside the loop"},
            "flight": stats,
            "roofline_whole_step": {"alg_bytes_per_scene_step": step_bytes, "achieved": round(value * step_bytes / 1e9, 2), "unit": "GB/s",
                                    "frac": round(value * step_bytes / 1e9 / HBM_PEAK_GBS, 5),
                                    "note": "SURVEY 8(d) bytes per step x steps/s over the HBM peak: with ~1 warm solve of a few "
                                            "iterations per step the index builds (HBM-bound) are most of a period"},
            "parity": parity}
    print(json.dumps(line), flush=True)
    pl.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--scenes", type=int, default=256, help="scenes per GPU per step (BASELINE configs[2])")
    ap.add_argument("--config", default=None, choices=("yaml",),
                    help="yaml: the reference's own configuration (AM/config/mpc_parameters.yaml: 640 x 480 / 10 sensor = 3072-point "
                         "frames, T = 1.0 -> N = 30, nearest_point_num = 3; with --workload flight --keyframes 100 its default regime) "
                         "-- shorthand for --points 3072 --T 1.0 --K 3, 16 slots x 4 frames per launch, 120 periods unless given")
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--T", type=float, default=0.66)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--streams", type=int, default=10,
                    help="pipeline slots = independent launches in flight (each on its own HIP stream with its own handles)")
    ap.add_argument("--gang", type=int, default=0,
                    help="steps (frames) that share one set of launches on a slot (amk_pipeline_config.gang): streams x gang steps "
                         "are in flight or staged; 0 = 4, flight workload 8.  10 x 4 against the 20 x 1 of rounds 2-3a, same box: 519 k "
                         "vs 466 k scene-steps/s steady, 410-422 k vs 378 k over the driver's 20 steps; the warm-started flights, whose "
                         "launches are shorter and end with longer tails, want more frames in flight: 10 x 8 1.24 M against 1.12 M (10 x 4), "
                         "same box, 52 periods")
    ap.add_argument("--queue-depth", type=int, default=0, help="steps queued per pipeline slot (0: 1; flight workload: 2)")
    ap.add_argument("--precision", type=int, default=64, choices=(32, 64),
                    help="arithmetic of the MPC solve (64 = the reference's; 32 = BASELINE configs[4] variant, not the headline)")
    ap.add_argument("--ipm-max-iter", type=int, default=None, help="iteration cap of the solve (default: the library's)")
    ap.add_argument("--solve-budget", type=int, default=None,
                    help="interior-point iterations per solve launch of a step's budgeted rounds (amk_mpc_set_solve_budget; 0: plain "
                         "schedule; default: the shipped setting)")
    ap.add_argument("--budget-rounds", type=int, default=0, help="budgeted rounds of a step (0: mpc_max_iter - 1)")
    ap.add_argument("--tie-order", type=int, default=0, choices=(0, 1),
                    help="1: amk_kd_set_tie_order(AMK_TIES_NANOFLANN) on both indices (not the headline configuration)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-parity", action="store_true")
    ap.add_argument("--steady-steps", type=int, default=1024,
                    help="extra untimed-by-contract run reported as value_steady_state when --steps is smaller")
    ap.add_argument("--breakdown", action="store_true", help="extra untimed pass with every kernel class timed")
    ap.add_argument("--workload", default="cold", choices=("cold", "flight"),
                    help="cold (the headline: fresh frame + zero warm start every step) or flight (closed loop: every step is one "
                         "control period of a batch of flights -- fresh frame, GetInitPath, warm start, command, vehicle)")
    ap.add_argument("--keyframes", type=int, default=0,
                    help="flight workload: max_frame_count of the keyframe map every slot keeps (amk_pipeline_config.keyframes; 0: "
                         "single-frame map).  The reference's default regime (FrameKDMap.cpp:29-32); mind the pool: (N + 2) x "
                         "gang x scenes index slots per pipeline slot")
    ap.add_argument("--frames-behind", type=float, default=None,
                    help="flight workload: how far behind the nominal position a frame's points reach, metres (default 6; with "
                         "--keyframes -1: the frame starts 1 m ahead, as a forward-looking sensor's does)")
    ap.add_argument("--periods", type=int, default=0, help="flight workload: control periods per flight (0: from --steps)")
    ap.add_argument("--inputs", default="device", choices=("device", "host"),
                    help="host: every step's clouds, edge clouds and odometry start in pinned host memory and cross PCIe inside the "
                         "timed region (the PCIe-inclusive rate DESIGN.md quotes; never the headline)")
    ap.add_argument("--dry-run", action="store_true",
                    help="launch path only (CPU, gloo): ranks rendezvous, partition the scenes, exchange a gather-shaped buffer and "
                         "rank 0 prints a JSON line without a value -- what tests/test_bench_launch.py runs without a GPU")
    ap.add_argument("--full", action="store_true",
                    help="default workload: also measure and check what the headline does not need -- the HBM copy probe's figure, the "
                         "per-kernel HIP-event timings in the timed region, the steady-state run (--steady-steps), single-launch "
                         "kernel times, the roofline blocks, the fixture parity gate, the CPU baseline and the check of the timed "
                         "scenes against the CPU oracle (--no-cpu-baseline / --no-parity leave those out)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="default workload: after the timed steps, write what the last timed step returned to its caller (u, "
                         "x0array, flags, ref_path of its S scenes) as DIR/<name>.npy, float64, at most 64 MB in all")
    args = ap.parse_args()
    if args.dump_outputs and (args.workload != "cold" or args.dry_run):
        ap.error("--dump-outputs: the default (cold) workload only")
    if args.config == "yaml":
        args.points, args.T, args.K = 3072, 1.0, 3
        if args.workload == "flight":
            if "--streams" not in sys.argv: args.streams = 16
            if "--gang" not in sys.argv: args.gang = 4
            if args.periods == 0 and args.steps == 2048: args.periods = 120

    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(self_launch(args.gpus))
    if args.dry_run:
        return dry_run(args)
    if args.workload == "flight":
        return flight_main(args)

    # one hardware queue per in-flight step (ROCm defaults to 4 and multiplexes streams onto them: two streams on one
    # queue serialise); measured on MI355X: 4 queues 280k, 8 -> 315k, 24 -> 390k steps/s at 16 streams
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "32")
    import numpy as np
    import torch
    from avoid_mpc_amd import capi, fsm, synth
    from avoid_mpc_amd.host import Pipeline, Shard, step_batch

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:   # a launcher's WORLD_SIZE wins over the flag (it decided how many ranks exist)
        if rank == 0:
            print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: running on {world} rank(s)", file=sys.stderr)
        args.gpus = world
    launched = "RANK" in os.environ and "MASTER_ADDR" in os.environ   # under torch.distributed.run (also with 1 rank)
    dist = None
    if world > 1 or launched:
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    else:
        torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    lib = capi.load()
    # SURVEY 8(d) / BASELINE.md 3: the achievable HBM rate beside the vendor peak, before the pipeline's buffers exist
    # Runs in a plain run too, unreported: it is also the device warm-up every headline of this benchmark was measured after
    # (without it the timed region is 2.5 % slower, same box, 2000 steps)
    hbm_measured = measured_hbm_peak(torch, lib) if rank == 0 else None
    collective = dist is not None   # the exchange step runs whenever a process group exists (RCCL also at world 1)

    prm = synth.MpcParams(T=args.T, K=args.K)
    S, n, ne, N = args.scenes, args.points, args.points // 10, prm.N
    nslots = max(1, args.streams)
    gang = args.gang if args.gang > 0 else 4
    nframes = nslots * gang   # distinct frame sets: every step in flight (or staged) owns its inputs

    class Frames:
        """The inputs one in-flight step owns: its frames (obstacle + edge clouds of S scenes) and odometry.  Consecutive
        steps are independent frames, so several are kept in flight (amk_pipeline: one slot = HIP stream + dual KD indices +
        MPC batch + outputs); while one step sits in its latency-bound solve another streams its clouds."""

        def __init__(self, i):
            seed = 100000 + (rank * nframes + i) * S
            self.clouds, self.edges = synth.make_clouds_torch(n, S, seed, dev)
            sq = np.zeros((S, prm.max_iter, 10)); ref0 = np.zeros((S, N, 10)); posx = np.zeros(S)
            for s in range(S):
                pos, vel, acc, yaw = synth.make_odom(seed + s, prm)
                sq[s] = fsm.state_quads(pos, vel, acc, yaw, prm.decay, prm.max_iter)
                ref0[s] = synth.make_ref_path(pos, prm); posx[s] = pos[0]
            self.sq_h, self.ref0_h, self.posx_h = sq, ref0, posx
            self.sq = torch.from_numpy(sq).to(dev); self.ref0 = torch.from_numpy(ref0).to(dev)
            self.posx = torch.from_numpy(posx).to(dev)
            self.last_row = 0
            self.ticket = None
            if args.inputs == "host":   # the step's inputs as a host application holds them: pinned, copied every step
                self.host = [t.cpu().pin_memory() for t in (self.clouds, self.edges, self.sq, self.posx, self.ref0)]

    # the C ABI's pipeline (include/avoid_mpc_amd.h: amk_pipeline_*): what a C++ host would call; bench.py only feeds it.
    # Steps queued per slot before submit() blocks: 1 (+1-2 % against deeper queues).  Rounds 2-3 used 8 whenever a process
    # group existed because a live RCCL communicator cost 35 % at depth 1 -- with 20 slots.  Cause (round 4,
    # tools/experiments/rccl_presence2.py): hardware queues.  A communicator brings its own streams; with 20 pipeline streams the
    # process then holds more streams than it gets hardware queues, the runtime maps two streams onto one queue and they
    # serialise -- the same loss as GPU_MAX_HW_QUEUES=16 without any communicator (338 k vs 334 k steps/s; <= 16 slots: no loss).
    # The shipped 10 slots x gang 4 holds 10 streams and is unaffected (558.9 k without, 558.3 k with a communicator, depth 1).
    qdepth = args.queue_depth if args.queue_depth > 0 else 1
    pl = Pipeline(nslots, S, n, ne, prm, queue_depth=qdepth, gang=gang)
    for i in range(nslots):
        pl.kd(i, 0).set_tie_order(args.tie_order); pl.kd(i, 1).set_tie_order(args.tie_order)
        pl.mpc(i).set_precision(args.precision)
        if args.ipm_max_iter is not None:
            pl.mpc(i).set_solver_options(1e-4, args.ipm_max_iter)
        if args.solve_budget is not None:
            pl.mpc(i).set_solve_budget(args.solve_budget, args.budget_rounds)
    slots = [Frames(i) for i in range(nframes)]
    run_steady = args.full and args.steps < args.steady_steps   # the timed region is then mostly ramp-up / drain of the slots
    max_rows = max(args.steps, args.steady_steps if run_steady else 0, nframes, args.warmup, 64)
    u_sweep = torch.zeros((max_rows, S, 4), dtype=torch.float64, device=dev)   # the sweep's controls, one row per step
    sh = None
    rccl_info = None

    def gather_or_die(what, timeout_s=float(os.environ.get("AMK_BENCH_GATHER_TIMEOUT_S", "180"))):
        """amk_shard_wait behind every exchange step: a hung collective ends the rank with a message instead of the whole run
        with the launcher's timeout."""
        rc = sh.wait(timeout_s=timeout_s)
        if rc == capi.AMK_OK:
            return
        msg = (f"bench.py: rank {rank}/{world}: {what} did not finish within {timeout_s:.0f} s (amk_shard_wait -> {rc}); RCCL bound: "
               f"{rccl_info}; re-run with NCCL_DEBUG=INFO NCCL_DEBUG_SUBSYS=INIT,COLL")
        print(msg, file=sys.stderr, flush=True)
        write_rank_file(rank, {"rank": rank, "world": world, "error": msg})
        os._exit(3)

    if collective:   # RCCL through the library's own binding (amk_shard_*); torch.distributed only carries the 128-byte id
        ids = [Shard.unique_id() if rank == 0 else None]
        dist.broadcast_object_list(ids, src=0)
        sh = Shard(rank, world, ids[0])
        rccl_info = rccl_report(torch)
        write_rank_file(rank, {"rank": rank, "world": world, "device": torch.cuda.get_device_name(dev), "local_rank": local_rank,
                               "rccl": rccl_info, "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "stage": "communicator created"})
        warm = torch.zeros((world, 8), dtype=torch.float64, device=dev)
        sh.gather(warm[rank].clone(), warm)   # RCCL sets a communicator's channels up at its first collective: not in the clock
        gather_or_die("the communicator's first collective")
    step_no = [0]
    copy_stream = torch.cuda.Stream(device=dev) if args.inputs == "host" else None
    # diagnostics only (tools/experiments): AMK_BENCH_SKIP=build|step leaves that half out of every step -- the printed
    # value is then NOT the metric (the JSON line says so)
    DIAG_SKIP = os.environ.get("AMK_BENCH_SKIP", "")
    assert not (DIAG_SKIP in ("build", "step") and gang > 1), "AMK_BENCH_SKIP=build|step drives the slots' handles directly: --gang 1"
    diag_streams = [torch.cuda.ExternalStream(lib.amk_pipeline_stream(pl.h, i), device=dev) for i in range(nslots)] \
        if DIAG_SKIP in ("build", "step") else None
    diag_ref = [fr.ref0.clone() for fr in slots] if diag_streams else None
    diag_x0 = torch.empty((S, N, 14), dtype=torch.float64, device=dev) if diag_streams else None
    diag_fl = torch.empty((S, 4), dtype=torch.int32, device=dev) if diag_streams else None

    def one_step(row, frames=None):
        """Submits one step (a fresh frame of S scenes); returns its ticket (= slot when gang == 1)."""
        i = step_no[0] % nframes
        fr = slots[i if frames is None else frames]
        step_no[0] += 1
        fr.last_row = row
        if diag_streams is None and args.inputs == "host":
            if fr.ticket is not None:
                pl.wait(fr.ticket)   # the launch that last read this frame set's device buffers
            with torch.cuda.stream(copy_stream):
                for dst, src in zip((fr.clouds, fr.edges, fr.sq, fr.posx, fr.ref0), fr.host):
                    dst.copy_(src, non_blocking=True)
                fr.ticket = pl.submit(fr.clouds, fr.edges, fr.sq, fr.posx, fr.ref0, u_out=u_sweep[row], order_after_current_stream=True)
            return fr.ticket
        if diag_streams is None:
            return pl.submit(fr.clouds, fr.edges, fr.sq, fr.posx, fr.ref0, u_out=u_sweep[row], order_after_current_stream=False)
        st = diag_streams[i]
        with torch.cuda.stream(st):
            diag_ref[i].copy_(fr.ref0, non_blocking=True)
            pl.mpc(i).reset_warm_start(st)
            if DIAG_SKIP != "build" or step_no[0] <= nslots:
                pl.kd(i, 0).build(fr.clouds, stream=st); pl.kd(i, 1).build(fr.edges, stream=st)
            if DIAG_SKIP != "step":
                step_batch(pl.kd(i, 0), pl.kd(i, 1), pl.mpc(i), prm, fr.sq, fr.posx, diag_ref[i], stream=st,
                           out=dict(u=u_sweep[row], x0array=diag_x0, flags=diag_fl))

    def barrier():
        if diag_streams is None:
            pl.drain()   # (launches a gang that the steps so far left partly filled)
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(steps):
        t0 = time.perf_counter()
        ticket = None
        for j in range(steps):
            ticket = one_step(j)
        t_enq = time.perf_counter() - t0   # host time in submit(): enqueue + back-pressure waits on busy slots
        if diag_streams is None:
            pl.drain()
        t_drain = time.perf_counter() - t0
        if collective:   # the ONE exchange step of the sweep: every rank's controls to every rank (ncclAllGather)
            write_rank_file(rank, {"rank": rank, "world": world, "device": torch.cuda.get_device_name(dev), "steps": steps,
                                   "local_steps_per_s": S * steps / t_drain, "drain_s": t_drain, "rccl": rccl_info,
                                   "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "stage": "before the gather"})
            tg = time.perf_counter()
            sh.gather(u_sweep[:steps], u_gather(steps))
            gather_or_die("the sweep's gather")
            torch.cuda.synchronize()
            phases["gather_ms_this_rank"] = 1e3 * (time.perf_counter() - tg)
        t_gather = time.perf_counter() - t0
        barrier()
        t_all = time.perf_counter() - t0
        phases["submit_s"], phases["drain_s"], phases["gather_s"], phases["barrier_s"] = t_enq, t_drain - t_enq, t_gather - t_drain, t_all - t_gather
        return t_all, t_enq, ticket

    gather_bufs = {}
    phases = {}

    def u_gather(steps):
        if steps not in gather_bufs:
            gather_bufs[steps] = torch.empty((world, steps, S, 4), dtype=torch.float64, device=dev)
        return gather_bufs[steps]

    def max_over_ranks(seconds):
        if sh is None:
            return float(seconds)
        t = torch.tensor([seconds], dtype=torch.float64, device=dev)
        sh.max(t)
        gather_or_die("the max over ranks")
        torch.cuda.synchronize()
        return float(t.item())

    for j in range(nframes):               # untimed priming: every slot allocates its workspace once
        one_step(j)
    barrier()
    if DIAG_SKIP in ("knn", "plan", "solve", "knn+plan"):   # diagnostics: kernel classes left out of the step from here on
        lib.amk__diag_skip({"knn": 1, "plan": 2, "solve": 4, "knn+plan": 3}[DIAG_SKIP])
    for j in range(args.warmup):
        one_step(j)
    barrier()
    for k_ in (args.steps, args.steady_steps) if run_steady else (args.steps,):   # the gather's receive buffers exist before the clock starts
        if collective:
            u_gather(k_)
    if args.full:
        lib.amk__timing_enable(1)          # HIP events around the solve and build kernels, on their launch stream
    dt, t_enq, last_ticket = timed(args.steps)
    timed_phases = {k: round(v, 5) for k, v in phases.items()}
    if args.full:
        ms = (C.c_double * 8)(); cnt = (C.c_int * 8)()
        capi.check(lib.amk__timing_collect(ms, cnt), "timing")
        lib.amk__timing_enable(0)
    if args.dump_outputs and rank == 0:   # before anything else runs on the last step's slot
        if last_ticket is None:
            sys.exit("bench.py: --dump-outputs needs the pipeline's outputs (not with AMK_BENCH_SKIP=build|step)")
        dump_outputs(args.dump_outputs, pl.outputs(last_ticket))
    dt = max_over_ranks(dt)

    flags = np.concatenate([pl.outputs(t)["flags"] for t in range(nframes)]) if diag_streams is None else np.zeros((1, 4), np.int32)
    solves = float(flags[:, 1].mean()); ipm_iters = float(flags[:, 3].mean())
    steady = None
    if run_steady:
        dts, _, _ = timed(args.steady_steps)
        dts = max_over_ranks(dts)
        steady = S * world * args.steady_steps / dts
    # The kernels' OWN durations: a pass with ONE step on the chip at a time (submit, wait, submit, ...), every kernel class
    # bracketed by HIP events on its launch stream.  Nothing else is resident, so submit-to-complete is the kernel's duration
    # (+ a few us of launch latency) -- the number `rocprofv3 --kernel-trace` of `bench.py --streams 1` reports
    # (profiles/r04_kernel_stats_streams1.md; same scenes: the frames of in-flight slot 0).  In the timed region above the same events also contain the wait for CUs the
    # other launches in flight occupy, which is why that figure is reported separately as in_flight_submit_to_complete_ms.
    lone = None
    ticket_of_frames0 = None
    if rank == 0 and args.full and diag_streams is None:
        lib.amk__timing_enable(2)
        reps = 6   # always the frames of in-flight slot 0 = the scenes of `bench.py --streams 1` (the committed rocprof trace)
        for j in range(reps):   # one LAUNCH at a time: the `gang` steps that share it (frames 0 .. gang-1), then wait
            for g in range(gang):
                t = one_step(j * gang + g, frames=g)
                if g == 0:
                    ticket_of_frames0 = t   # where the slot keeps the flags of frame set 0 (the CPU check below reads them)
            pl.wait(t)
        torch.cuda.synchronize()
        ms1 = (C.c_double * 8)(); cnt1 = (C.c_int * 8)()
        capi.check(lib.amk__timing_collect(ms1, cnt1), "timing")
        lib.amk__timing_enable(0)
        lone = {KCLASS[i]: {"avg_launch_us": round(1e3 * ms1[i] / cnt1[i], 2), "launches_per_step": cnt1[i] / (reps * gang)}
                for i in range(8) if cnt1[i] and KCLASS[i]}
    chk = None   # frame set 0's controls and flags for the CPU check, taken before anything else runs on that slot
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline and diag_streams is None:
        if ticket_of_frames0 is None:   # (no single-launch pass ran: run frame set 0 once more)
            ticket_of_frames0 = one_step(0, frames=0)
        pl.wait(ticket_of_frames0)
        torch.cuda.synchronize()
        chk = (u_sweep[slots[0].last_row].cpu().numpy().copy(), pl.outputs(ticket_of_frames0)["flags"].copy())
    breakdown = None
    if args.breakdown and world == 1:   # (extra steps on one rank would unbalance the collectives)
        lib.amk__timing_enable(2)
        reps = max(3, min(args.steps, 64))
        for j in range(reps):
            one_step(j)
        torch.cuda.synchronize()
        ms2 = (C.c_double * 8)(); cnt2 = (C.c_int * 8)()
        capi.check(lib.amk__timing_collect(ms2, cnt2), "timing")
        lib.amk__timing_enable(0)
        breakdown = {KCLASS[i]: {"ms_per_step": round(ms2[i] / reps, 4), "launches_per_step": cnt2[i] / reps}
                     for i in range(8) if cnt2[i]}

    parity, cpu = None, None
    if rank == 0 and args.full and not args.no_parity:
        parity = {"fixtures": fixture_parity(torch, args.precision)}
    if chk is not None:
        sl = slots[0]
        torch.cuda.synchronize()
        cl, ed = sl.clouds.cpu().numpy(), sl.edges.cpu().numpy()
        scenes = [(cl[s], ed[s], sl.sq_h[s], float(sl.posx_h[s]), sl.ref0_h[s]) for s in range(S)]
        cpu, check = cpu_baseline_and_check(scenes, args.T, args.K, chk[0], chk[1])
        parity = dict(parity or {}, timed_workload_vs_cpu_oracle=check)

    if rank == 0:
        total_scenes = S * world * args.steps
        value = total_scenes / dt
        line = {
            "metric": f"MPC steps/sec ({n // 1000}k-pt cloud, N={N}, {prm.K} obstacle constraints)",
            "value": round(value, 1), "unit": "MPC steps/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1e3 * dt / args.steps, 4), "higher_is_better": True,
            **({"INVALID_diagnostic_run": "AMK_BENCH_SKIP=" + DIAG_SKIP} if DIAG_SKIP else {}),
            **({"NOT_THE_HEADLINE_pcie_inclusive": f"--inputs host: {12 * (n + ne) * S + 8 * S * (10 * prm.max_iter + 1 + 10 * N)} bytes per "
                                                   "step cross PCIe from pinned host memory inside the timed region"}
               if args.inputs == "host" else {}),
            "scaling": "weak", "vs_baseline": None, "dtype": "f64" if args.precision == 64 else "f32", "data": "synthetic",
            "config": {"workload": f"BASELINE configs[1] batched as configs[2]: {S} scenes/GPU x ({n}-pt obstacle "
                                   f"cloud + {ne}-pt edge cloud, N={N}, K={prm.K}), fresh frame + zero warm start "
                                   f"every step, every in-flight step on its own frames", "scenes_per_gpu": S, "points": n,
                       "horizon": N, "K": prm.K, "mpc_max_iter": prm.max_iter,
                       "ipm_max_iter": args.ipm_max_iter if args.ipm_max_iter is not None else capi.AMK_MPC_DEFAULT_MAX_ITER,
                       "ipm_tol": 1e-4, "solves_per_step": round(solves, 3), "ipm_iters_per_step": round(ipm_iters, 2),
                       "streams_in_flight": nslots, "steps_per_launch": gang, "scenes_per_launch": S * gang,
                       "distinct_frames_bytes": int(nframes * S * 12 * (n + ne)),
                       "hw_queues": int(os.environ["GPU_MAX_HW_QUEUES"]),
                       "tie_order": "nanoflann" if args.tie_order else "lowest index",
                       "host_submit_ms_per_step": round(1e3 * t_enq / args.steps, 4), "timed_region_phases_s": timed_phases,
                       "parallelism": (f"scenes sharded over {world} GPU(s); one ncclAllGather (amk_shard_gather) of the sweep's "
                                       f"controls, {args.steps} x {S} x 4 doubles per rank, inside the timed region" if collective
                                       else "single GPU, no process group"),
                       "orchestration": f"amk_pipeline_* (C ABI): submit() per step, drain() at the end; {nslots} slots x gang {gang} "
                                        f"(= {gang} consecutive steps share one set of launches of {S * gang} scenes)",
                       "queue_depth_per_slot": qdepth,
                       "rccl": rccl_info if collective else "no process group (single GPU, plain run): RCCL not used",
                       "multi_gpu_measured": "no N > 1 line has been measured by this project (no multi-GPU node was available to it "
                                             "in any round); per-rank files: gpurun_out/bench_ranks/"},
        }
        if args.full:
            step_bytes = alg_bytes_per_step(n, ne, N, prm.K)
            alg_launch = solve_alg_bytes(N, prm.K) * S * gang
            build_alg = 28 * S * gang * (n + ne)            # 12 B read + 16 B written per point; ONE launch builds the obstacle and the edge index (amk_kd_build_pair)
            inflight_solve_ms = ms[5] / max(cnt[5], 1)
            inflight_build_ms = ms[7] / max(cnt[7], 1)
            solve_us = lone["mpc_solve_kernel"]["avg_launch_us"] if lone else None
            build_us = lone["kd_build_kernel"]["avg_launch_us"] if lone else None
            prof = {}
            for key, fname in (("traffic", "pmc_traffic"), ("issue", "pmc_solve_issue"), ("kt1", "kernel_stats_streams1"),
                               ("kt20", "kernel_stats")):
                fpath = os.path.join(ROOT, "profiles", f"{PROFILE_TAG}_{fname}.json")
                if os.path.exists(fpath):
                    prof[key] = json.load(open(fpath))
            traffic = build_traffic = traffic_src = None
            tj = prof.get("traffic")
            if tj:   # PMC passes cannot run inside this process: reuse the committed rocprofv3 result of the same command
                m = tj.get("_meta", {})
                if (m.get("scenes_per_gpu"), m.get("gang", 1), m.get("points"), m.get("horizon"), m.get("K")) == (S, gang, n, N, prm.K):
                    kk = tj["kernels"].get(f"mpc_solve_kernel<{N}>"); kb = tj["kernels"].get("kd_build_kernel")
                    traffic = round(kk["hbm_bytes_per_launch_x2"]) if kk else None
                    build_traffic = round(kb["hbm_bytes_per_launch_x2"]) if kb else None
                    traffic_src = f"profiles/{PROFILE_TAG}_pmc_traffic.json (rocprofv3 FETCH_SIZE x2 + WRITE_SIZE, KiB, separate passes)"

            def rocprof_us(which, kernel):
                k = (prof.get(which) or {}).get("kernels", {}).get(kernel)
                return k["avg_us"] if k else None
            # what bounds the dominant kernel (SQ counters of the committed profile): VALU issue slots.  Live part: how many
            # solves the timed region ran per second; committed part: VALU instructions per wave-solve (a property of the
            # kernel on this workload, profiles/r04_pmc_solve_issue.json), 4 issue cycles each on one of 1024 SIMDs.
            issue = prof.get("issue")
            valu_per_solve = issue["valu_instructions_per_wave_solve"] if issue else None
            solves_per_s = value * solves
            # issue cycles one VALU instruction of this kernel holds a SIMD for, MEASURED (SQ_ACTIVE_INST_VALU / SQ_INSTS_VALU of the
            # committed profile: 4.27, the fp64 share of the mix; a wave64 fp32 instruction would be 4 on paper, an fp64 FMA 4+)
            valu_cpi = (issue["frac_of_wave_time_issuing_valu"] * issue["wave_cycles_per_wave"] / valu_per_solve) if valu_per_solve else None
            valu_frac_timed = (solves_per_s * valu_per_solve * valu_cpi / (N_CU * N_SIMD * CLOCK_GHZ * 1e9)) if valu_per_solve else None
            hbm_8d_gbs = value / max(world, 1) * step_bytes / 1e9      # per GPU: SURVEY 8(d)'s bytes per scene-step x this GPU's steps/s
            hbm = lambda nbytes, us: None if not us else round(nbytes / (us * 1e-6) / 1e9, 2)
            frac = lambda gbs: None if gbs is None else round(gbs / HBM_PEAK_GBS, 6)
            fracm = lambda gbs: None if gbs is None or not hbm_measured else round(gbs / hbm_measured, 6)   # against the measured copy rate
            roof_solve_hbm = {
                "bound": "hbm", "kernel": f"mpc_solve_kernel<{N}>", "alg_bytes_per_launch": alg_launch,
                "avg_launch_us": solve_us, "achieved": hbm(alg_launch, solve_us), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": frac(hbm(alg_launch, solve_us)), "frac_of_measured_copy": fracm(hbm(alg_launch, solve_us)),
                "traffic": traffic, "traffic_source": traffic_src,
                "rocprof_avg_us_same_command": rocprof_us("kt1", f"mpc_solve_kernel<{N}>"),
                "in_flight_submit_to_complete_ms": round(inflight_solve_ms, 4), "in_flight_launches": cnt[5],
                "in_flight_rocprof_avg_us": rocprof_us("kt20", f"mpc_solve_kernel<{N}>"),
                "note": "HBM view of the dominant kernel, kept because the contract asks for bytes / launch duration: the kernel "
                        "moves 4 MB per launch and is nowhere near this roofline by construction (a serial interior-point solve "
                        "per wavefront).  avg_launch_us: HIP events on the launch stream with one step on the chip at a time "
                        "(= rocprofv3's kernel duration of `bench.py --streams 1`, profiles/); in_flight_*: the same events in "
                        "the timed region, where they also contain the wait for CUs held by the other steps in flight"}
            line.update({
                "value_steady_state": round(steady, 1) if steady else None,
                "value_steady_state_steps": args.steady_steps if steady else None,
                "roofline": {"bound": "hbm",
                             "what": "SURVEY 8(d)'s ruler for the WHOLE step: algorithmic bytes per scene-step (every input read once, every "
                                     "output written once) x steps/s of this GPU, against the vendor's HBM peak.  The path is not HBM-bound: its "
                                     "dominant kernel is a serial interior-point solve per wavefront (frac_valu_issue, dominant_kernel below)",
                             "alg_bytes_per_scene_step": step_bytes,
                             "achieved": round(hbm_8d_gbs, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": round(hbm_8d_gbs / HBM_PEAK_GBS, 5), "frac_hbm_8d": round(hbm_8d_gbs / HBM_PEAK_GBS, 5),
                             "frac_of_measured_copy": fracm(hbm_8d_gbs),
                             "frac_valu_issue": None if valu_frac_timed is None else round(valu_frac_timed, 4),
                             "valu_issue_cycles_per_instruction_measured": None if valu_cpi is None else round(valu_cpi, 3),
                             "kernel": f"mpc_solve_kernel<{N}>",
                             "traffic": traffic,
                             "dominant_kernel": {
                                 "kernel": f"mpc_solve_kernel<{N}>", "bound": "valu-issue / dependent fp64 + LDS latency at 2 waves per SIMD (neither HBM nor MFMA)",
                                 "hbm_alg_bytes_per_launch": alg_launch, "avg_launch_us": solve_us,
                                 "hbm_achieved_gbs": hbm(alg_launch, solve_us), "hbm_frac": frac(hbm(alg_launch, solve_us)),
                                 "hbm_traffic_per_launch": traffic,
                                 "valu_issue_achieved_gcycles_per_s": None if valu_frac_timed is None else round(valu_frac_timed * N_CU * N_SIMD * CLOCK_GHZ, 1),
                                 "valu_issue_peak_gcycles_per_s": round(N_CU * N_SIMD * CLOCK_GHZ, 1),
                                 "frac_valu_issue": None if valu_frac_timed is None else round(valu_frac_timed, 4),
                                 "frac_valu_issue_at_saturation_solves_only": issue.get("valu_issue_util_at_saturation") if issue else None,
                                 "lds_array_frac_at_saturation": issue.get("lds_array_util_at_saturation (conflict level of the lone wave)") if issue else None,
                                 "valu_instructions_per_wave_solve": valu_per_solve, "solves_per_s_timed_region": round(solves_per_s, 1)},
                             "note": "frac = frac_hbm_8d = steps/s x alg_bytes_per_scene_step / 8 TB/s.  frac_valu_issue = (solves/s of the timed "
                                     "region) x (VALU instructions per wave-solve, SQ_INSTS_VALU of the committed profile) x (measured issue cycles "
                                     "per VALU instruction, SQ_ACTIVE_INST_VALU / SQ_INSTS_VALU) / (1024 SIMDs x 2.4 GHz): the share of the chip's "
                                     "VALU issue slots the dominant kernel fills while the builds and searches of the other steps share the CUs; "
                                     "frac_valu_issue_at_saturation_solves_only is the same quantity with nothing but solves resident "
                                     "(tools/experiments/ms_parts.py).  What stops it below 1: two waves per SIMD (180 VGPRs and 17.8 KB of LDS per scene; a third wave was measured to buy nothing, DESIGN 5: "
                                     "per scene) cannot cover ~32-cycle dependent fp64 issue and LDS round trips "
                                     f"(profiles/{PROFILE_TAG}_pmc_solve_issue.md, DESIGN.md section 5)"},
                "roofline_hbm": roof_solve_hbm,
                "roofline_solve_issue": issue,
                "roofline_kd_build": {"bound": "hbm", "kernel": "kd_build_kernel (one launch: obstacle + edge index of every scene)",
                                      "alg_bytes_per_launch": build_alg, "avg_launch_us": build_us,
                                      "achieved": hbm(build_alg, build_us), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                      "frac": frac(hbm(build_alg, build_us)), "frac_of_measured_copy": fracm(hbm(build_alg, build_us)),
                                      "traffic": build_traffic,
                                      "alg_bytes_per_launch_survey_8d": 12 * S * gang * (n + ne),
                                      "frac_survey_8d": frac(hbm(12 * S * gang * (n + ne), build_us)),
                                      "frac_survey_8d_of_measured_copy": fracm(hbm(12 * S * gang * (n + ne), build_us)),
                                      "rocprof_avg_us_same_command": rocprof_us("kt1", "kd_build_kernel"),
                                      "in_flight_submit_to_complete_ms": round(inflight_build_ms, 4), "in_flight_launches": cnt[7],
                                      "in_flight_rocprof_avg_us": rocprof_us("kt20", "kd_build_kernel"),
                                      "note": "the HBM-heavy kernel: 28 B per point (12 read, 16 written as an (x, y, z, index) bucket "
                                              "record), both trees of a frame in one launch (grid.y = tree); avg_launch_us with one step "
                                              "on the chip at a time.  frac_survey_8d is the same duration against SURVEY 8(d)'s own accounting "
                                              "(inputs read once: 12 B per point; the survey's K1 budgeted a 4-byte permutation, 16 B per point): "
                                              "the 16-byte record is this design's choice -- it makes every search a run of contiguous records "
                                              "instead of a gather through a permutation (DESIGN.md section 4)"},
                "roofline_whole_step": {"alg_bytes_per_scene_step": step_bytes,
                                        "achieved": round(value * step_bytes / 1e9, 2), "unit": "GB/s",
                                        "frac": round(value * step_bytes / 1e9 / HBM_PEAK_GBS, 5),
                                        "frac_of_measured_copy": fracm(value * step_bytes / 1e9)},
                "hbm_peak_vendor_gbs": HBM_PEAK_GBS,
                "hbm_peak_measured_gbs": None if not hbm_measured else round(hbm_measured, 1),
                "hbm_peak_measured_how": "float4 device copy of 1 GiB (amk__hbm_copy_probe, csrc/probe.hip): bytes read + bytes written "
                                         "over the copy's duration, best of 20 launch shapes -- 18 persistent ones (2 / 4 / 8 loads in flight per "
                                         "thread, plain / non-temporal, 8 / 16 / 32 blocks per CU) and one 16-byte element per thread on a grid as large "
                                         "as the data, plain / non-temporal stores (the shape that reaches 6.29 TB/s: "
                                         f"profiles/r06_hbm_probe_shapes.txt) -- 10 repetitions each, HIP events; every HBM fraction of "
                                         "this line is given against the vendor peak (frac) and against this figure (frac_of_measured_copy)",
                "kernels_single_stream": lone,
                "parity": parity,
                "cpu_baseline": cpu,
            })
        if breakdown:
            line["kernel_breakdown"] = breakdown
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    sys.exit(main() or 0)
