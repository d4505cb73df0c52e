"""Call latency of the host-memory entry points an integrator calls (include/avoid_mpc_amd.h, the *_host functions): host clock
around the call -- every one of them ends in a wait --, WARM calls first, then the median of CALLS calls per entry, one process.
  kd_search_host      amk_kd_search_host, one scene of 50 k points, 1 query, k = 8 (INTEGRATION.md's SearchForNearest)
  mpc_solve_host      amk_mpc_solve_host, S = 1, config C1 (N = 10, K = 3), from a zero warm start every call
  step_batch_host     amk_step_batch_host, S = 1, C1, a 5 k-point scene, from a zero warm start every call
  kfmap_query_host    amk_kfmap_query_nearest_host, S = 1, 20 queries, k = 8, a map of three 5 k-point frames
  depth_clouds_host   amk_depth_to_clouds_host, one 640 x 480 float frame at the yaml's scale
usage: python tools/experiments/host_entry_latency.py [--calls N]            this tree's library -> one JSON line (medians, us)
       python tools/experiments/host_entry_latency.py --against DIR [--out FILE]
           DIR: a built checkout of the commit to compare with.  Runs DIR, this tree, DIR, this tree, each in a fresh process, and
           prints both trees' medians, the spread between DIR's own two runs, and whether each median of this tree is within
           DIR's median (the mean of its two) plus that spread -- the only noise the measurement can show."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

WARM, CALLS = 30, 300
ENTRIES = ["kd_search_host", "mpc_solve_host", "step_batch_host", "kfmap_query_host", "depth_clouds_host"]


def measure(calls):
    sys.path.insert(0, ".")
    import numpy as np
    import torch
    from avoid_mpc_amd import capi, synth
    from avoid_mpc_amd.host import KdBatch, KfMap, MpcBatch, depth_params
    lib = capi.load()
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    legs = {}

    def timed(call, before=None):
        t = []
        for i in range(WARM + calls):
            if before:
                before()
                torch.cuda.synchronize()
            t0 = time.perf_counter_ns()
            capi.check(call(), "timed call")
            t1 = time.perf_counter_ns()
            if i >= WARM:
                t.append((t1 - t0) * 1e-3)
        return float(np.median(t))

    # SearchForNearest
    cloud, _ = synth.make_cloud(50000, 1)
    kd = KdBatch(1, 50000); kd.build_host(cloud[None])
    q = np.array([[[3.0, 0.2, 1.5]]]); idx = np.zeros(8, np.int32); d2 = np.zeros(8); pts = np.zeros((8, 3), np.float32); cnt = np.zeros(1, np.int32)
    legs["kd_search_host"] = timed(lambda: lib.amk_kd_search_host(kd.h, vp(q), 1, 8, vp(idx), vp(d2), vp(pts), vp(cnt)))

    # the control step and the solve on its parameter vector
    c = synth.CONFIGS["C1"]
    prm = synth.MpcParams(T=c["T"], K=c["K"])
    sc = synth.make_scene(5000, 4242, prm)
    ko, ke = KdBatch(1, len(sc["cloud"])), KdBatch(1, len(sc["edge"]))
    ko.build_host(sc["cloud"][None]); ke.build_host(sc["edge"][None])
    mpc = MpcBatch(prm.T, prm.dt, prm.K, 1); mpc.configure(prm)
    sq = np.ascontiguousarray([[np.concatenate([sc["pos"] + sc["vel"] * prm.decay * (i + 1), [sc["yaw"]], sc["vel"], sc["acc"]])
                                for i in range(prm.max_iter)]])
    pos_x = np.array([sc["pos"][0]]); ref = sc["ref_path"][None].copy()
    u = np.zeros((1, 4)); x0 = np.zeros((1, mpc.N, 14)); flags = np.zeros((1, 4), np.int32); info = np.zeros((1, 4), np.int32)
    sp = capi.StepParams(float(prm.speed), float(prm.safety_distance), int(prm.max_iter), 0)

    def fresh_step():
        ref[:] = sc["ref_path"]
        mpc.reset_warm_start()
    legs["step_batch_host"] = timed(lambda: lib.amk_step_batch_host(ko.h, ke.h, mpc.h, C.byref(sp), vp(sq), vp(pos_x), vp(ref), vp(u), vp(x0), vp(flags)),
                                    fresh_step)
    P = mpc.ref_states()
    legs["mpc_solve_host"] = timed(lambda: lib.amk_mpc_solve_host(mpc.h, vp(P), vp(u), vp(x0), vp(info), 0), mpc.reset_warm_start)

    # QueryNearest over a small map
    gmap = KfMap(1, 5000, 500, 3, 0.1, 10, 0.1, np.eye(4))
    for t in range(3):
        cl, ed = synth.make_cloud(5000, 10 + t)
        Tw = np.eye(4)[None].copy(); Tw[0, 0, 3] = 0.3 * t
        gmap.add_vertex(torch.from_numpy(cl[None]).cuda(), torch.from_numpy(ed[None]).cuda(), torch.from_numpy(Tw).cuda())
        gmap.update()
    mq = np.random.default_rng(3).random((1, 20, 3)) * [10.0, 8.0, 3.0] + [1.0, -4.0, 0.0]
    mp = np.zeros((20, 8, 3), np.float32); md = np.zeros((20, 8)); mf = np.zeros((20, 8), np.int32); mc = np.zeros(20, np.int32)
    legs["kfmap_query_host"] = timed(lambda: lib.amk_kfmap_query_nearest_host(gmap.h, None, vp(mq), 3, 20, 8, 0, vp(mp), vp(md), vp(mf), vp(mc)))

    # AddVertex's image half
    rows, cols = 480, 640
    yy, xx = np.mgrid[0:rows, 0:cols]
    img = np.ascontiguousarray((2.0 + 0.01 * xx + (xx // 64 % 2) * 2.0 + (yy // 120) * 0.5).astype(np.float32))
    dp = depth_params()
    w, h = C.c_int(), C.c_int()
    capi.check(lib.amk_depth_out_size(rows, cols, dp.resize_scale, C.byref(w), C.byref(h)), "amk_depth_out_size")
    cap = w.value * h.value
    T = np.eye(4); dc = np.zeros((cap, 3), np.float32); de = np.zeros((cap, 3), np.float32); dn = np.zeros(1, np.int32); den = np.zeros(1, np.int32)
    legs["depth_clouds_host"] = timed(lambda: lib.amk_depth_to_clouds_host(vp(img), capi.AMK_DEPTH_F32, rows, cols, rows * cols, 1, C.byref(dp), vp(T),
                                                                           vp(T), vp(dc), cap * 3, vp(dn), vp(de), cap * 3, vp(den), 3))
    assert cnt[0] == 8 and flags[0, 1] >= 1 and (mc > 0).all() and dn[0] > 0
    return legs


def against(ref_dir, out_path):
    here = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    runs = {ref_dir: [], here: []}
    for tree in (ref_dir, here, ref_dir, here):   # fresh processes, alternating; the first failure ends the measurement
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=tree, stdout=subprocess.PIPE, text=True, timeout=600)
        if r.returncode:
            sys.exit(f"{tree}: exit status {r.returncode}")
        runs[tree].append(json.loads(r.stdout.strip().splitlines()[-1]))
    a, b = runs[ref_dir], runs[here]
    lines = [f"host entry latency, one MI355X; host clock around the call, median of {CALLS} calls after {WARM} warm-up calls; us",
             "two fresh processes per tree, alternating: reference, this, reference, this",
             f"  {'entry':18s} {'reference':>19s} {'spread':>8s} {'this tree':>19s} {'bound':>9s}  within"]
    ok = True
    for e in ENTRIES:
        spread = abs(a[0][e] - a[1][e])
        bound = (a[0][e] + a[1][e]) / 2 + spread
        good = max(b[0][e], b[1][e]) <= bound
        ok = ok and good
        lines.append(f"  {e:18s} {a[0][e]:9.1f} {a[1][e]:9.1f} {spread:8.1f} {b[0][e]:9.1f} {b[1][e]:9.1f} {bound:9.1f}  {'yes' if good else 'NO'}")
    print("\n".join(lines))
    if out_path:
        open(out_path, "w").write("\n".join(lines) + "\n")
    return ok


if __name__ == "__main__":
    arg = lambda name: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None
    if arg("--against"):
        sys.exit(0 if against(os.path.abspath(arg("--against")), arg("--out")) else 1)
    print(json.dumps(measure(int(arg("--calls") or CALLS))))
