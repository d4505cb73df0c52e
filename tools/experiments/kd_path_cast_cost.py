"""Cost of amk_kd_path_cast beside amk_kd_segment_cast on the same paths, and of the pipeline's audit stage
(profiles/kd_path_cast_cost.txt).

256 scenes x 50 000-point bench-style clouds, kd_segment_cast_cost.py's straight 20-point path at spacing 0.33 m (19 legs):
 (a) radius_sq 0.49: nearly every contact in these clouds is at the start, so the path cast walks one round where the yardstick,
     amk_kd_segment_cast on the same paths (unchanged code), walks 19 legs.  The bar: path cast <= yardstick + the run's spread.
 (b) radius_sq 0.0025: the same walks in serial rounds of W legs.  That path starts next to a cloud point and mostly still stops on
     leg 0, so the mostly free paths are measured as well: the same headings from the most open of 64 random spots per scene.  No
     bar; the ratios are recorded per W.
 (c) the pipeline with the audit in REPORT mode (radius 0.7 m and 0.05 m) against OFF on the same build: TASK-mode periods of
     256-scene frames, warm-started, on fixed frames (no vehicle in the loop), `periods` periods per repetition over slots x gang
     frames; host time from the first submit to the end of drain; ONE pipeline whose mode is switched between the repetitions (two
     pipelines alive side by side differ by more than the audit costs).  No bar.
The calls are timed with HIP events around `inner` launches on one stream, `reps` times, alternating.  W, the waves per block of the
path cast, is a build-time constant (kd_path_cast.h): run once per W, the other W from a library built with
AMK_HIPCC_FLAGS=-DAMK_PATH_CAST_WAVES=8, and say which with --waves.

    python tools/experiments/kd_path_cast_cost.py [--out FILE] [--no-pipeline] [--waves W]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from avoid_mpc_amd import capi, flight, synth  # noqa: E402
from avoid_mpc_amd.host import KdBatch, Pipeline  # noqa: E402
from tools.experiments.kd_segment_cost import timed  # noqa: E402


def pipeline_line(a, dev, lines):
    prm = synth.MpcParams(T=0.66, K=8)
    S, n, ne = a.scenes, a.points, a.points // 10
    nslots, gang = a.slots, a.gang
    frames = []
    for b in range(nslots * gang):
        cl, ed = synth.make_clouds_torch(n, S, 9100 + b, dev)
        st = [flight.initial_state(77000 + b * S + s, prm) for s in range(S)]
        frames.append(dict(cl=cl, ed=ed, odom=torch.from_numpy(np.stack([x for x, _ in st])).to(dev),
                           ref=torch.from_numpy(np.stack([r for _, r in st])).to(dev)))
    pl = Pipeline(nslots, S, n, ne, prm, queue_depth=2, gang=gang)     # ONE pipeline, the mode switched between the repetitions
    modes = {"audit OFF": (capi.AMK_AUDIT_OFF, 0.0), "audit REPORT, 0.7 m": (capi.AMK_AUDIT_REPORT, 0.7),
             "audit REPORT, 0.05 m": (capi.AMK_AUDIT_REPORT, 0.05)}

    def fly(periods, first):
        for p in range(periods):
            for fr in frames:
                pl.submit(fr["cl"], fr["ed"], ref_path_init=fr["ref"] if (first and p == 0) else None, odom=fr["odom"],
                          keep_warm_start=not (first and p == 0), order_after_current_stream=False)
        pl.drain()

    torch.cuda.synchronize()
    fly(2, True)
    t = {name: [] for name in modes}
    stops = {}
    for _ in range(a.reps):
        for name, (mode, radius) in modes.items():
            pl.set_path_audit(mode, radius)
            t0 = time.perf_counter()
            fly(a.periods, False)
            t[name].append(time.perf_counter() - t0)
            if mode != capi.AMK_AUDIT_OFF:
                stops[name] = np.concatenate([pl.audit_outputs(tk)["stop"] for tk in range(nslots * gang)])
    steps = a.periods * len(frames) * S
    med = {name: float(np.median(v)) for name, v in t.items()}
    lines.append(f"(c) pipeline, {nslots} slots x gang {gang} x {S} scenes x {n}-point clouds, N = {pl.N}, K = {prm.K}, TASK-mode periods, "
                 f"warm-started, {a.periods} periods per repetition, {a.reps} repetitions alternating on one pipeline; k scene-steps/s, median (min .. max)")
    for name in modes:
        r = [steps / v / 1e3 for v in t[name]]
        tail = f"   time / OFF = {med[name] / med['audit OFF']:.3f}; stop codes 0 / 1 / 2 of the last period {np.bincount(stops[name], minlength=3).tolist()}" if name in stops else ""
        lines.append(f"  {name:22s} {steps / med[name] / 1e3:9.1f} k/s   ({min(r):.1f} .. {max(r):.1f}){tail}")
    pl.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=256)
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--path-points", type=int, default=20)
    ap.add_argument("--inner", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--gang", type=int, default=2)
    ap.add_argument("--periods", type=int, default=20)
    ap.add_argument("--no-pipeline", action="store_true")
    ap.add_argument("--waves", default="4 (as built)", help="label only: the W the library under test was built with")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: nothing here is a CPU measurement"
    dev = torch.device("cuda", 0)
    S, n, P, r2, thin, spacing = a.scenes, a.points, a.path_points, 0.49, 0.0025, 10.0 * 0.033
    f64 = dict(device=dev, dtype=torch.float64)
    cloud, _edge = synth.make_clouds_torch(n, S, 9090, dev)
    kd = KdBatch(S, n)
    kd.build(cloud)
    g = torch.Generator(device=dev); g.manual_seed(7)      # kd_segment_cast_cost.py's path (b)
    pick = torch.randint(0, n, (S, 1), generator=g, device=dev)
    start = cloud.gather(1, pick[:, :, None].expand(S, 1, 3)).double() + (torch.rand((S, 1, 3), generator=g, **f64) - 0.5) * 0.1
    heading = torch.rand((S, 1, 3), generator=g, **f64) * torch.tensor([1.0, 0.6, 0.2], **f64) \
        - torch.tensor([0.0, 0.3, 0.1], **f64) + torch.tensor([0.5, 0.0, 0.0], **f64)
    heading = heading / heading.norm(dim=2, keepdim=True)
    path = (start + heading * (torch.arange(P, **f64) * spacing)[None, :, None]).contiguous()
    # that path starts within 0.09 m of a cloud point, so at radius_sq 0.0025 most paths still stop on leg 0.  The free paths (b)
    # asks for: the same headings from the most open of 64 random spots of each scene (kd_segment_cast_cost.py's origin of (a))
    lo3, hi3 = cloud.amin(dim=1, keepdim=True).double(), cloud.amax(dim=1, keepdim=True).double()
    spots = (lo3 + (hi3 - lo3) * torch.rand((S, 64, 3), generator=g, **f64)).contiguous()
    clear = kd.search(spots, 1)["sqdist"][:, :, 0].sqrt()
    origin = spots.gather(1, clear.argmax(dim=1)[:, None, None].expand(S, 1, 3))
    open_path = (origin + heading * (torch.arange(P, **f64) * spacing)[None, :, None]).contiguous()
    out = {"path_a": kd.path_cast(path, r2), "seg_a": kd.segment_cast(path, r2),
           "path_b": kd.path_cast(path, thin), "seg_b": kd.segment_cast(path, thin),
           "path_o": kd.path_cast(open_path, thin), "seg_o": kd.segment_cast(open_path, thin)}
    torch.cuda.synchronize()
    # the identity on these paths: the stop leg is the first leg with a hit
    for w in "abo":
        hit = out["seg_" + w]["hit"].cpu().numpy()
        first = np.where(hit.any(axis=1), hit.argmax(axis=1), -1)
        assert np.array_equal(first, out["path_" + w]["leg"].cpu().numpy()), w
    calls = {f"(a) amk_kd_path_cast, radius_sq = {r2}": lambda: kd.path_cast(path, r2, out=out["path_a"]),
             f"(a) amk_kd_segment_cast, {P - 1} legs (the yardstick)": lambda: kd.segment_cast(path, r2, out=out["seg_a"]),
             f"(b) amk_kd_path_cast, radius_sq = {thin}": lambda: kd.path_cast(path, thin, out=out["path_b"]),
             f"(b) amk_kd_segment_cast, {P - 1} legs": lambda: kd.segment_cast(path, thin, out=out["seg_b"]),
             f"(b) from an open spot: amk_kd_path_cast, radius_sq = {thin}": lambda: kd.path_cast(open_path, thin, out=out["path_o"]),
             f"(b) from an open spot: amk_kd_segment_cast, {P - 1} legs": lambda: kd.segment_cast(open_path, thin, out=out["seg_o"])}
    for fn in calls.values():   # warm-up: every shape of the timed window
        timed(fn, 5)
    t = {name: [] for name in calls}
    for _ in range(a.reps):
        for name, fn in calls.items():
            t[name].append(timed(fn, a.inner))
    waves = a.waves
    pa, pb = out["path_a"], out["path_b"]
    lines = [f"amk_kd_path_cast beside amk_kd_segment_cast on the same paths, W (waves per block) = {waves}; one MI355X, HIP events around "
             f"{a.inner} launches on one stream, {a.reps} repetitions, the calls alternating, median (min .. max) microseconds per launch",
             f"S = {S} scenes x {n}-point clouds; a straight {P}-point path per scene at spacing {spacing:.2f} m ({P - 1} legs)",
             f"(a) paths that stop {int((pa['stop'] != 0).sum())} of {S}, of them on leg 0 {int((pa['leg'] == 0).sum())}, at t = 0 "
             f"{int(((pa['t'] == 0) & (pa['stop'] == 1)).sum())};  (b) paths that stop {int((pb['stop'] != 0).sum())} of {S}, stop leg median "
             f"{float(pb['leg'][pb['stop'] != 0].double().median()) if int((pb['stop'] != 0).sum()) else -1:.0f}, free distance m: median {float(pb['free'].median()):.2f}"]
    names = list(calls)
    med = {name: float(np.median(v)) for name, v in t.items()}
    for name in names:
        lines.append(f"  {name:66s} {med[name]:9.1f} us   ({min(t[name]):.1f} .. {max(t[name]):.1f})")
    spread = max(max(t[nm]) - min(t[nm]) for nm in names[:2])
    over = med[names[0]] - med[names[1]]
    lines.append(f"  (a) path cast / yardstick = {med[names[0]] / med[names[1]]:.2f};  path cast - yardstick = {over:+.1f} us, the run's spread "
                 f"(max - min) {spread:.1f} us: the bar (path cast <= yardstick + spread) is {'MET' if over <= spread else 'NOT MET'}")
    po = out["path_o"]
    lines.append(f"  (b) path cast / segment cast = {med[names[2]] / med[names[3]]:.2f} (no bar);  from an open spot, {int((po['stop'] == 0).sum())} of {S} paths "
                 f"free to the end, free distance m median {float(po['free'].median()):.2f}: path cast / segment cast = {med[names[4]] / med[names[5]]:.2f} (no bar)")
    kd.close()
    del cloud, _edge
    if not a.no_pipeline:
        pipeline_line(a, dev, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
