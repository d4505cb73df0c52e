"""Cost of amk_kd_segment_search beside amk_kd_radius_search on the points of the same path (profiles/kd_segment_cost.txt).

256 scenes x 50 000-point bench-style clouds; per scene a straight 20-point path at spacing speed * dt = 10 m/s * 0.033 s = 0.33 m
(19 legs) that starts beside a cloud point.  radius_sq = 0.49: the drone radius 0.5 of synth.py plus the yaml's safety_distance 0.2,
squared.  The calls {segment max_results 8, radius max_results 8, segment count only, radius count only} are timed with HIP events
around `inner` launches on one stream, `reps` times, alternating.  Beside the times: the candidate records a leg and a ball make the
walk read, counted on the host for a few scenes from the clouds (the records of the cells the widened box touches, before the per-row
clip in x; the grid geometry taken over the full bounding box, where the build samples it).

    python tools/experiments/kd_segment_cost.py [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from avoid_mpc_amd import synth  # noqa: E402
from avoid_mpc_amd.host import KdBatch  # noqa: E402


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner * 1e3   # microseconds per launch


def grid_of(cloud):
    """csrc/kd_grid.h grid_geometry over the full bounding box: (bbmin, h, cells per axis)"""
    c = cloud.astype(np.float64)
    lo, ext = c.min(axis=0), c.max(axis=0) - c.min(axis=0)
    e = np.maximum(ext, max(ext.max() * 1e-6, 1e-30))
    h = np.cbrt(e.prod() / min(max(len(c) / 64.0, 1.0), 1024.0))
    for _ in range(64):
        g = np.clip(np.ceil(e / h), 1, 1024).astype(int)
        if g.prod() <= 1024:
            break
        h *= 1.26
    return lo, h, g


def records_in_box(cells, lo, h, g, qlo, qhi, rho):
    """records of the cells the box [qlo - rho, qhi + rho] touches"""
    c0 = np.clip(np.floor((qlo - rho - lo) / h), 0, g - 1)
    c1 = np.clip(np.floor((qhi + rho - lo) / h), 0, g - 1)
    return int(((cells >= c0) & (cells <= c1)).all(axis=1).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=256)
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--path-points", type=int, default=20)
    ap.add_argument("--inner", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--counted-scenes", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: nothing here is a CPU measurement"
    dev = torch.device("cuda", 0)
    S, n, P, K, r2, spacing = a.scenes, a.points, a.path_points, 8, 0.49, 10.0 * 0.033
    cloud, _edge = synth.make_clouds_torch(n, S, 9090, dev)
    kd = KdBatch(S, n)
    kd.build(cloud)
    g = torch.Generator(device=dev); g.manual_seed(7)
    pick = torch.randint(0, n, (S, 1), generator=g, device=dev)
    start = cloud.gather(1, pick[:, :, None].expand(S, 1, 3)).double() + (torch.rand((S, 1, 3), generator=g, device=dev, dtype=torch.float64) - 0.5) * 0.1
    heading = torch.rand((S, 1, 3), generator=g, device=dev, dtype=torch.float64) * torch.tensor([1.0, 0.6, 0.2], device=dev, dtype=torch.float64) \
        - torch.tensor([0.0, 0.3, 0.1], device=dev, dtype=torch.float64) + torch.tensor([0.5, 0.0, 0.0], device=dev, dtype=torch.float64)
    heading = heading / heading.norm(dim=2, keepdim=True)
    path = (start + heading * (torch.arange(P, device=dev, dtype=torch.float64) * spacing)[None, :, None]).contiguous()   # [S, P, 3]
    out = {("segment", K): kd.segment_search(path, r2, K), ("segment", 0): kd.segment_search(path, r2, 0),
           ("radius", K): kd.radius_search(path, r2, K), ("radius", 0): kd.radius_search(path, r2, 0)}
    torch.cuda.synchronize()
    leg_cnt, ball_cnt = out[("segment", 0)]["counts"].double(), out[("radius", 0)]["counts"].double()
    calls = {f"amk_kd_segment_search max_results = {K}, {P - 1} legs": lambda: kd.segment_search(path, r2, K, out=out[("segment", K)]),
             f"amk_kd_radius_search max_results = {K}, {P} points": lambda: kd.radius_search(path, r2, K, out=out[("radius", K)]),
             f"amk_kd_segment_search max_results = 0, {P - 1} legs": lambda: kd.segment_search(path, r2, 0, out=out[("segment", 0)]),
             f"amk_kd_radius_search max_results = 0, {P} points": lambda: kd.radius_search(path, r2, 0, out=out[("radius", 0)])}
    for fn in calls.values():   # warm-up: every shape of the timed window
        timed(fn, 5)
    t = {name: [] for name in calls}
    for _ in range(a.reps):
        for name, fn in calls.items():
            t[name].append(timed(fn, a.inner))
    lines = [f"amk_kd_segment_search beside amk_kd_radius_search on the points of the same path; one MI355X, HIP events around {a.inner} launches "
             f"on one stream, {a.reps} repetitions, the calls alternating, median (min .. max) microseconds per launch",
             f"S = {S} scenes x {n}-point clouds; a straight {P}-point path per scene at spacing {spacing:.2f} m ({P - 1} legs); radius_sq = {r2}",
             f"results per leg: median {leg_cnt.median():.0f}, mean {leg_cnt.mean():.1f}, max {leg_cnt.max():.0f};  per ball: median "
             f"{ball_cnt.median():.0f}, mean {ball_cnt.mean():.1f}, max {ball_cnt.max():.0f}"]
    names = list(calls)
    med = {name: float(np.median(v)) for name, v in t.items()}
    for name in names:
        lines.append(f"  {name:58s} {med[name]:9.1f} us   ({min(t[name]):.1f} .. {max(t[name]):.1f})")
    for seg, rad, what in ((names[0], names[1], f"max_results = {K}"), (names[2], names[3], "count only")):
        lines.append(f"  {what}: the launch {med[seg] / med[rad]:.2f} x the radius launch; per leg {med[seg] / (P - 1):.2f} us against "
                     f"{med[rad] / P:.2f} us per point query = {med[seg] / (P - 1) / (med[rad] / P):.2f} point queries")
    # candidate records read per leg against per ball, on the host
    hc, hp = cloud[:a.counted_scenes].cpu().numpy()[:, :, :3], path[:a.counted_scenes].cpu().numpy()
    rho = np.sqrt(r2)
    per_leg, per_ball = [], []
    for s in range(len(hc)):
        lo, h, gdim = grid_of(hc[s])
        cells = np.clip(np.floor((hc[s].astype(np.float64) - lo) / h), 0, gdim - 1)
        for j in range(P):
            per_ball.append(records_in_box(cells, lo, h, gdim, hp[s, j], hp[s, j], rho))
            if j + 1 < P:
                per_leg.append(records_in_box(cells, lo, h, gdim, np.minimum(hp[s, j], hp[s, j + 1]), np.maximum(hp[s, j], hp[s, j + 1]), rho))
    lines.append(f"candidate records in the cells the widened box touches (host count, first {len(hc)} scenes, cells about {h:.2f} m wide): per leg "
                 f"median {np.median(per_leg):.0f}, mean {np.mean(per_leg):.1f};  per ball median {np.median(per_ball):.0f}, mean "
                 f"{np.mean(per_ball):.1f};  leg / ball = {np.mean(per_leg) / np.mean(per_ball):.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    kd.close()


if __name__ == "__main__":
    main()
