"""Cost of amk_kd_radius_search beside amk_kd_search on the same handles and queries (profiles/kd_radius_cost.txt).

256 scenes x 50 000-point bench-style clouds x 20 queries per scene (cloud points moved by a few centimetres, so every ball
holds something).  Two radii, found by bisection on the count-only call: the median ball holds about 8 and about 700 points.
Per radius the pair {amk_kd_search k = 8, amk_kd_radius_search max_results = 8} is timed with HIP events around `inner` launches
on one stream, `reps` times, the two alternating; the count-only radius call (max_results = 0) rides along.

    python tools/experiments/kd_radius_cost.py [--out FILE]
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


def radius_for(kd, q, target):
    """squared radius whose median ball over the queries holds `target` points"""
    lo, hi = 1e-6, 100.0
    for _ in range(40):
        mid = np.sqrt(lo * hi)
        med = float(kd.radius_search(q, mid, 0)["counts"].double().median())
        lo, hi = (mid, hi) if med < target else (lo, mid)
    return hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=256)
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--queries", type=int, default=20)
    ap.add_argument("--inner", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: nothing here is a CPU measurement"
    dev = torch.device("cuda", 0)
    S, n, Q, K = a.scenes, a.points, a.queries, 8
    cloud, _edge = synth.make_clouds_torch(n, S, 9090, dev)
    kd = KdBatch(S, n)
    kd.build(cloud)
    g = torch.Generator(device=dev); g.manual_seed(7)
    pick = torch.randint(0, n, (S, Q), generator=g, device=dev)
    q = cloud.gather(1, pick[:, :, None].expand(S, Q, 3)).double() + (torch.rand((S, Q, 3), generator=g, device=dev, dtype=torch.float64) - 0.5) * 0.1
    q = q.contiguous()
    out_knn = kd.search(q, K)
    lines = [f"amk_kd_radius_search beside amk_kd_search; one MI355X, HIP events around {a.inner} launches on one stream, {a.reps} repetitions, "
             f"the calls alternating, median (min .. max) microseconds per launch",
             f"S = {S} scenes x {n}-point clouds x {Q} queries per scene; k = max_results = {K}"]
    for target in (8, 700):
        r2 = radius_for(kd, q, target)
        cnt = kd.radius_search(q, r2, 0)["counts"].double()
        out_rad = kd.radius_search(q, r2, K)
        out_cnt = kd.radius_search(q, r2, 0)
        calls = {"amk_kd_search k = 8": lambda: kd.search(q, K, out=out_knn),
                 "amk_kd_radius_search max_results = 8": lambda: kd.radius_search(q, r2, K, out=out_rad),
                 "amk_kd_radius_search max_results = 0 (count only)": lambda: kd.radius_search(q, r2, 0, out=out_cnt)}
        for fn in calls.values():   # warm-up: every shape of the timed window
            timed(fn, 5)
        t = {name: [] for name in calls}
        for _ in range(a.reps):
            for name, fn in calls.items():
                t[name].append(timed(fn, a.inner))
        lines.append(f"radius {np.sqrt(r2):.4f} (radius_sq {r2:.6g}): points per ball median {cnt.median():.0f}, mean {cnt.mean():.1f}, "
                     f"max {cnt.max():.0f}")
        base = float(np.median(t["amk_kd_search k = 8"]))
        for name, v in t.items():
            lines.append(f"  {name:52s} {np.median(v):9.1f} us   ({min(v):.1f} .. {max(v):.1f})   {np.median(v) / base:.2f} x the kNN")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    kd.close()


if __name__ == "__main__":
    main()
