"""Cost of amk_kd_segment_nearest beside amk_kd_search on the points of the same path, and beside amk_kd_segment_search at a fixed
radius (profiles/kd_segment_nearest_cost.txt).

256 scenes x 50 000-point bench-style clouds; per scene the straight 20-point path of kd_segment_cost.py at spacing speed * dt =
10 m/s * 0.033 s = 0.33 m (19 legs) that starts beside a cloud point.  The calls {segment nearest k 8, kNN k 8, segment nearest k 1,
kNN k 1, segment search radius_sq 0.49 max_results 8} are timed with HIP events around `inner` launches on one stream, `reps` times,
alternating.  Beside the times: what the two branch-and-bound walks do, counted on the host for a few scenes from the clouds -- the
shells walked until the stop rule holds (with the true k-th distance after every shell, the grid geometry taken over the full bounding
box, where the build samples it) and the records of the cells of those shells (before any clip to the k-th distance).

    python tools/experiments/kd_segment_nearest_cost.py [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from avoid_mpc_amd import synth  # noqa: E402
from avoid_mpc_amd.host import KdBatch  # noqa: E402
from tools.experiments.kd_segment_cost import grid_of, timed  # noqa: E402


def seg_d2(c, a, b):
    ab = b - a
    L2 = float(ab @ ab)
    t = np.clip(((c - a) @ ab) / L2, 0.0, 1.0) if L2 > 0 else np.zeros(len(c))
    e = a + t[:, None] * ab - c
    return (e * e).sum(axis=1)


def walk(c, cells, lo, h, g, a, b, k):
    """the shells grid_knn (a == b) / grid_segment_knn walk around [a, b] and the records of their cells -> (shells, records)"""
    qlo, qhi = np.minimum(a, b), np.maximum(a, b)
    clo = np.clip(np.floor((qlo - lo) / h), 0, g - 1).astype(int)
    chi = np.clip(np.floor((qhi - lo) / h), 0, g - 1).astype(int)
    cheb = np.maximum(np.maximum(clo - cells, cells - chi), 0).max(axis=1)
    d2 = seg_d2(c, a, b)
    rmax = int(max(clo.max(), (g - 1 - chi).max()))
    for r in range(rmax + 1):
        seen = cheb <= r
        if seen.sum() >= k:
            tau = np.partition(d2[seen], k - 1)[k - 1]
            faces = [qlo[i] - (lo[i] + (clo[i] - r) * h) for i in range(3) if clo[i] - r > 0] + \
                    [(lo[i] + (chi[i] + r + 1) * h) - qhi[i] for i in range(3) if chi[i] + r < g[i] - 1]
            if not faces or tau < max(0.0, min(faces)) ** 2:
                break
    return r + 1, int(seen.sum())


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
    out = {("nearest", K): kd.segment_nearest(path, K), ("nearest", 1): kd.segment_nearest(path, 1),
           ("knn", K): kd.search(path, K), ("knn", 1): kd.search(path, 1), ("segment", K): kd.segment_search(path, r2, K)}
    torch.cuda.synchronize()
    leg_d, pt_d = out[("nearest", K)]["sqdist"].sqrt(), out[("knn", K)]["sqdist"].sqrt()
    calls = {f"amk_kd_segment_nearest k = {K}, {P - 1} legs": lambda: kd.segment_nearest(path, K, out=out[("nearest", K)]),
             f"amk_kd_search k = {K}, {P} points": lambda: kd.search(path, K, out=out[("knn", K)]),
             f"amk_kd_segment_nearest k = 1, {P - 1} legs": lambda: kd.segment_nearest(path, 1, out=out[("nearest", 1)]),
             f"amk_kd_search k = 1, {P} points": lambda: kd.search(path, 1, out=out[("knn", 1)]),
             f"amk_kd_segment_search radius_sq = {r2}, max_results = {K}, {P - 1} legs": lambda: kd.segment_search(path, r2, K, out=out[("segment", K)])}
    for fn in calls.values():   # warm-up: every shape of the timed window
        timed(fn, 5)
    t = {name: [] for name in calls}
    for _ in range(a.reps):
        for name, fn in calls.items():
            t[name].append(timed(fn, a.inner))
    lines = [f"amk_kd_segment_nearest beside amk_kd_search on the points of the same path and amk_kd_segment_search at a fixed radius; one MI355X, "
             f"HIP events around {a.inner} launches on one stream, {a.reps} repetitions, the calls alternating, median (min .. max) microseconds per launch",
             f"S = {S} scenes x {n}-point clouds; a straight {P}-point path per scene at spacing {spacing:.2f} m ({P - 1} legs)",
             f"distance of the nearest point, m: per leg median {leg_d[..., 0].median():.3f}, max {leg_d[..., 0].max():.3f};  per point median "
             f"{pt_d[..., 0].median():.3f}, max {pt_d[..., 0].max():.3f};  of the {K}-th: per leg median {leg_d[..., K - 1].median():.3f}, per point "
             f"median {pt_d[..., K - 1].median():.3f}"]
    names = list(calls)
    med = {name: float(np.median(v)) for name, v in t.items()}
    for name in names:
        lines.append(f"  {name:66s} {med[name]:9.1f} us   ({min(t[name]):.1f} .. {max(t[name]):.1f})")
    for seg, knn, what in ((names[0], names[1], f"k = {K}"), (names[2], names[3], "k = 1")):
        lines.append(f"  {what}: the launch {med[seg] / med[knn]:.2f} x the kNN launch; per leg {med[seg] / (P - 1):.2f} us against "
                     f"{med[knn] / P:.2f} us per point query = {med[seg] / (P - 1) / (med[knn] / P):.2f} point kNN queries")
    lines.append(f"  k = {K} against the segment search at radius_sq = {r2}: {med[names[0]] / med[names[4]]:.2f} x")
    # what the walks do, on the host: shells until the stop rule holds, records of their cells
    hc, hp = cloud[:a.counted_scenes].cpu().numpy()[:, :, :3].astype(np.float64), path[:a.counted_scenes].cpu().numpy()
    for k in (K, 1):
        leg, pt = [], []
        for s in range(len(hc)):
            lo, h, gdim = grid_of(hc[s])
            cells = np.clip(np.floor((hc[s] - lo) / h), 0, gdim - 1).astype(int)
            for j in range(P):
                pt.append(walk(hc[s], cells, lo, h, gdim, hp[s, j], hp[s, j], k))
                if j + 1 < P:
                    leg.append(walk(hc[s], cells, lo, h, gdim, hp[s, j], hp[s, j + 1], k))
        leg, pt = np.array(leg, float), np.array(pt, float)
        lines.append(f"walks, k = {k} (host count, first {len(hc)} scenes, cells about {h:.2f} m wide): shells per leg mean {leg[:, 0].mean():.2f}, per point "
                     f"{pt[:, 0].mean():.2f};  records in their cells per leg median {np.median(leg[:, 1]):.0f}, mean {leg[:, 1].mean():.1f}, per point median "
                     f"{np.median(pt[:, 1]):.0f}, mean {pt[:, 1].mean():.1f};  leg / point = {leg[:, 1].mean() / pt[:, 1].mean():.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    kd.close()


if __name__ == "__main__":
    main()
