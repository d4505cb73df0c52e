"""Cost of amk_kd_segment_cast beside amk_kd_segment_search on the same legs (profiles/kd_segment_cast_cost.txt).

256 scenes x 50 000-point bench-style clouds, three workloads in one run:
 (a) one 12 m ray per scene (n_points = 2) that starts at the most open of 64 random spots and crosses all three axes, radius_sq 0.49; the
     yardstick is amk_kd_segment_search(max_results = 1) on the same rays -- the query a host had to use before, whose walk fills
     the ray's bounding box;
 (b) the 19 legs of kd_segment_cost.py's straight 20-point path at spacing 0.33 m, radius_sq 0.49, against the segment search
     (max_results = 1) on the same legs.  No bar: the cells are the same and the per-candidate arithmetic is heavier.
 (c) the rays of (a) at radius_sq 0.0025, both calls, no bar: the bench clouds are dense (a point every 0.3 m), so at 0.49 nearly
     every ray is in contact where it starts; a thin ray travels some metres first and shows the walk beyond its first slab.
The six calls are timed with HIP events around `inner` launches on one stream, `reps` times, alternating.  The bar for (a): the
cast's median must not exceed the yardstick's by more than the (max - min) spread this run shows.  Beside the times, counted on the
host for a few scenes: the records each walk visits on the rays of (a) and (c) -- grid_cast's slabs until its stop rule holds (cells of the
previous slab left out), grid_segment's widened bounding box (before its row clip) -- with the grid geometry taken over the full
bounding box, where the build samples it.

    python tools/experiments/kd_segment_cast_cost.py [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from avoid_mpc_amd import synth  # noqa: E402
from avoid_mpc_amd.host import KdBatch  # noqa: E402
from tools.experiments.kd_segment_cost import grid_of, records_in_box, timed  # noqa: E402


def contact_t(c, a, b, r2):
    """t of the first contact of every point (inf where there is none): the header's formula, vectorised"""
    ab, ap = b - a, c - a
    L2 = float(ab @ ab)
    q, dot = (ap * ap).sum(axis=1), ap @ ab
    with np.errstate(all="ignore"):
        disc = dot * dot - L2 * (q - r2)
        t = (dot - np.sqrt(disc)) / L2
    return np.where(q < r2, 0.0, np.where((dot > 0) & (disc > 0) & (t < 1), t, np.inf))


def cast_walk(c, cells, lo, h, g, a, b, r2):
    """grid_cast's slabs along a -> b -> (slabs walked, slabs in all, records visited)"""
    ab = b - a
    cell = lambda p: np.clip(np.floor((p - lo) / h), 0, g - 1).astype(int)
    rho = np.sqrt(r2)
    n = int(max(1, min(np.ceil(np.abs(ab).max() / h), 1024, np.abs(cell(b) - cell(a)).sum() + 1)))
    t = contact_t(c, a, b, r2)
    seen = np.zeros(len(c), bool)
    for i in range(n):
        p0, p1 = a + (i / n) * ab, a + ((i + 1) / n) * ab
        c0, c1 = cell(np.minimum(p0, p1) - rho), cell(np.maximum(p0, p1) + rho)
        seen |= ((cells >= c0) & (cells <= c1)).all(axis=1)
        if seen.any() and t[seen].min() <= (i + 1) / n:
            break
    return i + 1, n, int(seen.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=256)
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--path-points", type=int, default=20)
    ap.add_argument("--ray", type=float, default=12.0)
    ap.add_argument("--inner", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--counted-scenes", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: nothing here is a CPU measurement"
    dev = torch.device("cuda", 0)
    S, n, P, r2, thin, spacing = a.scenes, a.points, a.path_points, 0.49, 0.0025, 10.0 * 0.033
    f64 = dict(device=dev, dtype=torch.float64)
    cloud, _edge = synth.make_clouds_torch(n, S, 9090, dev)
    kd = KdBatch(S, n)
    kd.build(cloud)
    g = torch.Generator(device=dev); g.manual_seed(7)
    pick = torch.randint(0, n, (S, 1), generator=g, device=dev)
    start = cloud.gather(1, pick[:, :, None].expand(S, 1, 3)).double() + (torch.rand((S, 1, 3), generator=g, **f64) - 0.5) * 0.1
    heading = torch.rand((S, 1, 3), generator=g, **f64) * torch.tensor([1.0, 0.6, 0.2], **f64) \
        - torch.tensor([0.0, 0.3, 0.1], **f64) + torch.tensor([0.5, 0.0, 0.0], **f64)
    heading = heading / heading.norm(dim=2, keepdim=True)
    path = (start + heading * (torch.arange(P, **f64) * spacing)[None, :, None]).contiguous()   # (b): [S, P, 3]
    # (a): from a spot with at least 1 m of clearance (the first of 64 random spots in the cloud's box that has it, else the most open
    # one: a vehicle does not start a cast inside an obstacle), 12 m in a direction that crosses all three axes
    lo3, hi3 = cloud.amin(dim=1, keepdim=True).double(), cloud.amax(dim=1, keepdim=True).double()
    spots = (lo3 + (hi3 - lo3) * torch.rand((S, 64, 3), generator=g, **f64)).contiguous()
    clear = kd.search(spots, 1)["sqdist"][:, :, 0].sqrt()
    first = torch.where((clear > 1.0).any(dim=1), (clear > 1.0).int().argmax(dim=1), clear.argmax(dim=1))
    origin = spots.gather(1, first[:, None, None].expand(S, 1, 3))
    sign = torch.where(torch.rand((S, 1, 3), generator=g, **f64) < 0.5, -1.0, 1.0) * torch.tensor([1.0, 1.0, 0.0], **f64) \
        + torch.tensor([0.0, 0.0, 1.0], **f64)
    direction = torch.tensor([0.75, 0.6, 0.28], **f64) * sign
    direction = direction / direction.norm(dim=2, keepdim=True)
    ray = torch.cat([origin, origin + a.ray * direction], dim=1).contiguous()                    # [S, 2, 3]
    out = {"cast_a": kd.segment_cast(ray, r2), "seg_a": kd.segment_search(ray, r2, 1),
           "cast_b": kd.segment_cast(path, r2), "seg_b": kd.segment_search(path, r2, 1),
           "cast_c": kd.segment_cast(ray, thin), "seg_c": kd.segment_search(ray, thin, 1)}
    torch.cuda.synchronize()
    differ = sum(int(((out["cast_" + w]["hit"] > 0) != (out["seg_" + w]["counts"] > 0)).sum()) for w in "abc")
    calls = {f"(a) amk_kd_segment_cast, one {a.ray:g} m ray": lambda: kd.segment_cast(ray, r2, out=out["cast_a"]),
             f"(a) amk_kd_segment_search max_results = 1, one {a.ray:g} m ray": lambda: kd.segment_search(ray, r2, 1, out=out["seg_a"]),
             f"(b) amk_kd_segment_cast, {P - 1} legs": lambda: kd.segment_cast(path, r2, out=out["cast_b"]),
             f"(b) amk_kd_segment_search max_results = 1, {P - 1} legs": lambda: kd.segment_search(path, r2, 1, out=out["seg_b"]),
             f"(c) amk_kd_segment_cast, the rays at radius_sq = {thin}": lambda: kd.segment_cast(ray, thin, out=out["cast_c"]),
             f"(c) amk_kd_segment_search max_results = 1, radius_sq = {thin}": lambda: kd.segment_search(ray, thin, 1, out=out["seg_c"])}
    for fn in calls.values():   # warm-up: every shape of the timed window
        timed(fn, 5)
    t = {name: [] for name in calls}
    for _ in range(a.reps):
        for name, fn in calls.items():
            t[name].append(timed(fn, a.inner))
    ca, cb, cc = out["cast_a"], out["cast_b"], out["cast_c"]
    lines = [f"amk_kd_segment_cast beside amk_kd_segment_search on the same legs, radius_sq = {r2}; one MI355X, HIP events around {a.inner} "
             f"launches on one stream, {a.reps} repetitions, the calls alternating, median (min .. max) microseconds per launch",
             f"S = {S} scenes x {n}-point clouds; (a) one {a.ray:g} m ray per scene across all three axes, (b) a straight {P}-point path per scene "
             f"at spacing {spacing:.2f} m ({P - 1} legs)",
             f"(a) rays with a contact {int(ca['hit'].sum())} of {S}, of them inside at the start {int(((ca['t'] == 0) & (ca['hit'] > 0)).sum())}, "
             f"free distance m: median {float((ca['t'] * a.ray).median()):.2f}, max {float((ca['t'] * a.ray).max()):.2f};  (c) with a contact "
             f"{int(cc['hit'].sum())}, inside at the start {int(((cc['t'] == 0) & (cc['hit'] > 0)).sum())}, free distance m: median "
             f"{float((cc['t'] * a.ray).median()):.2f}, max {float((cc['t'] * a.ray).max()):.2f};  (b) legs with a contact {int(cb['hit'].sum())} of {S * (P - 1)}, "
             f"of them inside at the start {int(((cb['t'] == 0) & (cb['hit'] > 0)).sum())};  legs where hit != (segment count > 0): {differ}"]
    names = list(calls)
    med = {name: float(np.median(v)) for name, v in t.items()}
    for name in names:
        lines.append(f"  {name:66s} {med[name]:9.1f} us   ({min(t[name]):.1f} .. {max(t[name]):.1f})")
    spread = max(max(t[nm]) - min(t[nm]) for nm in names[:2])   # of the two calls of (a)
    over = med[names[0]] - med[names[1]]
    lines.append(f"  (a) cast / yardstick = {med[names[0]] / med[names[1]]:.2f};  cast - yardstick = {over:+.1f} us, the run's spread (max - min) "
                 f"{spread:.1f} us: the bar (cast <= yardstick + spread) is {'MET' if over <= spread else 'NOT MET'}")
    lines.append(f"  (b) cast / segment search = {med[names[2]] / med[names[3]]:.2f} (no bar);  (c) cast / segment search = "
                 f"{med[names[4]] / med[names[5]]:.2f} (no bar)")
    # what the two walks visit on the rays, on the host
    hc, hr = cloud[:a.counted_scenes].cpu().numpy()[:, :, :3].astype(np.float64), ray[:a.counted_scenes].cpu().numpy()
    for what, rr in (("(a)", r2), ("(c)", thin)):
        cw, sw = [], []
        for s in range(len(hc)):
            lo, h, gdim = grid_of(hc[s])
            cells = np.clip(np.floor((hc[s] - lo) / h), 0, gdim - 1).astype(int)
            cw.append(cast_walk(hc[s], cells, lo, h, gdim, hr[s, 0], hr[s, 1], rr))
            sw.append(records_in_box(cells, lo, h, gdim, np.minimum(hr[s, 0], hr[s, 1]), np.maximum(hr[s, 0], hr[s, 1]), np.sqrt(rr)))
        cw = np.array(cw, float)
        lines.append(f"walks on the rays of {what} (host count, first {len(hc)} scenes, cells about {h:.2f} m wide): grid_cast slabs walked mean "
                     f"{cw[:, 0].mean():.2f} of {cw[:, 1].mean():.2f}, records visited median {np.median(cw[:, 2]):.0f}, mean {cw[:, 2].mean():.1f};  "
                     f"grid_segment records in the widened box median {np.median(sw):.0f}, mean {np.mean(sw):.1f};  cast / segment = "
                     f"{cw[:, 2].mean() / np.mean(sw):.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    kd.close()


if __name__ == "__main__":
    main()
