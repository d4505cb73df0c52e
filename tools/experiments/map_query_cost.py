"""Cost of the map's own queries (amk_kfmap_query_nearest, csrc/map_query.hip) at the `--keyframes 3` flight shape: S = 256 scenes,
20 queries, K = 8, a map grown by 6 periods of 50 k-point frames.  Three legs, same queries:
  fast    every query on QueryNearest's fast path (cam = NULL)
  merge   every query on the merge path (a camera whose depth_max no query passes)
  floor   amk_kd_search on ONE 256-scene handle that holds the same current frame: the same searches without the map's indirection
HIP events around REPS launches on one stream, LEGS alternating inside every cycle, median over the cycles after warm-up; one process.
usage: python tools/experiments/map_query_cost.py [--out FILE]"""
import sys
sys.path.insert(0, ".")
import numpy as np, torch
from avoid_mpc_amd import capi
from avoid_mpc_amd.host import KdBatch, KfMap

S, NQ, K, N, NE, PERIODS, STEP = 256, 20, 8, 50000, 5000, 6, 0.3
REPS, CYCLES, WARM = 200, 9, 2
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
dev = torch.device("cuda")
g = torch.Generator(device="cuda"); g.manual_seed(5)
Tbc = np.eye(4); Tbc[:3, :3] = [[0, 0, 1], [-1, 0, 0], [0, -1, 0]]        # the camera looks along body +x
gmap = KfMap(S, N, NE, 3, 0.1, 10, 0.1, Tbc)
box = lambda n, d: torch.rand((S, n, 3), generator=g, device=dev) * torch.tensor([20.0, 20.0, 5.0], device=dev) + torch.tensor([d + 2.0, -10.0, 0.0], device=dev)
for t in range(PERIODS):
    d = STEP * t
    cloud, edge = box(N, d).contiguous(), box(NE, d).contiguous()
    Twc = np.tile(Tbc, (S, 1, 1)); Twc[:, 0, 3] = d; Twc[:, 2, 3] = 1.5
    gmap.add_vertex(cloud, edge, torch.from_numpy(Twc).to(dev))
    gmap.update()
torch.cuda.synchronize()
state = gmap.state()
kd = KdBatch(S, N); kd.build(cloud)
q = (torch.rand((S, NQ, 3), generator=g, device=dev, dtype=torch.float64) * torch.tensor([10.0, 8.0, 3.0], device=dev, dtype=torch.float64)
     + torch.tensor([d + 1.0, -4.0, 0.0], device=dev, dtype=torch.float64)).contiguous()
blind = capi.FrameCamera(32.0, 32.0, 32.0, 24.0, 1e-6, 64, 48)            # nothing is nearer than a micrometre: every query merges
o_fast, o_merge = gmap.query_nearest(q, K), gmap.query_nearest(q, K, cam=blind)
o_floor = kd.search(q, K)
torch.cuda.synchronize()
assert torch.equal(o_fast["sqdist"], o_floor["sqdist"]) and (o_fast["frame"] == 0).all()
n_frames = int(state["n_query_frames"].min()), int(state["n_query_frames"].max())
from_kf = float((o_merge["frame"] > 0).double().mean())
legs = {"fast": lambda: gmap.query_nearest(q, K, out=o_fast), "merge": lambda: gmap.query_nearest(q, K, cam=blind, out=o_merge),
        "floor": lambda: kd.search(q, K, out=o_floor)}
times = {k: [] for k in legs}
for c in range(WARM + CYCLES):
    for name, fn in legs.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record(); b.synchronize()
        if c >= WARM:
            times[name].append(a.elapsed_time(b) * 1e3 / REPS)
lines = [f"map query cost, one MI355X; HIP events around {REPS} launches, median of {CYCLES} cycles after {WARM} warm-up cycles, legs alternating, one process",
         f"S = {S} scenes x {NQ} queries, K = {K}; map grown by {PERIODS} periods of {N}-point frames (max_frame_count 3): {n_frames[0]} .. {n_frames[1]} query frames per scene; "
         f"{100 * from_kf:.1f} % of the merged neighbours come from a keyframe",
         "  leg      us per launch (median; min .. max)"]
for name in legs:
    v = np.array(times[name])
    lines.append(f"  {name:7s}  {np.median(v):8.1f}   ({v.min():.1f} .. {v.max():.1f})")
m = {k: float(np.median(v)) for k, v in times.items()}
lines.append(f"  fast / floor = {m['fast'] / m['floor']:.3f},  merge / floor = {m['merge'] / m['floor']:.3f},  merge / fast = {m['merge'] / m['fast']:.3f}")
print("\n".join(lines))
if out_path:
    open(out_path, "w").write("\n".join(lines) + "\n")
