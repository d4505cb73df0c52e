"""Cost of amk_sim_render_world and of a closed loop with walls and a tilting vehicle, after tools/experiments/sim_cost.py's method:
HIP events around one call, 9 timed calls after 2 warm-up calls, median (min .. max).
  (a) zero boxes: 256 scenes x 480 x 640 and x 48 x 64 with 16 and 110 cylinders through amk_sim_render_depth (the parent's code,
      unchanged) and through amk_sim_render_world with max_box == 0, three repetitions interleaved old / new / old.  The condition:
      the world entry's median lies inside the range of the old entry's own 18 timings.  That range is whatever this run measures.
  (b) the same sizes with 16 and 64 boxes per scene added: us per call, and the added time per pixel and box beside the time per pixel
      and cylinder of (a).  Nothing is gated on these.
  (c) wall time per period of a 256-robot, 40-period flight through flight.WallWorld with AMK_SIM_ATT_ACCEL
      (tests/_sim_world.py device_world_flights), beside device_depth_flights on the same seeds (profiles/sim_cost.txt: 2.4 ms).
usage: python tools/experiments/sim_world_cost.py [--out FILE] [--robots 256] [--periods 40]"""
import sys
import time
sys.path.insert(0, ".")
import numpy as np, torch
from avoid_mpc_amd import flight
from avoid_mpc_amd.host import depth_params, sim_render_depth, sim_render_world
from tests import _sim_flight, _sim_world

REPS, WARM, S = 9, 2, 256
arg = lambda name, default: type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
out_path, ROBOTS, PERIODS = arg("--out", ""), arg("--robots", 256), arg("--periods", 40)
assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = torch.device("cuda")
lines = [f"amk_sim_render_world; {torch.cuda.get_device_name(0)}, one process; HIP events around one call, median of {REPS} after {WARM} warm-up calls"]


def timed(call):
    for _ in range(WARM):
        call()
    torch.cuda.synchronize()
    t = []
    for _ in range(REPS):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); call(); z.record(); z.synchronize()
        t.append(a.elapsed_time(z) * 1e3)
    return t


def scene(rows, cols, ncyl, nbox):
    """sim_cost.py's worlds and poses, plus nbox wall-like boxes per scene along the same corridor"""
    rng = np.random.default_rng(ncyl)
    cyl = np.stack([np.stack([np.sort(rng.uniform(3.0, 80.0, ncyl)), rng.uniform(-8.0, 8.0, ncyl), rng.uniform(0.1, 0.5, ncyl)], axis=1)
                    for _ in range(S)])
    Twb = np.tile(np.eye(4), (S, 1, 1)); Twb[:, 0, 3] = rng.uniform(0.0, 40.0, S); Twb[:, 1, 3] = rng.uniform(-2.0, 2.0, S); Twb[:, 2, 3] = 1.5
    rb = np.random.default_rng([ncyl, nbox])
    yaw = rb.uniform(-0.3, 0.3, (S, nbox))
    box = np.stack([rb.uniform(3.0, 80.0, (S, nbox)), rb.uniform(-8.0, 8.0, (S, nbox)), np.full((S, nbox), 0.05), rb.uniform(0.5, 3.0, (S, nbox)),
                    np.cos(yaw), np.sin(yaw), np.where(rb.uniform(size=(S, nbox)) < 0.3, 2.5, 0.0), np.full((S, nbox), 4.0)], axis=2)
    p = depth_params(pixel2meter=1e-3, fx=cols / 2.0, fy=cols / 2.0, cx=cols / 2.0, cy=rows / 2.0, Tbc=flight.TBC_YAML)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return up(cyl), up(box), up(Twb), p, torch.zeros((S, rows, cols), dtype=torch.int16, device=dev)


fmt = lambda t: f"{float(np.median(t)):9.1f} us ({min(t):.1f} .. {max(t):.1f})"
lines.append("(a) zero boxes: amk_sim_render_depth / amk_sim_render_world(max_box = 0) / amk_sim_render_depth again")
base = {}
for rows, cols in ((480, 640), (48, 64)):
    for ncyl in (16, 110):
        cyl, box, Twb, p, out = scene(rows, cols, ncyl, 0)
        old = lambda: sim_render_depth(cyl, Twb, p, rows, cols, out=out)
        new = lambda: sim_render_world(cyl, box, Twb, p, rows, cols, out=out)
        o1, n1, o2 = timed(old), timed(new), timed(old)
        lo, hi, med = min(o1 + o2), max(o1 + o2), float(np.median(n1))
        base[rows, cols, ncyl] = med
        lines.append(f"  S = {S}, {rows} x {cols}, {ncyl:3d} cylinders: old {fmt(o1)}   world {fmt(n1)}   old {fmt(o2)}   "
                     f"old's range {lo:.1f} .. {hi:.1f} (spread {hi - lo:.1f} us): the world entry's median is {'INSIDE' if lo <= med <= hi else 'OUTSIDE'}"
                     f"   {med * 1e3 / (S * rows * cols * ncyl):.4f} ns per pixel and cylinder")
lines.append("(b) boxes added; us per call, and the time the boxes add per pixel and box")
for rows, cols in ((480, 640), (48, 64)):
    for ncyl in (16, 110):
        for nbox in (16, 64):
            cyl, box, Twb, p, out = scene(rows, cols, ncyl, nbox)
            t = timed(lambda: sim_render_world(cyl, box, Twb, p, rows, cols, out=out))
            med = float(np.median(t))
            none = torch.zeros_like(out); sim_render_world(cyl, box[:, :0].contiguous(), Twb, p, rows, cols, out=none)
            lines.append(f"  S = {S}, {rows} x {cols}, {ncyl:3d} cylinders, {nbox:2d} boxes: {fmt(t)}   "
                         f"{(med - base[rows, cols, ncyl]) * 1e3 / (S * rows * cols * nbox):.4f} ns per pixel and box; a box answers "
                         f"{float((out != none).float().mean()):.2f} of the pixels")

seeds = list(range(5000, 5000 + ROBOTS))
kw = dict(cyl_per_m=1.5, x_first=3.0, length=60.0)
lines.append(f"(c) {ROBOTS} robots x {PERIODS} periods, configuration C1, sensor 48 x 64 / 2; wall ms per period (set-up and final copies included)")
for name, fn in (("device_world_flights (WallWorld: cylinders and 12 boxes, AMK_SIM_ATT_ACCEL)", lambda s, P: _sim_world.device_world_flights(s, "C1", P, world_kw=kw)),
                 ("device_depth_flights (cylinders only, level: profiles/sim_cost.txt's loop)", lambda s, P: _sim_flight.device_depth_flights(s, "C1", P, world_kw=kw))):
    fn(seeds[:4], 2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    log = fn(seeds, PERIODS)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / PERIODS
    extra = ""
    if "Twb" in log:
        extra = (f"; largest tilt {float(np.degrees(np.arccos(np.clip(log['Twb'][:, :, 2, 2], -1, 1))).max()):.1f} deg; least clearance: cylinders "
                 f"{float(log['clearance'].min()):.2f} m, box faces {float(log['box_clearance'].min()):.2f} m")
    lines.append(f"  {name:<80s} {ms:8.2f} ms per period   (mean x flown {float((log['x'][:, -1, 0] - log['x'][:, 0, 0]).mean()):.2f} m{extra})")
text = "\n".join(lines)
print(text)
if out_path:
    open(out_path, "w").write(text + "\n")
