"""Cost of the device-side sensor and of a closed loop that never leaves the device.
  (a) amk_sim_render_depth, 256 scenes x 480 x 640 and x 48 x 64, with 16 and with 110 cylinders per scene (uint16 millimetres; the
      yaml's camera, scaled; every robot at its own pose over its own corridor).  HIP events around one call, 9 repetitions after 2
      warm-up calls, median.
  (b) wall time per period of a 256-robot, 40-period closed-loop depth flight: tests/_sim_flight.py device_depth_flights (sensor and
      vehicle on the device, no host copy until the end) against tests/_flight.py gpu_depth_flights (the parent's own path: command
      back, numpy vehicle, numpy render with a Python loop over the cylinders, upload, every period) on the same box, same sensor
      (48 x 64 / 2), same worlds.  The two fly slightly different vehicles and see different cylinder sets (tests/_sim_flight.py says
      how), so this compares the cost of a period, not trajectories.  One run each after a 2-period warm-up flight.
Nothing is gated on these numbers.
usage: python tools/experiments/sim_cost.py [--out FILE] [--robots 256] [--periods 40]"""
import sys
import time
sys.path.insert(0, ".")
import numpy as np, torch
from avoid_mpc_amd import flight
from avoid_mpc_amd.host import depth_params, sim_render_depth
from tests import _flight, _sim_flight

REPS, WARM = 9, 2
arg = lambda name, default: type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
out_path, ROBOTS, PERIODS = arg("--out", ""), arg("--robots", 256), arg("--periods", 40)
assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = torch.device("cuda")
lines = [f"amk_sim_render_depth and the closed loop on the device; {torch.cuda.get_device_name(0)}, one process",
         f"(a) HIP events around one call, median of {REPS} after {WARM} warm-up calls; us per call (min .. max), ns per pixel and cylinder"]


def render_cost(S, rows, cols, ncyl):
    rng = np.random.default_rng(ncyl)
    cyl = np.stack([np.stack([np.sort(rng.uniform(3.0, 80.0, ncyl)), rng.uniform(-8.0, 8.0, ncyl), rng.uniform(0.1, 0.5, ncyl)], axis=1)
                    for _ in range(S)])
    Twb = np.tile(np.eye(4), (S, 1, 1)); Twb[:, 0, 3] = rng.uniform(0.0, 40.0, S); Twb[:, 1, 3] = rng.uniform(-2.0, 2.0, S); Twb[:, 2, 3] = 1.5
    p = depth_params(pixel2meter=1e-3, fx=cols / 2.0, fy=cols / 2.0, cx=cols / 2.0, cy=rows / 2.0, Tbc=flight.TBC_YAML)
    cyl_d, Twb_d = torch.from_numpy(cyl).to(dev), torch.from_numpy(Twb).to(dev)
    out = torch.zeros((S, rows, cols), dtype=torch.int16, device=dev)
    call = lambda: sim_render_depth(cyl_d, Twb_d, p, rows, cols, out=out)
    for _ in range(WARM):
        call()
    torch.cuda.synchronize()
    t = []
    for _ in range(REPS):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); call(); z.record(); z.synchronize()
        t.append(a.elapsed_time(z) * 1e3)
    med = float(np.median(t))
    lines.append(f"  S = {S}, {rows} x {cols}, {ncyl:3d} cylinders: {med:10.1f} us   ({min(t):.1f} .. {max(t):.1f})   "
                 f"{med * 1e3 / (S * rows * cols * ncyl):.4f} ns per pixel and cylinder; returns in {float((out != 0).float().mean()):.2f} of the pixels")


for rows, cols in ((480, 640), (48, 64)):
    for ncyl in (16, 110):
        render_cost(256, rows, cols, ncyl)

seeds = list(range(5000, 5000 + ROBOTS))
kw = dict(cyl_per_m=1.5, x_first=3.0, length=60.0)
lines.append(f"(b) {ROBOTS} robots x {PERIODS} periods, configuration C1, sensor 48 x 64 / 2, {int(round(1.5 * 57))} cylinders per world; wall ms per period")
for name, fn in (("device_depth_flights (sensor and vehicle on the device)", lambda s, P: _sim_flight.device_depth_flights(s, "C1", P, world_kw=kw)),
                 ("gpu_depth_flights (numpy sensor and vehicle, every period)", lambda s, P: _flight.gpu_depth_flights(s, "C1", P, world_kw=kw, cam=_sim_flight.SIM_CAM))):
    fn(seeds[:4], 2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    log = fn(seeds, PERIODS)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / PERIODS
    lines.append(f"  {name:<62s} {ms:10.2f} ms per period   (mean x flown {float((log['x'][:, -1, 0] - log['x'][:, 0, 0]).mean()):.2f} m; "
                 f"includes the flight's set-up and its final copies)")
text = "\n".join(lines)
print(text)
if out_path:
    open(out_path, "w").write(text + "\n")
