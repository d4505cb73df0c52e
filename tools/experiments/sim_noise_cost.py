"""Cost of amk_sim_depth_noise and a first study of what the loop does with noisy frames, after tools/experiments/sim_truth_cost.py's
method: HIP events around one call, 9 timed calls after 2 warm-up calls, median (min .. max), one process.
  (a) a call at 256 x 480 x 640 and 256 x 48 x 64, U16 and F32, with everything on and with only the axial stage; beside each the
      achieved bytes/s (one read plus one write of the image) and this process's own device-to-device copy of the same buffer.
  (b) wall time per period of the 256-robot, 40-period flight through flight.WallWorld: without the noise call, with it (every stage
      off: the same flight plus the call; and the moderate setting), and without it again, in that order in this process.
  (c) the fleet flown with a keyframe map at three settings -- clean, moderate, harsh (SETTINGS below: this project's choices, no
      camera's data sheet is behind them and nothing is calibrated against a device) -- per setting the obstacle and edge cloud sizes
      per frame, the keyframe map's last_outliers and keyframe counts, and from amk_sim_clearance on the logged states the least true
      clearance and the robots that end inside a solid.
Nothing is gated on any of it.
usage: python tools/experiments/sim_noise_cost.py [--out FILE] [--robots 256] [--periods 40] [--study 1]"""
import sys
import time
sys.path.insert(0, ".")
import numpy as np

REPS, WARM, S = 9, 2, 256
P2M, Z_TOP = 1e-3, 4.0
AXIAL = dict(seed=1, sigma0=0.002, sigma2=0.0015)
SETTINGS = {
    "clean": dict(seed=11),
    "moderate": dict(seed=11, sigma0=0.001, sigma2=0.0015, p_drop=0.01, edge_jump=0.25, p_edge_drop=0.3, p_edge_fly=0.3, focal_baseline=38.0,
                     disparity_quantum=0.125, z_min=0.3, z_max=20.0),
    "harsh": dict(seed=11, sigma0=0.005, sigma2=0.006, p_drop=0.08, edge_jump=0.15, p_edge_drop=0.4, p_edge_fly=0.6, focal_baseline=19.0,
                  disparity_quantum=0.25, z_min=0.5, z_max=10.0),
}
KEYFRAMES = dict(max_frame_count=3, th_dist=0.1, th_count=10)
arg = lambda name, default: type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


if __name__ == "__main__":
    import torch
    from avoid_mpc_amd.host import sim_clearance, sim_depth_noise, sim_noise_params
    from tests import _sim_noise, _sim_world
    out_path, ROBOTS, PERIODS, STUDY = arg("--out", ""), arg("--robots", 256), arg("--periods", 40), arg("--study", 1)
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda")
    lines = [f"amk_sim_depth_noise; {torch.cuda.get_device_name(0)}, one process; HIP events around one call, median of {REPS} after {WARM} warm-up calls"]

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

    fmt = lambda t: f"{float(np.median(t)):8.1f} us ({min(t):.1f} .. {max(t):.1f})"
    rate = lambda nbytes, t: f"{2 * nbytes / (float(np.median(t)) * 1e-6) / 1e12:5.2f} TB/s"
    lines.append(f"(a) S = {S} scenes of tests/_sim_noise.py noise_images' frame (one frame, repeated; the stream differs per scene); bytes = one read + one write")
    for rows, cols in ((480, 640), (48, 64)):
        for dtype, tdtype in ((np.uint16, torch.int16), (np.float32, torch.float32)):
            one = _sim_noise.noise_images(1, 1, rows, cols, dtype)
            src = torch.from_numpy(one.view(np.int16) if dtype == np.uint16 else one).to(dev).repeat(S, 1, 1).contiguous()
            dst = torch.empty_like(src)
            nbytes = src.numel() * src.element_size()
            tc = timed(lambda: dst.copy_(src))
            row = f"  {S} x {rows} x {cols} {'U16' if dtype == np.uint16 else 'F32'} ({2 * nbytes / 1e6:7.1f} MB): copy {fmt(tc)} {rate(nbytes, tc)}"
            for name, setting in (("everything on", _sim_noise.EVERY_STAGE), ("axial only", AXIAL), ("everything off", {})):
                prm = sim_noise_params(setting)
                t = timed(lambda: sim_depth_noise(src, prm, P2M, 3, out=dst))
                row += f"   {name} {fmt(t)} {rate(nbytes, t)}"
            lines.append(row)
            del src, dst

    seeds = list(range(5000, 5000 + ROBOTS))
    kw = dict(cyl_per_m=1.5, x_first=3.0, length=60.0)
    lines.append(f"(b) {ROBOTS} robots x {PERIODS} periods, configuration C1, sensor 48 x 64 / 2, WallWorld, AMK_SIM_ATT_ACCEL, single frame; wall ms per period "
                 f"(set-up and final copies included)")
    _sim_world.device_world_flights(seeds[:4], "C1", 2, world_kw=kw)
    _sim_noise.device_noisy_flights(seeds[:4], SETTINGS["moderate"], "C1", 2, world_kw=kw)
    ms = []
    for name, run in (("without the noise call (device_world_flights itself)", lambda: _sim_world.device_world_flights(seeds, "C1", PERIODS, world_kw=kw)),
                      ("with the call, every stage off (the same flight)", lambda: _sim_noise.device_noisy_flights(seeds, SETTINGS["clean"], "C1", PERIODS, world_kw=kw)),
                      ("with the call, the moderate setting", lambda: _sim_noise.device_noisy_flights(seeds, SETTINGS["moderate"], "C1", PERIODS, world_kw=kw)),
                      ("without the noise call (device_world_flights itself)", lambda: _sim_world.device_world_flights(seeds, "C1", PERIODS, world_kw=kw))):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        log = run()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / PERIODS)
        lines.append(f"  {name:<56s} {ms[-1]:8.2f} ms per period   (mean x flown {float((log['x'][:, -1, 0] - log['x'][:, 0, 0]).mean()):.2f} m)")
    lines.append(f"  the call with every stage off adds {ms[1] - 0.5 * (ms[0] + ms[3]):+.2f} ms, the moderate setting {ms[2] - 0.5 * (ms[0] + ms[3]):+.2f} ms per period "
                 f"against the mean of the two runs without it, which differ from each other by {abs(ms[0] - ms[3]):.2f} ms")

    if STUDY:
        lines.append(f"(c) {ROBOTS} robots x {PERIODS} periods with a keyframe map {KEYFRAMES}; the settings (this project's choices, calibrated against no device):")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        for name, setting in SETTINGS.items():
            lines.append(f"    {name}: {setting}")
        for name, setting in SETTINGS.items():
            log = _sim_noise.device_noisy_flights(seeds, setting, "C1", PERIODS, world_kw=kw, keyframes=KEYFRAMES, study=True)
            truth = sim_clearance(up(log["cyl"]), up(log["box"]), up(log["x"]), cyl_counts=up(log["cyl_counts"]), z_top=Z_TOP)
            torch.cuda.synchronize()
            dist = truth["dist"].cpu().numpy()                                      # [F, periods + 1]
            cc, ec = log["cloud_counts"], log["edge_counts"]
            lines.append(f"  {name:<9s} obstacle cloud per frame: mean {cc.mean():6.1f} (min {cc.min()}, max {cc.max()}) of 768;  edge cloud: mean {ec.mean():6.1f} "
                         f"(min {ec.min()}, max {ec.max()});  keyframes per robot: mean {log['n_keyframes'].mean():.2f} (max {log['n_keyframes'].max()}), "
                         f"last_outliers: mean {log['last_outliers'].mean():.1f} (max {log['last_outliers'].max()}), map points: mean {log['map_points'].mean():.0f};  "
                         f"least true clearance of the fleet {dist.min():+.3f} m, robots ever inside a solid {int((dist < 0).any(axis=1).sum())}, "
                         f"ending inside one {int((dist[:, -1] < 0).sum())} of {ROBOTS};  mean x flown {float((log['x'][:, -1, 0] - log['x'][:, 0, 0]).mean()):.2f} m")
    text = "\n".join(lines)
    print(text)
    if out_path:
        open(out_path, "w").write(text + "\n")
