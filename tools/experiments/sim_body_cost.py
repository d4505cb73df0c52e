"""Cost of amk_sim_vehicle_step_body and a first study of a fleet whose plant is not the planner's model, after
tools/experiments/sim_noise_cost.py's method: HIP events around one call, 9 timed calls after 2 warm-up calls, median (min .. max),
one process.
  (a) a call at 256 scenes for n_sub 1, 8 and 33, beside amk_sim_vehicle_step_att (the affine vehicle with AMK_SIM_ATT_ACCEL).
  (b) wall time per period of the 256-robot, 40-period flight through flight.WallWorld with the affine vehicle, the rigid body, and
      both again, in that order in this process: the spread between two runs of the same vehicle is the yardstick.  Beside each the
      solves and interior-point iterations per robot and period (the step's flags): what the step spends on the state it is given.
  (c) the fleet under amk_sim_clearance on the logged states, for the affine vehicle and the rigid body (defaults: this project's
      choices, calibrated against no vehicle): robots ever inside a solid, the least true clearance; for both vehicles (the affine one
      flown once more under tests/_sim_truth.py's monitor) the distance between the MPC's predicted first state (x0array row 1) and the
      plant's next state per period; and the first-order time constant fitted to the rigid body's acceleration response, beside the
      model's 1 / prm.tau.
Nothing is gated on any of it.
usage: python tools/experiments/sim_body_cost.py [--out FILE] [--robots 256] [--periods 40] [--study 1]"""
import sys
import time
sys.path.insert(0, ".")
import numpy as np

REPS, WARM, S = 9, 2, 256
Z_TOP = 4.0
arg = lambda name, default: type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


if __name__ == "__main__":
    import torch
    from avoid_mpc_amd import flight
    from avoid_mpc_amd.host import plant_model, sim_body_params, sim_body_reset, sim_clearance, sim_vehicle_step_att, sim_vehicle_step_body
    from tests import _flight, _sim_body, _sim_truth, _sim_world
    out_path, ROBOTS, PERIODS, STUDY = arg("--out", ""), arg("--robots", 256), arg("--periods", 40), arg("--study", 1)
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda")
    prm, _ = _flight.make_prm("C1")
    lines = [f"amk_sim_vehicle_step_body; {torch.cuda.get_device_name(0)}, one process; HIP events around one call, median of {REPS} after {WARM} warm-up calls"]

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
    rng = np.random.default_rng(1)
    x = torch.from_numpy(np.concatenate([rng.uniform(-5, 5, (S, 3)), np.zeros((S, 7))], axis=1)).to(dev)
    cmd = torch.from_numpy(np.array([0.0, 0.0, flight.GZ]) + rng.uniform(-3, 3, (S, 3))).to(dev)
    body = torch.zeros((S, flight.BODY_DOUBLES), dtype=torch.float64, device=dev)
    Twb = torch.zeros((S, 4, 4), dtype=torch.float64, device=dev)
    sim_body_reset(body, flight.GZ)
    lines.append(f"(a) one call at {S} scenes (one block of four wavefronts), control period {prm.dt} s, pose_quantum 1e6, d_Twb given")
    for n_sub in (1, 8, 33):
        p = sim_body_params(prm.dt, n_sub=n_sub)
        t = timed(lambda: sim_vehicle_step_body(p, cmd, x, body, Twb, pose_quantum=1e6))
        lines.append(f"  n_sub = {n_sub:2d}: {fmt(t)}")
    ABc = plant_model(prm.tau, prm.dt)
    t = timed(lambda: sim_vehicle_step_att(ABc, cmd, x, Twb, pose_quantum=1e6))
    lines.append(f"  amk_sim_vehicle_step_att, AMK_SIM_ATT_ACCEL (two launches): {fmt(t)}")
    t = timed(lambda: None)
    lines.append(f"  an empty pair of events: {fmt(t)}")

    seeds = list(range(5000, 5000 + ROBOTS))
    kw = dict(cyl_per_m=1.5, x_first=3.0, length=60.0)
    lines.append(f"(b) {ROBOTS} robots x {PERIODS} periods, configuration C1, sensor 48 x 64 / 2, WallWorld, single frame; wall ms per period (set-up and "
                 f"final copies included)")
    _sim_world.device_world_flights(seeds[:4], "C1", 2, world_kw=kw)
    _sim_body.device_body_flights(seeds[:4], "C1", 2, world_kw=kw)
    ms, logs = [], []
    affine_run = ("the affine vehicle, AMK_SIM_ATT_ACCEL (device_world_flights)", lambda: _sim_world.device_world_flights(seeds, "C1", PERIODS, world_kw=kw))
    body_run = ("the rigid body, defaults (device_body_flights)", lambda: _sim_body.device_body_flights(seeds, "C1", PERIODS, world_kw=kw, study=True))
    for name, run in (affine_run, body_run, affine_run, body_run):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        log = run()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / PERIODS)
        logs.append(log)
        fl = log["flags"]                                                          # {isSafety, solves done, worst status, interior-point iterations}
        lines.append(f"  {name:<62s} {ms[-1]:8.2f} ms per period   (mean x flown {float((log['x'][:, -1, 0] - log['x'][:, 0, 0]).mean()):.2f} m;  per robot and "
                     f"period {fl[:, :, 1].mean():.3f} solves, {fl[:, :, 3].mean():.2f} interior-point iterations, {100.0 * (fl[:, :, 0] == 0).mean():.1f} % not safe)")
    lines.append(f"  the rigid body (with the study's copy of the predicted state per period) differs by {0.5 * (ms[1] + ms[3]) - 0.5 * (ms[0] + ms[2]):+.2f} ms per period "
                 f"from the affine vehicle; the two affine runs differ from each other by {abs(ms[0] - ms[2]):.2f} ms, the two rigid-body runs by {abs(ms[1] - ms[3]):.2f} ms")

    if STUDY:
        p = flight.body_params(prm.dt)
        lines.append(f"(c) the same flights under amk_sim_clearance on the logged states; the rigid body's parameters (this project's choices, calibrated "
                     f"against no vehicle): n_sub {p.n_sub}, h {p.h:.6f}, k_att {p.k_att}, rate_max {p.rate_max}, k_rate {p.k_rate:.4f}, k_thrust {p.k_thrust:.4f}, "
                     f"f in [{p.f_min}, {p.f_max:.2f}], drag {p.drag}, cog_window {p.cog_window}")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        for name, log in (("affine", logs[0]), ("rigid body", logs[1])):
            truth = sim_clearance(up(log["cyl"]), up(log["box"]), up(log["x"]), cyl_counts=up(log["cyl_counts"]), z_top=Z_TOP)
            torch.cuda.synchronize()
            dist = truth["dist"].cpu().numpy()                                      # [F, periods + 1]
            lines.append(f"  {name:<10s} robots ever inside a solid {int((dist < 0).any(axis=1).sum())}, ending inside one {int((dist[:, -1] < 0).sum())} of "
                         f"{ROBOTS};  least true clearance of the fleet {dist.min():+.3f} m, median over robots of the least {float(np.median(dist.min(axis=1))):+.3f} m;  "
                         f"largest tilt {float(np.arccos(np.clip(log['Twb'][:, :, 2, 2], -1, 1)).max()):.3f} rad")
        # the MPC's predicted first state against the plant's next state.  The step starts a pass from the odometry advanced by its clock
        # model, so the affine vehicle does not give 0 either: it is flown once more under tests/_sim_truth.py's monitor, which logs x0array
        affine = _sim_truth.device_truth_flights(seeds, "C1", PERIODS, world_kw=kw)
        assert np.array_equal(affine["x"], logs[0]["x"])                            # (the monitor only reads: the same flight)
        lines.append("  the MPC's predicted first state (x0array row 1) against the plant's next state; per period over the fleet, median (max):")
        for name, pred, log in (("affine", affine["x0array"][:, :, 1, :10], affine), ("rigid body", logs[1]["x_pred"], logs[1])):
            err = pred - log["x"][:, 1:]
            dp, dv, da = (np.linalg.norm(err[:, :, a:b], axis=2) for a, b in ((0, 3), (4, 7), (7, 10)))
            for t in list(range(0, PERIODS, max(1, PERIODS // 4))):
                lines.append(f"    {name:<10s} period {t:2d}: |dp| {np.median(dp[:, t]):.4f} ({dp[:, t].max():.4f}) m   |dv| {np.median(dv[:, t]):.4f} ({dv[:, t].max():.4f}) m/s   "
                             f"|da| {np.median(da[:, t]):.4f} ({da[:, t].max():.4f}) m/s^2")
            lines.append(f"    {name:<10s} all periods: |dp| median {np.median(dp):.4f} m, max {dp.max():.4f} m;  |dv| median {np.median(dv):.4f}, max {dv.max():.4f} m/s;  "
                         f"|da| median {np.median(da):.4f}, max {da.max():.4f} m/s^2")
        log = logs[1]
        # first-order fit a+ - a = k (u - g - a): least squares over the fleet and the periods, per axis; tau_fit = -dt / log(1 - k)
        g = np.array([0.0, 0.0, flight.GZ])
        a0, a1, u = log["x"][:, :-1, 7:10], log["x"][:, 1:, 7:10], log["cmd"] - g
        fit = []
        for i in range(3):
            num, den = ((a1[..., i] - a0[..., i]) * (u[..., i] - a0[..., i])).sum(), ((u[..., i] - a0[..., i]) ** 2).sum()
            k = num / den
            fit.append(-prm.dt / np.log(1.0 - k) if 0 < k < 1 else float("nan"))
        lines.append(f"  first-order time constant fitted to the plant's acceleration response (x, y, z): {fit[0]:.4f}, {fit[1]:.4f}, {fit[2]:.4f} s;  "
                     f"the MPC's model: 1 / prm.tau = {1.0 / prm.tau[0]:.4f}, {1.0 / prm.tau[1]:.4f}, {1.0 / prm.tau[2]:.4f} s")
    text = "\n".join(lines)
    print(text)
    if out_path:
        open(out_path, "w").write(text + "\n")
