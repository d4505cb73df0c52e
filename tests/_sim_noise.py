"""Closed-loop flights that see the world through a noisy sensor (TEST INFRASTRUCTURE, beside tests/_sim_world.py).

device_noisy_flights is tests/_sim_world.py's device_world_flights loop with a second depth buffer: per period
    sim_depth_noise(render -> noisy, frame = t)  ->  Pipeline.submit(depth=noisy, ...)  ->  wait_stream  ->  sim_vehicle_step_att  ->  sim_render_world
on the device, still without a host copy or a host wait in the loop.  host_twin_noisy_flights is host_twin_world_flights with
flight.depth_noise_ordered applied to the host frames.  Robot i of a fleet is scene scene_id0 + i of the stream, whatever the fleet."""
import numpy as np

from avoid_mpc_amd import flight
from tests._sim_flight import MAX_RANGE, POSE_QUANTUM, Z_TOP
from tests._sim_world import _empty_logs, _finish, _setup, host_frames


P2M = 1e-3                # the flights' pixel2meter
# a noise setting that exercises every stage (this project's choice, calibrated against no device)
EVERY_STAGE = dict(seed=2024, sigma0=0.002, sigma2=0.0015, p_drop=0.03, edge_jump=0.25, p_edge_drop=0.3, p_edge_fly=0.4,
                   focal_baseline=38.0, disparity_quantum=0.125, z_min=0.3, z_max=25.0)


def noise_images(seed, S, rows, cols, dtype, pixel2meter=P2M):
    """Hand-made frames for the noise tests, [S, rows, cols] of `dtype`: a near surface and a far one with a slanted step edge through
    the interior (so every border and corner has edge pixels in some scene), a no-return block and isolated no-return pixels, depths
    on the U16 clamp (65.535 m at 1e-3) and on both sides of the range gates 0.3 m and 25 m, and for float32 NaN, +-inf and
    negative pixels."""
    rng = np.random.default_rng([seed, rows, cols])
    v, u = np.mgrid[0:rows, 0:cols]
    img = np.zeros((S, rows, cols))
    for s in range(S):
        a, b = rng.uniform(-1.0, 1.0), rng.uniform(-0.4, 0.4)
        near = 1.5 + 0.01 * u + 0.02 * v + rng.uniform(0.0, 0.5)
        far = 6.0 + 0.05 * u + rng.uniform(0.0, 2.0)
        img[s] = np.where((u - cols / 2.0) + a * (v - rows / 2.0) + b < 0, near, far)
        k = max(1, rows * cols // 12)
        pick = lambda n: (rng.integers(0, rows, n), rng.integers(0, cols, n))
        img[s][pick(k)] = 0.0                                                     # isolated pixels without a return
        img[s][pick(k)] = rng.choice([0.25, 0.2999, 0.3, 0.3001, 24.999, 25.0, 25.001, 65.535, 65.6, 70.0, 0.0004], k)
        if rows >= 4 and cols >= 4:
            img[s, rows // 4:rows // 4 + 2, cols // 4:cols // 4 + 3] = 0.0       # a block without a return
        img[s, 0, 0] = [1.0, 0.0, 9.0][s % 3]                                     # a corner that holds a return, none, a far one
    pix = img / pixel2meter
    if np.dtype(dtype) == np.uint16:
        return np.clip(np.rint(pix), 0, 65535).astype(np.uint16)
    pix = pix.astype(np.float32)
    flat = pix.reshape(S, -1)
    for s in range(S):
        where = rng.integers(0, rows * cols, 5)
        flat[s, where] = np.array([np.nan, np.inf, -np.inf, -1500.0, -0.0], np.float32)[:where.size]
    if rows * cols > 8:
        flat[0, 7] = np.array(0x7FC12345, np.uint32).view(np.float32)             # a NaN with a payload: copied bit for bit
    return pix


def device_noisy_flights(seeds, noise, cfg="C1", periods=40, world_kw=None, keyframes=None, cam=None, attitude=flight.ATT_ACCEL, gz=flight.GZ,
                         scene_id0=0, study=False):
    """-> device_world_flights' dict; `noise`: what host.sim_noise_params takes.  study=True (measurements, not tests) also logs
    cloud_counts / edge_counts [F, periods] -- amk_depth_to_clouds on the frames the pipeline is given, with the previous period's
    camera pose as Twc -- and the keyframe map's last_outliers."""
    from avoid_mpc_amd.host import sim_depth_noise, sim_noise_params, sim_render_world, sim_vehicle_step_att
    torch, c, worlds, x0, ref0, cyl, counts, box, Twb0, dp, pl, ABc = _setup(seeds, cfg, world_kw, cam, keyframes, queue_depth=2)
    dev = torch.device("cuda", torch.cuda.current_device())
    F = len(seeds)
    f64 = dict(dtype=torch.float64, device=dev)
    up = lambda a: torch.from_numpy(a).to(dev)
    x, Twb, cyl_d, counts_d, box_d, r0 = up(x0), up(Twb0), up(cyl), up(counts), up(box), up(ref0)
    cmd = torch.zeros((F, 3), **f64)
    depth = torch.zeros((F, c["rows"], c["cols"]), dtype=torch.int16, device=dev)
    noisy = torch.zeros_like(depth)
    prm = sim_noise_params(noise)
    log_x = torch.zeros((periods, F, 10), **f64); log_u = torch.zeros((periods, F, 4), **f64); log_cmd = torch.zeros((periods, F, 3), **f64)
    log_T = torch.zeros((periods, F, 4, 4), **f64); log_flags = torch.zeros((periods, F, 4), dtype=torch.int32, device=dev)
    render = lambda: sim_render_world(cyl_d, box_d, Twb, dp, c["rows"], c["cols"], cyl_counts=counts_d, z_top=Z_TOP, max_range=MAX_RANGE, out=depth)
    render()
    if study:
        from avoid_mpc_amd.host import depth_to_clouds
        Tbc = up(np.ascontiguousarray(c["Tbc"], np.float64))
        Twc_prev = torch.matmul(Twb, Tbc)
        log_counts = torch.zeros((periods, 2, F), dtype=torch.int32, device=dev)
    for t in range(periods):                                   # no host copy and no host wait in here
        sim_depth_noise(depth, prm, c["pixel2meter"], t, scene_id0=scene_id0, out=noisy)
        if study:
            _, n_cloud, _, n_edge = depth_to_clouds(noisy, dp, Twb, Twc_prev)
            log_counts[t, 0].copy_(n_cloud); log_counts[t, 1].copy_(n_edge)
            Twc_prev = torch.matmul(Twb, Tbc)
        tk = pl.submit(None, None, ref_path_init=r0 if t == 0 else None, odom=x, cmd_out=cmd, keep_warm_start=t > 0, depth=noisy, Twb=Twb)
        pl.wait_stream(tk)
        o = pl.output_tensors(tk)
        log_u[t].copy_(o["u"]); log_flags[t].copy_(o["flags"]); log_cmd[t].copy_(cmd)
        sim_vehicle_step_att(ABc, cmd, x, Twb, pose_quantum=POSE_QUANTUM, attitude=attitude, gz=gz)
        log_x[t].copy_(x); log_T[t].copy_(Twb)                 # the state and the pose AFTER period t
        render()
    pl.drain()
    torch.cuda.synchronize()
    logs = _empty_logs(F, periods, x0, Twb0)
    for key, log in (("x", log_x), ("Twb", log_T)):
        logs[key][:, 1:] = np.moveaxis(log.cpu().numpy(), 0, 1)
    for key, log in (("u", log_u), ("flags", log_flags), ("cmd", log_cmd)):
        logs[key][:] = np.moveaxis(log.cpu().numpy(), 0, 1)
    if study:
        logs["cloud_counts"], logs["edge_counts"] = log_counts[:, 0].cpu().numpy().T, log_counts[:, 1].cpu().numpy().T
        if keyframes:
            logs["last_outliers"] = pl.kfmap_state(0)["last_outliers"]
    return _finish(logs, pl, keyframes, worlds, cyl, counts, box)


def host_twin_noisy_flights(seeds, noise, cfg="C1", periods=40, world_kw=None, keyframes=None, cam=None, attitude=flight.ATT_ACCEL, gz=flight.GZ,
                            scene_id0=0):
    """The same pipeline; the sensor, its noise and the vehicle in numpy on the host between the periods -> the same dict of arrays,
    and `changed` [periods]: how many pixels of each period's frames the noise altered."""
    torch, c, worlds, x0, ref0, cyl, counts, box, Twb, dp, pl, ABc = _setup(seeds, cfg, world_kw, cam, keyframes, queue_depth=1)
    dev = torch.device("cuda", torch.cuda.current_device())
    F = len(seeds)
    x = x0.copy()
    logs = _empty_logs(F, periods, x0, Twb)
    changed = np.zeros(periods, np.int64)
    for t in range(periods):
        clean = host_frames(cyl, counts, box, Twb, c)
        frames = flight.depth_noise_ordered(clean, noise, c["pixel2meter"], t, scene_id0)
        changed[t] = int((frames != clean).sum())
        depth = torch.from_numpy(frames.view(np.int16)).to(dev)
        Twb_d = torch.from_numpy(Twb).to(dev); odom = torch.from_numpy(x).to(dev); cmd = torch.zeros((F, 3), dtype=torch.float64, device=dev)
        r0 = torch.from_numpy(ref0).to(dev) if t == 0 else None
        tk = pl.submit(None, None, ref_path_init=r0, odom=odom, cmd_out=cmd, keep_warm_start=t > 0, depth=depth, Twb=Twb_d)
        pl.wait(tk)
        o = pl.outputs(tk)
        a = cmd.cpu().numpy()
        x, Twb = flight.vehicle_attitude_ordered(ABc, x, a, POSE_QUANTUM, attitude, gz)
        logs["x"][:, t + 1] = x; logs["Twb"][:, t + 1] = Twb; logs["u"][:, t] = o["u"]; logs["flags"][:, t] = o["flags"]; logs["cmd"][:, t] = a
    logs["changed"] = changed
    return _finish(logs, pl, keyframes, worlds, cyl, counts, box)
