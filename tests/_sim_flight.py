"""Closed-loop depth flights whose sensor and vehicle run on the device (TEST INFRASTRUCTURE, beside tests/_flight.py).

device_depth_flights flies the loop of _flight.gpu_depth_flights -- TASK-mode pipeline frames that start at the depth image -- with
amk_sim_vehicle_step and amk_sim_render_depth between the periods instead of numpy: per period
    Pipeline.submit(depth=..., Twb=..., odom=x, cmd_out=cmd)  ->  wait_stream  ->  sim_vehicle_step  ->  sim_render_depth  ->  next submit,
the slot's stream ordered behind the sensor by input_ready.  Nothing is copied to the host until the flight ends: the logs are
device-side ring buffers.  host_twin_depth_flights is the same pipeline with numpy's restatements (flight.vehicle_step_ordered,
flight.render_depth_ordered + quantise_depth) between the periods and a host copy each way, period by period.

Both differ from gpu_depth_flights in three stated ways: the vehicle is the affine model at con_dt (not RK4 re-integrated per period),
the sensor sees every cylinder of the world (no per-period selection around the vehicle), and the frames are float64-ordered.
"""
import numpy as np

from avoid_mpc_amd import flight
from tests import _flight

SIM_CAM = dict(rows=48, cols=64, pixel2meter=1e-3, depth_min=0.1, depth_max=60.0, resize_scale=2.0, fx=32.0, fy=32.0, cx=32.0, cy=24.0,
               Tbc=flight.TBC_YAML)   # the yaml's 640 x 480 sensor / 10, down-scaled by 2 more: 768-point frames
POSE_QUANTUM = 1e6                     # the depth callback's pose: the odometry rounded to a micrometre (_flight._depth_frame)
Z_TOP, MAX_RANGE = 4.0, 60.0           # flight.render_depth's defaults


def _setup(seeds, cfg, world_kw, cam, keyframes, queue_depth):
    import torch
    from avoid_mpc_amd.host import Pipeline, depth_params, plant_model
    prm, _ = _flight.make_prm(cfg)
    c = cam or SIM_CAM
    F = len(seeds)
    worlds = [flight.FlightWorld(int(s), prm, 1000, **(world_kw or {})) for s in seeds]
    st = [flight.initial_state(int(s), prm) for s in seeds]
    x0 = np.stack([a for a, _ in st]); ref0 = np.stack([b for _, b in st])
    cyl = np.stack([np.stack([w.cx, w.cy, w.cr], axis=1) for w in worlds])          # [F, ncyl, 3]: every world has the same count
    Twb0 = np.tile(np.eye(4), (F, 1, 1)); Twb0[:, :3, 3] = np.rint(x0[:, 0:3] * POSE_QUANTUM) / POSE_QUANTUM
    cap = int(c["cols"] / c["resize_scale"]) * int(c["rows"] / c["resize_scale"])
    dp = depth_params(c["pixel2meter"], c["depth_min"], c["depth_max"], c["resize_scale"], c["fx"], c["fy"], c["cx"], c["cy"], c["Tbc"])
    pl = Pipeline(1, F, cap, cap, prm, queue_depth=queue_depth, depth=dp,
                  keyframes=dict(keyframes, depth_min=c["depth_min"]) if keyframes else None)
    ABc = plant_model(prm.tau, prm.dt)
    return torch, prm, c, worlds, x0, ref0, cyl, Twb0, dp, pl, ABc


def device_depth_flights(seeds, cfg="C1", periods=40, world_kw=None, keyframes=None, cam=None, ring=None):
    """-> dict of arrays [F, ...]: x [F, periods + 1, 10], u [F, periods, 4], flags [F, periods, 4], cmd [F, periods, 3], clearance.
    ring: periods the device-side logs hold (default: all of them; fewer keeps the newest `ring` periods, older rows are zero)."""
    from avoid_mpc_amd.host import sim_render_depth, sim_vehicle_step
    torch, prm, c, worlds, x0, ref0, cyl, Twb0, dp, pl, ABc = _setup(seeds, cfg, world_kw, cam, keyframes, queue_depth=2)
    dev = torch.device("cuda", torch.cuda.current_device())
    F, R = len(seeds), int(ring or periods)
    f64 = dict(dtype=torch.float64, device=dev)
    x = torch.from_numpy(x0).to(dev); Twb = torch.from_numpy(Twb0).to(dev); cyl_d = torch.from_numpy(cyl).to(dev)
    r0 = torch.from_numpy(ref0).to(dev); cmd = torch.zeros((F, 3), **f64)
    depth = torch.zeros((F, c["rows"], c["cols"]), dtype=torch.int16, device=dev)
    log_x = torch.zeros((R, F, 10), **f64); log_u = torch.zeros((R, F, 4), **f64); log_cmd = torch.zeros((R, F, 3), **f64)
    log_flags = torch.zeros((R, F, 4), dtype=torch.int32, device=dev)
    render = lambda: sim_render_depth(cyl_d, Twb, dp, c["rows"], c["cols"], z_top=Z_TOP, max_range=MAX_RANGE, out=depth)
    render()
    for t in range(periods):                                   # no host copy and no host wait in here
        tk = pl.submit(None, None, ref_path_init=r0 if t == 0 else None, odom=x, cmd_out=cmd, keep_warm_start=t > 0, depth=depth, Twb=Twb)
        pl.wait_stream(tk)                                     # torch's stream behind the step; the next submit's input_ready behind what follows
        o = pl.output_tensors(tk)
        log_u[t % R].copy_(o["u"]); log_flags[t % R].copy_(o["flags"]); log_cmd[t % R].copy_(cmd)
        sim_vehicle_step(ABc, cmd, x, Twb, pose_quantum=POSE_QUANTUM)
        log_x[t % R].copy_(x)                                  # the state AFTER period t
        render()
    pl.drain()
    torch.cuda.synchronize()
    logs = dict(x=np.zeros((F, periods + 1, 10)), u=np.zeros((F, periods, 4)), flags=np.zeros((F, periods, 4), np.int32),
                cmd=np.zeros((F, periods, 3)))
    logs["x"][:, 0] = x0
    hx, hu, hf, hc = (v.cpu().numpy() for v in (log_x, log_u, log_flags, log_cmd))
    for t in range(max(0, periods - R), periods):
        logs["x"][:, t + 1] = hx[t % R]; logs["u"][:, t] = hu[t % R]; logs["flags"][:, t] = hf[t % R]; logs["cmd"][:, t] = hc[t % R]
    _map_summary(pl, keyframes, logs)
    pl.close()
    logs["clearance"] = np.stack([w.clearance(logs["x"][i, :, 0:3]) for i, w in enumerate(worlds)])
    return logs


def _map_summary(pl, keyframes, logs):
    """After the flight: what the slot's keyframe map holds (n_keyframes, n_query_frames, map_points per robot)"""
    if keyframes:
        ms = pl.kfmap_state(0)
        logs.update(n_keyframes=ms["n_keyframes"], n_query_frames=ms["n_query_frames"], map_points=np.maximum(ms["frame_sizes"], 0).sum(axis=1))


def host_frames(cyl, Twb, c):
    """The frames amk_sim_render_depth hands the pipeline, in numpy: uint16 [F, rows, cols]"""
    return np.stack([flight.quantise_depth(flight.render_depth_ordered((cyl[i, :, 0], cyl[i, :, 1], cyl[i, :, 2]), Twb[i], c["Tbc"], c["rows"],
                                                                         c["cols"], c["fx"], c["fy"], c["cx"], c["cy"], Z_TOP, MAX_RANGE),
                                           c["pixel2meter"], np.uint16) for i in range(len(cyl))])


def host_twin_depth_flights(seeds, cfg="C1", periods=40, world_kw=None, keyframes=None, cam=None):
    """The same pipeline, the sensor and the vehicle in numpy on the host between the periods -> the same dict of arrays."""
    torch, prm, c, worlds, x0, ref0, cyl, Twb, dp, pl, ABc = _setup(seeds, cfg, world_kw, cam, keyframes, queue_depth=1)
    dev = torch.device("cuda", torch.cuda.current_device())
    F = len(seeds)
    x = x0.copy()
    logs = dict(x=np.zeros((F, periods + 1, 10)), u=np.zeros((F, periods, 4)), flags=np.zeros((F, periods, 4), np.int32),
                cmd=np.zeros((F, periods, 3)))
    logs["x"][:, 0] = x
    for t in range(periods):
        depth = torch.from_numpy(host_frames(cyl, Twb, c).view(np.int16)).to(dev)
        Twb_d = torch.from_numpy(Twb).to(dev); odom = torch.from_numpy(x).to(dev); cmd = torch.zeros((F, 3), dtype=torch.float64, device=dev)
        r0 = torch.from_numpy(ref0).to(dev) if t == 0 else None
        tk = pl.submit(None, None, ref_path_init=r0, odom=odom, cmd_out=cmd, keep_warm_start=t > 0, depth=depth, Twb=Twb_d)
        pl.wait(tk)
        o = pl.outputs(tk)
        a = cmd.cpu().numpy()
        x, Twb = flight.vehicle_step_ordered(ABc, x, a, POSE_QUANTUM)
        logs["x"][:, t + 1] = x; logs["u"][:, t] = o["u"]; logs["flags"][:, t] = o["flags"]; logs["cmd"][:, t] = a
    _map_summary(pl, keyframes, logs)
    pl.close()
    logs["clearance"] = np.stack([w.clearance(logs["x"][i, :, 0:3]) for i, w in enumerate(worlds)])
    return logs
