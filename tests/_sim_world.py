"""Closed-loop depth flights through worlds with walls, flown by a vehicle that tilts (TEST INFRASTRUCTURE, beside tests/_sim_flight.py).

device_world_flights and host_twin_world_flights are tests/_sim_flight.py's two loops with the world of flight.WallWorld (cylinders
and boxes) and an `attitude`: per period
    Pipeline.submit(depth=..., Twb=..., odom=x, cmd_out=cmd)  ->  wait_stream  ->  sim_vehicle_step_att  ->  sim_render_world  ->  next submit
on the device with device-side ring logs, and the same pipeline with flight.vehicle_attitude_ordered and flight.render_world_ordered +
quantise_depth on the host between the periods.  The worlds of a fleet hold different cylinder counts (WallWorld leaves out the
cylinders that would stand in a wall), so the cylinder list is padded and goes with its counts.  Both log the pose of every period."""
import numpy as np

from avoid_mpc_amd import flight
from tests import _flight
from tests._sim_flight import MAX_RANGE, POSE_QUANTUM, SIM_CAM, Z_TOP, _map_summary


def _setup(seeds, cfg, world_kw, cam, keyframes, queue_depth):
    import torch
    from avoid_mpc_amd.host import Pipeline, depth_params, plant_model
    prm, _ = _flight.make_prm(cfg)
    c = cam or SIM_CAM
    F = len(seeds)
    worlds = [flight.WallWorld(int(s), prm, 1000, **(world_kw or {})) for s in seeds]
    st = [flight.initial_state(int(s), prm) for s in seeds]
    x0 = np.stack([a for a, _ in st]); ref0 = np.stack([b for _, b in st])
    counts = np.array([w.cx.size for w in worlds], np.int32)
    cyl = np.zeros((F, int(counts.max()), 3))                                       # padded: scene i holds counts[i] cylinders
    for i, w in enumerate(worlds):
        cyl[i, :counts[i]] = np.stack([w.cx, w.cy, w.cr], axis=1)
    box = np.stack([w.box for w in worlds])                                         # [F, n_box, 8]: every world has the same count
    Twb0 = np.tile(np.eye(4), (F, 1, 1)); Twb0[:, :3, 3] = np.rint(x0[:, 0:3] * POSE_QUANTUM) / POSE_QUANTUM
    cap = int(c["cols"] / c["resize_scale"]) * int(c["rows"] / c["resize_scale"])
    dp = depth_params(c["pixel2meter"], c["depth_min"], c["depth_max"], c["resize_scale"], c["fx"], c["fy"], c["cx"], c["cy"], c["Tbc"])
    pl = Pipeline(1, F, cap, cap, prm, queue_depth=queue_depth, depth=dp,
                  keyframes=dict(keyframes, depth_min=c["depth_min"]) if keyframes else None)
    ABc = plant_model(prm.tau, prm.dt)
    return torch, c, worlds, x0, ref0, cyl, counts, box, Twb0, dp, pl, ABc


def _empty_logs(F, periods, x0, Twb0):
    logs = dict(x=np.zeros((F, periods + 1, 10)), u=np.zeros((F, periods, 4)), flags=np.zeros((F, periods, 4), np.int32),
                cmd=np.zeros((F, periods, 3)), Twb=np.zeros((F, periods + 1, 4, 4)))
    logs["x"][:, 0] = x0; logs["Twb"][:, 0] = Twb0
    return logs


def _finish(logs, pl, keyframes, worlds, cyl, counts, box):
    _map_summary(pl, keyframes, logs)
    pl.close()
    logs["clearance"] = np.stack([w.clearance(logs["x"][i, :, 0:3]) for i, w in enumerate(worlds)])
    logs["box_clearance"] = np.stack([w.box_clearance(logs["x"][i, :, 0:3]) for i, w in enumerate(worlds)])
    logs.update(cyl=cyl, cyl_counts=counts, box=box)
    return logs


def device_world_flights(seeds, cfg="C1", periods=40, world_kw=None, keyframes=None, cam=None, attitude=flight.ATT_ACCEL, gz=flight.GZ):
    """-> dict of arrays [F, ...]: x [F, periods + 1, 10], Twb [F, periods + 1, 4, 4] (the pose each frame was rendered at), u, flags,
    cmd, clearance (cylinders), box_clearance, and the world as rendered (cyl, cyl_counts, box)."""
    from avoid_mpc_amd.host import sim_render_world, sim_vehicle_step_att
    torch, c, worlds, x0, ref0, cyl, counts, box, Twb0, dp, pl, ABc = _setup(seeds, cfg, world_kw, cam, keyframes, queue_depth=2)
    dev = torch.device("cuda", torch.cuda.current_device())
    F = len(seeds)
    f64 = dict(dtype=torch.float64, device=dev)
    up = lambda a: torch.from_numpy(a).to(dev)
    x, Twb, cyl_d, counts_d, box_d, r0 = up(x0), up(Twb0), up(cyl), up(counts), up(box), up(ref0)
    cmd = torch.zeros((F, 3), **f64)
    depth = torch.zeros((F, c["rows"], c["cols"]), dtype=torch.int16, device=dev)
    log_x = torch.zeros((periods, F, 10), **f64); log_u = torch.zeros((periods, F, 4), **f64); log_cmd = torch.zeros((periods, F, 3), **f64)
    log_T = torch.zeros((periods, F, 4, 4), **f64); log_flags = torch.zeros((periods, F, 4), dtype=torch.int32, device=dev)
    render = lambda: sim_render_world(cyl_d, box_d, Twb, dp, c["rows"], c["cols"], cyl_counts=counts_d, z_top=Z_TOP, max_range=MAX_RANGE, out=depth)
    render()
    for t in range(periods):                                   # no host copy and no host wait in here
        tk = pl.submit(None, None, ref_path_init=r0 if t == 0 else None, odom=x, cmd_out=cmd, keep_warm_start=t > 0, depth=depth, Twb=Twb)
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
    return _finish(logs, pl, keyframes, worlds, cyl, counts, box)


def host_frames(cyl, counts, box, Twb, c):
    """The frames amk_sim_render_world hands the pipeline, in numpy: uint16 [F, rows, cols]"""
    return np.stack([flight.quantise_depth(flight.render_world_ordered((cyl[i, :counts[i], 0], cyl[i, :counts[i], 1], cyl[i, :counts[i], 2]), box[i], Twb[i],
                                                                         c["Tbc"], c["rows"], c["cols"], c["fx"], c["fy"], c["cx"], c["cy"], Z_TOP,
                                                                         MAX_RANGE), c["pixel2meter"], np.uint16) for i in range(len(cyl))])


def host_twin_world_flights(seeds, cfg="C1", periods=40, world_kw=None, keyframes=None, cam=None, attitude=flight.ATT_ACCEL, gz=flight.GZ):
    """The same pipeline, the sensor and the vehicle in numpy on the host between the periods -> the same dict of arrays."""
    torch, c, worlds, x0, ref0, cyl, counts, box, Twb, dp, pl, ABc = _setup(seeds, cfg, world_kw, cam, keyframes, queue_depth=1)
    dev = torch.device("cuda", torch.cuda.current_device())
    F = len(seeds)
    x = x0.copy()
    logs = _empty_logs(F, periods, x0, Twb)
    for t in range(periods):
        depth = torch.from_numpy(host_frames(cyl, counts, box, Twb, c).view(np.int16)).to(dev)
        Twb_d = torch.from_numpy(Twb).to(dev); odom = torch.from_numpy(x).to(dev); cmd = torch.zeros((F, 3), dtype=torch.float64, device=dev)
        r0 = torch.from_numpy(ref0).to(dev) if t == 0 else None
        tk = pl.submit(None, None, ref_path_init=r0, odom=odom, cmd_out=cmd, keep_warm_start=t > 0, depth=depth, Twb=Twb_d)
        pl.wait(tk)
        o = pl.outputs(tk)
        a = cmd.cpu().numpy()
        x, Twb = flight.vehicle_attitude_ordered(ABc, x, a, POSE_QUANTUM, attitude, gz)
        logs["x"][:, t + 1] = x; logs["Twb"][:, t + 1] = Twb; logs["u"][:, t] = o["u"]; logs["flags"][:, t] = o["flags"]; logs["cmd"][:, t] = a
    return _finish(logs, pl, keyframes, worlds, cyl, counts, box)
