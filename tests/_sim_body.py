"""Closed-loop flights flown by the rigid-body vehicle (TEST INFRASTRUCTURE, beside tests/_sim_world.py).

device_body_flights and host_twin_body_flights are tests/_sim_world.py's two loops with amk_sim_vehicle_step_body in the place of
amk_sim_vehicle_step_att: per period
    Pipeline.submit(depth=..., Twb=..., odom=x, cmd_out=cmd)  ->  wait_stream  ->  sim_vehicle_step_body  ->  sim_render_world  ->  next submit
on the device, without a host copy or a host wait in the loop, and the same pipeline with flight.body_step_ordered and
flight.render_world_ordered + quantise_depth on the host between the periods.  The plant is no longer the MPC's own model: the odometry
x holds the body's position and velocity and the filtered IMU acceleration, and the camera rides the body's attitude, which lags its
command.  Both loops also log the vehicle's hidden state `body` [F, periods + 1, 64] of every period."""
import numpy as np

from avoid_mpc_amd import flight
from tests._sim_flight import MAX_RANGE, POSE_QUANTUM, Z_TOP
from tests._sim_world import _empty_logs, _finish, _setup, host_frames


def _body_prm(cfg_prm, body):
    """`body`: None (the defaults at the flight's control period) or what flight.body_params takes as keywords"""
    return flight.body_params(cfg_prm.dt, **(body or {}))


def device_body_flights(seeds, cfg="C1", periods=40, world_kw=None, keyframes=None, cam=None, body=None, study=False):
    """-> device_world_flights' dict and body [F, periods + 1, 64].  study=True (measurements, not tests) also logs x_pred
    [F, periods, 10]: row 1 of the step's x0array, the MPC's own prediction of the next state."""
    from avoid_mpc_amd.host import sim_body_params, sim_body_reset, sim_render_world, sim_vehicle_step_body
    from tests import _flight
    torch, c, worlds, x0, ref0, cyl, counts, box, Twb0, dp, pl, ABc = _setup(seeds, cfg, world_kw, cam, keyframes, queue_depth=2)
    prm = _body_prm(_flight.make_prm(cfg)[0], body)
    dev = torch.device("cuda", torch.cuda.current_device())
    F = len(seeds)
    f64 = dict(dtype=torch.float64, device=dev)
    up = lambda a: torch.from_numpy(a).to(dev)
    x, Twb, cyl_d, counts_d, box_d, r0 = up(x0), up(Twb0), up(cyl), up(counts), up(box), up(ref0)
    cmd = torch.zeros((F, 3), **f64)
    state = torch.zeros((F, flight.BODY_DOUBLES), **f64)
    sim_body_reset(state, prm.gz)
    p = sim_body_params(None, prm)
    depth = torch.zeros((F, c["rows"], c["cols"]), dtype=torch.int16, device=dev)
    log_x = torch.zeros((periods, F, 10), **f64); log_u = torch.zeros((periods, F, 4), **f64); log_cmd = torch.zeros((periods, F, 3), **f64)
    log_T = torch.zeros((periods, F, 4, 4), **f64); log_flags = torch.zeros((periods, F, 4), dtype=torch.int32, device=dev)
    log_b = torch.zeros((periods, F, flight.BODY_DOUBLES), **f64)
    log_pred = torch.zeros((periods, F, 10), **f64) if study else None
    render = lambda: sim_render_world(cyl_d, box_d, Twb, dp, c["rows"], c["cols"], cyl_counts=counts_d, z_top=Z_TOP, max_range=MAX_RANGE, out=depth)
    render()
    for t in range(periods):                                   # no host copy and no host wait in here
        tk = pl.submit(None, None, ref_path_init=r0 if t == 0 else None, odom=x, cmd_out=cmd, keep_warm_start=t > 0, depth=depth, Twb=Twb)
        pl.wait_stream(tk)
        o = pl.output_tensors(tk)
        log_u[t].copy_(o["u"]); log_flags[t].copy_(o["flags"]); log_cmd[t].copy_(cmd)
        if study:
            log_pred[t].copy_(o["x0array"][:, 1, :10])
        sim_vehicle_step_body(p, cmd, x, state, Twb, pose_quantum=POSE_QUANTUM)
        log_x[t].copy_(x); log_T[t].copy_(Twb); log_b[t].copy_(state)   # the state, the pose and the body AFTER period t
        render()
    pl.drain()
    torch.cuda.synchronize()
    logs = _empty_logs(F, periods, x0, Twb0)
    logs["body"] = np.zeros((F, periods + 1, flight.BODY_DOUBLES)); logs["body"][:, 0] = flight.body_state0(F, prm.gz)
    for key, log in (("x", log_x), ("Twb", log_T), ("body", log_b)):
        logs[key][:, 1:] = np.moveaxis(log.cpu().numpy(), 0, 1)
    for key, log in (("u", log_u), ("flags", log_flags), ("cmd", log_cmd)):
        logs[key][:] = np.moveaxis(log.cpu().numpy(), 0, 1)
    if study:
        logs["x_pred"] = np.moveaxis(log_pred.cpu().numpy(), 0, 1)
    return _finish(logs, pl, keyframes, worlds, cyl, counts, box)


def host_twin_body_flights(seeds, cfg="C1", periods=40, world_kw=None, keyframes=None, cam=None, body=None):
    """The same pipeline, the sensor and the rigid-body vehicle in numpy on the host between the periods -> the same dict of arrays."""
    from tests import _flight
    torch, c, worlds, x0, ref0, cyl, counts, box, Twb, dp, pl, ABc = _setup(seeds, cfg, world_kw, cam, keyframes, queue_depth=1)
    prm = _body_prm(_flight.make_prm(cfg)[0], body)
    dev = torch.device("cuda", torch.cuda.current_device())
    F = len(seeds)
    x, state = x0.copy(), flight.body_state0(F, prm.gz)
    logs = _empty_logs(F, periods, x0, Twb)
    logs["body"] = np.zeros((F, periods + 1, flight.BODY_DOUBLES)); logs["body"][:, 0] = state
    for t in range(periods):
        depth = torch.from_numpy(host_frames(cyl, counts, box, Twb, c).view(np.int16)).to(dev)
        Twb_d = torch.from_numpy(Twb).to(dev); odom = torch.from_numpy(x).to(dev); cmd = torch.zeros((F, 3), dtype=torch.float64, device=dev)
        r0 = torch.from_numpy(ref0).to(dev) if t == 0 else None
        tk = pl.submit(None, None, ref_path_init=r0, odom=odom, cmd_out=cmd, keep_warm_start=t > 0, depth=depth, Twb=Twb_d)
        pl.wait(tk)
        o = pl.outputs(tk)
        a = cmd.cpu().numpy()
        x, state, Twb = flight.body_step_ordered(prm, x, state, a, POSE_QUANTUM)
        logs["x"][:, t + 1] = x; logs["Twb"][:, t + 1] = Twb; logs["body"][:, t + 1] = state
        logs["u"][:, t] = o["u"]; logs["flags"][:, t] = o["flags"]; logs["cmd"][:, t] = a
    return _finish(logs, pl, keyframes, worlds, cyl, counts, box)
