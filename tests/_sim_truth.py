"""Closed-loop flights with a ground-truth monitor beside the loop (TEST INFRASTRUCTURE, beside tests/_sim_world.py).

device_truth_flights is tests/_sim_world.py's device_world_flights loop with three additions: the pipeline audits its own plan
against the map (AMK_AUDIT_REPORT), and per period two ground-truth queries run against the world the sensor renders --
    Pipeline.submit  ->  wait_stream  ->  sim_path_cast(x0array)  ->  sim_vehicle_step_att  ->  sim_clearance(x)  ->  sim_render_world
-- all on the stream that waited for the frame.  The truth answers and the audit's go into device ring buffers beside the existing logs;
there is still no host copy or wait inside the loop.  The monitor only reads what the loop produces, so the flight is
device_world_flights' bit for bit.  truth_answers_ordered replays the monitor in numpy from the logged x and x0array."""
import ctypes as C

import numpy as np

from avoid_mpc_amd import capi, flight
from tests._sim_flight import MAX_RANGE, POSE_QUANTUM, Z_TOP
from tests._sim_world import _empty_logs, _finish, _setup

AUDIT_RADIUS = 0.5       # [m] synth's drone_radius: the sphere both verdicts are cast with
CAST_KEYS = ("stop", "leg", "t", "free", "pts", "kind", "index")
AUDIT_KEYS = (("stop", (), np.int32), ("leg", (), np.int32), ("t", (), np.float64), ("free", (), np.float64), ("pts", (3,), np.float32),
              ("src", (), np.int32))


def _audit_tensors(pl, ticket, torch):
    """Pipeline.audit_outputs without the host copies: the frame's audit answers as tensors aliasing the slot's buffers"""
    ptr = [C.c_void_p() for _ in AUDIT_KEYS]
    capi.check(pl.lib.amk_pipeline_audit_outputs(pl.h, int(ticket), *[C.byref(p) for p in ptr]), "amk_pipeline_audit_outputs")
    return {name: capi.tensor_from_ptr(p.value, (pl.S, *shp), getattr(torch, np.dtype(dt).name)) for p, (name, shp, dt) in zip(ptr, AUDIT_KEYS)}


def device_truth_flights(seeds, cfg="C1", periods=40, world_kw=None, keyframes=None, cam=None, attitude=flight.ATT_ACCEL, gz=flight.GZ,
                         radius=AUDIT_RADIUS, n_legs=0, monitor=True):
    """-> device_world_flights' dict, and with the monitor: x0array [F, periods, N, 14], truth_clear_dist / _kind / _index
    [F, periods] (the clearance of the state AFTER each period), truth_stop / _leg / _t / _free / _pts / _kind / _index [F, periods] (the
    truth cast of each period's plan), audit_stop / _leg / _t / _free / _pts / _src [F, periods] (the map's verdict on the same plan),
    radius and n_legs.  monitor=False is device_world_flights itself (the pipeline's audit off, no truth query)."""
    from avoid_mpc_amd.host import sim_clearance, sim_path_cast, sim_path_cast_out, sim_render_world, sim_vehicle_step_att
    torch, c, worlds, x0, ref0, cyl, counts, box, Twb0, dp, pl, ABc = _setup(seeds, cfg, world_kw, cam, keyframes, queue_depth=2)
    dev = torch.device("cuda", torch.cuda.current_device())
    F, N = len(seeds), pl.N
    legs = int(n_legs) if n_legs else N - 1
    if monitor:
        pl.set_path_audit(capi.AMK_AUDIT_REPORT, radius, n_legs)
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    up = lambda a: torch.from_numpy(a).to(dev)
    x, Twb, cyl_d, counts_d, box_d, r0 = up(x0), up(Twb0), up(cyl), up(counts), up(box), up(ref0)
    cmd = torch.zeros((F, 3), **f64)
    depth = torch.zeros((F, c["rows"], c["cols"]), dtype=torch.int16, device=dev)
    log_x = torch.zeros((periods, F, 10), **f64); log_u = torch.zeros((periods, F, 4), **f64); log_cmd = torch.zeros((periods, F, 3), **f64)
    log_T = torch.zeros((periods, F, 4, 4), **f64); log_flags = torch.zeros((periods, F, 4), **i32)
    if monitor:
        log_plan = torch.zeros((periods, F, N, 14), **f64)
        clear = {"dist": torch.zeros((periods, F, 1), **f64), "kind": torch.zeros((periods, F, 1), **i32), "index": torch.zeros((periods, F, 1), **i32)}
        cast = [sim_path_cast_out(F, dev) for _ in range(periods)]             # one set of outputs per period: the ring
        # all legs audited: x0array goes in as it is; fewer: its audited rows, copied so that a scene starts every legs + 1 rows
        plan = None if legs == N - 1 else torch.zeros((F, legs + 1, 14), **f64)
        log_audit = {name: torch.zeros((periods, F, *shp), dtype=getattr(torch, np.dtype(dt).name), device=dev) for name, shp, dt in AUDIT_KEYS}
    render = lambda: sim_render_world(cyl_d, box_d, Twb, dp, c["rows"], c["cols"], cyl_counts=counts_d, z_top=Z_TOP, max_range=MAX_RANGE, out=depth)
    render()
    for t in range(periods):                                   # no host copy and no host wait in here
        tk = pl.submit(None, None, ref_path_init=r0 if t == 0 else None, odom=x, cmd_out=cmd, keep_warm_start=t > 0, depth=depth, Twb=Twb)
        pl.wait_stream(tk)
        o = pl.output_tensors(tk)
        log_u[t].copy_(o["u"]); log_flags[t].copy_(o["flags"]); log_cmd[t].copy_(cmd)
        if monitor:                                            # the plan of this period against the world as it is, and the map's verdict on it
            log_plan[t].copy_(o["x0array"])
            if plan is not None:
                plan.copy_(o["x0array"][:, :legs + 1])
            sim_path_cast(cyl_d, box_d, o["x0array"] if plan is None else plan, radius, cyl_counts=counts_d, z_top=Z_TOP, out=cast[t])
            for name, a in _audit_tensors(pl, tk, torch).items():
                log_audit[name][t].copy_(a)
        sim_vehicle_step_att(ABc, cmd, x, Twb, pose_quantum=POSE_QUANTUM, attitude=attitude, gz=gz)
        log_x[t].copy_(x); log_T[t].copy_(Twb)                 # the state and the pose AFTER period t
        if monitor:                                            # where the vehicle now is relative to the true solids
            sim_clearance(cyl_d, box_d, x.view(F, 1, 10), cyl_counts=counts_d, z_top=Z_TOP,
                          out={k: v[t] for k, v in clear.items()})
        render()
    pl.drain()
    torch.cuda.synchronize()
    logs = _empty_logs(F, periods, x0, Twb0)
    for key, log in (("x", log_x), ("Twb", log_T)):
        logs[key][:, 1:] = np.moveaxis(log.cpu().numpy(), 0, 1)
    for key, log in (("u", log_u), ("flags", log_flags), ("cmd", log_cmd)):
        logs[key][:] = np.moveaxis(log.cpu().numpy(), 0, 1)
    if monitor:
        logs["x0array"] = np.moveaxis(log_plan.cpu().numpy(), 0, 1)
        for k, v in clear.items():
            logs["truth_clear_" + k] = np.moveaxis(v.cpu().numpy()[:, :, 0], 0, 1)
        for k in CAST_KEYS:
            logs["truth_" + k] = np.stack([cast[t][k].cpu().numpy() for t in range(periods)], axis=1)
        for name, _, _ in AUDIT_KEYS:
            logs["audit_" + name] = np.moveaxis(log_audit[name].cpu().numpy(), 0, 1)
        logs.update(radius=float(radius), n_legs=legs)
    return _finish(logs, pl, keyframes, worlds, cyl, counts, box)


def truth_answers_ordered(logs):
    """The monitor in numpy: flight.world_clearance_ordered on the logged states and flight.world_path_cast_ordered on the logged plans
    -> the truth_* entries of device_truth_flights' dict, recomputed"""
    F, periods = logs["u"].shape[:2]
    out = {"truth_clear_dist": np.zeros((F, periods)), "truth_clear_kind": np.zeros((F, periods), np.int32),
           "truth_clear_index": np.zeros((F, periods), np.int32), "truth_pts": np.zeros((F, periods, 3))}
    for k, dt in (("stop", np.int32), ("leg", np.int32), ("t", np.float64), ("free", np.float64), ("kind", np.int32), ("index", np.int32)):
        out["truth_" + k] = np.zeros((F, periods), dt)
    for i in range(F):
        cyl, box = logs["cyl"][i, :logs["cyl_counts"][i]], logs["box"][i]
        d, kd, ix = flight.world_clearance_ordered(cyl, box, logs["x"][i, 1:], Z_TOP)
        out["truth_clear_dist"][i], out["truth_clear_kind"][i], out["truth_clear_index"][i] = d, kd, ix
        for t in range(periods):
            r = flight.world_path_cast_ordered(cyl, box, logs["x0array"][i, t, :logs["n_legs"] + 1], logs["radius"], Z_TOP)
            for k in CAST_KEYS:
                out["truth_" + k][i, t] = r[k]
    return out
