"""Cost of the ground-truth queries (amk_sim_clearance, amk_sim_segment_cast, amk_sim_path_cast) and of a monitored closed loop, and the
study profiles/sim_world_cost.txt (c) left open, after tools/experiments/sim_world_cost.py's method: HIP events around one call, 9 timed
calls after 2 warm-up calls, median (min .. max), one process.
  (a) each of the three entries at S = 256 scenes, N = 20 path points of stride 14, radius 0.5 m, with 16 / 110 cylinders x 0 / 12 / 64 boxes.
  (b) wall time per period of the 256-robot, 40-period flight through flight.WallWorld with AMK_SIM_ATT_ACCEL, without / with /
      without the monitor (tests/_sim_truth.py device_truth_flights), in that order in this process.  Nothing is gated on it.
  (c) over the monitored flight: the 2 x 2 table of the truth cast's verdict against the map audit's over all (robot, period) pairs,
      and for every robot whose true clearance goes negative the period, the solid, the camera's tilt at that period, and how many
      periods before the contact the truth cast first stopped a plan at that solid, the audit first stopped one at a map point on that
      solid (the audit names a point, not a solid), and the audit first stopped one at all -- each searched on its own.
usage: python tools/experiments/sim_truth_cost.py [--out FILE] [--robots 256] [--periods 40]"""
import sys
import time
sys.path.insert(0, ".")
import numpy as np
from avoid_mpc_amd import flight

REPS, WARM, S, N, STRIDE, RADIUS = 9, 2, 256, 20, 14, 0.5
KINDS = {0: "the ground", 1: "cylinder", 2: "box"}
NEAR, Z_TOP = 0.1, 4.0   # [m] an audit stop counts as "at that solid" when the map point it touched lies this near the solid's surface
arg = lambda name, default: type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def study(log):
    """(c) from device_truth_flights' logs -> lines of text"""
    truth, audit = log["truth_stop"] != 0, log["audit_stop"] != 0
    F, P = truth.shape
    lines = [f"(c) truth cast against map audit, radius {log['radius']} m, {log['n_legs']} legs, over {F} x {P} = {truth.size} (robot, period) pairs",
             f"                      audit free   audit stops",
             f"    truth free        {int((~truth & ~audit).sum()):10d}   {int((~truth & audit).sum()):11d}",
             f"    truth stops       {int((truth & ~audit).sum()):10d}   {int((truth & audit).sum()):11d}",
             f"    truth stops by kind of solid: " + ", ".join(f"{KINDS[k]} {int((truth & (log['truth_kind'] == k)).sum())}" for k in KINDS)
             + f"; unjudgeable plans (stop 2): truth {int((log['truth_stop'] == 2).sum())}, audit {int((log['audit_stop'] == 2).sum())}"]
    inside = log["truth_clear_dist"] < 0
    lines.append(f"    robots whose true clearance goes negative: {int(inside.any(axis=1).sum())} of {F}"
                 f" (least clearance of the fleet {float(log['truth_clear_dist'].min()):.3f} m)")
    lines.append(f"    per robot: the solid it ends in; the first period whose plan the truth cast stopped AT THAT SOLID; the first period whose plan the audit"
                 f" stopped at a map point within {NEAR} m of that solid's surface; the first period the audit stopped a plan at all -- each searched"
                 f" on its own over periods 0 .. contact")
    tally = {"audit earlier": 0, "same period": 0, "audit later": 0, "truth never": 0, "audit never at that solid": 0}
    leads = []
    for i in np.nonzero(inside.any(axis=1))[0]:
        pc = int(np.argmax(inside[i]))                                           # the state after period pc is inside a solid
        kind, index = int(log["truth_clear_kind"][i, pc]), int(log["truth_clear_index"][i, pc])
        R = log["Twb"][i, pc + 1, :3, :3]
        tilt, pitch = np.degrees(np.arccos(np.clip(R[2, 2], -1, 1))), np.degrees(np.arcsin(np.clip(-R[2, 0], -1, 1)))
        named = np.nonzero(truth[i, :pc + 1] & (log["truth_kind"][i, :pc + 1] == kind) & (log["truth_index"][i, :pc + 1] == index))[0]
        pts = log["audit_pts"][i, :pc + 1].astype(np.float64)                    # the map point each audit stop touched
        if kind == 1:
            off = flight.cylinder_distance_ordered(pts, log["cyl"][i, index:index + 1], Z_TOP)[:, 0]
        elif kind == 2:
            off = flight.box_distance_ordered(pts, log["box"][i, index:index + 1])[:, 0]
        else:
            off = pts[:, 2]
        at_solid = np.nonzero((log["audit_stop"][i, :pc + 1] == 1) & (np.abs(off) <= NEAR))[0]
        anywhere = np.nonzero(audit[i, :pc + 1])[0]
        first = lambda a: int(a[0]) if a.size else None
        pt, pa, pany = first(named), first(at_solid), first(anywhere)
        if pt is not None:
            leads.append(pc - pt)
        tally["truth never" if pt is None else "audit never at that solid" if pa is None else
              "audit earlier" if pa < pt else "same period" if pa == pt else "audit later"] += 1
        ago = lambda p: "never" if p is None else f"period {p} ({pc - p} before)"
        lines.append(f"    robot {i:3d}: inside {KINDS[kind]}{'' if kind == 0 else ' ' + str(index)} after period {pc} ({float(log['truth_clear_dist'][i, pc]):+.3f} m), "
                     f"tilt {tilt:.1f} deg (nose down {pitch:+.1f}); truth at that solid: {ago(pt)}; audit at that solid: {ago(pa)}; audit at all: {ago(pany)}")
    lines.append("    over these robots, the audit's first stop at that solid against the truth cast's: " + ", ".join(f"{k} {v}" for k, v in tally.items())
                 + (f"; the truth cast's lead over the contact: median {float(np.median(leads)):.0f} periods ({min(leads)} .. {max(leads)})" if leads else ""))
    return lines


if __name__ == "__main__":
    import torch
    from avoid_mpc_amd.host import sim_clearance, sim_path_cast, sim_segment_cast
    from tests import _sim_truth
    out_path, ROBOTS, PERIODS = arg("--out", ""), arg("--robots", 256), arg("--periods", 40)
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda")
    lines = [f"amk_sim_clearance / amk_sim_segment_cast / amk_sim_path_cast; {torch.cuda.get_device_name(0)}, one process; HIP events around one call, "
             f"median of {REPS} after {WARM} warm-up calls"]

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

    def scene(ncyl, nbox):
        """sim_world_cost.py's corridor; plans of N points 0.5 m apart from poses along it"""
        rng = np.random.default_rng([ncyl, nbox])
        cyl = np.stack([np.sort(rng.uniform(3.0, 80.0, (S, ncyl)), axis=1), rng.uniform(-8.0, 8.0, (S, ncyl)), rng.uniform(0.1, 0.5, (S, ncyl))], axis=2)
        yaw = rng.uniform(-0.3, 0.3, (S, nbox))
        box = np.stack([rng.uniform(3.0, 80.0, (S, nbox)), rng.uniform(-8.0, 8.0, (S, nbox)), np.full((S, nbox), 0.05), rng.uniform(0.5, 3.0, (S, nbox)),
                        np.cos(yaw), np.sin(yaw), np.where(rng.uniform(size=(S, nbox)) < 0.3, 2.5, 0.0), np.full((S, nbox), 4.0)], axis=2)
        step = rng.normal([0.5, 0.0, 0.0], [0.05, 0.1, 0.03], (S, N, 3))
        step[:, 0] = np.stack([rng.uniform(0.0, 40.0, S), rng.uniform(-2.0, 2.0, S), np.full(S, 1.5)], axis=1)
        path = rng.normal(size=(S, N, STRIDE)); path[:, :, 0:3] = np.cumsum(step, axis=1)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return up(cyl.reshape(S, ncyl, 3)), up(box.reshape(S, nbox, 8)), up(path)

    fmt = lambda t: f"{float(np.median(t)):7.1f} us ({min(t):.1f} .. {max(t):.1f})"
    lines.append(f"(a) S = {S}, N = {N} points of stride {STRIDE} (clearance: {N} points, casts: {N - 1} legs), radius {RADIUS} m; us per call")
    for ncyl in (16, 110):
        for nbox in (0, 12, 64):
            cyl, box, path = scene(ncyl, nbox)
            c, s, p = sim_clearance(cyl, box, path), sim_segment_cast(cyl, box, path, RADIUS), sim_path_cast(cyl, box, path, RADIUS)
            tc = timed(lambda: sim_clearance(cyl, box, path, out=c))
            ts = timed(lambda: sim_segment_cast(cyl, box, path, RADIUS, out=s))
            tp = timed(lambda: sim_path_cast(cyl, box, path, RADIUS, out=p))
            lines.append(f"  {ncyl:3d} cylinders, {nbox:2d} boxes: clearance {fmt(tc)}   segment cast {fmt(ts)}   path cast {fmt(tp)}   "
                         f"(legs with a contact {float(s['hit'].float().mean()):.2f}, paths stopped {float((p['stop'] != 0).float().mean()):.2f}, "
                         f"mean stop leg {float(p['leg'][p['stop'] != 0].float().mean()) if (p['stop'] != 0).any() else -1:.1f})")

    seeds = list(range(5000, 5000 + ROBOTS))
    kw = dict(cyl_per_m=1.5, x_first=3.0, length=60.0)
    lines.append(f"(b) {ROBOTS} robots x {PERIODS} periods, configuration C1, sensor 48 x 64 / 2, WallWorld, AMK_SIM_ATT_ACCEL; wall ms per period "
                 f"(set-up and final copies included)")
    _sim_truth.device_truth_flights(seeds[:4], "C1", 2, world_kw=kw, monitor=True)
    _sim_truth.device_truth_flights(seeds[:4], "C1", 2, world_kw=kw, monitor=False)
    ms, logs = [], None
    for monitor in (False, True, False):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        log = _sim_truth.device_truth_flights(seeds, "C1", PERIODS, world_kw=kw, monitor=monitor)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / PERIODS)
        logs = log if monitor else logs
        lines.append(f"  {'with the monitor (audit REPORT, path cast, clearance, ring logs)' if monitor else 'without the monitor (device_world_flights itself)':<66s}"
                     f" {ms[-1]:8.2f} ms per period   (mean x flown {float((log['x'][:, -1, 0] - log['x'][:, 0, 0]).mean()):.2f} m)")
    lines.append(f"  the monitor adds {ms[1] - 0.5 * (ms[0] + ms[2]):+.2f} ms per period against the mean of the two unmonitored runs, "
                 f"which differ from each other by {abs(ms[0] - ms[2]):.2f} ms")
    lines += study(logs)
    text = "\n".join(lines)
    print(text)
    if out_path:
        open(out_path, "w").write(text + "\n")
