"""BENCH AND TEST HARNESS (not part of the product path): closed-loop flights around the control step -- the world, the sensor
frames, the vehicle and the host twins of the TASK prologue / epilogue that bench.py --workload flight and tests/_flight.py share.
Nothing under csrc/ or include/ depends on it.

The reference is a 30 Hz loop (timer of con_dt = 0.033 s, AM/src/AvoidanceStateMachine.cpp:110-111,
AM/launch/mpc_obstacle_avoidance_sim.launch:8): every period takes a fresh depth frame
(DepthCallback -> FrameKDMap::AddVertex, :153-164), shifts mRefPath (GetInitPath, :24-54), re-reads the odometry
(GetCurStateQuad, :183-203), runs the TASK branch (:322-355) from the previous period's solution
(mNlpW0 = sol, AM/src/HighLvlMpc.cpp:129) and publishes the first control (PubCmd :369-378) or the slow-down
command (PubSlowDownCmd :379-397).  This module holds what a flight needs AROUND the step and is shared by the
GPU driver (tests/_flight.py, bench.py --workload flight) and the CPU-oracle driver (tests/_flight.py):

  plant_step / affine_plant   the vehicle = the MPC's own model (mpc_obstacle_casadi.py:106-122 integrated by :338-357),
                              driven by the published command; the reference flies AirSim + bfctrl, absent here
  FlightWorld                 a static corridor of vertical cylinders; frame(t) = what a forward-looking sensor
                              returns in period t: surface points RESAMPLED every period (fresh frame, fresh indices)
  period_inputs / apply_command   GetInitPath + the clock model on one side of the step, PubCmd / PubSlowDownCmd on the other
  render_depth / render_depth_ordered / quantise_depth / vehicle_step_ordered   the depth sensor and the affine vehicle in numpy;
                              the *_ordered ones restate csrc/sim.hip (amk_sim_render_depth, amk_sim_vehicle_step) operation for operation
  render_world_ordered / vehicle_attitude_ordered / box_clearance / WallWorld   the same for amk_sim_render_world (cylinders and
                              boxes) and amk_sim_vehicle_step_att (the vehicle tilts into its thrust); a corridor with walls and gates
  world_clearance_ordered / world_segment_cast_ordered / world_path_cast_ordered   csrc/sim_truth.hip (amk_sim_clearance, amk_sim_segment_cast,
                              amk_sim_path_cast) restated operation for operation: a point or a plan against the world's TRUE solids
  noise_words / depth_noise_ordered   csrc/sim_noise.hip (amk_sim_depth_noise) restated operation for operation: the counter-based
                              stream and what it does to a batch of depth frames (dropouts, flying pixels, axial noise, disparity steps)
  body_params / body_state0 / body_step_ordered   csrc/sim_body.hip (amk_sim_body_reset, amk_sim_vehicle_step_body) restated operation
                              for operation: a rigid body flown by bfctrl's geometric attitude controller in sub-steps, and the node's COGFilter

Nothing here computes neighbours or solves anything: that is the step's job (amk_step_batch / the oracle's stepo_run).
"""
import numpy as np

from . import fsm, synth

GZ = 9.81   # mpc_obstacle_casadi.py:33 (self._gz)


def model_f(x, u, tau):
    """x_dot of mpc_obstacle_casadi.py:106-122 (drag off): x = [p(3), yaw, v(3), a(3)], u = [a_cmd(3), yaw_dot].
    Vectorised over leading dimensions."""
    x, u = np.asarray(x, np.float64), np.asarray(u, np.float64)
    d = np.empty_like(x)
    d[..., 0:3] = x[..., 4:7]
    d[..., 3] = u[..., 3]
    d[..., 4:7] = x[..., 7:10]
    d[..., 7] = (u[..., 0] - x[..., 7]) * tau[0]
    d[..., 8] = (u[..., 1] - x[..., 8]) * tau[1]
    d[..., 9] = (u[..., 2] - GZ - x[..., 9]) * tau[2]
    return d


def plant_step(x, u, tau, dt, refine=4):
    """F(x, u): `refine` classic RK4 sub-steps over dt (sys_dynamics, mpc_obstacle_casadi.py:338-357)."""
    h = dt / refine
    x = np.array(x, np.float64)
    for _ in range(refine):
        k1 = h * model_f(x, u, tau)
        k2 = h * model_f(x + 0.5 * k1, u, tau)
        k3 = h * model_f(x + 0.5 * k2, u, tau)
        k4 = h * model_f(x + k3, u, tau)
        x = x + (k1 + 2 * k2 + 2 * k3 + k4) / 6
    return x


def affine_plant(tau, dt):
    """(A [10,10], B [10,4], c [10]) with F(x, u) = A x + B u + c -- exact, the model is affine for fixed tau."""
    c = plant_step(np.zeros(10), np.zeros(4), tau, dt)
    A = np.stack([plant_step(e, np.zeros(4), tau, dt) - c for e in np.eye(10)], axis=1)
    B = np.stack([plant_step(np.zeros(10), e, tau, dt) - c for e in np.eye(4)], axis=1)
    return A, B, c


class FlightWorld:
    """One flight's world: vertical cylinders scattered over a corridor (x from `x_first` on, |y| <= 8 m, 4 m high), the
    obstacle model of synth.make_cloud stretched along the flight.  frame(t) is the sensor return of period t around the
    NOMINAL position x_nom(t) = x0 + speed * con_dt * t: surface points of the cylinders whose axis lies in
    [x_nom - back, x_nom + ahead], resampled every period (rng seeded by (seed, t): the GPU driver and the CPU oracle see
    identical frames whatever their trajectories do), plus ground returns.  The window follows the nominal position, not the
    flown one, so that a frame is a pure function of (seed, t); drivers report how far a flight strays from it."""

    def __init__(self, seed, prm, n_points, cyl_per_m=1.0, length=80.0, x_first=8.0, back=6.0, ahead=30.0, ground_frac=0.15,
                 con_dt=None):
        self.seed, self.prm, self.n = int(seed), prm, int(n_points)
        self.back, self.ahead, self.ground_frac = float(back), float(ahead), float(ground_frac)
        self.con_dt = prm.dt if con_dt is None else float(con_dt)
        rng = np.random.default_rng([self.seed, 0xF11])
        ncyl = max(1, int(round(cyl_per_m * (length - x_first))))
        self.cx = np.sort(rng.uniform(x_first, length, ncyl))
        self.cy = rng.uniform(-8.0, 8.0, ncyl)
        self.cr = rng.uniform(0.1, 0.5, ncyl)

    def x_nom(self, t):
        return self.prm.speed * self.con_dt * t

    def frame(self, t):
        """-> (cloud float32 [n, 3], edge float32 [n // 10, 3]) of period t."""
        n, ne = self.n, self.n // 10
        rng = np.random.default_rng([self.seed, 0xF12, int(t)])
        xn = self.x_nom(t)
        lo, hi = xn - self.back, xn + self.ahead
        sel = np.nonzero((self.cx >= lo) & (self.cx <= hi))[0]
        if sel.size == 0:   # open space: everything is a ground return
            sel = None
        n_g = n if sel is None else int(self.ground_frac * n)
        n_c = n - n_g
        parts = []
        if n_c:
            ci = sel[rng.integers(0, sel.size, n_c)]
            th = rng.uniform(0.0, 2.0 * np.pi, n_c)
            parts.append(np.stack([self.cx[ci] + self.cr[ci] * np.cos(th), self.cy[ci] + self.cr[ci] * np.sin(th),
                                   rng.uniform(0.0, 4.0, n_c)], axis=1))
        parts.append(np.stack([rng.uniform(lo, hi, n_g), rng.uniform(-8.0, 8.0, n_g), np.zeros(n_g)], axis=1))
        cloud = np.concatenate(parts).astype(np.float32)
        cloud = cloud[rng.permutation(n)]
        # edge cloud: the silhouette lines of the cylinders ahead, seen from the nominal camera position
        if sel is None:
            edge = np.stack([rng.uniform(lo, hi, ne), rng.uniform(-8.0, 8.0, ne), np.zeros(ne)], axis=1).astype(np.float32)
            return cloud, edge
        ahead = sel[self.cx[sel] > xn + 0.6]
        src = ahead if ahead.size else sel
        ei = src[rng.integers(0, src.size, ne)]
        side = rng.integers(0, 2, ne) * 2 - 1
        dx, dy = self.cx[ei] - xn, self.cy[ei]
        dist = np.sqrt(dx * dx + dy * dy)
        ang = np.arctan2(dy, dx) + side * (np.pi / 2.0 + np.arcsin(np.clip(self.cr[ei] / dist, -1.0, 1.0)))
        edge = np.stack([self.cx[ei] + self.cr[ei] * np.cos(ang), self.cy[ei] + self.cr[ei] * np.sin(ang),
                         rng.uniform(0.0, 4.0, ne)], axis=1).astype(np.float32)
        return cloud, edge

    def clearance(self, p):
        """Distance from position(s) p [..., 3] to the nearest cylinder SURFACE in the horizontal plane (negative: inside)."""
        p = np.asarray(p, np.float64)
        d = np.sqrt((p[..., 0:1] - self.cx) ** 2 + (p[..., 1:2] - self.cy) ** 2) - self.cr
        return d.min(axis=-1)


def initial_state(seed, prm):
    """Plant state [p, yaw, v, a] at t = 0 and mRefPath as GetInitPath's "forward" task leaves it in cruise
    (synth.make_odom / make_ref_path: the bench scenes' start)."""
    pos, vel, acc, yaw = synth.make_odom(seed, prm)
    x = np.concatenate([pos, [yaw], vel, acc])
    return x, synth.make_ref_path(pos, prm)


def period_inputs(x, ref_path, prm, farest=500.0, shift=True, task="forward", global_goal=None):
    """Host side of one period BEFORE the step, for a batch: x [S, 10] plant states (= odometry: perfect sensing),
    ref_path [S, N, 10] in/out.  GetInitPath (:24-54; task "forward", goal_x = 500 of mpc_parameters.yaml:55), then the
    per-pass initial states of the clock model (fsm.state_quads).  -> (state_quad [S, max_iter, 10], pos_x [S])"""
    S = x.shape[0]
    sq = np.empty((S, prm.max_iter, 10))
    for s in range(S):
        if shift:
            fsm.get_init_path(ref_path[s], prm.speed, prm.T, x[s, 0], farest, prm.height, task=task,
                              global_goal=None if global_goal is None else global_goal[s], dt=prm.dt)
        sq[s] = fsm.state_quads(x[s, 0:3], x[s, 4:7], x[s, 7:10], x[s, 3], prm.decay, prm.max_iter)
    return sq, x[:, 0].copy()


def command(u, flags, x, prm, kp=0.3, kd=0.3):
    """What the node publishes after the step (:345-350): PubCmd(u) when isSafety, else PubSlowDownCmd (:379-397;
    slow_down_kp / kd of mpc_parameters.yaml:79-80; z clamped to +-aMaxZ like the reference).  Batched:
    u [S, 4], flags [S, 4], x [S, 10] -> a_cmd [S, 3]"""
    u, x = np.asarray(u, np.float64), np.asarray(x, np.float64)
    slow = -kp * x[:, 4:7] - kd * x[:, 7:10] + np.array([0.0, 0.0, 9.8])
    slow[:, 0:2] = np.clip(slow[:, 0:2], -prm.a_max_xy, prm.a_max_xy)
    slow[:, 2] = np.clip(slow[:, 2], -prm.a_max_z, prm.a_max_z)
    safe = (np.asarray(flags)[:, 0] != 0)[:, None]
    return np.where(safe, u[:, 0:3], slow)


def apply_command(x, a_cmd, prm, con_dt=None):
    """The vehicle over one control period: the model driven by the published acceleration command; Command.yaw = 0
    (:376) holds the heading, so yaw_dot = 0."""
    uu = np.concatenate([a_cmd, np.zeros((a_cmd.shape[0], 1))], axis=1)
    return plant_step(x, uu, prm.tau, prm.dt if con_dt is None else con_dt)


class FlightWorldsTorch:
    """S flights' worlds and frames generated ON the device (bench.py --workload flight: frames are made before the clock starts
    and stay resident in HBM).  The scene model of FlightWorld -- vertical cylinders along a corridor, a window of surface points
    around the nominal position resampled every period, ground returns, silhouette points as the edge cloud -- on torch's random
    stream (values differ from the numpy generator's; the drivers that compare GPU and CPU flights hand the SAME frames to
    both)."""

    def __init__(self, S, n_points, prm, seed, device, cyl_per_m=1.5, length=80.0, x_first=8.0, back=6.0, ahead=30.0,
                 ground_frac=0.15, con_dt=None):
        import torch
        self.S, self.n, self.prm, self.seed, self.dev = int(S), int(n_points), prm, int(seed), device
        self.back, self.ahead, self.ground_frac = float(back), float(ahead), float(ground_frac)
        self.con_dt = prm.dt if con_dt is None else float(con_dt)
        g = torch.Generator(device=device); g.manual_seed(self.seed)
        self.ncyl = max(1, int(round(cyl_per_m * (length - x_first))))
        r = lambda: torch.rand((self.S, self.ncyl), generator=g, device=device, dtype=torch.float64)
        self.cx = torch.sort(x_first + (length - x_first) * r(), dim=1).values.contiguous()
        self.cy = -8.0 + 16.0 * r()
        self.cr = 0.1 + 0.4 * r()

    def x_nom(self, t):
        return self.prm.speed * self.con_dt * t

    def frame(self, t):
        """-> (cloud float32 [S, n, 3], edge float32 [S, n // 10, 3]) of period t."""
        import math
        import torch
        S, n, ne, dev = self.S, self.n, self.n // 10, self.dev
        g = torch.Generator(device=dev); g.manual_seed(self.seed * 1000003 + 7919 * int(t) + 1)
        rnd = lambda *shape: torch.rand(shape, generator=g, device=dev, dtype=torch.float32)
        xn = self.x_nom(t)
        lo, hi = xn - self.back, xn + self.ahead
        lo_i = torch.searchsorted(self.cx, torch.full((S, 1), lo, device=dev, dtype=torch.float64))
        hi_i = torch.searchsorted(self.cx, torch.full((S, 1), hi, device=dev, dtype=torch.float64), right=True)
        cnt = (hi_i - lo_i).clamp_(min=1)
        n_g = int(self.ground_frac * n); n_c = n - n_g
        ci = (lo_i + (rnd(S, n_c) * cnt).long()).clamp_(max=self.ncyl - 1)
        th = 2.0 * math.pi * rnd(S, n_c)
        gx, gy, gr = (v.gather(1, ci).float() for v in (self.cx, self.cy, self.cr))
        on_cyl = torch.stack([gx + gr * torch.cos(th), gy + gr * torch.sin(th), 4.0 * rnd(S, n_c)], dim=2)
        ground = torch.stack([lo + (hi - lo) * rnd(S, n_g), -8.0 + 16.0 * rnd(S, n_g), torch.zeros((S, n_g), device=dev)], dim=2)
        cloud = torch.cat([on_cyl, ground], dim=1)
        perm = torch.argsort(rnd(S, n), dim=1)
        cloud = cloud.gather(1, perm[:, :, None].expand(S, n, 3)).contiguous()
        a_i = torch.searchsorted(self.cx, torch.full((S, 1), xn + 0.6, device=dev, dtype=torch.float64), right=True)
        a_i = torch.minimum(a_i, hi_i - 1).clamp_(min=0)
        cnt2 = (hi_i - a_i).clamp_(min=1)
        ei = (a_i + (rnd(S, ne) * cnt2).long()).clamp_(max=self.ncyl - 1)
        side = (rnd(S, ne) < 0.5).float() * 2.0 - 1.0
        ex0, ey0, er = (v.gather(1, ei).float() for v in (self.cx, self.cy, self.cr))
        dx = ex0 - xn
        dist = torch.sqrt(dx * dx + ey0 * ey0)
        ang = torch.atan2(ey0, dx) + side * (math.pi / 2.0 + torch.asin((er / dist).clamp(-1.0, 1.0)))
        edge = torch.stack([ex0 + er * torch.cos(ang), ey0 + er * torch.sin(ang), 4.0 * rnd(S, ne)], dim=2).contiguous()
        return cloud, edge

    def clearance(self, pos):
        """pos float64 [S, P, 3] (numpy) -> horizontal distance to the nearest cylinder surface [S, P]."""
        cx, cy, cr = (v.cpu().numpy() for v in (self.cx, self.cy, self.cr))
        d = np.sqrt((pos[:, :, 0:1] - cx[:, None, :]) ** 2 + (pos[:, :, 1:2] - cy[:, None, :]) ** 2) - cr[:, None, :]
        return d.min(axis=2)


# T_b_c of AM/config/mpc_parameters.yaml:67-71: camera (x right, y down, z forward) in the body frame (x forward, y left, z up)
TBC_YAML = np.array([[0.0, 0.0, 1.0, 0.05], [-1.0, 0.0, 0.0, 0.0], [0.0, -1.0, 0.0, 0.01], [0.0, 0.0, 0.0, 1.0]])


def render_depth(cyl, Twb, Tbc, rows, cols, fx, fy, cx, cy, z_top=4.0, max_range=60.0):
    """Planar depth image (metres, float32 [rows, cols]; 0 = no return) of vertical cylinders cyl = (cx, cy, r) arrays standing
    on the ground plane z = 0, seen by a pinhole camera at Twb * Tbc -- the synthetic counterpart of the depth frames the
    reference receives (AirSim's DepthPlanar, AM/src/AvoidanceStateMachine.cpp:153-164).  Pixel (u, v) looks along
    ((u - cx) / fx, (v - cy) / fy, 1) in the camera frame; the value is the z coordinate of the first hit in that frame, which is
    what FrameKDMap::UV2Camera back-projects (FrameKDMap.cpp:131-138)."""
    ccx, ccy, cr = (np.asarray(v, np.float64) for v in cyl)
    Twc = np.asarray(Twb, np.float64).reshape(4, 4) @ np.asarray(Tbc, np.float64).reshape(4, 4)
    R, o = Twc[:3, :3], Twc[:3, 3]
    v, u = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    dc = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=-1)      # camera-frame ray, z component 1: t = planar depth
    d = dc @ R.T                                                                    # world-frame ray
    best = np.full((rows, cols), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        tg = np.where(d[..., 2] < 0, -o[2] / d[..., 2], np.inf)                     # ground plane
        best = np.minimum(best, np.where(tg > 0, tg, np.inf))
        a = d[..., 0] ** 2 + d[..., 1] ** 2
        for k in range(ccx.size):
            ox, oy = o[0] - ccx[k], o[1] - ccy[k]
            b = ox * d[..., 0] + oy * d[..., 1]
            c = ox * ox + oy * oy - cr[k] ** 2
            disc = b * b - a * c
            t = (-b - np.sqrt(np.where(disc >= 0, disc, np.nan))) / a
            z = o[2] + t * d[..., 2]
            ok = (disc >= 0) & (t > 0) & (z >= 0) & (z <= z_top)
            best = np.where(ok & (t < best), t, best)
    return np.where(best <= max_range, best, 0.0).astype(np.float32)


def render_depth_ordered(cyl, Twb, Tbc, rows, cols, fx, fy, cx, cy, z_top=4.0, max_range=60.0):
    """The ray parameter t = planar depth of every pixel's first hit (float64 [rows, cols] in metres; 0 = no return), the scene of
    render_depth in the OPERATION ORDER of amk_sim_render_depth (include/avoid_mpc_amd.h, "Closed-loop simulation"): every product
    and sum written out, left to right in index order, no matrix product -- numpy's element-wise float64 operations, its division
    and its square root are the IEEE operations the kernel performs, so the two agree bit for bit.  quantise_depth turns t into
    the pixels of either depth type."""
    ccx, ccy, cr = (np.asarray(v, np.float64).reshape(-1) for v in cyl)
    A, B = np.asarray(Twb, np.float64).reshape(4, 4), np.asarray(Tbc, np.float64).reshape(4, 4)
    M = np.empty((3, 4))
    for i in range(3):
        for j in range(4):
            M[i, j] = ((A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]) + A[i, 3] * B[3, j]
    o = M[:, 3]
    v, u = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    dc0, dc1 = (u - cx) / fx, (v - cy) / fy
    dx, dy, dz = ((M[i, 0] * dc0 + M[i, 1] * dc1) + M[i, 2] * 1.0 for i in range(3))
    best = np.full((rows, cols), np.inf)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        tg = -o[2] / dz                                                              # ground plane
        best = np.where((dz < 0) & (tg > 0), tg, best)
        a = dx * dx + dy * dy
        for k in range(ccx.size):
            ox, oy = o[0] - ccx[k], o[1] - ccy[k]
            b = ox * dx + oy * dy
            c = (ox * ox + oy * oy) - cr[k] * cr[k]
            disc = b * b - a * c
            t = (-b - np.sqrt(np.where(disc >= 0, disc, np.nan))) / a
            z = o[2] + t * dz
            ok = (disc >= 0) & (t > 0) & (z >= 0) & (z <= z_top)
            best = np.where(ok & (t < best), t, best)                                # strict <: the earlier hit keeps an equal t
    return np.where(best <= max_range, best, 0.0)


def quantise_depth(t, pixel2meter, dtype=np.uint16):
    """The pixels amk_sim_render_depth writes for ray parameters t: float32(t) / float32(pixel2meter) in float32 (AMK_DEPTH_F32),
    and that value rounded to the nearest integer, ties to even, clamped to [0, 65535] (AMK_DEPTH_U16) -- the rule of the depth
    flights' frames (np.clip(np.round(float32 image / pixel2meter), 0, 65535))."""
    q = np.asarray(t, np.float64).astype(np.float32) / np.float32(pixel2meter)
    if np.dtype(dtype) == np.float32:
        return q
    assert np.dtype(dtype) == np.uint16
    return np.clip(np.rint(q), 0, 65535).astype(np.uint16)


def vehicle_step_ordered(ABc, x, cmd, pose_quantum=0.0):
    """amk_sim_vehicle_step in numpy, operation for operation: x [S, 10], cmd [S, 3] -> (x+ [S, 10], Twb [S, 4, 4]) with
    x+_i = ((sum_j A_ij x_j) + (sum_j B_ij u_j)) + c_i, u = (cmd, 0), the sums left to right from j = 0, and
    Twb = [Rz(yaw) | rint(p q) / q] (exactly the identity rotation at yaw == 0; numpy's cos / sin otherwise)."""
    ABc = np.asarray(ABc, np.float64).reshape(-1)
    A, B, c = ABc[:100].reshape(10, 10), ABc[100:140].reshape(10, 4), ABc[140:150]
    x, cmd = np.asarray(x, np.float64), np.asarray(cmd, np.float64)
    u = np.concatenate([cmd, np.zeros((cmd.shape[0], 1))], axis=1)
    xn = np.empty_like(x)
    for i in range(10):
        ax = A[i, 0] * x[:, 0]
        for j in range(1, 10):
            ax = ax + A[i, j] * x[:, j]
        bu = B[i, 0] * u[:, 0]
        for j in range(1, 4):
            bu = bu + B[i, j] * u[:, j]
        xn[:, i] = (ax + bu) + c[i]
    T = np.tile(np.eye(4), (x.shape[0], 1, 1))
    yaw = xn[:, 3]
    cs, sn = np.where(yaw != 0, np.cos(yaw), 1.0), np.where(yaw != 0, np.sin(yaw), 0.0)
    T[:, 0, 0] = cs; T[:, 0, 1] = 0.0 - sn; T[:, 1, 0] = sn; T[:, 1, 1] = cs
    T[:, :3, 3] = np.rint(xn[:, 0:3] * pose_quantum) / pose_quantum if pose_quantum > 0 else xn[:, 0:3]
    return xn, T


# ---- boxes and attitude: amk_sim_render_world, amk_sim_vehicle_step_att --------------------------------------------------------------
ATT_YAW, ATT_ACCEL = 0, 1   # AMK_SIM_ATT_YAW, AMK_SIM_ATT_ACCEL


def _box_slab(lo_o, hi_o, d, inv, inside):
    """One slab of amk_sim_render_world: lo_o = lo - o, hi_o = hi - o, inv = 1.0 / d -> (near, far); a parallel ray (d == 0) gets
    (-inf, +inf) when the origin lies in the slab and (+inf, -inf), a miss, when it does not."""
    t1, t2 = lo_o * inv, hi_o * inv
    lt = t1 < t2
    near, far = np.where(lt, t1, t2), np.where(lt, t2, t1)
    par = d == 0
    return np.where(par, -np.inf if inside else np.inf, near), np.where(par, np.inf if inside else -np.inf, far)


def render_world_ordered(cyl, box, Twb, Tbc, rows, cols, fx, fy, cx, cy, z_top=4.0, max_range=60.0):
    """render_depth_ordered in a world that also holds boxes, in the OPERATION ORDER of amk_sim_render_world (include/avoid_mpc_amd.h,
    "Closed-loop simulation"): box float64 [n, 8] = (cx, cy, hx, hy, c, s, z0, z1).  The ground and the cylinders are
    render_depth_ordered's lines; then every box in index order by three slabs, one reciprocal each, a strict < throughout.
    -> t float64 [rows, cols], 0 = no return."""
    ccx, ccy, cr = (np.asarray(v, np.float64).reshape(-1) for v in cyl)
    box = np.asarray(box, np.float64).reshape(-1, 8)
    A, B = np.asarray(Twb, np.float64).reshape(4, 4), np.asarray(Tbc, np.float64).reshape(4, 4)
    M = np.empty((3, 4))
    for i in range(3):
        for j in range(4):
            M[i, j] = ((A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]) + A[i, 3] * B[3, j]
    o = M[:, 3]
    v, u = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    dc0, dc1 = (u - cx) / fx, (v - cy) / fy
    dx, dy, dz = ((M[i, 0] * dc0 + M[i, 1] * dc1) + M[i, 2] * 1.0 for i in range(3))
    best = np.full((rows, cols), np.inf)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        tg = -o[2] / dz                                                              # ground plane
        best = np.where((dz < 0) & (tg > 0), tg, best)
        a = dx * dx + dy * dy
        for k in range(ccx.size):
            ox, oy = o[0] - ccx[k], o[1] - ccy[k]
            b = ox * dx + oy * dy
            c = (ox * ox + oy * oy) - cr[k] * cr[k]
            disc = b * b - a * c
            t = (-b - np.sqrt(np.where(disc >= 0, disc, np.nan))) / a
            z = o[2] + t * dz
            ok = (disc >= 0) & (t > 0) & (z >= 0) & (z <= z_top)
            best = np.where(ok & (t < best), t, best)
        inv_z = 1.0 / dz
        for bx, by, hx, hy, c, s, z0, z1 in box:
            ox, oy = o[0] - bx, o[1] - by
            olx, oly = c * ox + s * oy, c * oy - s * ox
            dlx, dly = c * dx + s * dy, c * dy - s * dx
            n0, f0 = _box_slab(-hx - olx, hx - olx, dlx, 1.0 / dlx, bool(-hx <= olx and olx <= hx))
            n1, f1 = _box_slab(-hy - oly, hy - oly, dly, 1.0 / dly, bool(-hy <= oly and oly <= hy))
            n2, f2 = _box_slab(z0 - o[2], z1 - o[2], dz, inv_z, bool(z0 <= o[2] and o[2] <= z1))
            tn, tf = np.where(n0 > n1, n0, n1), np.where(f0 < f1, f0, f1)
            tn, tf = np.where(n2 > tn, n2, tn), np.where(f2 < tf, f2, tf)
            ok = (n0 <= f0) & (n1 <= f1) & (n2 <= f2) & (tn > 0) & (tn <= tf)
            best = np.where(ok & (tn < best), tn, best)                              # strict <: the earlier hit keeps an equal t
    return np.where(best <= max_range, best, 0.0)


def vehicle_attitude_ordered(ABc, x, cmd, pose_quantum=0.0, attitude=ATT_ACCEL, gz=GZ, cs_sn=None):
    """amk_sim_vehicle_step_att in numpy, operation for operation: vehicle_step_ordered's x+ and pose, and for ATT_ACCEL the rotation
    [xb yb zb] of acc2rotmat (mpc_obstacle_casadi.py:253-264) on the NEW acceleration plus (0, 0, gz), with the yaw mode's cs, sn;
    Rz(yaw) stays unless n > 0 and m > 0.  cs_sn = (cs [S], sn [S]) replaces numpy's cos / sin of the yaw by the caller's (the device's
    own, read from a yaw-mode pose: the two libraries differ by an ulp at some yaws).  -> (x+ [S, 10], Twb [S, 4, 4])"""
    xn, T = vehicle_step_ordered(ABc, x, cmd, pose_quantum)
    if cs_sn is not None:
        T[:, 0, 0] = T[:, 1, 1] = cs_sn[0]; T[:, 1, 0] = cs_sn[1]; T[:, 0, 1] = 0.0 - np.asarray(cs_sn[1])
    if attitude == ATT_YAW:
        return xn, T
    assert attitude == ATT_ACCEL
    cs, sn = T[:, 0, 0].copy(), T[:, 1, 0].copy()
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t0, t1, t2 = xn[:, 7], xn[:, 8], xn[:, 9] + gz
        n = np.sqrt((t0 * t0 + t1 * t1) + t2 * t2)
        zb0, zb1, zb2 = t0 / n, t1 / n, t2 / n
        y0, y1, y2 = 0.0 - zb2 * sn, zb2 * cs, zb0 * sn - zb1 * cs
        m = np.sqrt((y0 * y0 + y1 * y1) + y2 * y2)
        yb0, yb1, yb2 = y0 / m, y1 / m, y2 / m
        R = np.empty((len(xn), 3, 3))
        R[:, 0, 0] = yb1 * zb2 - yb2 * zb1; R[:, 0, 1] = yb0; R[:, 0, 2] = zb0
        R[:, 1, 0] = yb2 * zb0 - yb0 * zb2; R[:, 1, 1] = yb1; R[:, 1, 2] = zb1
        R[:, 2, 0] = yb0 * zb1 - yb1 * zb0; R[:, 2, 1] = yb2; R[:, 2, 2] = zb2
    ok = (n > 0) & (m > 0)
    T[ok, :3, :3] = R[ok]
    return xn, T


def box_clearance(p, box):
    """Horizontal distance from position(s) p [..., 3] to the nearest FACE of the boxes box [n, 8] whose vertical extent [z0, z1] holds
    p's height (negative: inside a box; +inf where no box is at that height).  For reports, not for the contract."""
    p, box = np.asarray(p, np.float64), np.asarray(box, np.float64).reshape(-1, 8)
    ox, oy = p[..., 0:1] - box[:, 0], p[..., 1:2] - box[:, 1]
    qx = np.abs(box[:, 4] * ox + box[:, 5] * oy) - np.abs(box[:, 2])
    qy = np.abs(box[:, 4] * oy - box[:, 5] * ox) - np.abs(box[:, 3])
    out = np.sqrt(np.maximum(qx, 0.0) ** 2 + np.maximum(qy, 0.0) ** 2) + np.minimum(np.maximum(qx, qy), 0.0)
    level = (p[..., 2:3] >= box[:, 6]) & (p[..., 2:3] <= box[:, 7])
    return np.where(level, out, np.inf).min(axis=-1, initial=np.inf)


# ---- ground truth against the world: amk_sim_clearance, amk_sim_segment_cast, amk_sim_path_cast ---------------------------------------
KIND_NONE, KIND_GROUND, KIND_CYLINDER, KIND_BOX = -1, 0, 1, 2


def _truth_world(cyl, box):
    cyl = np.zeros((0, 3)) if cyl is None else np.asarray(cyl, np.float64).reshape(-1, 3)
    box = np.zeros((0, 8)) if box is None else np.asarray(box, np.float64).reshape(-1, 8)
    return cyl, box


def cylinder_distance_ordered(p, cyl, z_top):
    """Signed distance from points p [P, >= 3] to each solid cylinder {rho <= r, z <= z_top} of cyl [n, 3] -> [P, n], in the operation
    order of amk_sim_clearance."""
    p, cyl = np.asarray(p, np.float64), np.asarray(cyl, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        ox, oy = p[:, 0:1] - cyl[:, 0], p[:, 1:2] - cyl[:, 1]
        qr = np.sqrt(ox * ox + oy * oy) - cyl[:, 2]
        qz = np.broadcast_to(p[:, 2:3] - z_top, qr.shape)
        mr, mz = np.where(qr > 0, qr, 0.0), np.where(qz > 0, qz, 0.0)
        m = np.where(qr > qz, qr, qz)
        return np.sqrt(mr * mr + mz * mz) + np.where(m < 0, m, 0.0)


def box_distance_ordered(p, box):
    """Signed distance from points p [P, >= 3] to each box of box [n, 8] -> [P, n]: box_clearance in three dimensions, in the operation
    order of amk_sim_clearance."""
    p, box = np.asarray(p, np.float64), np.asarray(box, np.float64).reshape(-1, 8)
    with np.errstate(invalid="ignore", over="ignore"):
        ox, oy = p[:, 0:1] - box[:, 0], p[:, 1:2] - box[:, 1]
        c, s = box[:, 4], box[:, 5]
        olx, oly = c * ox + s * oy, c * oy - s * ox
        qx, qy = np.abs(olx) - np.abs(box[:, 2]), np.abs(oly) - np.abs(box[:, 3])
        lo, hi = box[:, 6] - p[:, 2:3], p[:, 2:3] - box[:, 7]
        qz = np.where(lo > hi, lo, hi)
        mx, my, mz = np.where(qx > 0, qx, 0.0), np.where(qy > 0, qy, 0.0), np.where(qz > 0, qz, 0.0)
        m = np.where(qx > qy, qx, qy)
        m = np.where(qz > m, qz, m)
        return np.sqrt((mx * mx + my * my) + mz * mz) + np.where(m < 0, m, 0.0)


def world_clearance_ordered(cyl, box, pts, z_top=4.0):
    """amk_sim_clearance for ONE scene in numpy, operation for operation: cyl [n, 3] = (cx, cy, r), box [m, 8], pts [P, >= 3]
    -> (dist float64 [P], kind int32 [P], index int32 [P]).  The scan starts at the ground (p_z, kind 0, index -1) and goes through the
    cylinders and then the boxes in index order; a solid takes over under a strict <; a solid with a NaN entry is passed over."""
    cyl, box = _truth_world(cyl, box)
    pts = np.asarray(pts, np.float64)
    best = pts[:, 2].copy()
    kind, index = np.zeros(len(pts), np.int32), np.full(len(pts), -1, np.int32)
    for code, solids, dist in ((KIND_CYLINDER, cyl, cylinder_distance_ordered(pts, cyl, z_top)), (KIND_BOX, box, box_distance_ordered(pts, box))):
        for k in range(len(solids)):
            if np.isnan(solids[k]).any():
                continue
            with np.errstate(invalid="ignore"):
                win = dist[:, k] < best
            best = np.where(win, dist[:, k], best)
            kind[win] = code; index[win] = k
    return best, kind, index


def _truth_half_space(h, az, dz, inv_z):
    """z <= h along a_z + t d_z -> (near, far): one bound, near or far by the sign of d_z; d_z == 0: all or nothing by the origin"""
    bound = (h - az) * inv_z
    near, far = np.where(dz < 0, bound, -np.inf), np.where(dz > 0, bound, np.inf)
    par, inside = dz == 0, az <= h
    return np.where(par, np.where(inside, -np.inf, np.inf), near), np.where(par, np.where(inside, np.inf, -np.inf), far)


def _truth_slab(lo_o, hi_o, d, inv, inside):
    """_box_slab with `inside` an array (one origin per leg)"""
    t1, t2 = lo_o * inv, hi_o * inv
    lt = t1 < t2
    near, far = np.where(lt, t1, t2), np.where(lt, t2, t1)
    par = d == 0
    return np.where(par, np.where(inside, -np.inf, np.inf), near), np.where(par, np.where(inside, np.inf, -np.inf), far)


def _truth_touched(ok, tn, tf):
    return ok & (tn <= tf) & (tf >= 0) & (tn <= 1), np.where(tn > 0, tn, 0.0)


def path_legs(path):
    """path [n_points, >= 3] -> (a [L, 3], d = b - a [L, 3], judgeable [L]: every coordinate of a, b and d finite)"""
    path = np.asarray(path, np.float64)
    a, b = path[:-1, 0:3], path[1:, 0:3]
    with np.errstate(invalid="ignore", over="ignore"):
        d = b - a
    return a, d, np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1) & np.isfinite(d).all(axis=1)


def world_segment_cast_ordered(cyl, box, path, radius, z_top=4.0):
    """amk_sim_segment_cast for ONE scene in numpy, operation for operation: path [n_points, >= 3] -> (hit int32 [L], t float64 [L],
    kind int32 [L], index int32 [L]) per leg; t = 1.0, kind = index = -1 without contact.  The sphere's centre is cast against the
    solids inflated by `radius`; every solid is an intersection of per-axis intervals [near, far] of the leg's parameter."""
    cyl, box = _truth_world(cyl, box)
    a, d, judgeable = path_legs(path)
    L = len(a)
    ax, ay, az, dx, dy, dz = a[:, 0], a[:, 1], a[:, 2], d[:, 0], d[:, 1], d[:, 2]
    best, pos_kind, pos_index = np.full(L, np.inf), np.full(L, KIND_NONE, np.int32), np.full(L, -1, np.int32)
    found = np.zeros(L, bool)

    def take(hit, t, code, k):
        nonlocal best, found
        win = hit & (t < best)                                                       # strict <: the earlier solid keeps an equal t
        best = np.where(win, t, best)
        pos_kind[win] = code; pos_index[win] = k
        found |= win

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv_z = 1.0 / dz
        a2 = dx * dx + dy * dy
        n0, f0 = _truth_half_space(radius, az, dz, inv_z)                            # the ground, inflated: z <= radius
        take(*_truth_touched(n0 <= f0, n0, f0), KIND_GROUND, -1)
        top = z_top + radius
        n1, f1 = _truth_half_space(top, az, dz, inv_z)
        for k, (cx, cy, r) in enumerate(cyl):
            if np.isnan(cyl[k]).any():
                continue
            ox, oy, R = ax - cx, ay - cy, r + radius
            b = ox * dx + oy * dy
            c = (ox * ox + oy * oy) - R * R
            disc = b * b - a2 * c
            sq = np.sqrt(np.where(disc >= 0, disc, np.nan))
            roots = (a2 != 0) & (disc >= 0)
            n0 = np.where(roots, (-b - sq) / a2, np.where((a2 == 0) & (c <= 0), -np.inf, np.inf))
            f0 = np.where(roots, (-b + sq) / a2, np.where((a2 == 0) & (c <= 0), np.inf, -np.inf))
            tn, tf = np.where(n0 > n1, n0, n1), np.where(f0 < f1, f0, f1)
            take(*_truth_touched((n0 <= f0) & (n1 <= f1), tn, tf), KIND_CYLINDER, k)
        for k, (bx, by, hx, hy, c, s, z0, z1) in enumerate(box):
            if np.isnan(box[k]).any():
                continue
            ox, oy = ax - bx, ay - by
            hx, hy, z0, z1 = np.abs(hx) + radius, np.abs(hy) + radius, z0 - radius, z1 + radius
            olx, oly = c * ox + s * oy, c * oy - s * ox
            dlx, dly = c * dx + s * dy, c * dy - s * dx
            n0, f0 = _truth_slab(-hx - olx, hx - olx, dlx, 1.0 / dlx, (-hx <= olx) & (olx <= hx))
            n1b, f1b = _truth_slab(-hy - oly, hy - oly, dly, 1.0 / dly, (-hy <= oly) & (oly <= hy))
            n2, f2 = _truth_slab(z0 - az, z1 - az, dz, inv_z, (z0 <= az) & (az <= z1))
            tn, tf = np.where(n0 > n1b, n0, n1b), np.where(f0 < f1b, f0, f1b)
            tn, tf = np.where(n2 > tn, n2, tn), np.where(f2 < tf, f2, tf)
            take(*_truth_touched((n0 <= f0) & (n1b <= f1b) & (n2 <= f2), tn, tf), KIND_BOX, k)
    found &= judgeable                                                               # a non-finite leg has no contact here
    return (found.astype(np.int32), np.where(found, best, 1.0), np.where(found, pos_kind, KIND_NONE).astype(np.int32),
            np.where(found, pos_index, -1).astype(np.int32))


def path_cast_reduction(path, hit, t, kind, index):
    """The reduction amk_sim_path_cast applies to amk_sim_segment_cast's per-leg answers on the same path: the first leg, in leg order,
    that has a contact (stop 1) or is unjudgeable (stop 2) -> dict(stop, leg, t, free, pts [3], kind, index) of ONE scene;
    free = ((len_0 + len_1) + ...) + t len_leg, the last term left out at stop 2; pts = a + t d at a contact, else zeros."""
    a, d, judgeable = path_legs(path)
    with np.errstate(invalid="ignore", over="ignore"):
        length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    out = dict(stop=0, leg=-1, t=1.0, free=0.0, pts=np.zeros(3), kind=KIND_NONE, index=-1)
    acc = np.float64(0.0)
    for j in range(len(a)):
        if not judgeable[j]:
            out.update(stop=2, leg=j, t=0.0)
            break
        if hit[j]:
            tj = np.float64(t[j])
            acc = acc + tj * length[j]
            out.update(stop=1, leg=j, t=float(tj), pts=a[j] + tj * d[j], kind=int(kind[j]), index=int(index[j]))
            break
        acc = acc + length[j]
    out["free"] = float(acc)
    return out


def world_path_cast_ordered(cyl, box, path, radius, z_top=4.0):
    """amk_sim_path_cast for ONE scene in numpy: the legs are cast one after the other, each on its own as a two-point path, and the
    walk ends at the stop leg -- the legs behind it are never looked at.  -> path_cast_reduction's dict."""
    path = np.asarray(path, np.float64)
    L = len(path) - 1
    hit, t = np.zeros(L, np.int32), np.ones(L)
    kind, index = np.full(L, KIND_NONE, np.int32), np.full(L, -1, np.int32)
    judgeable = path_legs(path)[2]
    for j in range(L):
        if not judgeable[j]:
            break
        h, tt, kd, ix = world_segment_cast_ordered(cyl, box, path[j:j + 2], radius, z_top)
        hit[j], t[j], kind[j], index[j] = h[0], tt[0], kd[0], ix[0]
        if h[0]:
            break
    return path_cast_reduction(path, hit, t, kind, index)


# ---- sensor noise: amk_sim_depth_noise ------------------------------------------------------------------------------------------------
NOISE_FIELDS = ("seed", "sigma0", "sigma2", "p_drop", "edge_jump", "p_edge_drop", "p_edge_fly", "focal_baseline", "disparity_quantum",
                "z_min", "z_max")   # amk_sim_noise_params, in its order
NOISE_SCALE = 2.6428997921303014e-05   # 1 / sqrt((65536^2 - 1) / 3): the sum of four 16-bit fields to variance 1
_M64 = (1 << 64) - 1


def noise_params(params=None, **fields):
    """amk_sim_noise_params as a plain namespace: `params` (a dict or any object with some of NOISE_FIELDS) overridden by keywords;
    what is not given is 0, which switches its stage off."""
    got = {name: 0 if name == "seed" else 0.0 for name in NOISE_FIELDS}
    for name in NOISE_FIELDS:
        if isinstance(params, dict) and name in params:
            got[name] = params[name]
        elif params is not None and not isinstance(params, dict) and hasattr(params, name):
            got[name] = getattr(params, name)
    assert set(fields) <= set(NOISE_FIELDS), sorted(set(fields) - set(NOISE_FIELDS))
    got.update(fields)
    return type("NoiseParams", (), got)()


def noise_mix(z):
    """mix of amk_sim_depth_noise on np.uint64 (an array or a scalar), modulo 2^64"""
    with np.errstate(over="ignore"):
        z = np.asarray(z, np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def noise_words(seed, scene_id0, frame, n_scenes, rows, cols):
    """The stream of amk_sim_depth_noise (amk__sim_noise_words): uint64 [n_scenes, rows, cols, 3] = w_0, w_1, w_2 of every pixel, with
    k = mix(mix(mix(seed) ^ (scene_id0 + s)) ^ frame) and w_j = mix(k ^ (4 i + j)), i = v cols + u."""
    scene = np.array([(int(scene_id0) + s) & _M64 for s in range(n_scenes)], np.uint64)
    k = noise_mix(noise_mix(noise_mix(np.uint64(int(seed) & _M64)) ^ scene) ^ np.uint64(int(frame) & _M64))
    ctr = np.uint64(4) * np.arange(rows * cols, dtype=np.uint64).reshape(1, rows, cols, 1) + np.arange(3, dtype=np.uint64)
    return noise_mix(k.reshape(-1, 1, 1, 1) ^ ctr)


def noise_threshold(p):
    """T(p) of amk_sim_depth_noise: a draw of 32 bits succeeds when it is < T"""
    return np.uint64(1 << 32 if p >= 1.0 else int(p * 4294967296.0))


def _depth_z(pixels, pixel2meter):
    """what depth.hip's inv_depth reads of a pixel, widened: (float)((double)(float)pixel * pixel2meter)"""
    return (pixels.astype(np.float32).astype(np.float64) * float(pixel2meter)).astype(np.float32).astype(np.float64)


def _noise_neighbours(z):
    """z [S, rows, cols] -> the four neighbours of every pixel in the contract's order left, right, up, down: (z_n, inside the image)"""
    S, rows, cols = z.shape
    v, u = np.arange(rows).reshape(1, rows, 1), np.arange(cols).reshape(1, 1, cols)
    full = lambda m: np.broadcast_to(m, z.shape)
    return [(np.roll(z, 1, axis=2), full(u > 0)), (np.roll(z, -1, axis=2), full(u + 1 < cols)),
            (np.roll(z, 1, axis=1), full(v > 0)), (np.roll(z, -1, axis=1), full(v + 1 < rows))]


def depth_noise_ordered(depth, params, pixel2meter, frame, scene_id0=0, parts=None):
    """amk_sim_depth_noise in numpy, operation for operation: depth uint16 or float32 [S, rows, cols] -> the noisy frames, same shape
    and dtype.  `parts`, a dict, receives what the stages decided (valid, disc, partner, partner_z, flown, zero, z_in) for the tests."""
    depth = np.ascontiguousarray(depth)
    assert depth.ndim == 3 and depth.dtype in (np.uint16, np.float32)
    p = noise_params(params)
    S, rows, cols = depth.shape
    w = noise_words(p.seed, scene_id0, frame, S, rows, cols)
    w0, w1, w2 = w[..., 0], w[..., 1], w[..., 2]
    with np.errstate(all="ignore"):
        z0 = _depth_z(depth, pixel2meter)
        valid = (z0 > 0.0) & (z0 < np.inf)                                           # 1. the others are copied as they are
        z = z0.copy()
        zero = np.zeros(z.shape, bool)
        flown = np.zeros(z.shape, bool)
        if p.edge_jump > 0.0:                                                        # 2. discontinuity
            disc = np.zeros(z.shape, bool); have = np.zeros(z.shape, bool); zp = np.zeros(z.shape)
            for zn, inside in _noise_neighbours(z0):
                step = inside & (zn > 0.0) & (zn < np.inf) & (np.abs(zn - z0) > p.edge_jump)
                disc |= (inside & ~(zn > 0.0)) | step
                zp = np.where(step & ~have, zn, zp)
                have |= step
            r = w1 & np.uint64(0xffffffff)
            t_drop, t_fly = noise_threshold(p.p_edge_drop), noise_threshold(p.p_edge_fly)
            edge_drop = disc & (r < t_drop)
            fly = disc & ~edge_drop & (r < t_drop + t_fly)
            zero |= edge_drop | (fly & ~have)
            flown = fly & have & valid
            f = (w2 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
            z = np.where(flown, z0 + f * (zp - z0), z0)
            if parts is not None:
                parts.update(disc=disc & valid, partner=have & valid, partner_z=zp)
        zero |= (w1 >> np.uint64(32)) < noise_threshold(p.p_drop)                    # 3. dropout
        axial, disparity = p.sigma0 > 0.0 or p.sigma2 > 0.0, p.disparity_quantum > 0.0
        if axial:                                                                    # 4. axial noise
            m = np.uint64(0xffff)
            total = (w0 & m) + ((w0 >> np.uint64(16)) & m) + ((w0 >> np.uint64(32)) & m) + (w0 >> np.uint64(48))
            g = (total.astype(np.int64) - 131070).astype(np.float64) * NOISE_SCALE
            z = z + (p.sigma0 + (p.sigma2 * z) * z) * g
        if disparity:                                                                # 5. disparity
            dq = np.rint((p.focal_baseline / z) / p.disparity_quantum) * p.disparity_quantum
            zero |= ~(dq > 0.0)
            z = p.focal_baseline / dq
        zero |= ~(z > 0.0) | (z < p.z_min) | ((z > p.z_max) if p.z_max > 0.0 else False)   # 6. range
        touched = flown | axial | disparity                                          # 7. store
        out = np.where(touched, quantise_depth(z, pixel2meter, depth.dtype), depth)
        out = np.where(zero, np.zeros((), depth.dtype), out)
        out = np.where(valid, out, depth).astype(depth.dtype)
    if parts is not None:
        parts.update(valid=valid, flown=flown, zero=zero & valid, z_in=z0)
    return out


# ---- the rigid-body vehicle: amk_sim_vehicle_step_body -------------------------------------------------------------------------------
BODY_DOUBLES, COG_MAX = 64, 16   # AMK_SIM_BODY_DOUBLES, AMK_SIM_COG_MAX
BODY_FIELDS = ("h", "n_sub", "gz", "k_att", "rate_max", "k_rate", "k_thrust", "f_min", "f_max", "drag", "yaw_cs", "yaw_sn", "cog_window",
               "cog_weight")   # amk_sim_body_params, in its order
BODY_Q, BODY_RATE, BODY_F, BODY_HELD, BODY_HEAD, BODY_RING = 0, 4, 7, 8, 9, 10   # where the hidden state lies in a scene's 64 doubles


def cog_weights(decay=0.8):
    """The node's COGFilter weights, [COG_MAX] float64: weight idx = float(std::pow(float decay, int idx)), which C++ evaluates in double
    on the float32 decay and rounds to float32 (COGFilter.cpp:15)."""
    d = float(np.float32(decay))
    return np.array([float(np.float32(d ** idx)) for idx in range(COG_MAX)])


def body_params(con_dt, params=None, tau_rate=0.03, tau_thrust=0.05, **fields):
    """amk_sim_body_params as a plain namespace for a control period of con_dt seconds: `params` (a dict or an object with some of
    BODY_FIELDS) overridden by keywords.  The defaults are THIS PROJECT'S CHOICES, calibrated against no vehicle: 33 sub-steps per
    period, gravity 9.81, attitude gain 20 / s, body rates clamped at 10 rad/s, a 0.03 s rate lag and a 0.05 s thrust lag (as
    k = min(1, h / tau)), collective thrust in [0, 4 gz], no drag, yaw 0, and the node's COGFilter (window 10, decay 0.8)."""
    got = {}
    for name in BODY_FIELDS:
        if isinstance(params, dict) and name in params:
            got[name] = params[name]
        elif params is not None and not isinstance(params, dict) and hasattr(params, name):
            got[name] = getattr(params, name)
    assert set(fields) <= set(BODY_FIELDS), sorted(set(fields) - set(BODY_FIELDS))
    got.update(fields)
    n_sub = int(got.setdefault("n_sub", 33))
    if "h" not in got:
        got["h"] = float(con_dt) / n_sub
    h = float(got["h"])
    gz = float(got.setdefault("gz", GZ))
    for name, value in (("k_att", 20.0), ("rate_max", 10.0), ("k_rate", min(1.0, h / tau_rate)), ("k_thrust", min(1.0, h / tau_thrust)),
                        ("f_min", 0.0), ("f_max", 4.0 * gz), ("drag", (0.0, 0.0, 0.0)), ("yaw_cs", 1.0), ("yaw_sn", 0.0), ("cog_window", 10)):
        got.setdefault(name, value)
    w = np.zeros(COG_MAX)
    given = np.asarray(got.get("cog_weight", cog_weights()), np.float64).reshape(-1)
    w[:given.size] = given
    got["cog_weight"] = w
    got["drag"] = tuple(float(v) for v in got["drag"])
    return type("BodyParams", (), got)()


def body_state0(S, gz=GZ):
    """amk_sim_body_reset: [S, BODY_DOUBLES] -- level (q = 1, 0, 0, 0), at rest, hovering (f = gz), an empty IMU window, the rest 0"""
    body = np.zeros((int(S), BODY_DOUBLES))
    body[:, BODY_Q] = 1.0
    body[:, BODY_F] = gz
    return body


def _body_clamp(v, lo, hi):
    """v < lo ? lo : (v > hi ? hi : v): a NaN fails both comparisons and passes through"""
    return np.where(v < lo, lo, np.where(v > hi, hi, v))


def _body_rotation(qw, qx, qy, qz):
    """The nine polynomial entries of the rotation of a (nearly unit) quaternion, rows of [S] arrays"""
    return ((1.0 - 2.0 * ((qy * qy) + (qz * qz)), 2.0 * ((qx * qy) - (qw * qz)), 2.0 * ((qx * qz) + (qw * qy))),
            (2.0 * ((qx * qy) + (qw * qz)), 1.0 - 2.0 * ((qx * qx) + (qz * qz)), 2.0 * ((qy * qz) - (qw * qx))),
            (2.0 * ((qx * qz) - (qw * qy)), 2.0 * ((qy * qz) + (qw * qx)), 1.0 - 2.0 * ((qx * qx) + (qy * qy))))


def _body_index(v, hi):
    """One of the two integers kept as doubles: truncated towards zero; a value outside [0, hi] (or a NaN) reads as 0"""
    v = np.asarray(v, np.float64)
    ok = (v >= 0.0) & (v <= hi)
    return np.where(ok, np.trunc(np.where(ok, v, 0.0)), 0.0).astype(np.int64)


def body_step_ordered(prm, x, body, cmd, pose_quantum=0.0):
    """amk_sim_vehicle_step_body in numpy, operation for operation (include/avoid_mpc_amd.h, "The rigid-body vehicle"): a small rigid
    body flown by bfctrl's geometric controller in acceleration mode through prm.n_sub sub-steps of prm.h seconds, and the node's
    COGFilter over its body-frame specific force.  x [S, 10], body [S, BODY_DOUBLES], cmd [S, 3] -> (x+, body+, Twb [S, 4, 4]); the
    inputs are not modified.  Every sum is written out left to right; no matrix product, no transcendental.  A NaN's sign and
    payload are not part of the contract."""
    x, body, cmd = (np.array(a, np.float64) for a in (x, body, cmd))
    S = x.shape[0]
    rows = np.arange(S)
    h, hh, gz = float(prm.h), 0.5 * float(prm.h), float(prm.gz)
    d0, d1, d2 = prm.drag
    cs, sn = float(prm.yaw_cs), float(prm.yaw_sn)
    p = [x[:, 0].copy(), x[:, 1].copy(), x[:, 2].copy()]
    v = [x[:, 4].copy(), x[:, 5].copy(), x[:, 6].copy()]
    qw, qx, qy, qz = (body[:, BODY_Q + i].copy() for i in range(4))
    w = [body[:, BODY_RATE + i].copy() for i in range(3)]
    f = body[:, BODY_F].copy()
    held, head = _body_index(body[:, BODY_HELD], COG_MAX), _body_index(body[:, BODY_HEAD], COG_MAX - 1)
    ring = body[:, BODY_RING:BODY_RING + 3 * COG_MAX].reshape(S, COG_MAX, 3)      # (a view: the pushes land in `body`)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        # once per call: the desired attitude R_d = [X Y Z] of acc2rotmat on the command itself (gravity is already in it)
        T = (cmd[:, 0], cmd[:, 1], cmd[:, 2])
        n = np.sqrt((T[0] * T[0] + T[1] * T[1]) + T[2] * T[2])
        Z = (T[0] / n, T[1] / n, T[2] / n)
        y = (0.0 - Z[2] * sn, Z[2] * cs, Z[0] * sn - Z[1] * cs)
        m = np.sqrt((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2])
        Y = (y[0] / m, y[1] / m, y[2] / m)
        X = (Y[1] * Z[2] - Y[2] * Z[1], Y[2] * Z[0] - Y[0] * Z[2], Y[0] * Z[1] - Y[1] * Z[0])
        valid = (n > 0) & (m > 0)
        col = lambda D, R, j: (D[0] * R[0][j] + D[1] * R[1][j]) + D[2] * R[2][j]
        for _ in range(int(prm.n_sub)):
            R = _body_rotation(qw, qx, qy, qz)
            e = (0.5 * (col(Z, R, 1) - col(Y, R, 2)), 0.5 * (col(X, R, 2) - col(Z, R, 0)), 0.5 * (col(Y, R, 0) - col(X, R, 1)))   # 1.
            wc = [np.where(valid, _body_clamp(-(prm.k_att * e[i]), -prm.rate_max, prm.rate_max), 0.0) for i in range(3)]         # 2.
            fc = _body_clamp((T[0] * R[0][2] + T[1] * R[1][2]) + T[2] * R[2][2], prm.f_min, prm.f_max)                          # 3.
            w = [w[i] + prm.k_rate * (wc[i] - w[i]) for i in range(3)]                                                            # 4.
            f = f + prm.k_thrust * (fc - f)
            vb = [(R[0][i] * v[0] + R[1][i] * v[1]) + R[2][i] * v[2] for i in range(3)]                                           # 5.
            sb = (-(d0 * vb[0]), -(d1 * vb[1]), f - d2 * vb[2])
            aw = [(R[i][0] * sb[0] + R[i][1] * sb[1]) + R[i][2] * sb[2] for i in range(3)]
            aw[2] = aw[2] - gz
            for i in range(3):
                ring[rows, head, i] = sb[i]
            head = (head + 1) % COG_MAX
            held = np.minimum(held + 1, COG_MAX)
            v = [v[i] + h * aw[i] for i in range(3)]                                                                              # 6.
            p = [p[i] + h * v[i] for i in range(3)]
            dw = -(((qx * w[0]) + (qy * w[1])) + (qz * w[2]))                                                                     # 7.
            dx = ((qw * w[0]) + (qy * w[2])) - (qz * w[1])
            dy = ((qw * w[1]) + (qz * w[0])) - (qx * w[2])
            dz = ((qw * w[2]) + (qx * w[1])) - (qy * w[0])
            qw, qx, qy, qz = qw + hh * dw, qx + hh * dx, qy + hh * dy, qz + hh * dz
            nq = np.sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz)
            qw, qx, qy, qz = qw / nq, qx / nq, qy / nq, qz / nq
        R = _body_rotation(qw, qx, qy, qz)
        newest = lambda idx: ring[rows, (head - 1 - idx) % COG_MAX]                # [S, 3], the idx-th newest sample
        sbar = [newest(0)[:, i].copy() for i in range(3)]
        if prm.cog_window >= 2:
            cw = prm.cog_weight
            take = np.minimum(held, int(prm.cog_window))
            acc, wsum = [cw[0] * sbar[i] for i in range(3)], np.full(S, cw[0])
            for idx in range(1, int(prm.cog_window)):
                s, on = newest(idx), idx < take
                acc = [np.where(on, acc[i] + cw[idx] * s[:, i], acc[i]) for i in range(3)]
                wsum = np.where(on, wsum + cw[idx], wsum)
            sbar = [acc[i] / wsum for i in range(3)]
        a = [(R[i][0] * sbar[0] + R[i][1] * sbar[1]) + R[i][2] * sbar[2] for i in range(3)]
        a[2] = a[2] - gz
    for i in range(3):
        x[:, i] = p[i]; x[:, 4 + i] = v[i]; x[:, 7 + i] = a[i]; body[:, BODY_RATE + i] = w[i]
    for i, qi in enumerate((qw, qx, qy, qz)):
        body[:, BODY_Q + i] = qi
    body[:, BODY_F] = f; body[:, BODY_HELD] = held; body[:, BODY_HEAD] = head
    Twb = np.zeros((S, 4, 4))
    Twb[:, 3, 3] = 1.0
    for i in range(3):
        for j in range(3):
            Twb[:, i, j] = R[i][j]
        Twb[:, i, 3] = np.rint(p[i] * pose_quantum) / pose_quantum if pose_quantum > 0 else p[i]
    return x, body, Twb


class WallWorld(FlightWorld):
    """FlightWorld's corridor of cylinders with flat things in it: every `wall_every` metres from `wall_first` on a wall stands across
    the corridor (|y| <= 8 m, `thick` m deep, 4 m high) with one gap `gap` m wide at a seeded y.  A wall is two boxes, the piers left
    and right of the gap; every second wall has a lintel over the gap (z0 = `lintel` > 0: a gate), and every third is yawed a few
    degrees about its own middle, gap and lintel with it.  Cylinders that would stand in a wall are left out, so the worlds of a
    fleet hold different cylinder counts.  Seeded and pure, like FlightWorld: `box` float64 [n_box, 8] =
    (cx, cy, hx, hy, c, s, z0, z1), the layout of amk_sim_render_world."""

    def __init__(self, seed, prm, n_points, length=80.0, wall_first=9.0, wall_every=12.0, gap=3.0, thick=0.1, lintel=2.5, **kw):
        super().__init__(seed, prm, n_points, length=length, **kw)
        rng = np.random.default_rng([self.seed, 0xB0C5])
        rows = []
        for i, wx in enumerate(np.arange(wall_first, float(length), wall_every)):
            gy = rng.uniform(-4.0, 4.0)
            yaw = rng.uniform(-0.15, 0.15) if i % 3 == 2 else 0.0
            c, s = (np.cos(yaw), np.sin(yaw)) if yaw != 0.0 else (1.0, 0.0)
            for lo, hi in ((-8.0, gy - gap / 2), (gy + gap / 2, 8.0)):             # the two piers, along the wall's own y axis
                mid, half = (lo + hi) / 2, (hi - lo) / 2
                rows.append([wx - s * mid, c * mid, thick / 2, half, c, s, 0.0, 4.0])
            if i % 2 == 1:
                rows.append([wx - s * gy, c * gy, thick / 2, gap / 2, c, s, lintel, 4.0])
        self.box = np.array(rows, np.float64).reshape(-1, 8)
        footprint = self.box.copy(); footprint[:, 6] = 0.0                          # (a cylinder under a lintel would pierce it)
        keep = np.abs(box_clearance(np.stack([self.cx, self.cy, np.ones_like(self.cx)], axis=1), footprint)) > self.cr + 0.05
        self.cx, self.cy, self.cr = self.cx[keep], self.cy[keep], self.cr[keep]   # no cylinder stands in a wall

    def box_clearance(self, p):
        return box_clearance(p, self.box)
