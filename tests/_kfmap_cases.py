"""Inputs that aim at the keyframe map's own bookkeeping (TEST INFRASTRUCTURE): FrameKDMap's deque (AM/src/FrameKDMap.cpp:437-488)
past 64 entries and at its ceiling, DroneBehindPts (:233-252) on and next to each of its comparisons, and a restatement of both in
plain numpy that never calls tests/_kfmap.py: MapOracle.update.

  ceiling_script   135 periods per scene; the cloud of period t holds 12 + t points, so a frame is identified by its SIZE alone.
                   Clouds lie 8 to 10 m ahead of the drone, in z layers that keep consecutive clouds more than th_dist apart: with
                   th_count = 1 every swept keyframe is rebuilt from ALL its points and the list of query-frame sizes IS the deque.
                   The drone advances 0.05 m per period, jumps +5 m after period 115 (it passes the older keyframes: several pops
                   in one pass) and +40 m after period 125 (it passes all of them: the deque empties, the current frame is NOT
                   inserted, :459-461; the pass after that takes the first-keyframe branch, :445-448).
  ceiling_run      MapOracle over four such scenes: scene 1 gets an empty frame every 11th period, scene 2 is fed every other
                   period only (on the device through first_scene / sub-range calls)
  gate_cases       two-period scripts, one scene each: frame A with one special point, then frame B 30 m away at the pose that
                   tests A
  NumpyMap         the pop loop, the gate and the sweep with brute-force neighbours (np.argsort of squared distances)

tests/test_kfmap_cases.py proves on the CPU that these inputs reach every branch; tests/test_kfmap_deque_gpu.py runs them."""
import functools

import numpy as np

from tests import _kfmap, _oracle
from avoid_mpc_amd import synth

TBC = np.array([[0, 0, 1, 0.125], [-1, 0, 0, 0.0], [0, -1, 0, 0.0625], [0, 0, 0, 1.0]])          # dyadic translations
GATE_TBC = np.array([[0, 0, 1, 0.125], [-1, 0, 0, -0.25], [0, -1, 0, 0.0625], [0, 0, 0, 1.0]])   # three distinct non-zero ones
DEPTH_MIN = 0.25
TH_DIST, TH_COUNT = 0.05, 1
PERIODS, S, CAP, ECAP = 135, 4, 160, 8
JUMPS = ((115, 5.0), (125, 40.0))                 # (after period, metres)
MAX_FRAMES = (1, 2, 63, 64, 100)
EMPTY_SCENE, SKIP_SCENE = 1, 2
K = 8


def drone_x(t):
    return 0.05 * t + sum(d for after, d in JUMPS if t > after)


def twc_of_drone(x, Tbc=TBC):
    Twb = np.eye(4)
    Twb[:3, 3] = [x, 0.0, 1.5]
    return Twb @ Tbc


def fed(s, t):
    """does scene s get an AddVertex call in period t?"""
    return s != SKIP_SCENE or t % 2 == 0


@functools.lru_cache(maxsize=None)
def ceiling_script(seed):
    """[(cloud [12 + t, 3] f32, edge [8, 3] f32, Twc)] for PERIODS periods.  z layer (t mod 8) * 0.25 + [0, 0.125]: clouds whose
    periods differ by 1 .. 7 are at least 0.125 m > th_dist apart (the sweep only ever compares clouds 1 or 2 periods apart)."""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(PERIODS):
        n, x = 12 + t, drone_x(t)
        cloud = np.stack([x + 8.0 + rng.uniform(0, 2, n), rng.uniform(-3, 3, n), 0.25 * (t % 8) + rng.uniform(0, 0.125, n)], 1).astype(np.float32)
        out.append((cloud, cloud[:ECAP].copy(), twc_of_drone(x)))
    return tuple(out)


def scene_frame(s, t):
    """(cloud, edge, Twc) scene s is handed in period t, or None when it is skipped; the cloud is empty on scene 1's 11th periods"""
    if not fed(s, t):
        return None
    cloud, edge, Twc = ceiling_script(100 + s)[t]
    if s == EMPTY_SCENE and t % 11 == 7:
        cloud = cloud[:0]
    return cloud, edge, Twc


class _Run:
    pass


def _summary(m):
    nk, sizes = m.summary()
    return nk, sizes, m.last_outliers


def step_scene(s, x):
    """odometry and a straight reference path that starts at a drone at x (synth.make_scene, shifted)"""
    prm = synth.MpcParams(T=0.66, K=K, max_iter=1)
    sc = synth.make_scene(100, 1 + s, prm)
    sc["pos"] = np.array(sc["pos"], np.float64).copy(); sc["ref_path"] = sc["ref_path"].copy()
    sc["pos"][0] += x; sc["ref_path"][:, 0] += x
    return sc


STEP_CAM = (32.0, 32.0, 32.0, 24.0, 3.75, 64, 48)   # depth_max 3.75 m: reference points 10 .. N - 1 (3.99 m ahead and more) are out of range
PRM = synth.MpcParams(T=0.66, K=K, max_iter=1)


def oracle_step(m, s, x):
    sc = step_scene(s, x)
    mpc = _oracle.MpcOracle(PRM.T, PRM.dt, PRM.K); mpc.configure(PRM); mpc.set_solver_options(max_iter=1)
    rp = sc["ref_path"].copy()
    r = m.step(mpc, PRM, _oracle.scene_state_quads(sc, PRM), sc["pos"][0], rp, STEP_CAM)
    r["ref_path"] = rp
    return r


def step_periods(max_frames):
    """periods after which a step is taken: the deque at its ceiling, right after the pass with several pops, the empty deque, two
    periods later"""
    return (110, JUMPS[0][0] + 1, JUMPS[1][0] + 1, JUMPS[1][0] + 3) if max_frames in (64, 100) else ()


@functools.lru_cache(maxsize=None)
def ceiling_run(max_frames, reset_at=None, reset_scenes=()):
    """MapOracle over the four scenes.  -> object with summaries [period][scene] = (n_keyframes, query-frame sizes, last_outliers),
    pops [period][scene] (keyframes the pass removed), need [period][scene] (mbNeedProcessPtCloud before the pass), steps
    {period: [scene] oracle step at mpc_max_iter = 1}.  reset_at / reset_scenes: those scenes become NEW maps before that period."""
    maps = [_kfmap.MapOracle(max_frames, TH_DIST, TH_COUNT, DEPTH_MIN, TBC) for _ in range(S)]
    run = _Run()
    run.summaries, run.pops, run.need, run.steps = [], [], [], {}
    for t in range(PERIODS):
        if t == reset_at:
            for s in reset_scenes:
                maps[s] = _kfmap.MapOracle(max_frames, TH_DIST, TH_COUNT, DEPTH_MIN, TBC)
        row, pops, need = [], [], []
        for s in range(S):
            fr = scene_frame(s, t)
            if fr is not None:
                maps[s].add_vertex(fr[0], fr[1], fr[2], stamp=t)
            need.append(bool(maps[s].need))
            before = list(maps[s].kfs)
            maps[s].update()
            pops.append(sum(1 for f in before if all(f is not g for g in maps[s].kfs)))
            row.append(_summary(maps[s]))
        run.summaries.append(row); run.pops.append(pops); run.need.append(need)
        if t in step_periods(max_frames) and (reset_at is None or t > reset_at):
            run.steps[t] = [oracle_step(maps[s], s, drone_x(t)) for s in range(S)]
    return run


# -------------------------------------------------------------------------------------------- clouds that fill their capacity
FULL_CAP, FULL_PERIODS, FULL_MAX_FRAMES = 40, 10, 5


def full_x(t):
    return 1.5 * t + (6.0 if t >= 7 else 0.0)


@functools.lru_cache(maxsize=None)
def full_script(seed):
    """[(cloud [FULL_CAP, 3], edge [ECAP, 3], Twc)]: every cloud fills the map's capacity (AddVertex without counts); the drone
    advances 1.5 m per period and jumps 6 m before period 7, past most of its keyframes"""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(FULL_PERIODS):
        n, x = FULL_CAP, full_x(t)
        cloud = np.stack([x + 8.0 + rng.uniform(0, 2, n), rng.uniform(-3, 3, n), 0.25 * (t % 8) + rng.uniform(0, 0.125, n)], 1).astype(np.float32)
        out.append((cloud, cloud[:ECAP].copy(), twc_of_drone(x)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def full_run():
    """MapOracle over full_script(200 + s): summaries and pops like ceiling_run, a step after the last period"""
    maps = [_kfmap.MapOracle(FULL_MAX_FRAMES, TH_DIST, TH_COUNT, DEPTH_MIN, TBC) for _ in range(S)]
    run = _Run()
    run.summaries, run.pops, run.steps = [], [], {}
    for t in range(FULL_PERIODS):
        row, pops = [], []
        for s in range(S):
            maps[s].add_vertex(*full_script(200 + s)[t], stamp=t)
            before = list(maps[s].kfs)
            maps[s].update()
            pops.append(sum(1 for f in before if all(f is not g for g in maps[s].kfs)))
            row.append(_summary(maps[s]))
        run.summaries.append(row); run.pops.append(pops)
    t = FULL_PERIODS - 1
    run.steps[t] = [oracle_step(maps[s], s, full_x(t)) for s in range(S)]
    return run


# ------------------------------------------------------------------------------------------------------------------- the gate
YAW90 = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])


def _rot(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]]); Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    return Rz @ Ry @ Rx


GENERAL = _rot(0.5, -0.4, 2.6)                     # roll, pitch and yaw all non-zero: no entry of the rotation below 0.2
ULP = float(np.nextafter(np.float32(0.25), np.float32(1)))   # one float32 ulp above depth_min

# (name, rotation of the drone, its position, points of A besides the special one, the special point in the BODY frame or None,
#  keyframes left after period 1)
_GATE = (
    ("x_eq_depth_min", YAW90, (2.0, -1.0, 1.5), 14, (0.25, 0.5, 0.0), 0),
    ("x_one_ulp_above", YAW90, (2.0, 0.0, 1.5), 14, (ULP, 0.5, 0.0), 2),
    ("x_minus_one", YAW90, (2.0, -1.0, 1.5), 14, (-1.0, 0.5, 0.0), 0),
    ("eleven_behind_farthest", YAW90, (2.0, -1.0, 1.5), 10, (-8.0, 0.5, 0.0), 2),
    ("eleven_behind_nearest", YAW90, (2.0, -1.0, 1.5), 10, (-1.0, 0.5, 0.0), 0),
    ("ten_with_behind", YAW90, (2.0, -1.0, 1.5), 9, (-1.0, 0.5, 0.0), 2),
    ("one_point", YAW90, (2.0, -1.0, 1.5), 0, (-1.0, 0.5, 0.0), 2),
    ("general_below", GENERAL, (1.7, -2.3, 1.1), 14, (0.19, 0.6, -0.4), 0),
    ("general_above", GENERAL, (1.7, -2.3, 1.1), 14, (0.31, 0.6, -0.4), 2),
    ("general_behind", GENERAL, (1.7, -2.3, 1.1), 14, (-1.0, 0.6, -0.4), 0),
)
GATE_MARGIN = 0.05
GATE_MAX_FRAMES = 5


@functools.lru_cache(maxsize=None)
def gate_cases():
    """-> tuple of dict(name, frames = [(cloud, edge, Twc)] x 2, special (world, f32), Twb (period 1), expect)"""
    out = []
    for i, (name, R, pos, n, special, expect) in enumerate(_GATE):
        rng = np.random.default_rng(700 + i)
        Twb = np.eye(4); Twb[:3, :3] = R; Twb[:3, 3] = pos
        world = lambda pb: (pb @ R.T + np.asarray(pos)).astype(np.float32)
        body = np.stack([rng.uniform(4, 6, n), rng.uniform(-1, 1, n), rng.uniform(-0.5, 0.5, n)], 1)
        sp = world(np.asarray(special, np.float64)[None])
        k = int(rng.integers(0, n + 1))                                 # (the special point anywhere in the cloud)
        A = np.concatenate([world(body[:k]), sp, world(body[k:])]).astype(np.float32)
        nb = 20 + i
        B = world(np.stack([rng.uniform(30, 32, nb), rng.uniform(-1, 1, nb), rng.uniform(-0.5, 0.5, nb)], 1))
        Twb0 = Twb.copy(); Twb0[:3, 3] -= R[:, 0]                        # period 0: one metre further back
        out.append(dict(name=name, frames=[(A, A[:ECAP].copy(), Twb0 @ GATE_TBC), (B, B[:ECAP].copy(), Twb @ GATE_TBC)],
                        special=sp[0], Twb=Twb, expect=expect))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def gate_run():
    """MapOracle over every gate case -> [period][case] = (n_keyframes, query-frame sizes, last_outliers)"""
    cases = gate_cases()
    maps = [_kfmap.MapOracle(GATE_MAX_FRAMES, TH_DIST, TH_COUNT, DEPTH_MIN, GATE_TBC) for _ in cases]
    rows = []
    for t in range(2):
        for m, c in zip(maps, cases):
            m.add_vertex(*c["frames"][t], stamp=t); m.update()
        rows.append([_summary(m) for m in maps])
    return rows


# ------------------------------------------------------------------------------------------ the numpy restatement of the map
def _d2(cloud, q):
    c = np.asarray(cloud, np.float32).astype(np.float64)
    return ((q[0] - c[:, 0]) ** 2 + (q[1] - c[:, 1]) ** 2) + (q[2] - c[:, 2]) ** 2


class NumpyMap:
    """KeyframeThreadWorker's body on plain arrays: keyframes are point arrays, neighbours come from a full sort.  `ties` counts
    the searches whose answer depends on the order of equal distances (the inputs are chosen so that it stays 0)."""

    def __init__(self, max_frame_count, th_dist, th_count, depth_min, Tbc):
        self.mfc, self.th_dist, self.th_count, self.depth_min = max_frame_count, th_dist, th_count, depth_min
        T = np.asarray(Tbc, np.float64)
        self.Tbc_inv = np.eye(4); self.Tbc_inv[:3, :3] = T[:3, :3].T; self.Tbc_inv[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
        self.cur, self.kfs, self.need, self.Twc, self.ties = None, [], False, np.eye(4), 0

    def add_vertex(self, cloud, Twc):
        if len(cloud) == 0:
            return
        self.cur, self.Twc, self.need = np.asarray(cloud, np.float32), np.asarray(Twc, np.float64), True

    def behind(self, cloud):                       # DroneBehindPts: true = every examined point is ahead of the drone
        Twb = self.Twc @ self.Tbc_inv
        twb, Rbw = Twb[:3, 3], Twb[:3, :3].T
        cnt = min(len(cloud), 10)
        if not len(cloud) > cnt:                   # SearchForNearest yields nothing unless the cloud holds MORE than cnt points
            return True
        d2 = _d2(cloud, twb)
        order = np.argsort(d2, kind="stable")
        self.ties += int(len(np.unique(d2[order[:cnt + 1]])) != cnt + 1)
        for p in cloud[order[:cnt]].astype(np.float64):
            if (Rbw @ (p - twb))[0] <= self.depth_min:
                return False
        return True

    def update(self):
        if not self.need:
            return
        self.need = False
        if not self.kfs:
            self.kfs.append(self.cur)
            return
        while self.kfs and (len(self.kfs) > self.mfc or not self.behind(self.kfs[0])):
            self.kfs.pop(0)
        if not self.kfs or self.kfs[-1] is self.cur:
            return
        last = self.kfs[-1]
        if not len(self.cur) > 1:
            return
        nearest = np.array([_d2(self.cur, p.astype(np.float64)).min() for p in last])
        out = np.sqrt(nearest) > self.th_dist
        if out.sum() < self.th_count:
            return
        self.kfs[-1] = last[out]
        self.kfs.append(self.cur)

    def summary(self):
        fr = [] if self.cur is None else [self.cur] + self.kfs[:-1]
        return len(self.kfs), [len(f) for f in fr]
