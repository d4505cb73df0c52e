"""Keyframe-map scripts on which the ORDER OF EQUAL DISTANCES decides the answer (TEST INFRASTRUCTURE): the cases of
amk_kfmap_set_tie_order(AMK_TIES_NANOFLANN), shared by tests/test_kfmap_tie_cases.py (CPU: the cases are not vacuous) and
tests/test_kfmap_tie_order_gpu.py.

  script      S = 4 scenes x 6 periods.  Obstacle frames: unique points of a 0.25 m lattice (integer cells of a 12^3 cube, shuffled),
              300 (scenes 0, 3) or 600 (scene 1) of them, moved by whole lattice steps along +x from period to period -- every
              squared distance is a multiple of 1/64, so the sweep's comparison with th_dist = 0.1 is exact and queries at cell
              centres or on lattice points tie all the time.  A period without a move re-uses the cloud with four points exchanged:
              fewer than th_count = 10 outliers, the keyframe is kept; a move leaves hundreds, it is rebuilt from them.
              Scene 2: 4200 points of a 20^3 lattice (more than kExactBigNode = 4096: the workgroup-split path of the tree build).
              Scene 1 gets an empty frame in period 2, scene 3 becomes a new map before period 4.  Edge frames: 40 .. 150 lattice points.
  queries     32 per scene and period, half at cell centres, half on lattice points, inside the frame's cube
  steps       one per scene and period (step_scene); scenes 0 and 2 fly beside the camera's axis with reference point 0 outside the
              camera frame, so their first path rows, the edge 1-NN and the snapped point's re-query are merged over all the frames
              the map holds, the other rows take the fast path (step_rows: which row took which path, and whether the orders differ)
  NanoFrame   a frame of tests/_map_query.py's rules whose per-frame list is KdHandle.search: nanoflann's order (TreeFrame: cloud-index order)
  behind_pair the hand-built DroneBehindPts pair: nine points near the drone and ahead of it, A = p + (d, 0, 0) ahead and
              B = p - (d, 0, 0) behind at exactly the same distance, thirty far points; the tenth neighbour is A or B"""
import functools

import numpy as np

from avoid_mpc_amd import synth
from tests import _kfmap, _map_query as mq, _oracle

S, PERIODS, NQ = 4, 6, 32
H = 0.25                                    # the lattice
CAP, ECAP = 4200, 160
BIG_SCENE, EMPTY_SCENE, RESET_SCENE = 2, 1, 3
EMPTY_PERIOD, RESET_BEFORE = 2, 4
TH_DIST, TH_COUNT, DEPTH_MIN = 0.1, 10, 0.25
TBC = mq.look_x_pose([0.0, 0.0, 0.0])
CAM = (80.0, 80.0, 80.0, 60.0, 10.0, 160, 120)
MOVES = (0, 1, 0, 1, 1, 0)                  # lattice steps along +x before each period
# (max_frame_count, K, forced wide merge)
# (the forced run holds 3 frames: a map of 100 takes the wide merge anyway, the flag changes a launch only below that width)
CONFIGS = ((3, 8, 0), (100, 8, 0), (100, 10, 0), (3, 8, 1))
SAFETY_DISTANCE = 0.6
NO_SNAP_SCENE = 3                           # its reference point 0 stays 0.75 m in front of the cube
# scenes whose reference path runs beside the camera's axis (cell centres in y): the points nearer than the offset are outside
# the camera frame and take the merge over every frame, the others the fast path; their point 0 is placed outside the frame too
LATERAL = {0: 1.125, 2: -1.375}


def prm_of(K, max_iter=1):
    return synth.MpcParams(T=0.33, K=K, max_iter=max_iter, safety_distance=SAFETY_DISTANCE)   # N = 10


def side(s):
    return 20 if s == BIG_SCENE else 12


def n_points(s):
    return {0: 300, 1: 600, BIG_SCENE: 4200, 3: 300}[s]


def lattice(rng, n, L):
    cells = rng.permutation(L ** 3)[:n]
    return np.stack([cells // (L * L), (cells // L) % L, cells % L], 1).astype(np.float64) * H


def cum_moves(t):
    return sum(MOVES[:t + 1])


def drone(s, t):
    """the drone 1.25 m in front of the cube, at its centre line: every keyframe stays ahead of it (no pop by DroneBehindPts here)"""
    c = side(s) * H / 2
    return np.array([cum_moves(t) * H - 1.25, c, c])


def pose(s, t):
    Twb = np.eye(4)
    Twb[:3, 3] = drone(s, t)
    return Twb @ TBC


@functools.lru_cache(maxsize=None)
def script():
    """frames[t][s] = (cloud f32 [n, 3], edge f32 [m, 3], Twc)"""
    frames = []
    base = {}
    for t in range(PERIODS):
        row = []
        for s in range(S):
            rng = np.random.default_rng(1000 * s + t)
            L = side(s)
            if MOVES[t] or t == 0:
                base[s] = lattice(rng, n_points(s), L)
            else:                           # the same cloud with four points exchanged for free cells
                have = {tuple(p) for p in base[s]}
                fresh = [p for p in lattice(rng, 64, L) if tuple(p) not in have][:4]
                base[s] = np.concatenate([base[s][4:], np.array(fresh)])
            cloud = base[s] + [cum_moves(t) * H, 0.0, 0.0]
            edge = lattice(rng, int(rng.integers(40, 151)), L) + [cum_moves(t) * H, 0.0, 0.0]
            if s == EMPTY_SCENE and t == EMPTY_PERIOD:
                cloud = cloud[:0]
            row.append((cloud.astype(np.float32), edge.astype(np.float32), pose(s, t)))
        frames.append(tuple(row))
    return tuple(frames)


def queries(t, stride=3):
    """[S, NQ, stride]: 16 cell centres, 16 lattice points of the period's cube (some of them outside the camera's view)"""
    q = np.zeros((S, NQ, stride))
    for s in range(S):
        rng = np.random.default_rng(77 + 10 * s + t)
        L = side(s)
        cells = rng.integers(0, L - 1, size=(NQ, 3)).astype(np.float64) * H
        cells[:NQ // 2] += H / 2
        q[s, :, :3] = cells + [cum_moves(t) * H, 0.0, 0.0]
    return q


class NanoFrame:
    """One frame of a MapOracle answered in nanoflann's order: the per-frame list is KdHandle.search's."""

    def __init__(self, kd):
        self.kd, self.size = kd, kd.size()

    def answer(self, q, k):
        if self.size == 0:
            return np.zeros(0), np.zeros((0, 3), np.float32)
        _, d2, pts = self.kd.search(np.asarray(q, np.float64), k)
        return d2, pts


def frames_of(oracles, edge=False, nano=True):
    cls = NanoFrame if nano else mq.TreeFrame
    return [[cls(f.ke if edge else f.kd) for f in o.frames()] for o in oracles]


def new_map(max_frames, cls=_kfmap.MapOracle):
    return cls(max_frames, TH_DIST, TH_COUNT, DEPTH_MIN, TBC)


def step_scene(s, t, K):
    """odometry and a reference path on dyadic coordinates: straight ahead from the drone through the cube; reference point 0 is the
    midpoint of the two closest points of the period's edge cloud -- exactly equidistant from both, and inside the safety distance
    of some obstacle, so the step snaps it to ONE of them (scene 3: 0.75 m in front of the cube, no snap).  In the scenes of LATERAL
    the path is offset sideways and the pair is taken among the edge points outside the camera frame, with its midpoint outside:
    the edge 1-NN, the re-query of the snapped point and the first path rows are merged over all the frames the map holds."""
    prm = prm_of(K)
    sc = synth.make_scene(100, 1 + s, prm)
    d = drone(s, t)
    sc["pos"] = d.copy()
    rp = sc["ref_path"].copy()
    rp[:, 0] = d[0] + 0.5 + 0.25 * np.arange(len(rp))
    rp[:, 1] = d[1] + LATERAL.get(s, 0.125 if s % 2 else 0.0)
    rp[:, 2] = d[2] + 0.125
    if s != NO_SNAP_SCENE:
        e = script()[t][s][1].astype(np.float64)
        d2 = ((e[:, None, :] - e[None, :, :]) ** 2).sum(-1) + np.eye(len(e)) * 1e9
        if s in LATERAL:
            out = np.array([not mq.pt_in_frame(p, pose(s, t), CAM) for p in e])
            mid = np.array([[not mq.pt_in_frame((a + b) / 2, pose(s, t), CAM) for b in e] for a in e])
            d2 = np.where(out[:, None] & out[None, :] & mid, d2, 1e9)
        i, j = np.unravel_index(np.argmin(d2), d2.shape)
        rp[0, :3] = (e[i] + e[j]) / 2
    sc["ref_path"] = rp
    return sc


def oracle_step(m, s, t, K, max_iter=1, cam=CAM):
    prm = prm_of(K, max_iter)
    sc = step_scene(s, t, K)
    mpc = _oracle.MpcOracle(prm.T, prm.dt, prm.K); mpc.configure(prm)
    if max_iter == 1:
        mpc.set_solver_options(max_iter=1)
    rp = sc["ref_path"].copy()
    r = m.step(mpc, prm, _oracle.scene_state_quads(sc, prm), sc["pos"][0], rp, cam)
    r["ref_path"] = rp
    return r


def step_obstacles(m, K, res, nano=True):
    """[N, K, 3]: the obstacle block of one oracle step (mpc_max_iter = 1) restated by tests/_map_query.py's rules over the path the
    step packed, in nanoflann's order (what stepo_run_frames packed) or in cloud-index order (a map whose obstacle trees were given up)"""
    from tests import _frames_cases as fc
    N = prm_of(K).N
    path = fc.split_P(res["ref_log"][0], N, K)[1]
    frames = [(NanoFrame if nano else mq.TreeFrame)(f.kd) for f in m.frames()]
    out = np.full((N, K, 3), 10000.0)
    for i in range(N):
        a = mq.query_nearest(frames, path[i, :3], K, m.Twc, CAM)
        out[i, :a["count"]] = a["pts"][:a["count"]]
    return out


def step_rows(m, s, t, K, res):
    """The N K-NN rows and the edge 1-NN of one oracle step (mpc_max_iter = 1), restated by tests/_map_query.py's rules in both
    orders.  -> [(row (-1: the edge 1-NN of point 0 before the snap), path 'fast' | 'merge', frames held, the two orders differ)];
    the nanoflann-ordered restatement must be what stepo_run_frames packed."""
    from tests import _frames_cases as fc
    N = prm_of(K).N
    _, path, obst, _ = fc.split_P(res["ref_log"][0], N, K)
    obs, edge = ([NanoFrame(getattr(f, a)) for f in m.frames()] for a in ("kd", "ke"))
    obs_i, edge_i = ([mq.TreeFrame(getattr(f, a)) for f in m.frames()] for a in ("kd", "ke"))
    rows = []
    p0 = step_scene(s, t, K)["ref_path"][0, :3]
    if not np.array_equal(p0, path[0, :3]):                      # snapped: the edge 1-NN ran, on the point as it was given
        a, b = (mq.query_nearest(fr, p0, 1, m.Twc, CAM) for fr in (edge, edge_i))
        assert np.array_equal(a["pts"][0].astype(np.float64), path[0, :3]), (s, t)
        rows.append((-1, a["path"], len(edge), not np.array_equal(a["pts"], b["pts"])))
    for i in range(N):
        a, b = (mq.query_nearest(fr, path[i, :3], K, m.Twc, CAM) for fr in (obs, obs_i))
        want = np.full((K, 3), 10000.0)
        want[:a["count"]] = a["pts"][:a["count"]]
        assert np.array_equal(want, obst[i]), (s, t, i)
        rows.append((i, a["path"], len(obs), {tuple(p) for p in a["pts"][:a["count"]].tolist()} != {tuple(p) for p in b["pts"][:b["count"]].tolist()}))
    return rows


class _Run:
    pass


@functools.lru_cache(maxsize=None)
def run(max_frames, K):
    """MapOracle over the script -> object with, per period: summaries [s] = (n_keyframes, sizes, last_outliers), pops [s], and the
    expected answers in BOTH orders: nano / index = dict(obs_cam, obs_nocam, edge_cam (k = 1), dist); steps[t][s] (mpc_max_iter = 1);
    step_rows[t][s] = step_rows() of that step"""
    maps = [new_map(max_frames) for _ in range(S)]
    r = _Run()
    r.summaries, r.pops, r.nano, r.index, r.steps, r.full_steps, r.status_frames, r.p0_edge, r.step_rows = [], [], [], [], [], [], [], [], []
    for t in range(PERIODS):
        if t == RESET_BEFORE:
            maps[RESET_SCENE] = new_map(max_frames)
        pops = []
        for s, (c, e, T) in enumerate(script()[t]):
            maps[s].add_vertex(c, e, T, stamp=t)
            before = list(maps[s].kfs)
            maps[s].update()
            pops.append(sum(1 for f in before if all(f is not g for g in maps[s].kfs)))
        r.pops.append(pops)
        r.summaries.append([m.summary() + (m.last_outliers,) for m in maps])
        r.status_frames.append([len(m.frames()) for m in maps])
        q = queries(t)
        Twc = np.stack([m.Twc for m in maps])
        for nano, out in ((True, r.nano), (False, r.index)):
            obs, edge = frames_of(maps, False, nano), frames_of(maps, True, nano)
            out.append(dict(obs_cam=mq.expected_batch(obs, q, K, Twc, CAM), obs_nocam=mq.expected_batch(obs, q, K),
                            edge_cam=mq.expected_batch(edge, q, 1, Twc, CAM), dist=mq.expected_distance(obs, q)))
        r.steps.append([oracle_step(maps[s], s, t, K) for s in range(S)])
        r.step_rows.append([step_rows(maps[s], s, t, K, r.steps[t][s]) for s in range(S)])
        # the edge 1-NN of reference point 0 in both orders (what a snap moves it to)
        p0 = np.stack([step_scene(s, t, K)["ref_path"][:1, :3] for s in range(S)])
        r.p0_edge.append(tuple(mq.expected_batch(frames_of(maps, True, nano), p0, 1, Twc, CAM)["pts"][:, 0, 0] for nano in (True, False)))
    r.last_full = [oracle_step(maps[s], s, PERIODS - 1, K, max_iter=3) for s in range(S)]
    return r


def rows_that_differ(a, b):
    """[S, Q] bool: the two answers hold different point SETS"""
    S_, Q = a["pts"].shape[:2]
    out = np.zeros((S_, Q), bool)
    for s in range(S_):
        for i in range(Q):
            sa = {tuple(p) for p, f in zip(a["pts"][s, i].tolist(), a["frame"][s, i]) if f >= 0}
            sb = {tuple(p) for p, f in zip(b["pts"][s, i].tolist(), b["frame"][s, i]) if f >= 0}
            out[s, i] = sa != sb
    return out


# ---------------------------------------------------------------------------------------------- the DroneBehindPts pair
PAIR_P = np.array([4.0, 1.5, 1.5])          # the drone when the keyframe is tested (dyadic)
PAIR_D = 1.0                                # ptbx(B) = -1 <= depth_min < ptbx(A) = 1


class IndexOrderMap(_kfmap.MapOracle):
    """MapOracle whose DroneBehindPts takes its ten neighbours in cloud-index order (the default mode of the device map)"""

    def drone_behind_pts(self, frame):
        twb, bx = _kfmap.drone_pose(self.Twc, self.Tbc_inv)
        cnt = min(frame.kd.size(), 10)
        if frame.kd.size() == cnt:
            return True
        idx, _ = frame.kd.bruteforce(twb, cnt)
        pts = mq.tree_cloud(frame.kd)[idx]
        for p in pts.astype(np.float64):
            if (bx[0] * (p[0] - twb[0]) + bx[1] * (p[1] - twb[1])) + bx[2] * (p[2] - twb[2]) <= self.depth_min:
                return False
        return True


def behind_pair(a_first):
    """[(cloud, edge, Twc)] x 2 periods: the keyframe under test, then a far frame at the pose that tests it"""
    rng = np.random.default_rng(5)
    near = PAIR_P + np.stack([0.375 + 0.125 * rng.integers(0, 3, 9), 0.125 * rng.integers(-2, 3, 9), 0.125 * rng.integers(-2, 3, 9)], 1)
    far = PAIR_P + np.stack([3.0 + 0.25 * np.arange(30), 0.25 * rng.integers(-4, 5, 30), 0.25 * rng.integers(-4, 5, 30)], 1)
    A, B = PAIR_P + [PAIR_D, 0, 0], PAIR_P - [PAIR_D, 0, 0]
    pair = [A, B] if a_first else [B, A]
    kf = np.concatenate([near[:5], pair[:1], far[:15], pair[1:], near[5:], far[15:]]).astype(np.float32)
    cur = (PAIR_P + [30.0, 0, 0] + lattice(rng, 60, 8)).astype(np.float32)
    T0, T1 = np.eye(4), np.eye(4)
    T0[:3, 3] = PAIR_P - [20.0, 0, 0]
    T1[:3, 3] = PAIR_P
    return [(kf, kf[:8].copy(), T0 @ TBC), (cur, cur[:8].copy(), T1 @ TBC)]


def behind_outcome(a_first, cls):
    """number of keyframes after the two periods: 0 = the keyframe was popped, 2 = kept, swept, the current frame inserted"""
    m = cls(3, TH_DIST, TH_COUNT, DEPTH_MIN, TBC)
    for c, e, T in behind_pair(a_first):
        m.add_vertex(c, e, T)
        m.update()
    return len(m.kfs)
