"""FrameKDMap's queries over a multi-frame map, restated in Python (TEST INFRASTRUCTURE): the expected answers of
amk_kfmap_query_nearest / amk_kd_query_frames / *_nearest_distance.

The rules are those of include/avoid_mpc_amd.h ("The map's own queries") and of oracle/step_oracle.c: mapf_query /
mapf_nearest_distance; the per-frame answers come from

  CloudFrame   a cloud the test owns           _oracle.kd_brute_np                       (order by (distance, index), size rule)
  TreeFrame    a tree of _kfmap.MapOracle      KdHandle.bruteforce + _oracle.kd_count_rule

and on queries without an equal distance among a tree's k + 1 nearest TreeFrame checks itself against KdHandle.search (the
reference-shaped traversal)."""
import numpy as np

from tests import _oracle

DBL_MAX = _oracle.DBL_MAX
SQRT_DBL_MAX = np.sqrt(np.float64(DBL_MAX))

# cam-x -> world -y, cam-y -> world -z, cam-z -> world +x: a camera that looks along world +x
R_LOOK_X = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])


def look_x_pose(t):
    T = np.eye(4)
    T[:3, :3] = R_LOOK_X
    T[:3, 3] = t
    return T


def pt_in_frame(p, Twc, cam):
    """PtIsInFrame (FrameKDMap.cpp:215-231) in the operation order of oracle/step_oracle.c: pt_is_in_frame, every product and sum
    rounded on its own.  cam = (fx, fy, cx, cy, depth_max, width, height); Twc None: inside."""
    if Twc is None:
        return True
    T = np.asarray(Twc, np.float64).reshape(16)
    fx, fy, cx, cy, dmax, W, H = [np.float64(v) for v in cam]
    p = np.asarray(p, np.float64)
    with np.errstate(all="ignore"):
        dx, dy, dz = p[0] - T[3], p[1] - T[7], p[2] - T[11]
        x = T[0] * dx + T[4] * dy + T[8] * dz
        y = T[1] * dx + T[5] * dy + T[9] * dz
        z = T[2] * dx + T[6] * dy + T[10] * dz
        if z > dmax or z < 0:
            return False
        u = fx * x / z + cx
        v = fy * y / z + cy
        if u < 0 or u >= W or v < 0 or v >= H:
            return False
    return True


class CloudFrame:
    """One frame given by its cloud (float32 [n, >= 3]; NaN-x points are filtered as InitializeNew does)."""

    def __init__(self, cloud):
        cloud = np.asarray(cloud, np.float32).reshape(-1, 3)
        self.cloud = cloud[~np.isnan(cloud[:, 0])]
        self.size = len(self.cloud)

    def answer(self, q, k):
        """SearchForNearest(k) in the default tie order -> (sqdist [c], pts [c, 3])"""
        if self.size == 0:
            return np.zeros(0), np.zeros((0, 3), np.float32)
        idx, d2, _ = _oracle.kd_brute_np(self.cloud, q, k)
        return d2, self.cloud[idx]


def tree_cloud(kd):
    """The points a KdHandle (kdo) currently holds, by index: a search for size + 1 neighbours returns every point (size rule)."""
    n = kd.size()
    idx, _, pts = kd.search(np.zeros(3), n + 1)
    assert len(idx) == n and len(set(idx.tolist())) == n
    cloud = np.zeros((n, 3), np.float32)
    cloud[idx] = pts
    return cloud


class TreeFrame:
    """One frame given by a tree of the CPU oracle (a MapOracle frame, keyframes rebuilt from their outliers included)."""

    def __init__(self, kd):
        self.kd, self.size = kd, kd.size()
        self.cloud = tree_cloud(kd) if self.size else np.zeros((0, 3), np.float32)
        self.self_checks = 0

    def answer(self, q, k):
        if self.size == 0:
            return np.zeros(0), np.zeros((0, 3), np.float32)
        idx, d2 = self.kd.bruteforce(q, min(k + 1, self.size))
        if len(set(d2.tolist())) == len(d2):          # no equal distance among the k + 1 nearest: any exact search agrees
            si, sd, sp = self.kd.search(q, k)
            c = len(si)
            assert c == _oracle.kd_count_rule(self.size, k)
            assert np.array_equal(si, idx[:c]) and np.array_equal(sd, d2[:c]) and np.array_equal(sp, self.cloud[idx[:c]])
            self.self_checks += 1
        c = _oracle.kd_count_rule(self.size, k)
        return d2[:c], self.cloud[idx[:c]]


def query_nearest(frames, q, k, Twc=None, cam=None):
    """QueryNearest for one query.  frames: the scene's query vector, [CloudFrame | TreeFrame | None (absent)], frame 0 = current.
    -> dict(pts [k, 3] f32, sqdist [k], frame [k] i32, count, path 'fast' | 'merge' | 'nonfinite')"""
    pts = np.zeros((k, 3), np.float32); d2 = np.full(k, DBL_MAX); fr = np.full(k, -1, np.int32)
    q = np.asarray(q, np.float64)
    if not np.isfinite(q).all():                       # every slot empty; the count is unspecified
        return dict(pts=pts, sqdist=d2, frame=fr, count=None, path="nonfinite")
    f0 = frames[0] if frames else None
    if f0 is not None and f0.size >= k and pt_in_frame(q, Twc, cam):
        d, p = f0.answer(q, k)
        c = len(d)
        assert c == (k if f0.size > k else 0)
        d2[:c] = d; pts[:c] = p; fr[:c] = 0
        return dict(pts=pts, sqdist=d2, frame=fr, count=c, path="fast")
    cand = []                                          # (distance, frame, neighbour): the order of the merge
    for f, frm in enumerate(frames):
        if frm is None or frm.size <= k:               # k' = min(k, size): no result unless size > k'
            continue
        d, p = frm.answer(q, k)
        cand += [(d[j], f, j, p[j]) for j in range(len(d))]
    cand.sort(key=lambda c: (c[0], c[1], c[2]))
    cand = cand[:k]
    for i, (d, f, _j, p) in enumerate(cand):
        d2[i] = d; pts[i] = p; fr[i] = f
    return dict(pts=pts, sqdist=d2, frame=fr, count=len(cand), path="merge")


def nearest_distance(frames, q):
    """GetNearestDistance for one query: sqrt of the minimum 1-NN squared distance over the frames that hold more than one point."""
    q = np.asarray(q, np.float64)
    best = np.float64(DBL_MAX)
    if np.isfinite(q).all():
        for frm in frames:
            if frm is None or frm.size <= 1:
                continue
            d, _ = frm.answer(q, 1)
            if len(d) and d[0] < best:
                best = d[0]
    return np.sqrt(best)


def expected_batch(scene_frames, queries, k, Twc=None, cam=None):
    """scene_frames[s] = the frames of scene s; queries [S, Q, >= 3]; Twc [S, 4, 4] or None.
    -> dict(pts [S,Q,k,3], sqdist [S,Q,k], frame [S,Q,k], counts [S,Q] (-1: unspecified), path [S][Q])"""
    S, Q = queries.shape[:2]
    out = dict(pts=np.zeros((S, Q, k, 3), np.float32), sqdist=np.zeros((S, Q, k)), frame=np.zeros((S, Q, k), np.int32),
               counts=np.zeros((S, Q), np.int32), path=[[None] * Q for _ in range(S)])
    for s in range(S):
        for i in range(Q):
            r = query_nearest(scene_frames[s], queries[s, i, :3], k, None if Twc is None else Twc[s], cam)
            out["pts"][s, i], out["sqdist"][s, i], out["frame"][s, i] = r["pts"], r["sqdist"], r["frame"]
            out["counts"][s, i] = -1 if r["count"] is None else r["count"]
            out["path"][s][i] = r["path"]
    return out


def expected_distance(scene_frames, queries):
    S, Q = queries.shape[:2]
    return np.array([[nearest_distance(scene_frames[s], queries[s, i, :3]) for i in range(Q)] for s in range(S)])


def assert_query_equal(got, exp, what=""):
    """Bit-exact: points, squared distances, frame numbers everywhere; counts where the rules specify them (finite queries)."""
    g = {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in got.items() if v is not None}
    if "sqdist" in g:
        assert np.array_equal(g["sqdist"].view(np.int64), exp["sqdist"].view(np.int64)), what + ": squared distances"
    if "pts" in g:
        assert np.array_equal(g["pts"].view(np.int32), exp["pts"].view(np.int32)), what + ": points"
    if "frame" in g:
        assert np.array_equal(g["frame"], exp["frame"]), what + ": frame numbers"
    if "counts" in g:
        spec = exp["counts"] >= 0
        assert np.array_equal(g["counts"][spec], exp["counts"][spec]), what + ": counts"
