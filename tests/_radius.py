"""The specification of the radius searches (TEST INFRASTRUCTURE): a numpy brute force.

nanoflann's radiusSearch (AM/include/nanoflann_two.hpp:345-413,1611-1639) returns exactly the set
{i : ((qx - x)^2 + (qy - y)^2) + (qz - z)^2 < r2} in fp64 with contraction off, ascending (include/avoid_mpc_amd.h,
"Radius search"); this file restates that on the library's rules for a cloud: NaN-x points are dropped by the build and the
indices shift, a point is usable iff its squared distance is < DBL_MAX, equal distances order by cloud index -- over several frames
by frame first.  The count is never capped; the lists hold the nearest k and are padded with -1 / DBL_MAX / (0, 0, 0) / frame -1."""
import numpy as np

DBL_MAX = np.finfo(np.float64).max


def kept(cloud):
    """the points the build keeps: float32 [n, 3], x not NaN, order preserved"""
    cloud = np.asarray(cloud, np.float32).reshape(-1, np.asarray(cloud).shape[-1])[:, :3]
    return cloud[~np.isnan(cloud[:, 0])]


def sq_dists(cloud32, q):
    """the adaptor's left-to-right fp64 sum, float32 points widened first"""
    c = cloud32.astype(np.float64)
    with np.errstate(all="ignore"):
        return ((q[0] - c[:, 0]) ** 2 + (q[1] - c[:, 1]) ** 2) + (q[2] - c[:, 2]) ** 2


def radius_brute_frames(frames, q, r2, k):
    """frames: list of raw clouds float32 [n_f, >= 3]; q float64 [>= 3] -> dict(count, pts [k, 3] f32, sqdist [k], frame [k],
    indices [k]) of one query: count over all frames, the k nearest by (squared distance, frame, cloud index)"""
    ds, fs, ix, ps = [], [], [], []
    for f, cloud in enumerate(frames):
        c = kept(cloud)
        d = sq_dists(c, q)
        ok = np.flatnonzero((d < r2) & (d < DBL_MAX))   # strict; false for NaN, inf and overflow
        ds.append(d[ok]); fs.append(np.full(len(ok), f)); ix.append(ok); ps.append(c[ok])
    d = np.concatenate(ds) if ds else np.zeros(0)
    f = np.concatenate(fs) if fs else np.zeros(0, int)
    i = np.concatenate(ix) if ix else np.zeros(0, int)
    p = np.concatenate(ps) if ps else np.zeros((0, 3), np.float32)
    o = np.lexsort((i, f, d))[:k]
    out = dict(count=len(d), pts=np.zeros((k, 3), np.float32), sqdist=np.full(k, DBL_MAX), frame=np.full(k, -1, np.int32),
               indices=np.full(k, -1, np.int32))
    n = len(o)
    out["pts"][:n] = p[o]; out["sqdist"][:n] = d[o]; out["frame"][:n] = f[o]; out["indices"][:n] = i[o]
    return out


def radius_brute(cloud, q, r2, k):
    """one cloud: dict(count, indices, sqdist, pts) -- np.lexsort on (index, d2)"""
    out = radius_brute_frames([cloud], q, r2, k)
    del out["frame"]
    return out


def expected_batch(scene_frames, queries, r2, k):
    """scene_frames[s] = list of the frames (raw clouds) scene s holds; queries float64 [S, Q, >= 3]
    -> dict(counts [S, Q], pts [S, Q, k, 3], sqdist, frame, indices [S, Q, k])"""
    S, Q = queries.shape[:2]
    e = dict(counts=np.zeros((S, Q), np.int32), pts=np.zeros((S, Q, k, 3), np.float32), sqdist=np.zeros((S, Q, k)),
             frame=np.zeros((S, Q, k), np.int32), indices=np.zeros((S, Q, k), np.int32))
    for s in range(S):
        for i in range(Q):
            r = radius_brute_frames(scene_frames[s], queries[s, i], r2, k)
            e["counts"][s, i] = r["count"]
            for key in ("pts", "sqdist", "frame", "indices"):
                e[key][s, i] = r[key]
    return e


def assert_bitwise(got, want, keys, what=""):
    """bit for bit: counts, indices, distances, points, frames (no tolerance exists to choose)"""
    for key in keys:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, key, g.shape, w.shape, g.dtype, w.dtype)
        same = g.view(np.uint8).reshape(-1) == w.view(np.uint8).reshape(-1)
        if not same.all():
            bad = np.argwhere(g != w)
            raise AssertionError(f"{what}: {key} differs at {len(bad)} places, first {bad[:5].tolist()}: "
                                 f"got {g[tuple(bad[0])]!r}, want {w[tuple(bad[0])]!r}")


def grid_dims(cloud):
    """The index's grid over a cloud of finite points below 16384 (csrc/kd_grid.h grid_geometry over the full bounding box): cells
    per axis and tiles of 4096 points -- for tests that assert their inputs reach a mechanism (an item batch beyond 64)."""
    c = kept(cloud).astype(np.float64)
    ext = c.max(axis=0) - c.min(axis=0)
    efloor = max(ext.max() * 1e-6, 1e-30)
    e = np.maximum(ext, efloor)
    h = np.cbrt(e.prod() / min(max(len(c) / 64.0, 1.0), 1024.0))
    for _ in range(64):
        g = np.clip(np.ceil(e / h), 1, 1024).astype(int)
        if g.prod() <= 1024:
            break
        h *= 1.26
    return g, (len(c) + 4095) // 4096
