"""The specification of the segment searches (TEST INFRASTRUCTURE): a numpy brute force.

include/avoid_mpc_amd.h, "Segment search", restated: per leg a -> b in fp64, contraction off, sums left to right
    ab = b - a;  L2 = (ab0*ab0 + ab1*ab1) + ab2*ab2;  inv = 1.0 / L2
and per stored point p (float32, widened first)
    ap = p - a;  dot = (ap0*ab0 + ap1*ab1) + ap2*ab2;  t = dot > 0 ? dot*inv : 0;  t = t < 1 ? t : 1
    c = t < 1 ? a + t*ab : b;  e = c - p;  d2 = (e0*e0 + e1*e1) + e2*e2
on the library's rules for a cloud (tests/_radius.py: NaN-x points are dropped by the build and the indices shift; a point is
usable iff d2 < DBL_MAX).  A result has d2 < r2, strict; a leg with a non-finite endpoint coordinate or a non-finite L2 has none.
The count is never capped; the lists hold the nearest k by np.lexsort((index, frame, d2)) and are padded with
-1 / DBL_MAX / 0.0 / (0, 0, 0) / frame -1."""
import numpy as np

from tests._radius import DBL_MAX, assert_bitwise, grid_dims, kept  # noqa: F401  (re-exported for the tests)


def leg_ok(a, b):
    a, b = np.asarray(a, np.float64)[:3], np.asarray(b, np.float64)[:3]
    with np.errstate(all="ignore"):
        ab = b - a
        L2 = (ab[0] * ab[0] + ab[1] * ab[1]) + ab[2] * ab[2]
    return bool(np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(L2))


def seg_dists(cloud32, a, b):
    """-> (d2 [n], t [n]) of every point of the float32 cloud to the leg a -> b"""
    a, b = np.asarray(a, np.float64)[:3], np.asarray(b, np.float64)[:3]
    p = cloud32.astype(np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        ab = b - a
        L2 = (ab[0] * ab[0] + ab[1] * ab[1]) + ab[2] * ab[2]
        inv = np.float64(1.0) / L2
        ap = p - a
        dot = (ap[:, 0] * ab[0] + ap[:, 1] * ab[1]) + ap[:, 2] * ab[2]
        t = np.where(dot > 0, dot * inv, 0.0)
        t = np.where(t < 1, t, 1.0)
        c = np.where((t < 1)[:, None], a + t[:, None] * ab, b)
        e = c - p
        d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    return d2, t


def segment_brute_frames(frames, a, b, r2, k):
    """frames: list of raw clouds float32 [n_f, >= 3] -> dict(count, pts [k, 3] f32, sqdist [k], t [k], frame [k], indices [k]) of
    one leg: count over all frames, the k nearest by (d2, frame, cloud index)"""
    ds, ts, fs, ix, ps = [np.zeros(0)], [np.zeros(0)], [np.zeros(0, int)], [np.zeros(0, int)], [np.zeros((0, 3), np.float32)]
    if leg_ok(a, b):
        for f, cloud in enumerate(frames):
            c = kept(cloud)
            d, t = seg_dists(c, a, b)
            ok = np.flatnonzero((d < r2) & (d < DBL_MAX))   # strict; false for NaN, inf and overflow
            ds.append(d[ok]); ts.append(t[ok]); fs.append(np.full(len(ok), f)); ix.append(ok); ps.append(c[ok])
    d, t, f, i, p = (np.concatenate(x) for x in (ds, ts, fs, ix, ps))
    o = np.lexsort((i, f, d))[:k]
    out = dict(count=len(d), pts=np.zeros((k, 3), np.float32), sqdist=np.full(k, DBL_MAX), t=np.zeros(k), frame=np.full(k, -1, np.int32),
               indices=np.full(k, -1, np.int32))
    n = len(o)
    out["pts"][:n] = p[o]; out["sqdist"][:n] = d[o]; out["t"][:n] = t[o]; out["frame"][:n] = f[o]; out["indices"][:n] = i[o]
    return out


def segment_brute(cloud, a, b, r2, k):
    """one cloud: dict(count, indices, sqdist, t, pts)"""
    out = segment_brute_frames([cloud], a, b, r2, k)
    del out["frame"]
    return out


def expected_batch(scene_frames, path, r2, k):
    """scene_frames[s] = list of the frames (raw clouds) scene s holds; path float64 [S, P, >= 3]
    -> dict(counts [S, P-1], pts [S, P-1, k, 3], sqdist, t, frame, indices [S, P-1, k])"""
    S, L = path.shape[0], path.shape[1] - 1
    e = dict(counts=np.zeros((S, L), np.int32), pts=np.zeros((S, L, k, 3), np.float32), sqdist=np.zeros((S, L, k)), t=np.zeros((S, L, k)),
             frame=np.zeros((S, L, k), np.int32), indices=np.zeros((S, L, k), np.int32))
    for s in range(S):
        for j in range(L):
            r = segment_brute_frames(scene_frames[s], path[s, j], path[s, j + 1], r2, k)
            e["counts"][s, j] = r["count"]
            for key in ("pts", "sqdist", "t", "frame", "indices"):
                e[key][s, j] = r[key]
    return e
