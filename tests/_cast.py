"""The specification of the segment casts (TEST INFRASTRUCTURE): a numpy brute force.

include/avoid_mpc_amd.h, "Segment cast", restated: per leg a -> b in fp64, contraction off, sums left to right
    ab = b - a;  L2 = (ab0*ab0 + ab1*ab1) + ab2*ab2;  inv = 1.0 / L2
and per stored point p (float32, widened first), r2 = min(radius_sq, DBL_MAX)
    ap = p - a;  q = (ap0*ap0 + ap1*ap1) + ap2*ap2                 usable iff q < DBL_MAX
    q < r2:  contact at t = 0
    else:    dot = (ap0*ab0 + ap1*ab1) + ap2*ab2;  c = q - r2;  disc = dot*dot - L2*c
             contact iff dot > 0 and disc > 0 and t < 1, with t = (dot - sqrt(disc)) * inv
on the library's rules for a cloud (tests/_radius.py: NaN-x points are dropped by the build and the indices shift).  Every test is
strict; a leg with a non-finite endpoint coordinate or a non-finite L2 has no contact (tests/_segment.py: leg_ok).  The answer of a
leg is the first of np.lexsort((index, frame, t)); without a contact hit 0, t 1.0, (0, 0, 0), index -1, frame -1."""
import numpy as np

from tests._radius import DBL_MAX, assert_bitwise, grid_dims, kept  # noqa: F401  (re-exported for the tests)
from tests._segment import leg_ok


def contacts(cloud32, a, b, radius_sq):
    """-> (hit bool [n], t [n]) of every point of the float32 cloud against the leg a -> b"""
    a, b = np.asarray(a, np.float64)[:3], np.asarray(b, np.float64)[:3]
    p = cloud32.astype(np.float64).reshape(-1, 3)
    r2 = np.float64(min(radius_sq, DBL_MAX))
    with np.errstate(all="ignore"):
        ab = b - a
        L2 = (ab[0] * ab[0] + ab[1] * ab[1]) + ab[2] * ab[2]
        inv = np.float64(1.0) / L2
        ap = p - a
        q = (ap[:, 0] * ap[:, 0] + ap[:, 1] * ap[:, 1]) + ap[:, 2] * ap[:, 2]
        dot = (ap[:, 0] * ab[0] + ap[:, 1] * ab[1]) + ap[:, 2] * ab[2]
        c = q - r2
        disc = dot * dot - L2 * c
        tt = (dot - np.sqrt(disc)) * inv
        inside = q < r2
        hit = (q < DBL_MAX) & (inside | ((dot > 0) & (disc > 0) & (tt < 1)))
        t = np.where(inside, 0.0, tt)
    return hit, t


def cast_brute_frames(frames, a, b, radius_sq):
    """frames: list of raw clouds float32 [n_f, >= 3] -> dict(hit, t, pts [3] f32, frame, indices) of one leg: the first contact
    over all frames by (t, frame, cloud index)"""
    ts, fs, ix, ps = [np.zeros(0)], [np.zeros(0, int)], [np.zeros(0, int)], [np.zeros((0, 3), np.float32)]
    if leg_ok(a, b):
        for f, cloud in enumerate(frames):
            c = kept(cloud)
            hit, t = contacts(c, a, b, radius_sq)
            ok = np.flatnonzero(hit)
            ts.append(t[ok]); fs.append(np.full(len(ok), f)); ix.append(ok); ps.append(c[ok])
    t, f, i, p = (np.concatenate(x) for x in (ts, fs, ix, ps))
    o = np.lexsort((i, f, t))[:1]
    if len(o) == 0:
        return dict(hit=np.int32(0), t=np.float64(1.0), pts=np.zeros(3, np.float32), frame=np.int32(-1), indices=np.int32(-1))
    return dict(hit=np.int32(1), t=np.float64(t[o[0]]), pts=p[o[0]].astype(np.float32), frame=np.int32(f[o[0]]),
                indices=np.int32(i[o[0]]))


def cast_brute(cloud, a, b, radius_sq):
    """one cloud: dict(hit, t, pts, indices)"""
    out = cast_brute_frames([cloud], a, b, radius_sq)
    del out["frame"]
    return out


def expected_batch(scene_frames, path, radius_sq):
    """scene_frames[s] = list of the frames (raw clouds) scene s holds; path float64 [S, P, >= 3]
    -> dict(hit, t, frame, indices [S, P-1], pts [S, P-1, 3])"""
    S, L = path.shape[0], path.shape[1] - 1
    e = dict(hit=np.zeros((S, L), np.int32), t=np.zeros((S, L)), pts=np.zeros((S, L, 3), np.float32), frame=np.zeros((S, L), np.int32),
             indices=np.zeros((S, L), np.int32))
    for s in range(S):
        for j in range(L):
            r = cast_brute_frames(scene_frames[s], path[s, j], path[s, j + 1], radius_sq)
            for key in e:
                e[key][s, j] = r[key]
    return e
