"""The specification of the segment-nearest queries (TEST INFRASTRUCTURE): the numpy brute force of tests/_segment.py with no radius.

include/avoid_mpc_amd.h, "Segment nearest", identity 1: per leg the lists are those of the segment search at radius_sq = +inf and
max_results = k -- the k usable points (d2 < DBL_MAX) with the smallest d2 by np.lexsort((index, frame, d2)), padded with
-1 / DBL_MAX / 0.0 / (0, 0, 0) / frame -1 -- and the count is min(k, that search's count)."""
import numpy as np

from tests import _segment as G
from tests._segment import DBL_MAX, assert_bitwise, grid_dims, kept, seg_dists  # noqa: F401  (re-exported for the tests)


def expected_batch(scene_frames, path, k):
    """scene_frames[s] = list of the frames (raw clouds) scene s holds; path float64 [S, P, >= 3]
    -> dict(counts [S, P-1], pts [S, P-1, k, 3], sqdist, t, frame, indices [S, P-1, k])"""
    e = G.expected_batch(scene_frames, path, float("inf"), k)
    e["counts"] = np.minimum(e["counts"], k).astype(np.int32)
    return e


def nearest_brute(cloud, a, b, k):
    """one cloud, one leg: dict(count, indices, sqdist, t, pts)"""
    out = G.segment_brute(cloud, a, b, float("inf"), k)
    out["count"] = min(out["count"], k)
    return out


def nearest_brute_frames(frames, a, b, k):
    out = G.segment_brute_frames(frames, a, b, float("inf"), k)
    out["count"] = min(out["count"], k)
    return out
