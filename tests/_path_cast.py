"""The specification of the path casts (TEST INFRASTRUCTURE): a numpy restatement on top of tests/_cast.py.

include/avoid_mpc_amd.h, "Path cast", restated: every leg is answered as the segment cast answers it (tests/_cast.py:
expected_batch); the stop leg of a scene is the first leg j, in leg order, that (a) has a contact, or (b) is unjudgeable -- a
non-finite endpoint coordinate or a non-finite L2 (tests/_segment.py: leg_ok).  Per scene
    stop  0 free to the end, 1 contact, 2 unjudgeable       leg  the stop leg, -1 when free
    t     the contact's t; 0.0 when stop is 2, 1.0 when free
    free  ((len_0 + len_1) + ... + len_{leg-1}) + t * len_leg, len_j = sqrt(L2_j) in fp64, summed left to right; the last term is
          left out when stop is 2; a free path gives its whole length
    pts / indices / frame   the contact's; (0, 0, 0) / -1 / -1 unless stop is 1"""
import numpy as np

from tests import _cast as K
from tests._cast import assert_bitwise  # noqa: F401  (re-exported for the tests)
from tests._segment import leg_ok

KEYS = ("stop", "leg", "t", "free", "pts", "indices")
KEYS_FRAMES = ("stop", "leg", "t", "free", "pts", "frame")


def leg_lengths(path):
    """path float64 [S, P, >= 3] -> sqrt(L2) [S, P - 1], L2 as seg_leg forms it"""
    with np.errstate(all="ignore"):
        ab = path[:, 1:, :3] - path[:, :-1, :3]
        L2 = (ab[..., 0] * ab[..., 0] + ab[..., 1] * ab[..., 1]) + ab[..., 2] * ab[..., 2]
        return np.sqrt(L2)


def reduce_legs(per_leg, path):
    """per_leg: the segment cast's outputs for `path` (dict hit, t, pts and indices and / or frame, a row per leg) -> the path cast's
    answer, a row per scene.  This is the identity the header states: the library's answer equals this reduction applied to
    amk_kd_segment_cast's own outputs, bit for bit; free is rebuilt from the path."""
    S, L = path.shape[0], path.shape[1] - 1
    length = leg_lengths(path)
    out = dict(stop=np.zeros(S, np.int32), leg=np.full(S, -1, np.int32), t=np.ones(S), free=np.zeros(S), pts=np.zeros((S, 3), np.float32))
    ids = [k for k in ("indices", "frame") if k in per_leg]
    for k in ids:
        out[k] = np.full(S, -1, np.int32)
    for s in range(S):
        free = np.float64(0.0)
        for j in range(L):
            if not leg_ok(path[s, j], path[s, j + 1]):
                out["stop"][s], out["leg"][s], out["t"][s] = 2, j, 0.0
                break
            if per_leg["hit"][s, j]:
                t = np.float64(per_leg["t"][s, j])
                out["stop"][s], out["leg"][s], out["t"][s] = 1, j, t
                out["pts"][s] = per_leg["pts"][s, j]
                for k in ids:
                    out[k][s] = per_leg[k][s, j]
                free = free + t * length[s, j]
                break
            free = free + length[s, j]
        out["free"][s] = free
    return out


def expected_batch(scene_frames, path, radius_sq):
    """scene_frames[s] = list of the frames (raw clouds) scene s holds; path float64 [S, P, >= 3]
    -> dict(stop, leg, t, free, indices, frame [S], pts [S, 3])"""
    return reduce_legs(K.expected_batch(scene_frames, path, radius_sq), path)
