"""CPU: the inputs of tests/test_step_frames_edges_gpu.py reach what they are meant to reach.  The classifier of tests/
_frames_cases.py -- plain numpy, it never calls the oracle's step -- names the branch of FrameKDMap::QueryNearest every reference
point takes and the branch of PlanWapionts; here it is held against the oracle's packed parameter vector P (pass 0: a pure
function of the queries and the merge) on every scene, and every branch is required to occur, also at the LAST reference point,
whose neighbours no output of the step depends on.  Without these conditions the GPU comparisons could pass without merging."""
import collections

import numpy as np
import pytest

from tests import _frames_cases as fc
from avoid_mpc_amd import synth

K8 = 8
QUERY_TAGS = ["fast_K", "fast_0", "merge_0_cur_small", "merge_1_cur_small", "merge_2_cur_small", "merge_0_out_of_frame",
              "merge_1_out_of_frame", "merge_2_out_of_frame", "merge_3_out_of_frame"]   # 3 frames: every (frames that answer, cause)


def _check(scenes, runs, prm, cam, tags=None):
    """classifier == oracle on every scene: neighbour counts per reference point, flags[0], the snapped reference point 0"""
    N, K = prm.N, prm.K
    for s, (sc, r) in enumerate(zip(scenes, runs)):
        c = fc.classify(sc["obs"], sc["edge"], sc["Twc"], cam, sc["ref_path"], K, prm.safety_distance)
        _, path, ob, _ = fc.split_P(r["ref_log"][0], N, K)
        full = (ob != fc.PAD).all(axis=2).sum(axis=1); empty = (ob == fc.PAD).all(axis=2).sum(axis=1)
        assert np.array_equal(full + empty, np.full(N, K)), s                 # a row is a point or the padding, never a mix
        assert np.array_equal(full, c["counts"]), (s, full, c["counts"], c["tags"])
        assert r["flags"][0] == c["flag0"] and r["flags"][1] == 1, (s, r["flags"], c["plan"])
        assert np.array_equal(path[0, :3], c["p0"]), (s, c["plan"])
        assert np.array_equal(path[1:], sc["ref_path"][1:])
        if tags is not None:
            tags["plan:" + c["plan"]] += 1
            if c["cause"]:
                tags["cause:" + c["cause"]] += 1
            for i, t in enumerate(c["tags"]):
                tags["q:" + t] += 1
                if i == N - 1:
                    tags["last:" + t] += 1


def test_size_matrix_reaches_every_branch():
    prm = synth.MpcParams(T=0.66, K=K8, max_iter=1)
    scenes = fc.size_matrix(K8)
    assert 70 <= len(scenes) <= 74
    tags = collections.Counter()
    _check(scenes, fc.oracle_frames(scenes, prm, fc.CAM, "size"), prm, fc.CAM, tags)
    print(dict(tags))
    for t in fc.PLAN_TAGS:
        assert tags["plan:" + t] >= 1, t
    for t in fc.CAUSE_TAGS:
        assert tags["cause:" + t] >= 1, t
    for t in QUERY_TAGS:
        assert tags["q:" + t] >= 1, t
        assert tags["last:" + t] >= 1, t     # ... and at the row no output can see
    # every scene has its own camera pose and the poses take different decisions: a kernel reading scene 0's pose is caught
    poses = {tuple(sc["Twc"].reshape(-1)) for sc in scenes}
    assert len(poses) == 4
    # the snap is triggered by an obstacle that only a keyframe holds
    snapped_by_keyframe = 0
    for sc in scenes:
        c = fc.classify(sc["obs"], sc["edge"], sc["Twc"], fc.CAM, sc["ref_path"], K8, prm.safety_distance)
        p0 = sc["ref_path"][0, :3]
        near0 = len(sc["obs"][0]) > 1 and np.sqrt(fc._d2(sc["obs"][0], p0).min()) <= prm.safety_distance
        snapped_by_keyframe += c["plan"] != "far" and not near0
    assert snapped_by_keyframe >= 10, snapped_by_keyframe


@pytest.mark.parametrize("F,K", fc.WIDTH_CASES)
def test_partition_rows_merge_many_frames(F, K):
    prm = synth.MpcParams(T=0.66, K=K, max_iter=1)
    scenes = fc.partition(F, K)
    runs = fc.oracle_frames(scenes, prm, fc.CAM, ("partition", F))
    tags = collections.Counter()
    _check(scenes, runs, prm, fc.CAM, tags)
    assert tags["q:fast_K"] >= 1 and tags["q:merge_%d_out_of_frame" % F] >= 4 * 4 and tags["last:merge_%d_out_of_frame" % F] == 4
    # merged rows interleave the frames: the sources of a merged row, by brute force
    N, nsrc = prm.N, []
    for sc, r in zip(scenes, runs):
        ob = fc.split_P(r["ref_log"][0], N, K)[2].astype(np.float32)
        for i in range(N):
            if not fc.in_frame(r["ref_log"][0][10 + 10 * i:13 + 10 * i], sc["Twc"], fc.CAM):
                nsrc.append(len({f for j in range(K) for f in range(F) if (sc["obs"][f] == ob[i, j]).all(axis=1).any()}))
    assert max(nsrc) >= min(F, K, 2) and np.mean(nsrc) >= min(F, K) * 0.5, (max(nsrc), np.mean(nsrc))


def test_frustum_rows_decide_what_enters_P():
    prm = synth.MpcParams(T=1.0, K=K8, max_iter=1)
    scenes, names = fc.frustum()
    N = prm.N
    assert N == 30
    assert {n for n, _ in fc.frustum_rows()} == set(fc.FRUSTUM_EXPECT)
    for name, p in fc.frustum_rows():   # the edges sit where the arithmetic says
        assert fc.in_frame(p, fc.TWC_AXIS, fc.CAM) == fc.FRUSTUM_EXPECT[name], name
    runs = fc.oracle_frames(scenes, prm, fc.CAM, "frustum")
    _check(scenes, runs, prm, fc.CAM)
    at0, at_last, checked = set(), set(), 0
    for s, (sc, r) in enumerate(zip(scenes, runs)):
        _, path, ob, _ = fc.split_P(r["ref_log"][0], N, K8)
        at0.add(names[s][0]); at_last.add(names[s][N - 1])
        for i in range(N):
            if names[s][i] is None or not np.array_equal(path[i, :3], sc["ref_path"][i, :3]):
                continue   # (a row of the straight path, or reference point 0 after a snap)
            p = path[i, :3]
            fast, merged = fc.fast_and_merged(sc["obs"], p, K8)
            assert len(fast) == K8 and len(merged) == K8 and not np.array_equal(fast, merged), (s, i, names[s][i])
            d = np.sort(fc._d2(ob[i].astype(np.float32), p))
            assert np.array_equal(d, fast if fc.FRUSTUM_EXPECT[names[s][i]] else merged), (s, i, names[s][i])
            checked += 1
    assert checked >= len(scenes) * (len(fc.FRUSTUM_EXPECT) - 1)
    assert len(at0 - {None}) >= 3 and len(at_last - {None}) >= 3   # edge rows also at reference point 0 and at the last one


@pytest.mark.parametrize("F", [2, 16])
def test_lattice_frames_tie_across_frames(F):
    prm = synth.MpcParams(T=0.66, K=K8, max_iter=1)
    scenes = fc.ties(F)
    _check(scenes, fc.oracle_frames(scenes, prm, fc.TIES_CAM, ("ties", F)), prm, fc.TIES_CAM)
    assert fc.count_merged_ties(scenes, prm, fc.TIES_CAM) >= prm.N


@pytest.mark.parametrize("max_frames,deep", [(30, 24), (100, 56)])
def test_deep_map_script_reaches_small_keyframes_and_late_chunks(max_frames, deep):
    run = fc.deep_map_oracle(max_frames)
    sizes = {n for row in run.summaries for (_, sz, _) in row for n in sz[1:]}
    assert {1, 2, K8 - 1, K8, K8 + 1} <= sizes, sorted(sizes)[:12]
    assert max(len(sz) for row in run.summaries for (_, sz, _) in row) > deep
    for t in fc.DEEP_STEPS:   # the steps themselves see such frames, and rows that merge
        for s, r in enumerate(run.steps[t]):
            path = fc.split_P(r["ref_log"][0], run.prm.N, K8)[1]
            inf = [fc.in_frame(p[:3], fc.DEEP_TWC, fc.DEEP_CAM) for p in path]
            assert not inf[-1] and 5 <= sum(inf) <= run.prm.N - 5, (t, s, sum(inf))
    assert len(run.summaries[-1][0][1]) > deep


def test_target_rows_tell_a_contracted_product_from_the_ieee_one():
    prm = synth.MpcParams(T=0.66, K=K8, speed=fc.TARGET_SPEED, max_iter=1)
    scenes = fc.target_rows(K8)
    runs = fc.oracle_frames(scenes, prm, fc.CAM, "target")
    _check(scenes, runs, prm, fc.CAM)
    differ = 0
    for sc, r in zip(scenes, runs):
        m = sc["ref_path"][-1, 0] - sc["pos"][0]
        ieee, fused = fc.target_ieee_and_contracted(prm.speed, prm.T, m)
        assert 0 < m < prm.speed * prm.T and ieee > 0
        tg = fc.split_P(r["ref_log"][0], prm.N, K8)[3]
        assert tg[0] == sc["ref_path"][-1, 0] + ieee and tg[1] == 0.0     # the oracle: IEEE operations as written
        differ += (sc["ref_path"][-1, 0] + fused) != tg[0]
    assert differ >= 3, differ      # a fused multiply-add in the kernel would show in P
