"""CPU: the cases of tests/_kfmap_tie_cases.py are not vacuous -- on the oracle alone, the two tie orders give different answers on
them, and the scripts reach both query paths, both sweep outcomes, a pop by length, a snap to another edge point and a
DroneBehindPts decision that flips."""
import numpy as np
import pytest

from tests import _frames_cases as fc, _kfmap, _kfmap_tie_cases as tc


@pytest.mark.parametrize("max_frames,K", sorted({(m, k) for m, k, _ in tc.CONFIGS}))
def test_the_two_orders_differ_on_the_scripts(max_frames, K):
    r = tc.run(max_frames, K)
    knn = np.concatenate([tc.rows_that_differ(n[key], i[key]).reshape(-1) for n, i in zip(r.nano, r.index) for key in ("obs_cam", "obs_nocam")])
    edge = np.concatenate([tc.rows_that_differ(n["edge_cam"], i["edge_cam"]).reshape(-1) for n, i in zip(r.nano, r.index)])
    print(f"max_frame_count {max_frames}, K {K}: k-NN rows with another point set {knn.mean():.0%}, edge 1-NN rows {edge.mean():.0%}")
    assert knn.mean() >= 0.25, knn.mean()
    assert edge.mean() >= 0.10, edge.mean()
    # distances do not depend on the order
    for n, i in zip(r.nano, r.index):
        assert np.array_equal(n["dist"], i["dist"]) and np.array_equal(n["obs_cam"]["sqdist"], i["obs_cam"]["sqdist"])
    paths = np.array([n["obs_cam"]["path"] for n in r.nano])
    assert (paths == "fast").sum() >= 50 and (paths == "merge").sum() >= 50, ((paths == "fast").sum(), (paths == "merge").sum())
    multi = sum(len(set(f[f >= 0])) > 1 for n in r.nano for f in n["obs_cam"]["frame"].reshape(-1, K))
    assert multi >= 20, multi                                    # merges over several frames
    outl = [o for row in r.summaries for (_, _, o) in row if o > 0]
    assert any(o >= tc.TH_COUNT for o in outl) and any(o < tc.TH_COUNT for o in outl), outl   # both sweep outcomes
    if max_frames == 3:
        assert sum(map(sum, r.pops)) > 0, "no pop by length"
    # the empty frame left scene 1's map alone; the reset scene started over
    assert r.summaries[tc.EMPTY_PERIOD][tc.EMPTY_SCENE][:2] == r.summaries[tc.EMPTY_PERIOD - 1][tc.EMPTY_SCENE][:2]
    assert r.summaries[tc.RESET_BEFORE][tc.RESET_SCENE][0] == 1
    assert tc.n_points(tc.BIG_SCENE) > 4096                       # kExactBigNode
    # a snap that lands on another edge point in the other order
    snapped = other = 0
    for t in range(tc.PERIODS):
        for s in range(tc.S):
            p0 = tc.step_scene(s, t, K)["ref_path"][0, :3]
            packed = np.asarray(fc.split_P(r.steps[t][s]["ref_log"][0], tc.prm_of(K).N, K)[1]).reshape(-1, 10)[0, :3]   # point 0 as the solve got it
            if not np.array_equal(packed, p0):
                snapped += 1
                nano, index = r.p0_edge[t][0][s], r.p0_edge[t][1][s]
                assert np.array_equal(packed, nano.astype(np.float64)), (t, s)
                other += not np.array_equal(nano, index)
    print(f"steps that snapped {snapped}, to an edge point the default order would not have chosen {other}")
    assert 4 <= snapped < tc.PERIODS * tc.S and other >= 1, (snapped, other)
    # the step takes both paths: K-NN rows and edge 1-NN rows (row -1) merged over several frames, the merged lists differ between
    # the orders, and a snapped point 0 outside the camera frame is re-queried over several frames
    rows = [(i, path, nf, differ) for per in r.step_rows for sc in per for i, path, nf, differ in sc]
    count = lambda pred: sum(1 for row in rows if pred(*row))
    fast, merged = count(lambda i, p, nf, d: i >= 0 and p == "fast"), count(lambda i, p, nf, d: i >= 0 and p == "merge" and nf > 1)
    merged_differ = count(lambda i, p, nf, d: i >= 0 and p == "merge" and nf > 1 and d)
    edge_merged, edge_differ = count(lambda i, p, nf, d: i < 0 and p == "merge" and nf > 1), count(lambda i, p, nf, d: i < 0 and p == "merge" and nf > 1 and d)
    requery = sum(1 for per in r.step_rows for sc in per if sc[0][0] < 0 and sc[1][1] == "merge" and sc[1][2] > 1)
    print(f"step rows: fast {fast}, merged over several frames {merged} ({merged_differ} with another point set); edge 1-NN merged "
          f"{edge_merged} ({edge_differ} to another point); snapped points re-queried by the merge {requery}")
    assert fast >= 50 and merged >= 20 and merged_differ >= 10, (fast, merged, merged_differ)
    assert edge_merged >= 2 and edge_differ >= 1 and requery >= 2, (edge_merged, edge_differ, requery)


def test_the_drone_behind_pair_flips_in_exactly_one_cloud_order():
    out = {a: (tc.behind_outcome(a, _kfmap.MapOracle), tc.behind_outcome(a, tc.IndexOrderMap)) for a in (True, False)}
    print(out)
    assert all(v in (0, 2) for pair in out.values() for v in pair)
    assert sum(n != i for n, i in out.values()) == 1, out
    # in cloud-index order the earlier of A and B is the tenth neighbour: A first keeps the keyframe, B first pops it
    assert out[True][1] == 2 and out[False][1] == 0, out
