"""CPU: the inputs of tests/test_step_loop_gpu.py reach what tests/_step_loop_cases.py claims, shown on the oracle -- every solve
count 1 .. 8, the size classes, a scene that ends unsafe, every decision of every pass at least 1e-3 m from safety_distance
(so that the GPU test may ask for identical flags with no allowance); the placed obstacle really is the nearest point and really is
ON the threshold; snaps happen exactly where claimed; the lattice scenes tie and the plain ones do not."""
import numpy as np
import pytest

from tests import _frames_cases as fc
from tests import _oracle
from tests import _step_loop_cases as lc

KS = (1, 3, 8)


def _first_neighbours(cloud, K, rp):
    """sqrt of the first neighbour's squared distance for every reference point that gets neighbours (cloud of more than K points)"""
    if len(cloud) <= K:
        return np.zeros(0)
    kd = _oracle.kd_oracle(cloud)
    return np.sqrt(np.array([kd.search(p[:3], K)[1][0] for p in rp]))


@pytest.mark.parametrize("T,K", lc.SIZES)
def test_ladder_covers_every_pass_count_size_class_and_the_margin(T, K):
    scenes, kinds = lc.ladder(T, K)
    prm = lc.params(T, K)
    N, sd = prm.N, prm.safety_distance
    assert N in (10, 20) and len(scenes) == 21 and max(len(sc["cloud"]) for sc in scenes) <= 2001
    full = lc.ladder_oracle(T, K, lc.MAX_PASSES)
    for p in range(1, lc.MAX_PASSES + 1):
        assert sum(k == p for k in kinds) >= 2, p
    worst = np.inf
    for s, (sc, kind, r) in enumerate(zip(scenes, kinds, full)):
        dec = r["decisions"]
        mg = lc.decision_margin(dec, sd)
        worst = min(worst, mg)
        assert mg >= lc.MARGIN and not dec[:, 6].any(), (s, kind, mg)           # no scene left out, the exit pass included
        p = int(r["flags"][1])
        assert len(dec) == min(p + 1, lc.MAX_PASSES) and dec[-1, 5] == (p < lc.MAX_PASSES) and not dec[:-1, 5].any(), (s, kind)
        ob = np.stack([fc.split_P(P, N, K)[2] for P in r["ref_log"][:p]])
        if kind in range(1, 9):
            assert p == kind and r["flags"][0] == 1, (s, kind, r["flags"])
            assert (ob != fc.PAD).all()
        elif kind in ("two points", "K points"):      # cnt = 0: always needReplan; GetNearestDistance answers (more than one point)
            assert len(sc["cloud"]) == (2 if kind == "two points" else K)
            assert p == 8 and r["flags"][0] == 1 and dec[:, 2].all() and (dec[:, 0] < lc.NOTHING).all() and (ob == fc.PAD).all()
        elif kind in ("one point", "no point"):       # nearest = sqrt(DBL_MAX): safe, never exits
            assert len(sc["cloud"]) == (1 if kind == "one point" else 0)
            assert p == 8 and r["flags"][0] == 1 and (dec[:, 0] == np.sqrt(_oracle.DBL_MAX)).all() and (ob == fc.PAD).all()
            assert not dec[:, 4].any()
        else:
            assert kind == "unsafe" and len(sc["edge"]) <= 1
            assert p == 8 and r["flags"][0] == 0 and dec[-1, 3] == 0 and dec[-1, 0] <= sd - lc.MARGIN, (r["flags"], dec[:, 0])
            assert abs(dec[0, 0] - 0.05) < 1e-6 and not dec[:, 4].any()
        # the exit pass's margins once more, from what the step returned: the searches of that pass were made at this path
        if p < lc.MAX_PASSES:
            rp = r["ref_path"]
            kd = _oracle.kd_oracle(sc["cloud"])
            near = np.sqrt(kd.search(rp[0, :3], 1)[1][0])
            rows = _first_neighbours(sc["cloud"], K, rp)
            assert (near == dec[-1, 0] or dec[-1, 4]) and np.abs(rows - sd).min() == dec[-1, 1], (s, kind)
            assert min(abs(near - sd), np.abs(rows - sd).min()) >= lc.MARGIN
        # every pass gets its own initial state: a kernel that reads another row of d_state_quad shows in P
        sq = _oracle.scene_state_quads(sc, prm)
        assert len({tuple(row) for row in sq}) == lc.MAX_PASSES
        for i in range(p):
            assert np.array_equal(fc.split_P(r["ref_log"][i], N, K)[0], sq[i])
    print(f"T = {T}, K = {K}: worst decision margin {worst:.2e}")
    # mpc_max_iter = m: min(p, m) solves, and the step is the first m passes of the long one
    for m in range(1, lc.MAX_PASSES + 1):
        for s, (r, r8) in enumerate(zip(lc.ladder_oracle(T, K, m), full)):
            assert r["flags"][1] == min(r8["flags"][1], m), (m, s)
            assert np.array_equal(r["ref_log"][:r["flags"][1]], r8["ref_log"][:r["flags"][1]]), (m, s)
    # the flags differ between neighbours in the batch: a kernel that reads scene s + 1's done word or flags shows
    assert len({int(r["flags"][1]) for r in full}) == 8 and {int(r["flags"][0]) for r in full} == {0, 1}


@pytest.mark.parametrize("T,K", lc.SIZES)
def test_ladder_in_three_frames_keeps_the_margin(T, K):
    prm = lc.params(T, K)
    runs = lc.ladder_frames_oracle(T, K)
    scenes = lc.ladder_frames(T, K)
    for s, r in enumerate(runs):
        mg = lc.decision_margin(r["decisions"], prm.safety_distance)
        assert mg >= lc.MARGIN and not r["decisions"][:, 6].any(), (s, mg)
    passes = {int(r["flags"][1]) for r in runs}
    assert len(passes) >= 5 and {1, 8} <= passes, passes
    assert runs[-1]["flags"][0] == 0 and runs[-1]["flags"][1] == 8            # the unsafe scene stays unsafe in three frames
    # rows of both kinds: inside the current image (the current frame alone answers) and beyond depth_max (the frames merge)
    inside = [fc.in_frame(p[:3], scenes[0]["Twc"], lc.LADDER_CAM) for p in scenes[0]["ref_path"]]
    assert any(inside) and (T < 0.5 or not all(inside))


def _pass0(r, N, K):
    return fc.split_P(r["ref_log"][0], N, K)


@pytest.mark.parametrize("pair", sorted(lc.PAIRS))
@pytest.mark.parametrize("K", KS)
def test_threshold_scenes_sit_on_the_threshold(K, pair):
    off, sd = lc.PAIRS[pair]
    scenes = lc.threshold_scenes(K, pair)
    N = lc.params(lc.EDGE_T, K, 1).N
    assert np.array_equal(lc.P0.astype(np.float32).astype(np.float64), lc.P0)
    for s, sc in enumerate(scenes):
        d2 = fc._d2(sc["cloud"], lc.P0)
        assert np.argmin(d2) == 0 and np.sqrt(np.sort(d2)[1]) > 1.0 and len(sc["edge"]) >= 2 and len(sc["cloud"]) > K + 1
        assert d2[0] == (0.25 if pair == "exact" else 0.3125) and np.sqrt(d2[0]) == sd      # the squared distance is exact
        assert (np.sqrt(d2[0]) ** 2 == d2[0]) == (pair == "exact")                           # ... and its square root rounds or not
        assert np.array_equal(sc["ref_path"][0, :3], lc.P0)
    for side in lc.SIDES:
        v = lc.side_value(sd, side)
        assert (v == sd) == (side == "on") and abs(v - sd) <= 2.0 ** -53
        for s, (sc, r) in enumerate(zip(scenes, lc.pass0_oracle(scenes, K, v, ("threshold", pair)))):
            _, path, ob, _ = _pass0(r, N, K)
            assert r["decisions"][0, 0] == sd and r["decisions"][0, 4] == lc.SNAPS[side], (side, s)
            snapped = not np.array_equal(path[0, :3], lc.P0)
            assert snapped == lc.SNAPS[side] and r["flags"][0] == 1 and r["flags"][1] == 1, (side, s)
            if snapped:   # to the nearest edge point, and row 0 of the obstacle block is the re-query's answer there
                e = sc["edge"][np.argmin(fc._d2(sc["edge"], lc.P0))].astype(np.float64)
                assert np.array_equal(path[0, :3], e)
                assert np.array_equal(ob[0].astype(np.float32), _oracle.kd_oracle(sc["cloud"]).search(e, K)[2])
            else:
                assert np.array_equal(ob[0, 0].astype(np.float32), sc["cloud"][0])
            assert np.array_equal(path[1:], sc["ref_path"][1:])


@pytest.mark.parametrize("K", KS)
def test_size_scenes_reach_every_count_rule(K):
    scenes, sizes = lc.size_scenes(K)
    prm = lc.params(lc.EDGE_T, K, 1)
    N = prm.N
    assert {no for no, _ in sizes} == {0, 1, 2, K - 1, K, K + 1} and {ne for _, ne in sizes} == {0, 1, 2}
    seen = set()
    for (no, ne), sc, r in zip(sizes, scenes, lc.pass0_oracle(scenes, K, prm.safety_distance, "sizes")):
        assert len(sc["cloud"]) == no and len(sc["edge"]) == ne
        if no:
            assert abs(np.sqrt(fc._d2(sc["cloud"], lc.P0)[0]) - 0.125) < 1e-7
        _, path, ob, _ = _pass0(r, N, K)
        near = no > 1                      # `size > 1`: a cloud of one point answers no 1-NN query, the nearest distance is DBL_MAX
        snap = near and ne > 1             # ... and neither does an edge cloud of one point
        assert r["decisions"][0, 4] == snap and (not np.array_equal(path[0, :3], lc.P0)) == snap, (no, ne)
        assert r["flags"][0] == (0 if near and not snap else 1), (no, ne, r["flags"])
        assert (r["decisions"][0, 0] < lc.NOTHING) == near
        full = (ob != fc.PAD).all(axis=2).sum(axis=1)
        empty = (ob == fc.PAD).all(axis=2).sum(axis=1)
        assert np.array_equal(full, np.full(N, K if no > K else 0)) and np.array_equal(full + empty, np.full(N, K)), (no, ne)
        seen.add(("unsafe" if near and not snap else "snap" if snap else "far", "full" if no > K else "padded"))
    want = {("unsafe", "full"), ("snap", "full"), ("far", "padded")} | ({("unsafe", "padded"), ("snap", "padded")} if K > 1 else set())
    assert want <= seen, seen


@pytest.mark.parametrize("K", KS)
def test_requery_scenes_snap_and_tie_where_claimed(K):
    prm = lc.params(lc.EDGE_T, K, 1)
    N = prm.N
    for lattice in (False, True):
        scenes = lc.requery_scenes(K, lattice)
        runs = lc.pass0_oracle(scenes, K, prm.safety_distance, ("requery", lattice))
        tied_edge = tied_requery = tied_rows = 0
        for s, (sc, r) in enumerate(zip(scenes, runs)):
            _, path, ob, _ = _pass0(r, N, K)
            snapped = not np.array_equal(path[0, :3], sc["ref_path"][0, :3])
            assert snapped == (s < 6) == bool(r["decisions"][0, 4]), (lattice, s)
            assert (ob != fc.PAD).all() and np.array_equal(path[1:], sc["ref_path"][1:])
            e_tie = lc.has_tie(sc["edge"], sc["ref_path"][0, :3], 1)
            q_tie = snapped and lc.has_tie(sc["cloud"], path[0, :3], K)
            r_tie = sum(lc.has_tie(sc["cloud"], p[:3], K) for p in sc["ref_path"])
            if lattice:
                tied_edge += e_tie and snapped; tied_requery += q_tie; tied_rows += r_tie
            else:     # nothing ties: AMK_TIES_AUTO never needs a tree for these
                assert not e_tie and not q_tie and not r_tie, (s, e_tie, q_tie, r_tie)
            if snapped:
                d = fc._d2(sc["edge"], sc["ref_path"][0, :3])
                assert fc._d2(path[None, 0, :3].astype(np.float32), sc["ref_path"][0, :3])[0] == d.min()   # A nearest edge point
        if lattice:
            assert tied_edge == 6 and tied_requery == 6 and tied_rows >= 1, (tied_edge, tied_requery, tied_rows)


@pytest.mark.parametrize("T,K", lc.SIZES)
def test_exit_threshold_scenes_decide_the_second_solve_on_equality(T, K):
    for ox in lc.EXIT_OX:
        sc = lc.exit_threshold_scene(T, K, ox)
        O, E = sc["cloud"][0].astype(np.float64), sc["edge"][0].astype(np.float64)
        assert np.sqrt(fc._d2(sc["cloud"][:1], E)[0]) == lc.EXIT_SD and np.array_equal(E, O + lc.EXIT_OFFSET)
        runs = {side: lc.exit_oracle(T, K, ox, side) for side in lc.SIDES}
        on = runs["on"]["decisions"]
        # pass 0 and pass 1 both snap to E; on the threshold exactly one row sits ON it (the snapped point 0) and every other
        # decision of both passes is far from it
        assert len(on) == 2 and on[:, 4].all() and list(on[:, 6]) == [1, 1] and lc.decision_margin(on, lc.EXIT_SD) >= 0.02, on
        assert np.array_equal(fc.split_P(runs["on"]["ref_log"][1], lc.params(T, K).N, K)[1][0, :3], E)
        assert [int(runs[side]["flags"][1]) for side in lc.SIDES] == [2, 1, 2]          # `<=`: equality re-plans
        assert all(runs[side]["flags"][0] == 1 for side in lc.SIDES)
