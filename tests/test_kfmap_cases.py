"""CPU: the scripts of tests/_kfmap_cases.py reach every branch of the keyframe map's bookkeeping they aim at -- REQUIRED here by
assertion, on the oracle (tests/_kfmap.py: MapOracle), so that tests/test_kfmap_deque_gpu.py cannot pass without the device
having run them -- and a numpy restatement of the pop loop, the gate and the sweep that never calls MapOracle.update agrees with
the oracle on every period."""
import numpy as np
import pytest

from tests import _kfmap
from tests import _kfmap_cases as kc


def _nk(run, s):
    return [row[s][0] for row in run.summaries]


def test_clouds_are_identified_by_their_size_and_every_sweep_keeps_all_points():
    for s in range(kc.S):
        script = kc.ceiling_script(100 + s)
        assert [len(c) for c, _, _ in script] == [12 + t for t in range(kc.PERIODS)] and max(len(c) for c, _, _ in script) <= kc.CAP
        for t in range(kc.PERIODS):   # 8 to 10 m ahead of the drone
            x = script[t][0][:, 0].astype(np.float64) - kc.drone_x(t)
            assert x.min() >= 8.0 - 1e-5 and x.max() <= 10.0 + 1e-5
    for mf in kc.MAX_FRAMES:
        run = kc.ceiling_run(mf)
        for t, row in enumerate(run.summaries):
            for s, (nk, sizes, outl) in enumerate(row):
                assert len(set(sizes)) == len(sizes), (mf, t, s)                 # the sizes ARE the deque
                if outl >= 0:   # a sweep ran: the keyframe it swept is the LAST query frame now, rebuilt from ALL its points
                    assert outl == sizes[-1], (mf, t, s, outl, sizes)
                assert sizes[1:] == sorted(sizes[1:]), (mf, t, s)                # oldest first


def test_ceiling_script_reaches_every_deque_branch():
    r100, r64, r63 = kc.ceiling_run(100), kc.ceiling_run(64), kc.ceiling_run(63)
    for s in (0, 3):
        assert max(_nk(r100, s)) == 101 and max(_nk(r64, s)) == 65 and max(_nk(r63, s)) == 64   # the ceiling; both sides of the register boundary
        nk = _nk(r100, s)
        # a length pop with more than 64 entries: the deque stays at 101 over >= 15 periods, each of which popped one and inserted one
        at_ceiling = [t for t in range(1, kc.PERIODS) if nk[t] == 101 and nk[t - 1] == 101]
        assert len(at_ceiling) >= 15 and all(r100.pops[t][s] == 1 for t in at_ceiling)
        # one pass with >= 2 pops that crosses entry 64
        t1 = kc.JUMPS[0][0] + 1
        assert nk[t1 - 1] == 101 and r100.pops[t1][s] >= 2 and nk[t1] < 64 < nk[t1 - 1], (nk[t1 - 1], nk[t1])
        n64 = _nk(r64, s)
        assert n64[t1 - 1] == 65 and r64.pops[t1][s] >= 2 and n64[t1] < 64
        # a pop to empty (the current frame is NOT inserted), then the first-keyframe pass, then ordinary insertions
        t2 = kc.JUMPS[1][0] + 1
        for run in (r100, r64, r63):
            n = _nk(run, s)
            assert n[t2 - 1] > 1 and n[t2:t2 + 4] == [0, 1, 2, 3] and run.pops[t2][s] == n[t2 - 1]
            assert run.summaries[t2][s][1] == [12 + t2] and run.summaries[t2 + 1][s][1] == [12 + t2 + 1]
    # single pops by pose between the jumps (DroneBehindPts alone, the list is short of max_frame_count)
    assert any(r100.pops[t][s] == 1 and _nk(r100, s)[t - 1] <= 100 for s in (0, 3) for t in range(kc.JUMPS[0][0] + 2, kc.JUMPS[1][0] + 1))
    assert _nk(kc.ceiling_run(1), 0)[124:129] == [2, 2, 0, 1, 2] and _nk(kc.ceiling_run(2), 0)[124:130] == [3, 3, 0, 1, 2, 3]
    # the two deviating scenes: an empty frame, a skipped scene (mbNeedProcessPtCloud stays false)
    for run in (r100, r64):
        assert sum(1 for t in range(kc.PERIODS) if len(kc.scene_frame(kc.EMPTY_SCENE, t)[0]) == 0) >= 12
        for t in range(1, kc.PERIODS):
            if len(kc.scene_frame(kc.EMPTY_SCENE, t)[0]) == 0:
                assert not run.need[t][kc.EMPTY_SCENE] and run.summaries[t][kc.EMPTY_SCENE][:2] == run.summaries[t - 1][kc.EMPTY_SCENE][:2]
            if kc.scene_frame(kc.SKIP_SCENE, t) is None:
                assert not run.need[t][kc.SKIP_SCENE] and run.summaries[t][kc.SKIP_SCENE][:2] == run.summaries[t - 1][kc.SKIP_SCENE][:2]
        assert sum(1 for t in range(kc.PERIODS) if not run.need[t][kc.SKIP_SCENE]) == kc.PERIODS // 2
    # the steps are taken where the issue wants them
    assert kc.step_periods(100) == (110, 116, 126, 128)
    assert [r100.summaries[t][0][0] for t in kc.step_periods(100)][:3:2] == [101, 0] and len(r100.summaries[110][0][1]) == 101
    assert len(r100.summaries[126][0][1]) == 1


def test_gate_cases_have_the_stated_outcomes():
    cases, rows = kc.gate_cases(), kc.gate_run()
    assert len(cases) == 10 and sum(np.array_equal(c["Twb"][:3, :3], kc.YAW90) for c in cases) == 7
    Tinv = _kfmap.rigid_inverse(kc.GATE_TBC)
    assert len({abs(v) for v in kc.GATE_TBC[:3, 3]}) == 3 and (kc.GATE_TBC[:3, 3] != 0).all()
    for i, c in enumerate(cases):
        assert rows[0][i][0] == 1, c["name"]
        assert rows[1][i][0] == c["expect"], (c["name"], rows[1][i])
        A, B = c["frames"][0][0], c["frames"][1][0]
        assert rows[1][i][1] == ([len(B), len(A)] if c["expect"] == 2 else [len(B)]), c["name"]   # popped to empty: B is NOT inserted
        # body-frame x of the special point as the pass of period 1 sees it, in float64
        twb, bx = _kfmap.drone_pose(c["frames"][1][2], Tinv)
        assert np.array_equal(twb, c["Twb"][:3, 3]) if c["name"].startswith("x_") else np.abs(twb - c["Twb"][:3, 3]).max() < 1e-12
        px = float(bx @ (c["special"].astype(np.float64) - twb))
        if c["name"] == "x_eq_depth_min":
            assert px == 0.25
        elif c["name"] == "x_one_ulp_above":
            assert px == kc.ULP and kc.ULP - 0.25 == 2.0 ** -25
        elif c["name"].startswith("general"):
            R = c["Twb"][:3, :3]
            assert abs(px - kc.DEPTH_MIN) >= kc.GATE_MARGIN, (c["name"], px)   # rounding cannot decide the outcome
            assert np.abs(R).min() > 0.2 and np.abs(R - R.T).max() > 0.5   # nothing like a rotation about one axis
            # with the body x axis read from the wrong side of the rotation (row for column) the special point falls on the other
            # side of the gate in at least one case (asserted below over the three)
    flips = 0
    for c in cases:
        if c["name"].startswith("general"):
            R, t = c["Twb"][:3, :3], c["Twb"][:3, 3]
            d = c["special"].astype(np.float64) - t
            flips += int((float(R[0, :] @ d) <= kc.DEPTH_MIN) != (float(R[:, 0] @ d) <= kc.DEPTH_MIN))
    assert flips >= 1
    # sizes of A at the count rules: 11 (the behind point in or out of the ten nearest), 10 (no answer), 1
    assert [len(c["frames"][0][0]) for c in cases[3:7]] == [11, 11, 10, 1]
    for c in cases[3:6]:   # where the behind point ranks among A's points by distance from the drone
        d2 = kc._d2(c["frames"][0][0], c["Twb"][:3, 3]); rank = int((d2 < kc._d2(c["special"][None], c["Twb"][:3, 3])[0]).sum())
        assert rank == (10 if c["name"] == "eleven_behind_farthest" else 0), (c["name"], rank)


@pytest.mark.parametrize("max_frames", kc.MAX_FRAMES)
def test_numpy_restatement_agrees_with_the_oracle(max_frames):
    run = kc.ceiling_run(max_frames)
    maps = [kc.NumpyMap(max_frames, kc.TH_DIST, kc.TH_COUNT, kc.DEPTH_MIN, kc.TBC) for _ in range(kc.S)]
    for t in range(kc.PERIODS):
        for s, m in enumerate(maps):
            fr = kc.scene_frame(s, t)
            if fr is not None:
                m.add_vertex(fr[0], fr[2])
            m.update()
            assert m.summary() == run.summaries[t][s][:2], (t, s, m.summary(), run.summaries[t][s])
    assert all(m.ties == 0 for m in maps)            # no answer depended on the order of equal distances


def test_numpy_restatement_agrees_on_the_gate_cases():
    cases, rows = kc.gate_cases(), kc.gate_run()
    for i, c in enumerate(cases):
        m = kc.NumpyMap(kc.GATE_MAX_FRAMES, kc.TH_DIST, kc.TH_COUNT, kc.DEPTH_MIN, kc.GATE_TBC)
        for t in range(2):
            m.add_vertex(c["frames"][t][0], c["frames"][t][2]); m.update()
            assert m.summary() == rows[t][i][:2], (c["name"], t)
        assert m.ties == 0, c["name"]


def test_full_capacity_script_pops_by_pose_and_by_length():
    run = kc.full_run()
    assert all(len(c) == kc.FULL_CAP and len(e) == kc.ECAP for s in range(kc.S) for c, e, _ in kc.full_script(200 + s))
    nk = [[row[s][0] for row in run.summaries] for s in range(kc.S)]
    assert all(max(n) == kc.FULL_MAX_FRAMES + 1 for n in nk)                       # the ceiling of this map: pops by length
    assert all(run.pops[7][s] >= 3 for s in range(kc.S))                           # and, after the jump, by pose
