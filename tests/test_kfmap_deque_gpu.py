"""GPU: the keyframe map's own bookkeeping (csrc/kfmap.hip: kf_alloc_scene, kf_pop_kernel, kf_insert_kernel, kf_init_kernel)
on the scripts of tests/_kfmap_cases.py -- a deque past 64 entries and at its ceiling of max_frame_count + 1, several pops in one
pass across entry 64, a pop to empty and the first-keyframe pass after it, DroneBehindPts on and beside each of its comparisons
under a 90 degree yaw and a general rotation, amk_kfmap_reset on a sub-range, amk_kfmap_add_vertex with first_scene > 0, without
counts and with point_stride 4.

Every period the counts, query-frame sizes and sweep outliers equal the oracle's, and the RAW state (KfMap.slots(), the internal
hook amk__kfmap_slots_host) satisfies the invariants of the slot list; at the deque's ceiling, right after the pass with several
pops, on the empty deque and two periods later a control step at mpc_max_iter = 1 hands the solve the oracle's parameter vector
bit for bit (a slot overwritten while a keyframe still points at it shows there, and only there).  All comparisons are integer
or bit-exact.  tests/test_kfmap_cases.py proves on the CPU that the scripts reach every branch named here."""
import numpy as np
import pytest

from tests import _kfmap_cases as kc
from tests.test_step_frames_edges_gpu import assert_P_exact, assert_flags01

pytestmark = pytest.mark.gpu


def check_slots(sl, S, F, what):
    """The invariants of the raw state after amk_kfmap_update."""
    P = F + 1
    assert sl["kf_slots"].shape == (S, P)
    for s in range(S):
        nk, cur, dq = int(sl["kf_n"][s]), int(sl["cur_slot"][s]), sl["kf_slots"][s]
        assert 0 <= nk <= P - 1 and -1 <= cur < P, (what, s, nk, cur)
        held = dq[:nk].tolist()
        assert len(set(held)) == nk and all(0 <= v < P for v in held), (what, s, "deque entries", held)
        assert (dq[nk:] == -1).all(), (what, s, "stale tail", dq[nk:].tolist())
        assert cur not in held[:-1], (what, s, "the current frame's slot is held by an older keyframe", cur, held)
        want = [cur * S + s if cur >= 0 else -1] + [held[f - 1] * S + s if f - 1 < nk - 1 else -1 for f in range(1, F)]
        assert sl["fmap"][:, s].tolist() == want, (what, s, "fmap", sl["fmap"][:, s].tolist(), want)
        assert sl["need"][s] == 0, (what, s)


def check_state(st, row, what):
    """n_keyframes, n_query_frames, frame_sizes and last_outliers against the oracle's (n_keyframes, sizes, last_outliers)"""
    for s, (nk, sz, outl) in enumerate(row):
        assert st["n_keyframes"][s] == nk and st["n_query_frames"][s] == len(sz), (what, s, st["n_keyframes"][s], nk, st["n_query_frames"][s], len(sz))
        assert list(st["frame_sizes"][s][:len(sz)]) == sz and (st["frame_sizes"][s][len(sz):] == -1).all(), (what, s, st["frame_sizes"][s], sz)
        assert st["last_outliers"][s] == max(outl, 0), (what, s)


def _pack(frames, cap, ecap, stride=3, pad=0.0):
    """[(cloud, edge, Twc)] -> device tensors (clouds [n, cap, stride], edges, Twc, counts, edge counts)"""
    import torch
    n = len(frames)
    cl = np.zeros((n, cap, stride), np.float32); ed = np.zeros((n, ecap, stride), np.float32)
    if stride == 4:
        cl[:, :, 3] = pad; ed[:, :, 3] = pad
    cn = np.zeros(n, np.int32); en = np.zeros(n, np.int32); Tw = np.zeros((n, 4, 4))
    for i, (c, e, T) in enumerate(frames):
        e = e if len(c) else e[:0]
        cl[i, :len(c), :3] = c; cn[i] = len(c); ed[i, :len(e), :3] = e; en[i] = len(e); Tw[i] = T
    return [torch.from_numpy(a).cuda() for a in (cl, ed, Tw, cn, en)]


def feed_ceiling(gmap, t):
    """AddVertex of period t: one call over all scenes, or -- when scene 2 is skipped -- one per run of fed scenes (first_scene > 0)"""
    fed = [s for s in range(kc.S) if kc.fed(s, t)]
    runs = [fed] if len(fed) == kc.S else [[s for s in fed if s < kc.SKIP_SCENE], [s for s in fed if s > kc.SKIP_SCENE]]
    for scenes in runs:
        cl, ed, Tw, cn, en = _pack([kc.scene_frame(s, t) for s in scenes], kc.CAP, kc.ECAP)
        gmap.add_vertex(cl, ed, Tw, counts=cn, edge_counts=en, first_scene=scenes[0])


def step_and_compare(gmap, gmpc, x, want, scenes, what):
    import torch
    from avoid_mpc_amd import capi
    from tests import _oracle
    scs = [kc.step_scene(s, x) for s in range(kc.S)]
    sq = torch.from_numpy(np.stack([_oracle.scene_state_quads(sc, kc.PRM) for sc in scs])).cuda()
    px = torch.from_numpy(np.array([sc["pos"][0] for sc in scs])).cuda()
    dref = torch.from_numpy(np.stack([sc["ref_path"] for sc in scs])).cuda()
    out = gmap.step(gmpc, kc.PRM, sq, px, dref, cam=capi.FrameCamera(*kc.STEP_CAM))
    torch.cuda.synchronize()
    flags, P = out["flags"].cpu().numpy(), gmpc.ref_states()
    assert_flags01(flags[scenes], [want[s] for s in scenes])
    assert_P_exact(P[scenes], [want[s] for s in scenes], kc.PRM.N, kc.K, what)


def run_ceiling(max_frames, run, reset_at=None, reset=None):
    from avoid_mpc_amd.host import KfMap, MpcBatch
    gmap = KfMap(kc.S, kc.CAP, kc.ECAP, max_frames, kc.TH_DIST, kc.TH_COUNT, kc.DEPTH_MIN, kc.TBC)
    gmpc = MpcBatch(kc.PRM.T, kc.PRM.dt, kc.PRM.K, kc.S); gmpc.configure(kc.PRM)
    try:
        for t in range(kc.PERIODS):
            what = f"max_frame_count {max_frames}, period {t}"
            if t == reset_at:
                gmap.reset(*reset)
                sl = gmap.slots()
                check_slots(sl, kc.S, max_frames + 1, what + " after the reset")
                for s in range(reset[0], reset[0] + reset[1]):
                    assert sl["cur_slot"][s] == -1 and sl["kf_n"][s] == 0 and (sl["fmap"][:, s] == -1).all(), (what, s)
            feed_ceiling(gmap, t)
            gmap.update()
            check_state(gmap.state(), run.summaries[t], what)
            check_slots(gmap.slots(), kc.S, max_frames + 1, what)
            if t in run.steps:
                step_and_compare(gmap, gmpc, kc.drone_x(t), run.steps[t], list(range(kc.S)), what)
    finally:
        gmap.close()


@pytest.mark.parametrize("max_frames", kc.MAX_FRAMES)
def test_deque_at_and_past_the_register_boundary(max_frames):
    """max_frame_count 100: 101 keyframes over 15 periods of length pops, 101 -> fewer than 64 in ONE pass, the empty deque, the
    first-keyframe pass; 63 and 64: peaks of 64 and 65 entries, the two sides of the register boundary; 1 and 2: the smallest maps."""
    run_ceiling(max_frames, kc.ceiling_run(max_frames))


def test_reset_of_a_sub_range():
    """amk_kfmap_reset(map, 1, 2) before period 60 of the max_frame_count 64 map: scenes 1 and 2 equal NEW maps fed the rest of the
    script, scenes 0 and 3 are untouched -- state every period, P of the steps after periods 110, 116, 126 and 128."""
    run, plain = kc.ceiling_run(64, 60, (1, 2)), kc.ceiling_run(64)
    for t in range(kc.PERIODS):
        assert run.summaries[t][0] == plain.summaries[t][0] and run.summaries[t][3] == plain.summaries[t][3]
    assert run.summaries[59][1][0] > 1 and run.summaries[60][1][0] == 1 and run.summaries[60][2][0] == 1   # (period 60 feeds every scene)
    run_ceiling(64, run, reset_at=60, reset=(1, 2))


def test_gate_cases():
    """Every row of the gate table as a scene of one max_frame_count 5 map: after period 1 the deque holds 0 keyframes (A was
    popped and B is not inserted) or 2."""
    from avoid_mpc_amd.host import KfMap
    cases, rows = kc.gate_cases(), kc.gate_run()
    S = len(cases)
    gmap = KfMap(S, 32, kc.ECAP, kc.GATE_MAX_FRAMES, kc.TH_DIST, kc.TH_COUNT, kc.DEPTH_MIN, kc.GATE_TBC)
    try:
        for t in range(2):
            cl, ed, Tw, cn, en = _pack([c["frames"][t] for c in cases], 32, kc.ECAP)
            gmap.add_vertex(cl, ed, Tw, counts=cn, edge_counts=en)
            gmap.update()
            st = gmap.state()
            for s, c in enumerate(cases):
                if t == 1:
                    assert st["n_keyframes"][s] == c["expect"], (c["name"], st["n_keyframes"][s])
                check_state({k: v[s:s + 1] for k, v in st.items()}, rows[t][s:s + 1], c["name"])
            check_slots(gmap.slots(), S, kc.GATE_MAX_FRAMES + 1, f"gate cases, period {t}")
    finally:
        gmap.close()


@pytest.mark.parametrize("stride,with_counts", [(3, False), (4, True), (4, False)])
def test_add_vertex_without_counts_and_with_stride_4(stride, with_counts):
    """counts = NULL (every cloud fills its capacity) and point_stride 4 with NaN in the fourth lane: the same oracle, state every
    period, P of a step after the last one."""
    from avoid_mpc_amd.host import KfMap, MpcBatch
    run = kc.full_run()
    gmap = KfMap(kc.S, kc.FULL_CAP, kc.ECAP, kc.FULL_MAX_FRAMES, kc.TH_DIST, kc.TH_COUNT, kc.DEPTH_MIN, kc.TBC)
    gmpc = MpcBatch(kc.PRM.T, kc.PRM.dt, kc.PRM.K, kc.S); gmpc.configure(kc.PRM)
    try:
        for t in range(kc.FULL_PERIODS):
            cl, ed, Tw, cn, en = _pack([kc.full_script(200 + s)[t] for s in range(kc.S)], kc.FULL_CAP, kc.ECAP, stride, np.nan)
            assert (cn.cpu().numpy() == kc.FULL_CAP).all() and (en.cpu().numpy() == kc.ECAP).all()
            gmap.add_vertex(cl, ed, Tw, counts=cn if with_counts else None, edge_counts=en if with_counts else None)
            gmap.update()
            check_state(gmap.state(), run.summaries[t], f"stride {stride}, period {t}")
            check_slots(gmap.slots(), kc.S, kc.FULL_MAX_FRAMES + 1, f"stride {stride}, period {t}")
        t = kc.FULL_PERIODS - 1
        step_and_compare(gmap, gmpc, kc.full_x(t), run.steps[t], list(range(kc.S)), f"stride {stride}")
    finally:
        gmap.close()


def test_slots_hook_arguments():
    from avoid_mpc_amd import capi
    assert capi.load().amk__kfmap_slots_host(None, None, None, None, None, None) == capi.AMK_ERR_INVALID_ARG
