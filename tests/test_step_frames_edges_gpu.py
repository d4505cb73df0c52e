"""GPU: the packed parameter vector P of the multi-frame step (amk_step_batch_frames, amk_kfmap_step; csrc/step_frames.hip) and of
the single-frame step against the oracle's, BIT FOR BIT, on the inputs of tests/_frames_cases.py: frame sizes at every count rule
(0, 1, 2, K - 1, K, K + 1), one camera pose per scene, reference points on and next to every edge of PtIsInFrame, every
instantiation of the merge (1, 2, 4, 16 candidates per lane, the re-reading form, the AMK_TIES_NANOFLANN form), ties between
frames, and keyframe maps of up to 70 query frames (every chunk of the map-mode search).

P of pass 0 (mpc_max_iter = 1) depends on no solve: it is a pure function of the queries and the merge, and it shows every
neighbour -- u, x0array and flags do not (the last reference point's neighbours do not reach them at all).  It is read through
the internal hook amk__mpc_ref_states.  tests/test_step_frames_cases.py proves on the CPU that these inputs reach every branch."""
import numpy as np
import pytest

from tests import _frames_cases as fc
from tests import _oracle
from avoid_mpc_amd import synth

pytestmark = pytest.mark.gpu
K8 = 8


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _pad_batch(clouds):
    S = len(clouds)
    nmax = max(max(len(x) for x in clouds), 1)
    buf = np.zeros((S, nmax, 3), np.float32); cnt = np.zeros(S, np.int32)
    for s, x in enumerate(clouds):
        buf[s, :len(x)] = x; cnt[s] = len(x)
    return buf, cnt, nmax


def gpu_frames(scenes, prm, cam, tie_order=0):
    """amk_step_batch_frames over the scenes (one batch) -> dict(u, x0array, flags, ref_path, P) as numpy arrays"""
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import KdBatch, MpcBatch, step_batch_frames
    S, F = len(scenes), len(scenes[0]["obs"])
    kd_o, kd_e = [], []
    for f in range(F):
        for key, out in (("obs", kd_o), ("edge", kd_e)):
            buf, cnt, nmax = _pad_batch([sc[key][f] for sc in scenes])
            kd = KdBatch(S, nmax); kd.set_tie_order(tie_order)
            kd.build(torch.from_numpy(buf).cuda(), torch.from_numpy(cnt).cuda()); out.append(kd)
    mpc = MpcBatch(prm.T, prm.dt, prm.K, S); mpc.configure(prm)
    sq = np.stack([fc.state_quads(sc, prm) for sc in scenes])
    ref = torch.from_numpy(np.stack([sc["ref_path"] for sc in scenes])).cuda()
    pos_x = torch.from_numpy(np.array([sc["pos"][0] for sc in scenes])).cuda()
    Tw = torch.from_numpy(np.stack([sc["Twc"] for sc in scenes]).astype(np.float64)).cuda()
    out = step_batch_frames(kd_o, kd_e, mpc, prm, torch.from_numpy(sq).cuda(), pos_x, ref, Twc=Tw, cam=capi.FrameCamera(*cam))
    torch.cuda.synchronize()
    return dict(u=out["u"].cpu().numpy(), x0array=out["x0array"].cpu().numpy(), flags=out["flags"].cpu().numpy(),
                ref_path=ref.cpu().numpy(), P=mpc.ref_states())


def assert_P_exact(P, runs, N, K, what=""):
    """Every scene: state (10), path (10 N, a snapped point 0 included), obstacles (3 K N) and target (10) bit-identical to the
    oracle's pass-0 vecRefStates."""
    assert P.shape == (len(runs), 20 + 10 * N + 3 * K * N)
    for s, r in enumerate(runs):
        g, o = fc.split_P(P[s], N, K), fc.split_P(r["ref_log"][0], N, K)
        for name, a, b in zip(("state", "path", "obstacles", "target"), g, o):
            if not np.array_equal(_bits(a), _bits(b)):
                bad = np.argwhere(_bits(a) != _bits(b))
                raise AssertionError(f"{what} scene {s}: {name} block differs at {bad[:6].tolist()} ({len(bad)} entries): "
                                     f"gpu {a[tuple(bad[0])]!r} oracle {b[tuple(bad[0])]!r}")


def assert_flags01(flags, runs):
    for s, r in enumerate(runs):
        assert flags[s][0] == r["flags"][0] and flags[s][1] == r["flags"][1], (s, flags[s], r["flags"])


def assert_outputs(g, runs, what=""):
    """The project's rule for u, x0array and ref_path: <= 1e-6 where the flags agree; otherwise (a rounding-level branch flip
    inside a solve changed an iteration count) flags[0] equal and <= 1e-4, in at most max(1, S // 100) scenes."""
    flipped, worst = 0, 0.0
    for s, r in enumerate(runs):
        d = max(np.abs(g["u"][s] - r["u"]).max(), np.abs(g["x0array"][s] - r["x0array"]).max() if r["flags"][1] > 0 else 0.0,
                np.abs(g["ref_path"][s] - r["ref_path"]).max())
        if np.array_equal(g["flags"][s], r["flags"]):
            worst = max(worst, d)
            assert d <= 1e-6, (what, s, d)
        else:
            flipped += 1
            assert g["flags"][s][0] == r["flags"][0] and d <= 1e-4, (what, s, g["flags"][s], r["flags"], d)
    print(f"{what}: worst |gpu - oracle| = {worst:.3e} over {len(runs) - flipped} scenes, {flipped} with other flags")
    assert flipped <= max(1, len(runs) // 100), (what, flipped)


def _both_lengths(scenes, T, K, cam, key, tie_order=0):
    """P at mpc_max_iter = 1, the outputs at 3 -> the two GPU results"""
    p1 = synth.MpcParams(T=T, K=K, max_iter=1)
    g1 = gpu_frames(scenes, p1, cam, tie_order)
    r1 = fc.oracle_frames(scenes, p1, cam, key)
    assert_flags01(g1["flags"], r1)
    assert_P_exact(g1["P"], r1, p1.N, K, str(key))
    p3 = synth.MpcParams(T=T, K=K, max_iter=3)
    g3 = gpu_frames(scenes, p3, cam, tie_order)
    assert_outputs(g3, fc.oracle_frames(scenes, p3, cam, key), str(key))
    return g1, g3


def _wide(scenes, prm, cam):
    """the same step with the re-reading merge forced (always restored)"""
    from avoid_mpc_amd import capi
    lib = capi.load()
    lib.amk__frames_force_wide(1)
    try:
        return gpu_frames(scenes, prm, cam)
    finally:
        lib.amk__frames_force_wide(0)


def test_hook_needs_a_step():
    import ctypes as C
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import MpcBatch
    mpc = MpcBatch(0.66, 0.033, 3, 2)
    buf = np.zeros(4)
    assert capi.load().amk__mpc_ref_states(mpc.h, buf.ctypes.data_as(C.c_void_p), 4) == capi.AMK_ERR_INVALID_ARG


def test_size_matrix():
    """~72 scenes in one batch: three frames cut to 0, 1, 2, K - 1, K, K + 1 or all of their points, four camera poses."""
    scenes = fc.size_matrix(K8)
    g1, _ = _both_lengths(scenes, 0.66, K8, fc.CAM, "size")
    w1 = _wide(scenes, synth.MpcParams(T=0.66, K=K8, max_iter=1), fc.CAM)   # the count rules of the re-reading merge
    assert np.array_equal(_bits(w1["P"]), _bits(g1["P"])) and np.array_equal(w1["flags"], g1["flags"])


def test_frustum_edges():
    scenes, _ = fc.frustum()
    _both_lengths(scenes, 1.0, K8, fc.CAM, "frustum")


def test_target_row_is_not_contracted():
    """speed * T inexact and the last reference point well short of it: `speed*T - fmax(..)` evaluated with a fused multiply-add
    gives other bits than the oracle's two IEEE operations on most of these scenes (tests/test_step_frames_cases.py)."""
    prm = synth.MpcParams(T=0.66, K=K8, speed=fc.TARGET_SPEED, max_iter=1)
    scenes = fc.target_rows(K8)
    g = gpu_frames(scenes, prm, fc.CAM)
    runs = fc.oracle_frames(scenes, prm, fc.CAM, "target")
    assert_flags01(g["flags"], runs)
    assert_P_exact(g["P"], runs, prm.N, K8, "target rows")


@pytest.mark.parametrize("F,K", fc.WIDTH_CASES)
def test_merge_width(F, K):
    """Both sides of every boundary between the merge's instantiations; then the same with the re-reading merge forced: bit-identical."""
    scenes = fc.partition(F, K)
    g1, g3 = _both_lengths(scenes, 0.66, K, fc.CAM, ("partition", F))
    w1 = _wide(scenes, synth.MpcParams(T=0.66, K=K, max_iter=1), fc.CAM)
    w3 = _wide(scenes, synth.MpcParams(T=0.66, K=K, max_iter=3), fc.CAM)
    assert np.array_equal(_bits(w1["P"]), _bits(g1["P"])) and np.array_equal(w1["flags"], g1["flags"])
    for key in ("u", "x0array", "ref_path"):
        assert np.array_equal(_bits(w3[key]), _bits(g3[key])), key
    assert np.array_equal(w3["flags"], g3["flags"])


@pytest.mark.parametrize("F", [2, 16])
def test_ties_between_frames(F):
    """Handles in AMK_TIES_NANOFLANN mode (the merge's single-wavefront instantiation): points of DIFFERENT frames at exactly the
    same squared distance from a reference point that merges -- the earlier frame comes first, as in the oracle."""
    prm = synth.MpcParams(T=0.66, K=K8, max_iter=1)
    scenes = fc.ties(F)
    n_ties = fc.count_merged_ties(scenes, prm, fc.TIES_CAM)
    assert n_ties >= prm.N, n_ties
    g = gpu_frames(scenes, prm, fc.TIES_CAM, tie_order=1)
    runs = fc.oracle_frames(scenes, prm, fc.TIES_CAM, ("ties", F))
    assert_flags01(g["flags"], runs)
    assert_P_exact(g["P"], runs, prm.N, K8, f"ties F={F} ({n_ties} tied rows)")


@pytest.mark.parametrize("max_frames,deep", [(30, 24), (100, 56)])
def test_deep_map(max_frames, deep):
    """A keyframe map driven to 70 query frames (the 30-frame map: 30) with keyframes of 1, 2, K - 1, K and K + 1 points: the state
    of the map every period, P of a step whose path leaves the frustum halfway after periods 9, 25, 57 and 70 (one, two, three
    and four chunks of the map-mode search)."""
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import KfMap, MpcBatch
    run = fc.deep_map_oracle(max_frames)
    sizes = {n for row in run.summaries for (_, sz, _) in row for n in sz[1:]}
    assert {1, 2, K8 - 1, K8, K8 + 1} <= sizes and max(len(sz) for row in run.summaries for (_, sz, _) in row) > deep
    prm, S = run.prm, len(run.scripts)
    cap, ecap = fc.DEEP_POINTS + fc.DEEP_EXTRA, fc.DEEP_EDGE
    gmap = KfMap(S, cap, ecap, max_frames, 0.1, 1, 0.1, fc.DEEP_TBC)
    gmpc = MpcBatch(prm.T, prm.dt, prm.K, S); gmpc.configure(prm)
    gcam = capi.FrameCamera(*fc.DEEP_CAM)
    dev = torch.device("cuda")
    Twc = torch.from_numpy(np.repeat(fc.DEEP_TWC[None], S, 0).copy()).to(dev)
    sq = torch.from_numpy(np.stack([fc.state_quads(sc, prm) for sc in run.scenes])).to(dev)
    px = torch.from_numpy(np.array([sc["pos"][0] for sc in run.scenes])).to(dev)
    try:
        for t in range(fc.DEEP_PERIODS):
            clouds = np.zeros((S, cap, 3), np.float32); edges = np.zeros((S, ecap, 3), np.float32)
            cn = np.zeros(S, np.int32); en = np.zeros(S, np.int32)
            for s in range(S):
                c, e = run.scripts[s][t]
                clouds[s, :len(c)] = c; cn[s] = len(c); edges[s, :len(e)] = e; en[s] = len(e)
            gmap.add_vertex(torch.from_numpy(clouds).to(dev), torch.from_numpy(edges).to(dev), Twc,
                            counts=torch.from_numpy(cn).to(dev), edge_counts=torch.from_numpy(en).to(dev))
            gmap.update()
            st = gmap.state()
            for s in range(S):
                nk, sz, outl = run.summaries[t][s]
                assert st["n_keyframes"][s] == nk and st["n_query_frames"][s] == len(sz), (t, s)
                assert list(st["frame_sizes"][s][:len(sz)]) == sz and (st["frame_sizes"][s][len(sz):] == -1).all(), (t, s)
                assert st["last_outliers"][s] == max(outl, 0), (t, s)
            if t + 1 in fc.DEEP_STEPS:
                dref = torch.from_numpy(np.stack([sc["ref_path"] for sc in run.scenes])).to(dev)
                out = gmap.step(gmpc, prm, sq, px, dref, cam=gcam)
                torch.cuda.synchronize()
                assert_flags01(out["flags"].cpu().numpy(), run.steps[t + 1])
                assert_P_exact(gmpc.ref_states(), run.steps[t + 1], prm.N, K8, f"map of {max_frames}, period {t + 1}")
    finally:
        gmap.close()


@pytest.mark.parametrize("K", [1, 2, 10, 33, 64])
def test_single_frame_step_at_unused_k(K):
    """amk_step_batch at neighbour counts no other test uses, clouds of K - 1, K, K + 1 and 2000 points in one batch: P of pass 0
    (with the speed and the last reference points of fc.target_rows: the target entry of this path is not contracted either)."""
    import torch
    from avoid_mpc_amd.host import KdBatch, MpcBatch, step_batch
    prm = synth.MpcParams(T=0.66, K=K, max_iter=1, speed=fc.TARGET_SPEED)
    scenes = []
    for s, n in enumerate((K - 1, K, K + 1, 2000)):
        sc = synth.make_scene(2000, 5600 + s, prm)
        sc["cloud"] = sc["cloud"][:n].copy()
        sc["ref_path"][-1, 0] = fc.TARGET_LAST_X[2 + s]
        scenes.append(sc)
    S = len(scenes)
    cl, cn, nmax = _pad_batch([sc["cloud"] for sc in scenes]); ed, en, emax = _pad_batch([sc["edge"] for sc in scenes])
    kd_o, kd_e = KdBatch(S, nmax), KdBatch(S, emax)
    kd_o.build(torch.from_numpy(cl).cuda(), torch.from_numpy(cn).cuda()); kd_e.build(torch.from_numpy(ed).cuda(), torch.from_numpy(en).cuda())
    mpc = MpcBatch(prm.T, prm.dt, K, S); mpc.configure(prm)
    sq = np.stack([fc.state_quads(sc, prm) for sc in scenes])
    ref = torch.from_numpy(np.stack([sc["ref_path"] for sc in scenes])).cuda()
    pos_x = torch.from_numpy(np.array([sc["pos"][0] for sc in scenes])).cuda()
    out = step_batch(kd_o, kd_e, mpc, prm, torch.from_numpy(sq).cuda(), pos_x, ref)
    torch.cuda.synchronize()
    runs = []
    for s, sc in enumerate(scenes):
        m = _oracle.MpcOracle(prm.T, prm.dt, K); m.configure(prm); m.set_solver_options(max_iter=1)   # (P is packed before the solve)
        runs.append(_oracle.step_oracle(_oracle.kd_oracle(sc["cloud"]), _oracle.kd_oracle(sc["edge"]), m, prm, sq[s], sc["pos"][0],
                                        sc["ref_path"].copy(), want_log=True))
    assert_flags01(out["flags"].cpu().numpy(), runs)
    assert_P_exact(mpc.ref_states(), runs, prm.N, K, f"single frame, K = {K}")
    full = [(fc.split_P(r["ref_log"][0], prm.N, K)[2] != fc.PAD).all(axis=2).sum() for r in runs]
    assert full == [0, 0, K * prm.N, K * prm.N], full    # the count rule: n > K answers
