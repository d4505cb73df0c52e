"""GPU: the radius search over the frames -- amk_kfmap_radius_search on a keyframe map and amk_kd_radius_search_frames on a list of
handles (map_radius_kernel, csrc/map_query.hip) -- against the brute force of tests/_radius.py over the frames each scene holds.

A map with max_frame_count 3 is flown for five periods; the scenes join the flight at different periods, so that they hold 4, 2, 1,
0 and 3 frames.  The obstacle frames are read back with amk_kfmap_points_host (keyframes are rebuilt from their outliers: the map
itself says what they hold); the edge frames are the submitted edge clouds of the periods tests/_kfmap.MapOracle names.  Clouds and
queries are quantised, so equal distances across frames and points at exactly the radius occur.  Every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests import _map_query as mq
from tests import _radius as R

pytestmark = pytest.mark.gpu

S, CAP, ECAP, NQ = 5, 256, 48, 12
PERIODS, STEP, QUANTUM, MAX_FRAMES = 5, 0.4, 0.25, 3
START = [0, 3, 4, PERIODS, 2]         # the period a scene gets its first frame (scene 3: never)
HELD = [4, 2, 1, 0, 3]                # frames they hold after the flight
TH_DIST, TH_COUNT, DEPTH_MIN = 0.3, 1, 0.3
TBC = mq.look_x_pose([0.0, 0.0, 0.0])
MAP_KEYS = ("counts", "sqdist", "frame", "pts")


def pose(d):
    Twb = np.eye(4)
    Twb[:3, 3] = [d, 0.0, 1.5]
    return Twb @ TBC


def flight():
    """frames[t][s] = (cloud [n, 3] f32, edge [n // 6, 3] f32, Twc); empty before the scene's first period"""
    rngs = [np.random.default_rng(300 + s) for s in range(S)]
    frames = []
    for t in range(PERIODS):
        d, row = STEP * t, []
        for s in range(S):
            n = int(rngs[s].integers(150, CAP))
            box = lambda m: np.round((rngs[s].random((m, 3)) * [7.0, 8.0, 3.0] + [d + 2.0, -4.0, 0.0]) / QUANTUM) * QUANTUM
            cloud, edge = box(n), box(n // 6)
            if t < START[s]:
                cloud, edge = cloud[:0], edge[:0]
            row.append((cloud.astype(np.float32), edge.astype(np.float32), pose(d)))
        frames.append(row)
    return frames


def make_queries(stride=3):
    rng = np.random.default_rng(41)
    q = rng.normal(size=(S, NQ, stride)) * 20.0
    d = STEP * (PERIODS - 1)
    q[:, :, :3] = np.round((rng.random((S, NQ, 3)) * [8.0, 9.0, 3.5] + [d + 1.5, -4.5, -0.25]) / (QUANTUM / 2)) * (QUANTUM / 2)
    return q


@pytest.fixture(scope="module")
def flown():
    """(KfMap after the flight, per scene the obstacle frames the map holds, per scene its edge frames)"""
    import torch
    from avoid_mpc_amd.host import KfMap
    from tests import _kfmap
    frames = flight()
    gmap = KfMap(S, CAP, ECAP, MAX_FRAMES, TH_DIST, TH_COUNT, DEPTH_MIN, TBC)
    oracles = [_kfmap.MapOracle(MAX_FRAMES, TH_DIST, TH_COUNT, DEPTH_MIN, TBC) for _ in range(S)]
    for t, row in enumerate(frames):
        cl = np.zeros((S, CAP, 3), np.float32); ed = np.zeros((S, ECAP, 3), np.float32)
        cn = np.zeros(S, np.int32); en = np.zeros(S, np.int32); Tw = np.zeros((S, 4, 4))
        for s, (c, e, T) in enumerate(row):
            cl[s, :len(c)] = c; cn[s] = len(c); ed[s, :len(e)] = e; en[s] = len(e); Tw[s] = T
            oracles[s].add_vertex(c, e, T, stamp=t)
            oracles[s].update()
        a = [torch.from_numpy(x).cuda() for x in (cl, ed, Tw, cn, en)]
        gmap.add_vertex(a[0], a[1], a[2], counts=a[3], edge_counts=a[4])
        gmap.update()
    torch.cuda.synchronize()
    obs, edge = [], []
    for s in range(S):
        xyz, sizes = gmap.points(s)
        held = [int(n) for n in sizes if n >= 0]
        assert len(held) == HELD[s] and held == oracles[s].summary()[1], (s, held, oracles[s].summary())
        cuts = np.cumsum([0] + held)
        obs.append([xyz[cuts[f]:cuts[f + 1]] for f in range(len(held))])
        edge.append([frames[f.stamp][s][1] for f in oracles[s].frames()])
    yield gmap, obs, edge
    gmap.close()


def to_np(out):
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("k", [8, 64, 0])
def test_map_radius_search_sums_and_merges_the_frames(flown, edge, k):
    import torch
    gmap, obs, edges = flown
    held = edges if edge else obs
    q = make_queries(14)
    r2 = 4.125 if edge else 1.125   # sums of three squares of multiples of 1/8: points at exactly the radius exist (asserted below)
    got = to_np(gmap.radius_search(torch.from_numpy(q).cuda(), r2, k, edge=edge))
    torch.cuda.synchronize()
    want = R.expected_batch(held, q, r2, k)
    R.assert_bitwise(got, want, MAP_KEYS if k > 0 else ("counts",), f"edge {edge}, k {k}")
    # what the comparison must have seen: counts that ARE sums over several frames, no answer for the scene without a frame
    per_frame = np.array([[sum(R.radius_brute(f, q[0, i], r2, 1)["count"] > 0 for f in held[0])] for i in range(NQ)])
    assert (per_frame >= 2).sum() >= 3 and (got["counts"][3] == 0).all() and got["counts"][:3].max() > 8
    if k > 0:
        assert (got["frame"][3] == -1).all() and set(got["frame"][0].reshape(-1).tolist()) >= {0, 1, 2, 3}
        d, f = got["sqdist"], got["frame"]
        ties = ((d[..., :-1] == d[..., 1:]) & (f[..., 1:] >= 0) & (f[..., :-1] < f[..., 1:])).sum()
        assert ties >= 3, ties                                             # equal distances across frames: the earlier frame first
        assert (d[f >= 0] < r2).all() and any((R.sq_dists(c, q[s, i]) == r2).any() for s in range(S) for c in held[s] for i in range(NQ))   # strict
    # the host variant
    n = max(k, 1)
    hp, hd, hf = np.zeros((S, NQ, n, 3), np.float32), np.zeros((S, NQ, n)), np.zeros((S, NQ, n), np.int32)
    hc = np.zeros((S, NQ), np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if k > 0 or a is hc else None
    from avoid_mpc_amd import capi
    capi.check(gmap.lib.amk_kfmap_radius_search_host(gmap.h, q.ctypes.data_as(C.c_void_p), 14, NQ, r2, k, int(edge), vp(hp), vp(hd), vp(hf),
                                                     vp(hc)), "amk_kfmap_radius_search_host")
    assert np.array_equal(hc, got["counts"])
    if k > 0:
        R.assert_bitwise(dict(pts=hp, sqdist=hd, frame=hf), got, ("pts", "sqdist", "frame"), "host")


def handles_of(frames_per_scene, n_handles, cap):
    """n_handles KdBatch of S scenes: handle f holds frame f of every scene (an empty cloud where the scene holds fewer)"""
    import torch
    from avoid_mpc_amd.host import KdBatch
    out = []
    for f in range(n_handles):
        xyz = np.zeros((S, cap, 3), np.float32); cn = np.zeros(S, np.int32)
        for s in range(S):
            if f < len(frames_per_scene[s]):
                c = frames_per_scene[s][f]
                xyz[s, :len(c)] = c; cn[s] = len(c)
        kd = KdBatch(S, cap)
        kd.build(torch.from_numpy(xyz).cuda(), torch.from_numpy(cn).cuda())
        out.append(kd)
    return out


@pytest.mark.parametrize("n_handles", [1, 3, 16])
def test_handle_lists_answer_like_the_map(flown, n_handles):
    import torch
    from avoid_mpc_amd.host import radius_search_frames
    gmap, obs, _ = flown
    q, r2, k = make_queries(3), 1.125, 8
    qd = torch.from_numpy(q).cuda()
    hs = handles_of(obs, n_handles, CAP)
    try:
        got = to_np(radius_search_frames(hs, qd, r2, k))
        torch.cuda.synchronize()
        R.assert_bitwise(got, R.expected_batch([fr[:n_handles] for fr in obs], q, r2, k), MAP_KEYS, f"{n_handles} handles")
        on_map = to_np(gmap.radius_search(qd, r2, k))
        torch.cuda.synchronize()
        same = [s for s in range(S) if HELD[s] <= n_handles]      # the scenes whose whole map the handles hold
        assert len(same) >= 2
        for key in MAP_KEYS:
            assert np.array_equal(got[key][same], on_map[key][same]), key
    finally:
        for h in hs:
            h.close()


def test_truncation_across_a_frame_boundary_at_equal_distances():
    """the same cloud as two frames: every distance occurs in both, frame 0's entry first; an odd max_results ends between the two"""
    import torch
    from avoid_mpc_amd.host import radius_search_frames
    rng = np.random.default_rng(43)
    cloud = [[(rng.random((200, 3)) * 3.0).astype(np.float32)] * 2 for _ in range(S)]
    q = rng.random((S, 4, 3)) * 3.0
    hs = handles_of(cloud, 2, 200)
    try:
        got = to_np(radius_search_frames(hs, torch.from_numpy(q).cuda(), 0.8, 7))
        torch.cuda.synchronize()
        R.assert_bitwise(got, R.expected_batch(cloud, q, 0.8, 7), MAP_KEYS, "twice the same cloud")
        one = R.expected_batch([c[:1] for c in cloud], q, 0.8, 7)
        assert np.array_equal(got["counts"], 2 * one["counts"]) and got["counts"].min() >= 4
        assert np.array_equal(got["frame"], np.tile([0, 1, 0, 1, 0, 1, 0], (S, 4, 1)))
        assert np.array_equal(got["sqdist"][..., 0::2], one["sqdist"][..., :4])
    finally:
        for h in hs:
            h.close()


def test_too_many_handles_and_scan_mode_are_unsupported():
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import KdBatch
    lib = capi.load()
    kd = KdBatch(2, 32)
    try:
        kd.build(torch.rand((2, 32, 3), device="cuda"))
        q = torch.rand((2, 3, 3), dtype=torch.float64, device="cuda")
        cnt = torch.full((2, 3), -7, dtype=torch.int32, device="cuda"); d2 = torch.full((2, 3, 4), -7.0, dtype=torch.float64, device="cuda")

        def call(n, r2=1.0, k=4):
            ha = (C.c_void_p * n)(*[kd.h] * n)
            return lib.amk_kd_radius_search_frames(ha, n, capi.dptr(q), 3, 3, r2, k, None, capi.dptr(d2), None, capi.dptr(cnt), None)

        assert call(17) == capi.AMK_ERR_UNSUPPORTED and call(0) == capi.AMK_ERR_INVALID_ARG
        assert call(2, r2=-1.0) == capi.AMK_ERR_INVALID_ARG and call(2, k=65) == capi.AMK_ERR_UNSUPPORTED and call(2, k=0) == capi.AMK_ERR_INVALID_ARG
        capi.check(lib.amk__kd_set_mode(kd.h, 1), "scan mode")
        assert call(2) == capi.AMK_ERR_UNSUPPORTED
        capi.check(lib.amk__kd_set_mode(kd.h, 0), "index mode")
        torch.cuda.synchronize()
        assert (cnt == -7).all() and (d2 == -7).all()
        assert call(16) == capi.AMK_OK
        torch.cuda.synchronize()
        assert (cnt >= 0).all()
    finally:
        kd.close()
