"""GPU: the segment search over the frames -- amk_kfmap_segment_search on a keyframe map and amk_kd_segment_search_frames on a list of
handles (map_segment_kernel, csrc/map_query.hip) -- against the brute force of tests/_segment.py over the frames each scene holds.

The map is flown as in tests/test_kfmap_radius_gpu.py: max_frame_count 3, five periods, the scenes joining at different periods, so
that they hold 4, 2, 1, 0 and 3 frames; scene 0's current frame has 4 200 points, a second tile.  The obstacle frames are read back
with amk_kfmap_points_host, the edge frames are the submitted edge clouds of the periods tests/_kfmap.MapOracle names.  Clouds and
paths are quantised, so equal distances across frames occur.  Every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests import _map_query as mq
from tests import _segment as G

pytestmark = pytest.mark.gpu

S, CAP, ECAP, NP = 5, 4300, 48, 7
PERIODS, STEP, QUANTUM, MAX_FRAMES = 5, 0.4, 0.25, 3
START = [0, 3, 4, PERIODS, 2]         # the period a scene gets its first frame (scene 3: never)
HELD = [4, 2, 1, 0, 3]                # frames they hold after the flight
BIG = 4200                            # scene 0's last frame: more than one tile of 4 096 points
TH_DIST, TH_COUNT, DEPTH_MIN = 0.3, 1, 0.3
TBC = mq.look_x_pose([0.0, 0.0, 0.0])
MAP_KEYS = ("counts", "sqdist", "t", "frame", "pts")


def pose(d):
    Twb = np.eye(4)
    Twb[:3, 3] = [d, 0.0, 1.5]
    return Twb @ TBC


def flight():
    """frames[t][s] = (cloud [n, 3] f32, edge [<= 42, 3] f32, Twc); empty before the scene's first period"""
    rngs = [np.random.default_rng(700 + s) for s in range(S)]
    frames = []
    for t in range(PERIODS):
        d, row = STEP * t, []
        for s in range(S):
            n = BIG if (s == 0 and t == PERIODS - 1) else int(rngs[s].integers(150, 256))
            box = lambda m: np.round((rngs[s].random((m, 3)) * [7.0, 8.0, 3.0] + [d + 2.0, -4.0, 0.0]) / QUANTUM) * QUANTUM
            cloud, edge = box(n), box(min(n // 6, 42))
            if t < START[s]:
                cloud, edge = cloud[:0], edge[:0]
            row.append((cloud.astype(np.float32), edge.astype(np.float32), pose(d)))
        frames.append(row)
    return frames


def make_path(stride=3):
    """a path of NP points per scene through the region the last frames cover, every leg about 1 m, quantised to QUANTUM / 2"""
    rng = np.random.default_rng(43)
    path = rng.normal(size=(S, NP, stride)) * 20.0
    d = STEP * (PERIODS - 1)
    start = rng.random((S, 1, 3)) * [3.0, 5.0, 2.0] + [d + 2.0, -3.0, 0.25]
    steps = np.cumsum(rng.random((S, NP, 3)) * [1.0, 1.0, 0.4] * rng.choice([-1.0, 1.0], size=(S, NP, 3)), axis=1)
    path[:, :, :3] = np.round((start + steps) / (QUANTUM / 2)) * (QUANTUM / 2)
    return path


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
    assert len(obs[0][0]) == BIG
    yield gmap, obs, edge
    gmap.close()


def to_np(out):
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("k", [8, 64, 0])
def test_map_segment_search_sums_and_merges_the_frames(flown, edge, k):
    import torch
    from avoid_mpc_amd import capi
    gmap, obs, edges = flown
    held = edges if edge else obs
    path = make_path(14)
    r2 = 4.125 if edge else 1.125
    got = to_np(gmap.segment_search(torch.from_numpy(path).cuda(), r2, k, edge=edge))
    torch.cuda.synchronize()
    want = G.expected_batch(held, path, r2, k)
    G.assert_bitwise(got, want, MAP_KEYS if k > 0 else ("counts",), f"edge {edge}, k {k}")
    # what the comparison must have seen: counts that ARE sums over several frames, no answer for the scene without a frame
    for s in (0, 4):
        per_frame = np.array([[G.segment_brute(f, path[s, j], path[s, j + 1], r2, 1)["count"] for f in held[s]] for j in range(NP - 1)])
        assert np.array_equal(per_frame.sum(axis=1), got["counts"][s]) and ((per_frame > 0).sum(axis=1) >= 2).sum() >= 2, per_frame
    assert (got["counts"][3] == 0).all() and got["counts"].max() > 8
    if k > 0:
        assert (got["frame"][3] == -1).all() and (got["sqdist"][3] == G.DBL_MAX).all() and (got["t"][3] == 0).all()
        d, f = got["sqdist"], got["frame"]
        assert (d[f >= 0] < r2).all() and ((got["t"] >= 0) & (got["t"] <= 1)).all()
        if k == 64:
            assert len(set(f[4].reshape(-1).tolist()) - {-1}) >= 2       # (scene 4: three frames of about 200 points)
            ties = ((d[..., :-1] == d[..., 1:]) & (f[..., 1:] >= 0) & (f[..., :-1] < f[..., 1:])).sum()
            assert ties >= 1, ties                                         # equal distances across frames: the earlier frame first
    # the host variant
    n = max(k, 1)
    L = NP - 1
    hp, hd, ht = np.zeros((S, L, n, 3), np.float32), np.zeros((S, L, n)), np.zeros((S, L, n))
    hf, hc = np.zeros((S, L, n), np.int32), np.zeros((S, L), np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if k > 0 or a is hc else None
    capi.check(gmap.lib.amk_kfmap_segment_search_host(gmap.h, path.ctypes.data_as(C.c_void_p), 14, NP, r2, k, int(edge), vp(hp), vp(hd), vp(ht),
                                                      vp(hf), vp(hc)), "amk_kfmap_segment_search_host")
    assert np.array_equal(hc, got["counts"])
    if k > 0:
        G.assert_bitwise(dict(pts=hp, sqdist=hd, t=ht, frame=hf), got, ("pts", "sqdist", "t", "frame"), "host")


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
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import segment_search_frames
    gmap, obs, _ = flown
    path, r2, k = make_path(3), 1.125, 8
    pd = torch.from_numpy(path).cuda()
    hs = handles_of(obs, n_handles, CAP)
    try:
        got = to_np(segment_search_frames(hs, pd, r2, k))
        torch.cuda.synchronize()
        G.assert_bitwise(got, G.expected_batch([fr[:n_handles] for fr in obs], path, r2, k), MAP_KEYS, f"{n_handles} handles")
        on_map = to_np(gmap.segment_search(pd, r2, k))
        torch.cuda.synchronize()
        same = [s for s in range(S) if HELD[s] <= n_handles]      # the scenes whose whole map the handles hold
        assert len(same) >= 2
        for key in MAP_KEYS:
            assert np.array_equal(got[key][same], on_map[key][same]), key
        # the host variant of the handle list
        L = NP - 1
        hp, hd, ht = np.zeros((S, L, k, 3), np.float32), np.zeros((S, L, k)), np.zeros((S, L, k))
        hf, hc = np.zeros((S, L, k), np.int32), np.zeros((S, L), np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        ha = (C.c_void_p * n_handles)(*[h.h for h in hs])
        capi.check(capi.load().amk_kd_segment_search_frames_host(ha, n_handles, vp(path), 3, NP, r2, k, vp(hp), vp(hd), vp(ht), vp(hf), vp(hc)),
                   "amk_kd_segment_search_frames_host")
        G.assert_bitwise(dict(pts=hp, sqdist=hd, t=ht, frame=hf, counts=hc), got, MAP_KEYS, "host")
    finally:
        for h in hs:
            h.close()


def test_truncation_across_a_frame_boundary_at_equal_distances():
    """the same cloud as two frames: every distance occurs in both, frame 0's entry first; an odd max_results ends between the two"""
    import torch
    from avoid_mpc_amd.host import segment_search_frames
    rng = np.random.default_rng(47)
    cloud = [[(rng.random((200, 3)) * 3.0).astype(np.float32)] * 2 for _ in range(S)]
    path = rng.random((S, 4, 3)) * 3.0
    hs = handles_of(cloud, 2, 200)
    try:
        got = to_np(segment_search_frames(hs, torch.from_numpy(path).cuda(), 0.8, 7))
        torch.cuda.synchronize()
        G.assert_bitwise(got, G.expected_batch(cloud, path, 0.8, 7), MAP_KEYS, "twice the same cloud")
        one = G.expected_batch([c[:1] for c in cloud], path, 0.8, 7)
        assert np.array_equal(got["counts"], 2 * one["counts"]) and got["counts"].min() >= 8
        assert np.array_equal(got["frame"], np.tile([0, 1, 0, 1, 0, 1, 0], (S, 3, 1)))
        assert np.array_equal(got["sqdist"][..., 0::2], one["sqdist"][..., :4]) and np.array_equal(got["t"][..., 0::2], one["t"][..., :4])
    finally:
        for h in hs:
            h.close()


def test_bad_arguments_and_scan_mode_are_refused():
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import KdBatch
    lib = capi.load()
    kd = KdBatch(2, 32)
    try:
        kd.build(torch.rand((2, 32, 3), device="cuda"))
        path = torch.rand((2, 4, 3), dtype=torch.float64, device="cuda")
        cnt = torch.full((2, 3), -7, dtype=torch.int32, device="cuda"); tt = torch.full((2, 3, 4), -7.0, dtype=torch.float64, device="cuda")

        def call(n, r2=1.0, k=4, npts=4):
            ha = (C.c_void_p * n)(*[kd.h] * n)
            return lib.amk_kd_segment_search_frames(ha, n, capi.dptr(path), 3, npts, r2, k, None, None, capi.dptr(tt), None, capi.dptr(cnt), None)

        INV, UNS = capi.AMK_ERR_INVALID_ARG, capi.AMK_ERR_UNSUPPORTED
        assert call(17) == UNS and call(0) == INV and call(2, npts=1) == INV
        assert call(2, r2=-1.0) == INV and call(2, k=65) == UNS and call(2, k=0) == INV
        capi.check(lib.amk__kd_set_mode(kd.h, 1), "scan mode")
        assert call(2) == UNS
        capi.check(lib.amk__kd_set_mode(kd.h, 0), "index mode")
        torch.cuda.synchronize()
        assert (cnt == -7).all() and (tt == -7).all()
        assert call(16) == capi.AMK_OK
        torch.cuda.synchronize()
        assert (cnt >= 0).all() and ((tt >= 0) & (tt <= 1)).all()
    finally:
        kd.close()
