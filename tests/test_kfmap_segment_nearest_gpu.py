"""GPU: segment nearest over the frames -- amk_kfmap_segment_nearest on a keyframe map and amk_kd_segment_nearest_frames on a list of
handles (map_segment_nearest_kernel, csrc/map_query.hip) -- against the brute force of tests/_segment_nearest.py over the frames each
scene holds.

The map is flown as tests/test_kfmap_segment_gpu.py flies it (its flight, poses and path are imported): the scenes hold 4, 2, 1, 0 and
3 frames, scene 0's current frame has 4 200 points, clouds and paths are quantised, so equal distances across frames occur.  Every
comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests import _segment_nearest as N
from tests.test_kfmap_segment_gpu import (CAP, DEPTH_MIN, ECAP, HELD, MAP_KEYS, MAX_FRAMES, NP, S, TBC, TH_COUNT, TH_DIST, flight,
                                          handles_of, make_path, to_np)

pytestmark = pytest.mark.gpu


def fly(tie_order=None):
    """-> (KfMap after the flight, per scene the obstacle frames the map holds, per scene its edge frames)"""
    import torch
    from avoid_mpc_amd.host import KfMap
    from tests import _kfmap
    frames = flight()
    gmap = KfMap(S, CAP, ECAP, MAX_FRAMES, TH_DIST, TH_COUNT, DEPTH_MIN, TBC)
    if tie_order is not None:
        gmap.set_tie_order(tie_order)
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
        assert len(held) == HELD[s], (s, held)
        cuts = np.cumsum([0] + held)
        obs.append([xyz[cuts[f]:cuts[f + 1]] for f in range(len(held))])
        edge.append([frames[f.stamp][s][1] for f in oracles[s].frames()])
    return gmap, obs, edge


@pytest.fixture(scope="module")
def flown():
    gmap, obs, edge = fly()
    yield gmap, obs, edge
    gmap.close()


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("k", [1, 8, 64])
def test_map_segment_nearest_merges_the_frames(flown, edge, k):
    import torch
    from avoid_mpc_amd import capi
    gmap, obs, edges = flown
    held = edges if edge else obs
    path = make_path(14)
    got = to_np(gmap.segment_nearest(torch.from_numpy(path).cuda(), k, edge=edge))
    torch.cuda.synchronize()
    want = N.expected_batch(held, path, k)
    N.assert_bitwise(got, want, MAP_KEYS, f"edge {edge}, k {k}")
    total = np.array([sum(len(f) for f in fr) for fr in held])
    assert np.array_equal(got["counts"], np.minimum(total, k)[:, None].repeat(NP - 1, axis=1))   # min(k, the frames' usable points)
    assert (got["counts"][3] == 0).all() and (got["frame"][3] == -1).all() and (got["sqdist"][3] == N.DBL_MAX).all() and (got["t"][3] == 0).all()
    assert ((got["t"] >= 0) & (got["t"] <= 1)).all()
    if k == 64:
        d, f = got["sqdist"], got["frame"]
        assert len(set(f[4].reshape(-1).tolist()) - {-1}) >= 2 and len(set(f[0].reshape(-1).tolist()) - {-1}) >= 2   # several frames answer
        ties = ((d[..., :-1] == d[..., 1:]) & (f[..., 1:] >= 0) & (f[..., :-1] < f[..., 1:])).sum()
        assert ties >= 1, ties                                             # equal distances across frames: the earlier frame first
        if edge:
            assert (got["counts"][2] == total[2]).all() and total[2] < 64  # fewer points than k over the frames: empty slots
    # the host variant
    L = NP - 1
    hp, hd, ht = np.zeros((S, L, k, 3), np.float32), np.zeros((S, L, k)), np.zeros((S, L, k))
    hf, hc = np.zeros((S, L, k), np.int32), np.zeros((S, L), np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    capi.check(gmap.lib.amk_kfmap_segment_nearest_host(gmap.h, vp(path), 14, NP, k, int(edge), vp(hp), vp(hd), vp(ht), vp(hf), vp(hc)),
               "amk_kfmap_segment_nearest_host")
    N.assert_bitwise(dict(pts=hp, sqdist=hd, t=ht, frame=hf, counts=hc), got, MAP_KEYS, "host")


def test_the_map_answers_like_its_segment_search_without_a_radius(flown):
    """identity 1 over the frames, on the device"""
    import torch
    gmap = flown[0]
    pd = torch.from_numpy(make_path(3)).cuda()
    for k in (1, 8, 64):
        got, seg = to_np(gmap.segment_nearest(pd, k)), to_np(gmap.segment_search(pd, float("inf"), k))
        torch.cuda.synchronize()
        N.assert_bitwise(got, seg, ("sqdist", "t", "frame", "pts"), f"k {k}")
        assert np.array_equal(got["counts"], np.minimum(seg["counts"], k))


@pytest.mark.parametrize("n_handles", [1, 3, 16])
def test_handle_lists_answer_like_the_brute_force(flown, n_handles):
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import segment_nearest_frames
    gmap, obs, _ = flown
    path, k = make_path(3), 8
    pd = torch.from_numpy(path).cuda()
    hs = handles_of(obs, n_handles, CAP)
    try:
        got = to_np(segment_nearest_frames(hs, pd, k))
        torch.cuda.synchronize()
        N.assert_bitwise(got, N.expected_batch([fr[:n_handles] for fr in obs], path, k), MAP_KEYS, f"{n_handles} handles")
        on_map = to_np(gmap.segment_nearest(pd, k))
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
        capi.check(capi.load().amk_kd_segment_nearest_frames_host(ha, n_handles, vp(path), 3, NP, k, vp(hp), vp(hd), vp(ht), vp(hf), vp(hc)),
                   "amk_kd_segment_nearest_frames_host")
        N.assert_bitwise(dict(pts=hp, sqdist=hd, t=ht, frame=hf, counts=hc), got, MAP_KEYS, "host")
    finally:
        for h in hs:
            h.close()


def test_truncation_across_a_frame_boundary_at_equal_distances():
    """the same cloud as two frames: every distance occurs in both, frame 0's entry first; an odd k ends between the two"""
    import torch
    from avoid_mpc_amd.host import segment_nearest_frames
    rng = np.random.default_rng(47)
    cloud = [[(rng.random((200, 3)) * 3.0).astype(np.float32)] * 2 for _ in range(S)]
    path = rng.random((S, 4, 3)) * 3.0
    hs = handles_of(cloud, 2, 200)
    try:
        got = to_np(segment_nearest_frames(hs, torch.from_numpy(path).cuda(), 7))
        torch.cuda.synchronize()
        N.assert_bitwise(got, N.expected_batch(cloud, path, 7), MAP_KEYS, "twice the same cloud")
        one = N.expected_batch([c[:1] for c in cloud], path, 7)
        assert (got["counts"] == 7).all()
        assert np.array_equal(got["frame"], np.tile([0, 1, 0, 1, 0, 1, 0], (S, 3, 1)))
        assert np.array_equal(got["sqdist"][..., 0::2], one["sqdist"][..., :4]) and np.array_equal(got["t"][..., 0::2], one["t"][..., :4])
    finally:
        for h in hs:
            h.close()


def test_a_map_in_nanoflann_tie_order_answers_identically(flown):
    import torch
    from avoid_mpc_amd import capi
    gmap = flown[0]
    other, _, _ = fly(capi.AMK_TIES_NANOFLANN)
    try:
        pd = torch.from_numpy(make_path(3)).cuda()
        for edge in (False, True):
            a, b = to_np(gmap.segment_nearest(pd, 8, edge=edge)), to_np(other.segment_nearest(pd, 8, edge=edge))
            torch.cuda.synchronize()
            N.assert_bitwise(b, a, MAP_KEYS, f"nanoflann order, edge {edge}")
    finally:
        other.close()


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

        def call(n, k=4, npts=4, stride=3, outs=True):
            ha = (C.c_void_p * n)(*[kd.h] * n)
            return lib.amk_kd_segment_nearest_frames(ha, n, capi.dptr(path), stride, npts, k, None, None, capi.dptr(tt) if outs else None, None,
                                                     capi.dptr(cnt) if outs else None, None)

        INV, UNS = capi.AMK_ERR_INVALID_ARG, capi.AMK_ERR_UNSUPPORTED
        assert call(17) == UNS and call(0) == INV and call(2, npts=1) == INV and call(2, stride=2) == INV and call(2, outs=False) == INV
        assert call(2, k=65) == UNS and call(2, k=0) == INV and call(2, k=-1) == INV
        capi.check(lib.amk__kd_set_mode(kd.h, 1), "scan mode")
        assert call(2) == UNS
        capi.check(lib.amk__kd_set_mode(kd.h, 0), "index mode")
        torch.cuda.synchronize()
        assert (cnt == -7).all() and (tt == -7).all()
        assert call(16) == capi.AMK_OK
        torch.cuda.synchronize()
        assert (cnt == 4).all() and ((tt >= 0) & (tt <= 1)).all()
    finally:
        kd.close()
