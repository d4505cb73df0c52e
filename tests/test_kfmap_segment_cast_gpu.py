"""GPU: the segment cast over the frames -- amk_kfmap_segment_cast on a keyframe map and amk_kd_segment_cast_frames on a list of
handles (map_segment_cast_kernel, csrc/map_query.hip) -- against the brute force of tests/_cast.py over the frames each scene holds.

The map is the one tests/test_kfmap_segment_gpu.py flies (its fixture, flight and path are imported): the scenes hold 4, 2, 1, 0 and
3 frames of different sizes, scene 0's current frame has 4 200 points, clouds and paths are quantised.  Beside its 1 m legs a path of
6 m rays crosses the region.  Every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests import _cast as K
from tests.test_kfmap_segment_gpu import CAP, HELD, NP, PERIODS, QUANTUM, S, STEP, flown, handles_of, make_path, to_np  # noqa: F401

pytestmark = pytest.mark.gpu

MAP_KEYS = ("hit", "t", "frame", "pts")


def make_rays(stride=3):
    """8 points per scene: legs 0, 2, 4 and 6 are 6 m rays through the region the frames cover, quantised to QUANTUM / 2"""
    rng = np.random.default_rng(53)
    path = rng.normal(size=(S, 8, stride)) * 20.0
    d = STEP * (PERIODS - 1)
    a = rng.random((S, 4, 3)) * [3.0, 6.0, 2.0] + [d + 1.0, -3.0, 0.5]
    u = rng.normal(size=(S, 4, 3)) * [1.0, 1.0, 0.15]
    u[..., 0] = np.abs(u[..., 0]) + 0.5
    b = a + 6.0 * u / np.linalg.norm(u, axis=-1)[..., None]
    path[:, :, :3] = np.round(np.stack([a, b], axis=2).reshape(S, 8, 3) / (QUANTUM / 2)) * (QUANTUM / 2)
    return path


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("rays", [False, True])
def test_map_cast_takes_the_first_contact_of_all_frames(flown, edge, rays):
    import torch
    from avoid_mpc_amd import capi
    gmap, obs, edges = flown
    held = edges if edge else obs
    path = make_rays(14) if rays else make_path(14)
    npts = path.shape[1]
    r2 = 1.0 if edge else 0.25
    before = gmap.state()
    got = to_np(gmap.segment_cast(torch.from_numpy(path).cuda(), r2, edge=edge))
    torch.cuda.synchronize()
    want = K.expected_batch(held, path, r2)
    K.assert_bitwise(got, want, MAP_KEYS, f"edge {edge}, rays {rays}")
    assert (got["hit"][3] == 0).all() and (got["frame"][3] == -1).all() and (got["t"][3] == 1.0).all() and (got["pts"][3] == 0).all()
    assert ((got["t"] >= 0) & (got["t"] <= 1)).all() and ((got["t"] < 1) == (got["hit"] == 1)).all()
    assert (got["hit"][2] == 1).any()                                       # the scene that holds one frame answers
    if rays:
        f = got["frame"]
        assert len(set(f.reshape(-1).tolist()) - {-1}) >= 2, f                     # several frames answer
        # a contact in an older frame that begins earlier than the current frame's wins
        later = [(s, j) for s in (0, 1, 4) for j in range(npts - 1)
                 if f[s, j] >= 1 and K.cast_brute(held[s][0], path[s, j], path[s, j + 1], r2)["hit"] == 1]
        assert later or edge, f
        for s, j in later:
            assert got["t"][s, j] < K.cast_brute(held[s][0], path[s, j], path[s, j + 1], r2)["t"]
    # no map state changed
    after = gmap.state()
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    # the host variant
    L = npts - 1
    hh, ht, hp, hf = np.zeros((S, L), np.int32), np.zeros((S, L)), np.zeros((S, L, 3), np.float32), np.zeros((S, L), np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    capi.check(gmap.lib.amk_kfmap_segment_cast_host(gmap.h, vp(path), 14, npts, r2, int(edge), vp(hh), vp(ht), vp(hp), vp(hf)),
               "amk_kfmap_segment_cast_host")
    K.assert_bitwise(dict(hit=hh, t=ht, pts=hp, frame=hf), got, MAP_KEYS, "host")


@pytest.mark.parametrize("n_handles", [1, 3, 16])
def test_handle_lists_answer_like_the_brute_force(flown, n_handles):
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import segment_cast_frames
    gmap, obs, _ = flown
    path, r2 = make_rays(3), 0.25
    pd = torch.from_numpy(path).cuda()
    hs = handles_of(obs, n_handles, CAP)
    try:
        got = to_np(segment_cast_frames(hs, pd, r2))
        torch.cuda.synchronize()
        K.assert_bitwise(got, K.expected_batch([fr[:n_handles] for fr in obs], path, r2), MAP_KEYS, f"{n_handles} handles")
        on_map = to_np(gmap.segment_cast(pd, r2))
        torch.cuda.synchronize()
        same = [s for s in range(S) if HELD[s] <= n_handles]      # the scenes whose whole map the handles hold
        assert len(same) >= 2
        for key in MAP_KEYS:
            assert np.array_equal(got[key][same], on_map[key][same]), key
        if n_handles == 1:                                        # one frame: the single-handle call
            one = to_np(hs[0].segment_cast(pd, r2))
            torch.cuda.synchronize()
            K.assert_bitwise(got, one, ("hit", "t", "pts"), "n_frames = 1")
            assert np.array_equal(got["frame"], np.where(one["indices"] >= 0, 0, -1)) and (one["hit"] == 1).any()
        # the host variant of the handle list
        L = path.shape[1] - 1
        hh, ht, hp, hf = np.zeros((S, L), np.int32), np.zeros((S, L)), np.zeros((S, L, 3), np.float32), np.zeros((S, L), np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        ha = (C.c_void_p * n_handles)(*[h.h for h in hs])
        capi.check(capi.load().amk_kd_segment_cast_frames_host(ha, n_handles, vp(path), 3, path.shape[1], r2, vp(hh), vp(ht), vp(hp), vp(hf)),
                   "amk_kd_segment_cast_frames_host")
        K.assert_bitwise(dict(hit=hh, t=ht, pts=hp, frame=hf), got, MAP_KEYS, "host")
    finally:
        for h in hs:
            h.close()


def three_frames():
    """per scene up to three frames of different sizes (300, 120 and 40 points); frame 2 lies in front of the others, so rays
    heading +x meet it first; scene 1 holds two frames, scene 2 one, scene 3 none.  -> (frames per scene, path [S, 8, 3])"""
    rng = np.random.default_rng(61)
    frames = []
    for s, held in enumerate([3, 2, 1, 0, 3]):
        f0 = rng.random((300, 3)) * [6.0, 6.0, 3.0] + [4.0, -3.0, 0.0]
        f1 = rng.random((120, 3)) * [6.0, 6.0, 3.0] + [3.0, -3.0, 0.0]
        f2 = rng.random((40, 3)) * [2.0, 6.0, 3.0] + [1.0, -3.0, 0.0]
        frames.append([f.astype(np.float32) for f in (f0, f1, f2)][:held])
    a = rng.random((S, 4, 3)) * [0.5, 4.0, 2.0] + [-0.5, -2.0, 0.5]
    b = rng.random((S, 4, 3)) * [1.0, 4.0, 2.0] + [10.0, -2.0, 0.5]
    return frames, np.stack([a, b], axis=2).reshape(S, 8, 3)


def test_three_frames_of_different_sizes_and_a_scene_that_holds_fewer():
    """a contact in frame 2 that begins earlier than one in frame 0 wins; the scenes holding two, one and no frame answer from what
    they hold"""
    import torch
    from avoid_mpc_amd.host import segment_cast_frames
    frames, path = three_frames()
    hs = handles_of(frames, 3, 300)
    try:
        for r2 in (0.25, 0.49):
            got = to_np(segment_cast_frames(hs, torch.from_numpy(path).cuda(), r2))
            torch.cuda.synchronize()
            K.assert_bitwise(got, K.expected_batch(frames, path, r2), MAP_KEYS, f"three frames, r2 {r2}")
            f = got["frame"]
            assert (f[3] == -1).all() and (got["hit"][3] == 0).all() and set(f[2].tolist()) <= {0, -1} and set(f[1].tolist()) <= {0, 1, -1}
            assert (f[2] == 0).any() and (f[1] == 1).any()
            won = [(s, j) for s in (0, 4) for j in range(0, 7, 2)
                   if f[s, j] == 2 and K.cast_brute(frames[s][0], path[s, j], path[s, j + 1], r2)["hit"] == 1]
            assert won, f
            for s, j in won:
                assert got["t"][s, j] < K.cast_brute(frames[s][0], path[s, j], path[s, j + 1], r2)["t"]
            assert {0, 2} <= set(f[[0, 4]].reshape(-1).tolist())
    finally:
        for h in hs:
            h.close()


def test_the_same_point_in_two_frames_keeps_the_earlier_frame():
    """the same cloud as two frames: every contact occurs in both at the same t, and the answer names frame 0"""
    import torch
    from avoid_mpc_amd.host import segment_cast_frames
    rng = np.random.default_rng(47)
    twice = [[(rng.random((200, 3)) * 3.0).astype(np.float32)] * 2 for _ in range(S)]
    path = rng.random((S, 4, 3)) * 5.0 - 1.0
    hs = handles_of(twice, 2, 200)
    try:
        got = to_np(segment_cast_frames(hs, torch.from_numpy(path).cuda(), 0.04))
        torch.cuda.synchronize()
        K.assert_bitwise(got, K.expected_batch(twice, path, 0.04), MAP_KEYS, "twice the same cloud")
        one = K.expected_batch([c[:1] for c in twice], path, 0.04)
        K.assert_bitwise(got, one, MAP_KEYS, "as one frame")
        assert (got["frame"][got["hit"] == 1] == 0).all() and 3 <= (got["hit"] == 1).sum() < got["hit"].size
    finally:
        for h in hs:
            h.close()


def test_bad_arguments_scan_mode_and_tie_order_handles_are_refused():
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import KdBatch
    lib = capi.load()
    kd, tied = KdBatch(2, 32), KdBatch(2, 32)
    try:
        tied.set_tie_order(capi.AMK_TIES_NANOFLANN)
        kd.build(torch.rand((2, 32, 3), device="cuda")); tied.build(torch.rand((2, 32, 3), device="cuda"))
        path = torch.rand((2, 4, 3), dtype=torch.float64, device="cuda")
        hit = torch.full((2, 3), -7, dtype=torch.int32, device="cuda"); tt = torch.full((2, 3), -7.0, dtype=torch.float64, device="cuda")
        hq, hhit = np.zeros((2, 4, 3)), np.full((2, 3), -7, np.int32)

        def call(n, r2=1.0, npts=4, stride=3, outs=True, second=None):
            ha = (C.c_void_p * n)(*([kd.h] * n if second is None else [kd.h, second.h]))
            return lib.amk_kd_segment_cast_frames(ha, n, capi.dptr(path), stride, npts, r2, capi.dptr(hit) if outs else None,
                                                  capi.dptr(tt) if outs else None, None, None, None)

        def hcall(n, r2=1.0, npts=4, outs=True, second=None):
            ha = (C.c_void_p * n)(*([kd.h] * n if second is None else [kd.h, second.h]))
            return lib.amk_kd_segment_cast_frames_host(ha, n, hq.ctypes.data_as(C.c_void_p), 3, npts, r2,
                                                       hhit.ctypes.data_as(C.c_void_p) if outs else None, None, None, None)

        INV, UNS = capi.AMK_ERR_INVALID_ARG, capi.AMK_ERR_UNSUPPORTED
        assert call(17) == UNS and call(0) == INV and call(2, npts=1) == INV and call(2, stride=2) == INV and call(2, outs=False) == INV
        assert call(2, r2=-1.0) == INV and call(2, r2=float("nan")) == INV and call(2, second=tied) == UNS
        assert hcall(17) == UNS and hcall(2, npts=1) == INV and hcall(2, r2=-1.0) == INV and hcall(2, outs=False) == INV
        assert hcall(2, second=tied) == UNS
        capi.check(lib.amk__kd_set_mode(kd.h, 1), "scan mode")
        assert call(2) == UNS and hcall(2) == UNS
        capi.check(lib.amk__kd_set_mode(kd.h, 0), "index mode")
        torch.cuda.synchronize()
        assert (hit == -7).all() and (tt == -7).all() and (hhit == -7).all()
        assert call(16) == capi.AMK_OK and call(2, r2=0.0) == capi.AMK_OK and call(2, r2=float("inf")) == capi.AMK_OK
        torch.cuda.synchronize()
        assert (hit == 1).all() and (tt == 0).all()     # radius_sq = +inf: every point is inside at the start
    finally:
        kd.close(); tied.close()
