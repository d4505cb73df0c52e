"""GPU: the path cast over the frames -- amk_kfmap_path_cast on a keyframe map and amk_kd_path_cast_frames on a list of handles
(map_path_cast_kernel, csrc/map_query.hip) -- against the restatement of tests/_path_cast.py over the frames each scene holds AND
against the reduction of the map's own segment cast (the identity the header states).

The map is the one tests/test_kfmap_segment_gpu.py flies (its fixture and paths are imported, with the rays of the segment cast's
test): the scenes hold 4, 2, 1, 0 and 3 frames of different sizes.  Every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests import _path_cast as P
from tests.test_kfmap_segment_cast_gpu import make_rays, three_frames
from tests.test_kfmap_segment_gpu import CAP, HELD, S, flown, handles_of, make_path, to_np  # noqa: F401

pytestmark = pytest.mark.gpu

SEG = ("hit", "t", "frame", "pts")


def host_buffers():
    i32 = lambda: np.zeros(S, np.int32)
    return dict(stop=i32(), leg=i32(), t=np.zeros(S), free=np.zeros(S), pts=np.zeros((S, 3), np.float32), frame=i32())


def host_args(h):
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    return [vp(h[k]) for k in ("stop", "leg", "t", "free", "pts", "frame")]


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("rays", [False, True])
def test_map_path_cast_is_the_reduction_over_all_frames(flown, edge, rays):
    import torch
    from avoid_mpc_amd import capi
    gmap, obs, edges = flown
    assert sorted(HELD) == [0, 1, 2, 3, 4]
    held = edges if edge else obs
    path = make_rays(14) if rays else make_path(14)
    npts = path.shape[1]
    r2 = 1.0 if edge else 0.25
    before = gmap.state()
    pd = torch.from_numpy(path).cuda()
    got = to_np(gmap.path_cast(pd, r2, edge=edge))
    legs = to_np(gmap.segment_cast(pd, r2, edge=edge))
    torch.cuda.synchronize()
    want = P.expected_batch(held, path, r2)
    P.assert_bitwise(got, want, P.KEYS_FRAMES, f"edge {edge}, rays {rays}: specification")
    P.assert_bitwise(got, P.reduce_legs({k: legs[k] for k in SEG}, path), P.KEYS_FRAMES, f"edge {edge}, rays {rays}: reduction")
    # the scene that holds no frame is free to the end, whole length; the one that holds one frame answers from it
    assert got["stop"][3] == 0 and got["leg"][3] == -1 and got["frame"][3] == -1 and got["t"][3] == 1.0 and (got["pts"][3] == 0).all()
    acc = np.float64(0.0)
    for v in P.leg_lengths(path)[3]:
        acc = acc + v
    assert got["free"][3] == acc
    assert got["stop"][2] == 1 and set(got["frame"][got["stop"] == 1].tolist()) <= set(range(4))
    after = gmap.state()
    for key in before:
        assert np.array_equal(before[key], after[key]), key      # no map state changed
    h = host_buffers()
    capi.check(gmap.lib.amk_kfmap_path_cast_host(gmap.h, path.ctypes.data_as(C.c_void_p), 14, npts, r2, int(edge), *host_args(h)),
               "amk_kfmap_path_cast_host")
    P.assert_bitwise(h, got, P.KEYS_FRAMES, "host")


@pytest.mark.parametrize("n_handles", [1, 3])
def test_handle_lists_answer_like_the_restatement(flown, n_handles):
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import path_cast_frames
    gmap, obs, _ = flown
    path, r2 = make_rays(3), 0.25
    pd = torch.from_numpy(path).cuda()
    hs = handles_of(obs, n_handles, CAP)
    try:
        got = to_np(path_cast_frames(hs, pd, r2))
        torch.cuda.synchronize()
        P.assert_bitwise(got, P.expected_batch([fr[:n_handles] for fr in obs], path, r2), P.KEYS_FRAMES, f"{n_handles} handles")
        on_map = to_np(gmap.path_cast(pd, r2))
        torch.cuda.synchronize()
        same = [s for s in range(S) if HELD[s] <= n_handles]      # the scenes whose whole map the handles hold
        assert len(same) >= 2
        for key in P.KEYS_FRAMES:
            assert np.array_equal(got[key][same], on_map[key][same]), key
        if n_handles == 1:                                        # one frame: the single-handle call
            one = to_np(hs[0].path_cast(pd, r2))
            torch.cuda.synchronize()
            P.assert_bitwise(got, one, ("stop", "leg", "t", "free", "pts"), "n_frames = 1")
            assert np.array_equal(got["frame"], np.where(one["indices"] >= 0, 0, -1)) and (one["stop"] == 1).any()
        h = host_buffers()
        ha = (C.c_void_p * n_handles)(*[k.h for k in hs])
        capi.check(capi.load().amk_kd_path_cast_frames_host(ha, n_handles, path.ctypes.data_as(C.c_void_p), 3, path.shape[1], r2, *host_args(h)),
                   "amk_kd_path_cast_frames_host")
        P.assert_bitwise(h, got, P.KEYS_FRAMES, "host")
    finally:
        for k in hs:
            k.close()


def test_three_frames_of_different_sizes_and_a_scene_that_holds_fewer():
    """scenes of 3, 2, 1, 0 and 3 frames; the 10 m rays of the sibling's test joined into one path per scene"""
    import torch
    from avoid_mpc_amd.host import path_cast_frames
    frames, path = three_frames()
    hs = handles_of(frames, 3, 300)
    try:
        for r2 in (0.0025, 0.25):
            got = to_np(path_cast_frames(hs, torch.from_numpy(path).cuda(), r2))
            torch.cuda.synchronize()
            P.assert_bitwise(got, P.expected_batch(frames, path, r2), P.KEYS_FRAMES, f"three frames, r2 {r2}")
            assert got["stop"][3] == 0 and got["frame"][3] == -1
        assert (got["stop"][[0, 1, 2, 4]] == 1).all() and len(set(got["frame"].tolist()) - {-1}) >= 2
    finally:
        for k in hs:
            k.close()


def test_the_same_cloud_in_two_frames_keeps_the_earlier_frame():
    """the same cloud as two frames: every contact occurs in both at the same t, and the answer names frame 0"""
    import torch
    from avoid_mpc_amd.host import path_cast_frames
    rng = np.random.default_rng(47)
    twice = [[(rng.random((200, 3)) * 3.0).astype(np.float32)] * 2 for _ in range(S)]
    path = rng.random((S, 6, 3)) * 5.0 - 1.0
    hs = handles_of(twice, 2, 200)
    try:
        got = to_np(path_cast_frames(hs, torch.from_numpy(path).cuda(), 0.04))
        torch.cuda.synchronize()
        P.assert_bitwise(got, P.expected_batch(twice, path, 0.04), P.KEYS_FRAMES, "twice the same cloud")
        P.assert_bitwise(got, P.expected_batch([c[:1] for c in twice], path, 0.04), P.KEYS_FRAMES, "as one frame")
        assert (got["frame"][got["stop"] == 1] == 0).all() and (got["stop"] == 1).sum() >= 2
    finally:
        for k in hs:
            k.close()


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
        stop = torch.full((2,), -7, dtype=torch.int32, device="cuda"); free = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
        hq, hstop = np.zeros((2, 4, 3)), np.full(2, -7, np.int32)

        def call(n, r2=1.0, npts=4, stride=3, outs=True, second=None):
            ha = (C.c_void_p * n)(*([kd.h] * n if second is None else [kd.h, second.h]))
            return lib.amk_kd_path_cast_frames(ha, n, capi.dptr(path), stride, npts, r2, capi.dptr(stop) if outs else None, None, None,
                                               capi.dptr(free) if outs else None, None, None, None)

        def hcall(n, r2=1.0, npts=4, outs=True, second=None):
            ha = (C.c_void_p * n)(*([kd.h] * n if second is None else [kd.h, second.h]))
            return lib.amk_kd_path_cast_frames_host(ha, n, hq.ctypes.data_as(C.c_void_p), 3, npts, r2,
                                                    hstop.ctypes.data_as(C.c_void_p) if outs else None, None, None, None, None, None)

        INV, UNS = capi.AMK_ERR_INVALID_ARG, capi.AMK_ERR_UNSUPPORTED
        assert call(17) == UNS and call(0) == INV and call(2, npts=1) == INV and call(2, stride=2) == INV and call(2, outs=False) == INV
        assert call(2, r2=-1.0) == INV and call(2, r2=float("nan")) == INV and call(2, second=tied) == UNS
        assert hcall(17) == UNS and hcall(2, npts=1) == INV and hcall(2, r2=-1.0) == INV and hcall(2, outs=False) == INV
        assert hcall(2, second=tied) == UNS
        capi.check(lib.amk__kd_set_mode(kd.h, 1), "scan mode")
        assert call(2) == UNS and hcall(2) == UNS
        capi.check(lib.amk__kd_set_mode(kd.h, 0), "index mode")
        torch.cuda.synchronize()
        assert (stop == -7).all() and (free == -7).all() and (hstop == -7).all()
        assert call(16) == capi.AMK_OK and call(2, r2=0.0) == capi.AMK_OK and call(2, r2=float("inf")) == capi.AMK_OK
        torch.cuda.synchronize()
        assert (stop == 1).all() and (free == 0).all()     # radius_sq = +inf: every point is inside at the start of leg 0
    finally:
        kd.close(); tied.close()
