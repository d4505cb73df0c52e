"""GPU: amk_kd_query_frames / amk_kd_nearest_distance_frames (csrc/map_query.hip, the handle-list side of map_query_kernel) at
the edges the kernel can get wrong: a frame of exactly k points, a current frame of exactly k points, a current frame too small for
the fast path, an empty frame, equal distances across frames, the four sides of PtIsInFrame, one / five / seventy queries, the three
strides, k = 1 and k = 64 over 16 frames, every output NULL in turn, a NaN query between finite ones, and every error code.

Expected answers: tests/_map_query.py over _oracle.kd_brute_np.  Every comparison is bit-exact (the same fp64 sums as
amk_kd_search; the distance through a correctly rounded fp64 sqrt)."""
import ctypes as C

import numpy as np
import pytest

from tests import _map_query as mq

pytestmark = pytest.mark.gpu

S, F, CAP, K = 3, 3, 64, 4
CAM = (80.0, 80.0, 80.0, 60.0, 10.0, 160, 120)          # fx, fy, cx, cy, depth_max, width, height
POSE = mq.look_x_pose([0.0, 0.0, 1.0])                   # the camera at (0, 0, 1), looking along world +x
SIZES = [[40, 30, 4],                                    # A: the frame of exactly k points contributes nothing
         [4, 20, 25],                                    # B: a current frame of exactly k points
         [3, 5, 0]]                                      # C: always the merge path; only frame 1 answers
TIE_QUERY = np.array([-1.0, 2.5, 1.0])                   # behind the camera: merge path
# inside the frustum / behind the camera / beyond depth_max / outside the image sideways / the query next to the shared points
NAMED = np.array([[3.0, 0.5, 1.2], [-2.0, 0.0, 1.0], [12.0, 0.0, 1.0], [2.0, 5.0, 1.0], TIE_QUERY])


def make_clouds(sizes, seed=7, shared=(0, 1)):
    """clouds[f][s]: float32 [n, 3] in x [0, 10], y [-4, 4], z [0, 3]; frames shared[0] and shared[1] of scene 0 hold the same 6
    points next to TIE_QUERY (nearer to it than anything else)."""
    rng = np.random.default_rng(seed)
    nF = len(sizes[0])
    clouds = [[(rng.random((sizes[s][f], 3)) * [10, 8, 3] + [0, -4, 0]).astype(np.float32) for s in range(len(sizes))] for f in range(nF)]
    six = (TIE_QUERY + rng.normal(size=(6, 3)) * 0.05).astype(np.float32)
    for f in shared:
        clouds[f][0][:6] = six
    return clouds


def make_queries(Q, stride, seed=11):
    """[S, Q, stride]: the named queries first, then uniform ones in x [-3, 13], y [-6, 6], z [0, 3]; columns >= 3 hold junk"""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(S, Q, stride)) * 50.0
    q[:, :, :3] = rng.random((S, Q, 3)) * [16, 12, 3] + [-3, -6, 0]
    n = min(Q, len(NAMED))
    q[:, :n, :3] = NAMED[:n]
    return q


def build_handles(clouds, cap):
    import torch
    from avoid_mpc_amd.host import KdBatch
    hs = []
    for fr in clouds:
        xyz = np.zeros((len(fr), cap, 3), np.float32); cnt = np.zeros(len(fr), np.int32)
        for s, c in enumerate(fr):
            xyz[s, :len(c)] = c; cnt[s] = len(c)
        kd = KdBatch(len(fr), cap)
        kd.build(torch.from_numpy(xyz).cuda(), torch.from_numpy(cnt).cuda())
        hs.append(kd)
    torch.cuda.synchronize()
    return hs


def scene_frames(clouds):
    return [[mq.CloudFrame(clouds[f][s]) for f in range(len(clouds))] for s in range(len(clouds[0]))]


@pytest.fixture(scope="module")
def world():
    import torch
    clouds = make_clouds(SIZES)
    hs = build_handles(clouds, CAP)
    Twc = np.stack([POSE] * S)
    yield dict(clouds=clouds, handles=hs, frames=scene_frames(clouds), Twc=Twc, dTwc=torch.from_numpy(Twc).cuda())
    for h in hs:
        h.close()


def cam_struct():
    from avoid_mpc_amd import capi
    return capi.FrameCamera(*CAM)


def run(world, q, k, with_pose=True, **kw):
    import torch
    from avoid_mpc_amd import host
    out = host.query_frames(world["handles"], torch.from_numpy(q).cuda(), k, Twc=world["dTwc"] if with_pose else None,
                            cam=cam_struct() if with_pose else None, **kw)
    torch.cuda.synchronize()
    return out


def test_the_inputs_reach_the_edges(world):
    """The scenes and queries hold what the docstring says (so that no test below passes vacuously)."""
    q = make_queries(70, 3)
    e = mq.expected_batch(world["frames"], q, K, world["Twc"], CAM)
    inside = [mq.pt_in_frame(p, POSE, CAM) for p in NAMED]
    assert inside == [True, False, False, False, False]
    paths = np.array(e["path"])
    assert (paths[0] == "fast").sum() >= 5 and (paths[0] == "merge").sum() >= 5          # A: both paths
    assert (paths[1] == "fast").sum() >= 5 and (e["counts"][1][paths[1] == "fast"] == 0).all()   # B in frustum: count 0 ...
    assert (e["sqdist"][1][paths[1] == "fast"] == mq.DBL_MAX).all() and (e["frame"][1][paths[1] == "fast"] == -1).all()   # ... all empty
    assert set(np.unique(e["frame"][1][paths[1] == "merge"])) == {1, 2}                  # B out of frustum: frames 1 and 2
    assert (paths[2] == "merge").all() and set(np.unique(e["frame"][2])) == {1} and (e["counts"][2] == K).all()   # C: frame 1 only
    assert 2 not in np.unique(e["frame"][0])                                               # A's frame of exactly k points
    tie = e["sqdist"][0, 4]
    assert e["frame"][0, 4].tolist() == [0, 1, 0, 1] and tie[0] == tie[1] and tie[2] == tie[3]   # equal distances: earlier frame first


@pytest.mark.parametrize("Q", [1, 5, 70])
@pytest.mark.parametrize("stride", [3, 10, 14])
def test_query_frames(world, Q, stride):
    q = make_queries(Q, stride)
    mq.assert_query_equal(run(world, q, K), mq.expected_batch(world["frames"], q, K, world["Twc"], CAM), f"Q {Q} stride {stride}")


def test_without_pose_every_query_with_enough_points_takes_the_fast_path(world):
    q = make_queries(70, 3)
    e = mq.expected_batch(world["frames"], q, K, None, None)
    paths = np.array(e["path"])
    assert (paths[0] == "fast").all() and (paths[1] == "fast").all() and (paths[2] == "merge").all()
    mq.assert_query_equal(run(world, q, K, with_pose=False), e, "d_Twc = NULL")


def test_k_1(world):
    q = make_queries(70, 3)
    mq.assert_query_equal(run(world, q, 1), mq.expected_batch(world["frames"], q, 1, world["Twc"], CAM), "k = 1")


def test_equal_distances_keep_frame_1_before_frame_2():
    """Frames 1 and 2 of scene A hold the same 6 points next to the query; sizes 40 / 30 / 30 so that both contribute."""
    import torch
    from avoid_mpc_amd import host
    sizes = [[40, 30, 30], [4, 20, 25], [3, 5, 0]]
    clouds = make_clouds(sizes, seed=8, shared=(1, 2))
    hs = build_handles(clouds, CAP)
    try:
        q = make_queries(5, 3)
        Twc = np.stack([POSE] * S)
        e = mq.expected_batch(scene_frames(clouds), q, K, Twc, CAM)
        assert e["frame"][0, 4].tolist() == [1, 2, 1, 2] and e["sqdist"][0, 4, 0] == e["sqdist"][0, 4, 1]
        out = host.query_frames(hs, torch.from_numpy(q).cuda(), K, Twc=torch.from_numpy(Twc).cuda(), cam=cam_struct())
        torch.cuda.synchronize()
        mq.assert_query_equal(out, e, "frames 1 and 2 tie")
    finally:
        for h in hs:
            h.close()


def test_k_64_over_16_frames_of_70_points():
    """1024 candidates per merged query; in-frustum queries answer from frame 0's 64 nearest of 70."""
    import torch
    from avoid_mpc_amd import host
    clouds = make_clouds([[70] * 16] * S, seed=9)
    hs = build_handles(clouds, 128)
    try:
        q = make_queries(9, 3)
        Twc = np.stack([POSE] * S)
        e = mq.expected_batch(scene_frames(clouds), q, 64, Twc, CAM)
        paths = np.array(e["path"])
        assert (paths == "fast").sum() >= 3 and (paths == "merge").sum() >= 12
        assert max(len(np.unique(r)) for r in e["frame"].reshape(-1, 64)) >= 12      # a merged row draws on most of the 16 frames
        out = host.query_frames(hs, torch.from_numpy(q).cuda(), 64, Twc=torch.from_numpy(Twc).cuda(), cam=cam_struct())
        torch.cuda.synchronize()
        mq.assert_query_equal(out, e, "k = 64, 16 frames")
    finally:
        for h in hs:
            h.close()


@pytest.mark.parametrize("absent", ["pts", "sqdist", "frame", "counts"])
def test_each_output_may_be_null(world, absent):
    import torch
    q = make_queries(5, 3)
    e = mq.expected_batch(world["frames"], q, K, world["Twc"], CAM)
    dev = torch.device("cuda")
    out = dict(pts=torch.empty((S, 5, K, 3), dtype=torch.float32, device=dev), sqdist=torch.empty((S, 5, K), dtype=torch.float64, device=dev),
               frame=torch.empty((S, 5, K), dtype=torch.int32, device=dev), counts=torch.empty((S, 5), dtype=torch.int32, device=dev))
    out[absent] = None
    mq.assert_query_equal(run(world, q, K, out=out), e, absent + " = NULL")


def test_a_nan_query_among_finite_ones(world):
    q = make_queries(5, 3)
    e0 = mq.expected_batch(world["frames"], q, K, world["Twc"], CAM)
    qn = q.copy()
    qn[:, 2, 1] = np.nan
    qn[1, 3, 0] = np.inf
    e = mq.expected_batch(world["frames"], qn, K, world["Twc"], CAM)
    out = run(world, qn, K)
    mq.assert_query_equal(out, e, "NaN query")
    d2, fr, pts = out["sqdist"].cpu().numpy(), out["frame"].cpu().numpy(), out["pts"].cpu().numpy()
    assert (d2[:, 2] == mq.DBL_MAX).all() and (fr[:, 2] == -1).all() and (pts[:, 2] == 0).all() and (d2[1, 3] == mq.DBL_MAX).all()
    keep = [0, 1, 4]
    assert np.array_equal(d2[:, keep], e0["sqdist"][:, keep]) and np.array_equal(fr[:, keep], e0["frame"][:, keep])   # the neighbours' rows


@pytest.mark.parametrize("Q,stride", [(1, 3), (70, 14)])
def test_nearest_distance_frames(world, Q, stride):
    import torch
    from avoid_mpc_amd import host
    q = make_queries(Q, stride)
    d = host.nearest_distance_frames(world["handles"], torch.from_numpy(q).cuda())
    torch.cuda.synchronize()
    e = mq.expected_distance(world["frames"], q)
    assert (e < 20).all()
    assert np.array_equal(d.cpu().numpy().view(np.int64), e.view(np.int64))


def test_nearest_distance_when_no_frame_holds_more_than_one_point():
    import torch
    from avoid_mpc_amd import host
    clouds = make_clouds([[1, 0, 1], [0, 0, 0], [1, 1, 1]], shared=())
    hs = build_handles(clouds, CAP)
    try:
        q = make_queries(5, 3)
        d = host.nearest_distance_frames(hs, torch.from_numpy(q).cuda())
        torch.cuda.synchronize()
        assert (d.cpu().numpy() == mq.SQRT_DBL_MAX).all()
        out = host.query_frames(hs, torch.from_numpy(q).cuda(), 1)
        torch.cuda.synchronize()
        assert (out["counts"].cpu().numpy() == 0).all() and (out["frame"].cpu().numpy() == -1).all()
    finally:
        for h in hs:
            h.close()


def test_host_variant(world):
    from avoid_mpc_amd import capi
    q = make_queries(5, 10)
    pts = np.zeros((S, 5, K, 3), np.float32); d2 = np.zeros((S, 5, K)); fr = np.zeros((S, 5, K), np.int32); cnt = np.zeros((S, 5), np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    ha = (C.c_void_p * F)(*[h.h for h in world["handles"]])
    cam = cam_struct()
    Twc = np.ascontiguousarray(world["Twc"])
    qq = np.ascontiguousarray(q.reshape(-1)[:(S * 5 - 1) * 10 + 3])     # the shortest buffer the header allows
    capi.check(capi.load().amk_kd_query_frames_host(ha, F, vp(Twc), C.byref(cam), vp(qq), 10, 5, K, vp(pts), vp(d2), vp(fr), vp(cnt)), "host")
    mq.assert_query_equal(dict(pts=pts, sqdist=d2, frame=fr, counts=cnt), mq.expected_batch(world["frames"], q, K, world["Twc"], CAM), "host variant")


def test_error_codes(world):
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import KdBatch
    lib = capi.load()
    hs = world["handles"]
    q = torch.from_numpy(make_queries(5, 3)).cuda()
    d2 = torch.empty((S, 5, 64), dtype=torch.float64, device="cuda")
    dist = torch.empty((S, 5), dtype=torch.float64, device="cuda")
    cam = cam_struct()

    def query(handles, k=K, Twc=None, camp=None, nq=5, stride=3):
        ha = (C.c_void_p * len(handles))(*[h.h for h in handles])
        return lib.amk_kd_query_frames(ha, len(handles), capi.dptr(Twc), camp, capi.dptr(q), stride, nq, k, None, capi.dptr(d2), None, None,
                                       capi.stream_ptr())

    def distance(handles):
        ha = (C.c_void_p * len(handles))(*[h.h for h in handles])
        return lib.amk_kd_nearest_distance_frames(ha, len(handles), capi.dptr(q), 3, 5, capi.dptr(dist), capi.stream_ptr())

    assert query(hs) == capi.AMK_OK and distance(hs) == capi.AMK_OK
    assert query([hs[0]] * 16) == capi.AMK_OK
    assert query([hs[0]] * 17) == capi.AMK_ERR_UNSUPPORTED and distance([hs[0]] * 17) == capi.AMK_ERR_UNSUPPORTED
    assert query(hs, k=0) == capi.AMK_ERR_INVALID_ARG
    assert query(hs, k=64) == capi.AMK_OK and query(hs, k=65) == capi.AMK_ERR_UNSUPPORTED
    assert query(hs, nq=0) == capi.AMK_ERR_INVALID_ARG and query(hs, stride=2) == capi.AMK_ERR_INVALID_ARG
    assert query(hs, Twc=world["dTwc"]) == capi.AMK_ERR_INVALID_ARG                           # d_Twc without cam
    assert query(hs, Twc=world["dTwc"], camp=C.byref(cam)) == capi.AMK_OK
    other = KdBatch(S + 1, CAP)
    try:
        assert query([hs[0], other]) == capi.AMK_ERR_INVALID_ARG and distance([hs[0], other]) == capi.AMK_ERR_INVALID_ARG   # scene counts differ
    finally:
        other.close()
    for mode in (capi.AMK_TIES_NANOFLANN, capi.AMK_TIES_AUTO):
        t = KdBatch(S, CAP)
        try:
            t.set_tie_order(mode)
            assert query([hs[0], t]) == capi.AMK_ERR_UNSUPPORTED and distance([t]) == capi.AMK_ERR_UNSUPPORTED
        finally:
            t.close()
    scan = KdBatch(S, CAP)
    try:
        capi.check(lib.amk__kd_set_mode(scan.h, 1), "scan mode")
        assert query([scan, hs[1]]) == capi.AMK_ERR_UNSUPPORTED and distance([hs[0], scan]) == capi.AMK_ERR_UNSUPPORTED
    finally:
        scan.close()
    torch.cuda.synchronize()
