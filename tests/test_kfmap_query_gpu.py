"""GPU: FrameKDMap's QueryNearest, GetNearestDistance and GetPtCloud on the keyframe map (amk_kfmap_query_nearest,
amk_kfmap_nearest_distance, amk_kfmap_points_host; the map side of map_query_kernel, csrc/map_query.hip) and through a
pipeline slot (Pipeline.kfmap_query).

Five scenes fly for a few periods, fed straight to add_vertex + update and mirrored in tests/_kfmap.MapOracle; the expected
answers are tests/_map_query.py over the oracle's trees.  Scene 3's last frame holds exactly K points (fast path, count 0), scene 4
never gets a frame.  Every comparison is bit-exact; the test asserts about its own inputs that both paths, multi-frame merges and
equal distances across frames occur."""
import ctypes as C

import numpy as np
import pytest

from tests import _map_query as mq

pytestmark = pytest.mark.gpu

S, CAP, ECAP, NQ = 5, 512, 128, 16
CAM = (80.0, 80.0, 80.0, 60.0, 10.0, 160, 120)
TH_DIST, TH_COUNT, DEPTH_MIN = 0.3, 1, 0.3
TBC = mq.look_x_pose([0.0, 0.0, 0.0])
# (quantum, max_frame_count, periods, step, K)
CONFIGS = [(0.25, 3, 6, 0.8, 8),      # pops by length and by DroneBehindPts
           (0.25, 100, 14, 0.15, 8),
           (None, 100, 14, 0.15, 10),
           (0.25, 100, 40, 0.05, 8)]  # 34-38 query frames per scene: more than 16 frames, more than 64 candidates per lane-list


def pose(d):
    Twb = np.eye(4)
    Twb[:3, 3] = [d, 0.0, 1.5]
    return Twb @ TBC


def flight(quantum, periods, step, K):
    """frames[t][s] = (cloud [n, 3] f32, edge [n // 6, 3] f32, Twc) -- scene 4: empty clouds, never a frame"""
    rngs = [np.random.default_rng(100 + s) for s in range(S)]
    frames = []
    for t in range(periods):
        d = step * t
        row = []
        for s in range(S):
            rng = rngs[s]
            n = int(rng.integers(300, 512))
            box = lambda m: rng.random((m, 3)) * [7.0, 8.0, 3.0] + [d + 2.0, -4.0, 0.0]
            cloud, edge = box(n), box(n // 6)
            if quantum:
                cloud, edge = np.round(cloud / quantum) * quantum, np.round(edge / quantum) * quantum
            if s == 3 and t == periods - 1:
                cloud = cloud[:K]
            if s == 4:
                cloud, edge = cloud[:0], edge[:0]
            row.append((cloud.astype(np.float32), edge.astype(np.float32), pose(d)))
        frames.append(row)
    return frames


def make_queries(d, quantum, seed, stride=3):
    """[S, 16, stride] around a drone at (d, 0, 1.5): 8 ahead (inside the frustum), 4 behind or beside it, 4 far to the side"""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(S, NQ, stride)) * 30.0
    for s in range(S):
        ax = np.arange(8) + 1.5 + rng.random(8) * 0.5
        ahead = np.stack([d + ax, (rng.random(8) - 0.5) * ax, 1.5 + (rng.random(8) - 0.5) * 0.8 * np.minimum(ax, 3.0)], axis=1)
        near = np.array([[d - 1.0, 0.5, 1.5], [d - 3.0, -1.0, 1.0], [d + 0.2, 2.0, 1.5], [d - 0.5, -2.0, 2.0]]) + rng.random((4, 3)) * 0.2
        side = np.array([[d + 3.0, 9.0, 1.5], [d + 5.0, -10.0, 1.0], [d + 1.0, 6.0, 2.0], [d + 7.0, -12.0, 0.5]]) + rng.random((4, 3)) * 0.2
        q[s, :, :3] = np.concatenate([ahead, near, side])
    if quantum:
        q[:, :, :3] = np.round(q[:, :, :3] / (quantum / 2)) * (quantum / 2)
    return q


def new_oracles(max_frames):
    from tests import _kfmap
    return [_kfmap.MapOracle(max_frames, TH_DIST, TH_COUNT, DEPTH_MIN, TBC) for _ in range(S)]


def feed_oracle(oracles, row):
    for s, (c, e, T) in enumerate(row):
        oracles[s].add_vertex(c, e, T)
        oracles[s].update()


def pack(row):
    import torch
    cl = np.zeros((S, CAP, 3), np.float32); ed = np.zeros((S, ECAP, 3), np.float32)
    cn = np.zeros(S, np.int32); en = np.zeros(S, np.int32); Tw = np.zeros((S, 4, 4))
    for s, (c, e, T) in enumerate(row):
        cl[s, :len(c)] = c; cn[s] = len(c); ed[s, :len(e)] = e; en[s] = len(e); Tw[s] = T
    return [torch.from_numpy(a).cuda() for a in (cl, ed, Tw, cn, en)]


def feed_gpu(gmap, row):
    cl, ed, Tw, cn, en = pack(row)
    gmap.add_vertex(cl, ed, Tw, counts=cn, edge_counts=en)
    gmap.update()


def scene_frames(oracles, edge=False):
    return [[mq.TreeFrame(f.ke if edge else f.kd) for f in o.frames()] for o in oracles]


def cam_struct():
    from avoid_mpc_amd import capi
    return capi.FrameCamera(*CAM)


def check_inputs(e, quantum, K):
    """What the expected answers must hold for the comparison to mean something (module docstring)."""
    paths = np.array(e["path"])
    assert (paths == "fast").sum() >= 30 and (paths == "merge").sum() >= 30, ((paths == "fast").sum(), (paths == "merge").sum())
    multi = sum(1 for s in range(S) for i in range(NQ) if paths[s, i] == "merge" and len(set(e["frame"][s, i][e["frame"][s, i] >= 0])) > 1)
    assert multi >= 15, multi
    if quantum and K == 8:
        ties = 0
        for s in range(S):
            for i in range(NQ):
                d, f = e["sqdist"][s, i], e["frame"][s, i]
                ties += any(d[a] == d[a + 1] and f[a] != f[a + 1] and f[a + 1] >= 0 for a in range(K - 1))
        assert ties >= 3, ties
    assert ((paths[3] == "fast") & (e["counts"][3] == 0)).sum() >= 8
    assert (e["counts"][4] == 0).all() and (paths[4] == "merge").all()


def to_np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("quantum,max_frames,periods,step,K", CONFIGS)
def test_map_queries_follow_the_reference(quantum, max_frames, periods, step, K):
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import KfMap
    from tests import _oracle
    frames = flight(quantum, periods, step, K)
    oracles = new_oracles(max_frames)
    gmap = KfMap(S, CAP, ECAP, max_frames, TH_DIST, TH_COUNT, DEPTH_MIN, TBC)
    cam = cam_struct()
    try:
        mid = periods // 2
        for t, row in enumerate(frames):
            feed_oracle(oracles, row)
            feed_gpu(gmap, row)
            if t == mid:                                     # GetNearestDistance mid-flight, over rows of x0array
                q = make_queries(step * t, quantum, 50 + t, stride=14)
                d = gmap.nearest_distance(torch.from_numpy(q).cuda())
                torch.cuda.synchronize()
                e = mq.expected_distance(scene_frames(oracles), q)
                assert np.array_equal(d.cpu().numpy().view(np.int64), e.view(np.int64)), "nearest_distance mid-flight"
        d_last = step * (periods - 1)
        q = make_queries(d_last, quantum, 7)
        dq = torch.from_numpy(q).cuda()
        obs = scene_frames(oracles)
        Twc = np.stack([o.Twc for o in oracles])
        if max_frames == 100 and periods == 40:
            assert min(len(f) for f in obs[:4]) >= 32, [len(f) for f in obs]     # more than 16 frames, more than 64 candidates per query

        # QueryNearest with the camera
        e = mq.expected_batch(obs, q, K, Twc, CAM)
        check_inputs(e, quantum, K)
        st0 = gmap.state()
        out = to_np(gmap.query_nearest(dq, K, cam=cam))
        mq.assert_query_equal(out, e, "query_nearest with the camera")
        assert sum(f.self_checks for fr in obs for f in fr) >= (300 if not quantum else 30)   # the helper met the reference-shaped search on tie-free rows
        # a query changes nothing
        st1 = gmap.state()
        assert all(np.array_equal(st0[k], st1[k]) for k in st0)
        again = to_np(gmap.query_nearest(dq, K, cam=cam))
        assert all(np.array_equal(out[k].view(np.uint8), again[k].view(np.uint8)) for k in out)

        # without a camera; the edge clouds, k = 1
        mq.assert_query_equal(to_np(gmap.query_nearest(dq, K)), mq.expected_batch(obs, q, K, None, None), "query_nearest, cam = None")
        mq.assert_query_equal(to_np(gmap.query_nearest(dq, 1, edge=True)), mq.expected_batch(scene_frames(oracles, edge=True), q, 1, None, None),
                              "query_nearest, edge clouds, k = 1")
        # the host variants
        hp = np.zeros((S, NQ, K, 3), np.float32); hd = np.zeros((S, NQ, K)); hf = np.zeros((S, NQ, K), np.int32); hc = np.zeros((S, NQ), np.int32)
        hdist = np.zeros((S, NQ))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        capi.check(gmap.lib.amk_kfmap_query_nearest_host(gmap.h, C.byref(cam), vp(q), 3, NQ, K, 0, vp(hp), vp(hd), vp(hf), vp(hc)), "query host")
        mq.assert_query_equal(dict(pts=hp, sqdist=hd, frame=hf, counts=hc), e, "amk_kfmap_query_nearest_host")
        capi.check(gmap.lib.amk_kfmap_nearest_distance_host(gmap.h, vp(q), 3, NQ, vp(hdist)), "distance host")

        # GetNearestDistance after the last period
        ed = mq.expected_distance(obs, q)
        assert (ed[4] == mq.SQRT_DBL_MAX).all() and (ed[:4] < 20).all()
        d = gmap.nearest_distance(dq).cpu().numpy()
        assert np.array_equal(d.view(np.int64), ed.view(np.int64)) and np.array_equal(hdist.view(np.int64), ed.view(np.int64))

        # GetPtCloud: sizes, content and order of every frame
        rng = np.random.default_rng(3)
        for s in range(S):
            xyz, sizes = gmap.points(s)
            want = oracles[s].summary()[1]
            assert sizes[:len(want)].tolist() == want and (sizes[len(want):] == -1).all() and len(xyz) == sum(want), (s, sizes, want)
            o = 0
            for f, frm in enumerate(oracles[s].frames()):
                part = xyz[o:o + want[f]]; o += want[f]
                fresh = _oracle.kd_oracle(part)
                for p in rng.random((20, 3)) * [9.0, 10.0, 3.0] + [d_last, -5.0, 0.0]:
                    gi, gd, _ = fresh.search(p, 3)
                    wi, wd, _ = frm.kd.search(p, 3)
                    assert np.array_equal(gi, wi) and np.array_equal(gd, wd), (s, f)
                fresh.close()
        n = C.c_longlong(-1)
        total = sum(oracles[0].summary()[1])
        assert gmap.lib.amk_kfmap_points_host(gmap.h, 0, None, 0, None, C.byref(n)) == capi.AMK_OK and n.value == total      # the size probe
        small = np.full((total - 1, 3), -7.0, np.float32); n = C.c_longlong(-1)
        assert gmap.lib.amk_kfmap_points_host(gmap.h, 0, vp(small), total - 1, None, C.byref(n)) == capi.AMK_ERR_INVALID_ARG
        assert n.value == total and (small == -7.0).all()                                                                   # nothing written
        assert gmap.lib.amk_kfmap_points_host(gmap.h, S, None, 0, None, C.byref(n)) == capi.AMK_ERR_INVALID_ARG

        # reset of one scene: count 0 there, the others unchanged
        gmap.reset(1, 1)
        after = to_np(gmap.query_nearest(dq, K, cam=cam))
        assert (after["counts"][1] == 0).all() and (after["frame"][1] == -1).all() and (after["sqdist"][1] == mq.DBL_MAX).all()
        keep = [0, 2, 3, 4]
        assert all(np.array_equal(after[k][keep].view(np.uint8), out[k][keep].view(np.uint8)) for k in out)
        assert (gmap.nearest_distance(dq).cpu().numpy()[1] == mq.SQRT_DBL_MAX).all()
    finally:
        gmap.close()


def test_argument_errors():
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import KfMap
    gmap = KfMap(2, 64, 16, 3, TH_DIST, TH_COUNT, DEPTH_MIN, TBC)
    try:
        q = torch.zeros((2, 70, 3), dtype=torch.float64, device="cuda")
        d2 = torch.empty((2, 70, 64), dtype=torch.float64, device="cuda")
        call = lambda k, nq=70, stride=3, qp=q: gmap.lib.amk_kfmap_query_nearest(gmap.h, None, capi.dptr(qp), stride, nq, k, 0, None, capi.dptr(d2),
                                                                                  None, None, capi.stream_ptr())
        assert call(64) == capi.AMK_OK                       # 70 queries: no cap of AMK_MAX_QUERIES
        assert call(0) == capi.AMK_ERR_INVALID_ARG and call(65) == capi.AMK_ERR_UNSUPPORTED
        assert call(4, nq=0) == capi.AMK_ERR_INVALID_ARG and call(4, stride=2) == capi.AMK_ERR_INVALID_ARG and call(4, qp=None) == capi.AMK_ERR_INVALID_ARG
        assert gmap.lib.amk_kfmap_nearest_distance(gmap.h, capi.dptr(q), 3, 70, None, capi.stream_ptr()) == capi.AMK_ERR_INVALID_ARG
        assert gmap.lib.amk_kfmap_query_nearest(None, None, capi.dptr(q), 3, 70, 4, 0, None, None, None, None, None) == capi.AMK_ERR_INVALID_ARG
        torch.cuda.synchronize()
        assert (d2.cpu().numpy() == mq.DBL_MAX).all()        # a map without a frame
    finally:
        gmap.close()


def test_pipeline_slot_query_equals_a_stand_alone_map():
    """A TASK-mode pipeline with keyframes (gang 2, 2 scenes, cloud frames with d_Twc_cur + camera: the C1 depth camera's model) runs
    three periods; Pipeline.kfmap_query on the slot's stream equals the same query on a KfMap fed the same frames."""
    import torch
    from avoid_mpc_amd import capi, flight as amk_flight
    from avoid_mpc_amd.host import KfMap, Pipeline
    from tests import _flight
    B, gang, K, periods, step = 2, 2, 8, 3, 0.4
    GS = B * gang
    prm, _n = _flight.make_prm("C1")
    frames = flight(0.25, periods, step, K)
    cam = capi.FrameCamera(*_flight.depth_camera())
    st = [amk_flight.initial_state(s, prm) for s in range(GS)]
    pipe = Pipeline(1, B, CAP, ECAP, prm, queue_depth=1, gang=gang,
                    keyframes=dict(max_frame_count=3, th_dist=TH_DIST, th_count=TH_COUNT, depth_min=DEPTH_MIN, Tbc=TBC))
    gmap = KfMap(GS, CAP, ECAP, 3, TH_DIST, TH_COUNT, DEPTH_MIN, TBC)
    try:
        for t, row in enumerate(frames):
            cl, ed, Tw, cn, en = [a[:GS].contiguous() for a in pack(row)]
            gmap.add_vertex(cl, ed, Tw, counts=cn, edge_counts=en)
            gmap.update()
            keep = []
            for g in range(gang):
                sl = slice(g * B, (g + 1) * B)
                x = np.stack([st[i][0] for i in range(sl.start, sl.stop)]); x[:, 0] += step * t
                bufs = dict(clouds=cl[sl].contiguous(), edges=ed[sl].contiguous(), cloud_counts=cn[sl].contiguous(), edge_counts=en[sl].contiguous(),
                            Twc_cur=Tw[sl].contiguous(), odom=torch.from_numpy(x).cuda(), cmd_out=torch.empty((B, 3), dtype=torch.float64, device="cuda"),
                            ref_path_init=torch.from_numpy(np.stack([st[i][1] for i in range(sl.start, sl.stop)])).cuda() if t == 0 else None)
                keep.append(bufs)
                ticket = pipe.submit(keep_warm_start=t > 0, cam=cam, **bufs)      # (`keep` holds the buffers until the gang has run)
            q = make_queries(step * t, 0.25, 20 + t)[:GS]
            dq = torch.from_numpy(q).cuda()
            slot = ticket % pipe.n_slots
            got = pipe.kfmap_query(slot, dq, K, cam=cam)          # on the slot's stream, behind the gang's launches
            gotd = pipe.kfmap_query(slot, dq)
            want, wantd = gmap.query_nearest(dq, K, cam=cam), gmap.nearest_distance(dq)
            torch.cuda.synchronize()
            assert all(np.array_equal(got[k].cpu().numpy().view(np.uint8), want[k].cpu().numpy().view(np.uint8)) for k in want), t
            assert np.array_equal(gotd.cpu().numpy().view(np.int64), wantd.cpu().numpy().view(np.int64)), t
            assert (want["counts"].cpu().numpy() > 0).sum() >= GS * NQ // 2
            pipe.wait(ticket)
        after = pipe.kfmap_query(0, dq, K, cam=cam, after_wait=True)
        torch.cuda.synchronize()
        assert all(np.array_equal(after[k].cpu().numpy().view(np.uint8), want[k].cpu().numpy().view(np.uint8)) for k in want)
        assert len(set(np.unique(want["frame"].cpu().numpy()))) >= 3          # -1, the current frame and a keyframe at least
        xyz, sizes = pipe.kfmap_points(0, 1)
        wxyz, wsizes = gmap.points(1)
        assert np.array_equal(xyz, wxyz) and np.array_equal(sizes, wsizes) and len(xyz) > 0
    finally:
        pipe.close()
        gmap.close()
