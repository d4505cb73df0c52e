"""GPU: amk_kfmap_set_tie_order(AMK_TIES_NANOFLANN) -- the keyframe map answers in nanoflann's order of equal distances.

The scripts of tests/_kfmap_tie_cases.py (lattice clouds: ties everywhere) are fed to a map in the mode and to a second map left in
the default mode.  The first must equal tests/_kfmap.MapOracle and tests/_map_query.py's rules over KdHandle.search (nanoflann's
lists) bit for bit -- state, amk_kfmap_exact_status_host, QueryNearest on obstacle and edge clouds, the packed parameter vector of
a step -- the second the same rules over cloud-index order; tests/test_kfmap_tie_cases.py shows on the CPU that the two differ."""
import ctypes as C

import numpy as np
import pytest

from tests import _kfmap, _kfmap_tie_cases as tc, _map_query as mq

pytestmark = pytest.mark.gpu


def pack(row, cap=tc.CAP, ecap=tc.ECAP):
    import torch
    n = len(row)
    cl = np.zeros((n, cap, 3), np.float32); ed = np.zeros((n, ecap, 3), np.float32)
    cn = np.zeros(n, np.int32); en = np.zeros(n, np.int32); Tw = np.zeros((n, 4, 4))
    for s, (c, e, T) in enumerate(row):
        cl[s, :len(c)] = c; cn[s] = len(c); ed[s, :len(e)] = e; en[s] = len(e); Tw[s] = T
    return [torch.from_numpy(a).cuda() for a in (cl, ed, Tw, cn, en)]


def feed(gmap, row, first_scene=0):
    cl, ed, Tw, cn, en = pack(row, gmap.max_points, gmap.max_edge_points)
    gmap.add_vertex(cl, ed, Tw, counts=cn, edge_counts=en, first_scene=first_scene)


def new_map(max_frames, mode, S=tc.S, cap=tc.CAP, ecap=tc.ECAP):
    from avoid_mpc_amd.host import KfMap
    m = KfMap(S, cap, ecap, max_frames, tc.TH_DIST, tc.TH_COUNT, tc.DEPTH_MIN, tc.TBC)
    m.set_tie_order(mode)
    return m


def to_np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_state(st, summaries, what):
    for s, (nk, sizes, outliers) in enumerate(summaries):
        assert st["n_keyframes"][s] == nk and st["n_query_frames"][s] == len(sizes), (what, s, st["n_keyframes"][s], nk)
        assert list(st["frame_sizes"][s][:len(sizes)]) == sizes and (st["frame_sizes"][s][len(sizes):] == -1).all(), (what, s)
        assert st["last_outliers"][s] == max(outliers, 0), (what, s)


def gpu_step(gmap, gmpc, t, K, max_iter=1):
    import torch
    from avoid_mpc_amd import capi
    from tests import _oracle
    prm = tc.prm_of(K, max_iter)
    scs = [tc.step_scene(s, t, K) for s in range(tc.S)]
    sq = torch.from_numpy(np.stack([_oracle.scene_state_quads(sc, prm) for sc in scs])).cuda()
    px = torch.from_numpy(np.array([sc["pos"][0] for sc in scs])).cuda()
    dref = torch.from_numpy(np.stack([sc["ref_path"] for sc in scs])).cuda()
    out = gmap.step(gmpc, prm, sq, px, dref, cam=capi.FrameCamera(*tc.CAM))
    torch.cuda.synchronize()
    return dict(u=out["u"].cpu().numpy(), flags=out["flags"].cpu().numpy(), ref_path=dref.cpu().numpy(), P=gmpc.ref_states())


@pytest.mark.parametrize("max_frames,K,wide", tc.CONFIGS)
def test_the_map_answers_in_nanoflann_order_and_the_default_map_does_not(max_frames, K, wide):
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import MpcBatch
    from tests.test_step_frames_edges_gpu import assert_P_exact, assert_flags01
    lib = capi.load()
    r = tc.run(max_frames, K)
    cam = capi.FrameCamera(*tc.CAM)
    gmap, dmap = new_map(max_frames, capi.AMK_TIES_NANOFLANN), new_map(max_frames, capi.AMK_TIES_LOWEST_INDEX)
    gmpc = MpcBatch(tc.prm_of(K).T, tc.prm_of(K).dt, K, tc.S); gmpc.configure(tc.prm_of(K))
    differ = {"knn": [], "edge": []}
    lib.amk__frames_force_wide(int(wide))
    try:
        assert (gmap.exact_status()["obs"] == capi.AMK_EXACT_OFF).all()
        for t in range(tc.PERIODS):
            what = f"max_frame_count {max_frames}, K {K}, period {t}"
            for m in (gmap, dmap):
                if t == tc.RESET_BEFORE:
                    m.reset(tc.RESET_SCENE, 1)
                feed(m, tc.script()[t])
                m.update()
                check_state(m.state(), r.summaries[t], what)
            st = gmap.exact_status()
            dst = dmap.exact_status()
            for s in range(tc.S):
                nf = r.status_frames[t][s]
                for key in ("obs", "edge"):
                    assert (st[key][s, :nf] == capi.AMK_EXACT_IN_USE).all() and (st[key][s, nf:] == capi.AMK_EXACT_OFF).all(), (what, s, key, st[key][s])
                    assert (dst[key][s] == capi.AMK_EXACT_OFF).all()
            dq = torch.from_numpy(tc.queries(t)).cuda()
            got = {}
            for name, m, exp in (("mode", gmap, r.nano[t]), ("default", dmap, r.index[t])):
                got[name] = dict(obs_cam=to_np(m.query_nearest(dq, K, cam=cam)), obs_nocam=to_np(m.query_nearest(dq, K)),
                                 edge_cam=to_np(m.query_nearest(dq, 1, cam=cam, edge=True)))
                for key, out in got[name].items():
                    mq.assert_query_equal(out, exp[key], f"{what}, {name} map, {key}")
                d = m.nearest_distance(dq).cpu().numpy()
                assert np.array_equal(d.view(np.int64), exp["dist"].view(np.int64)), (what, name)
            assert np.array_equal(r.nano[t]["dist"], r.index[t]["dist"])          # GetNearestDistance: the same in both modes
            for key in ("obs_cam", "obs_nocam"):
                differ["knn"].append(tc.rows_that_differ(got["mode"][key], got["default"][key]))
            differ["edge"].append(tc.rows_that_differ(got["mode"]["edge_cam"], got["default"]["edge_cam"]))
            # the step at mpc_max_iter = 1: the packed parameter vector, bit for bit
            g = gpu_step(gmap, gmpc, t, K)
            assert_flags01(g["flags"], r.steps[t])
            assert_P_exact(g["P"], r.steps[t], tc.prm_of(K).N, K, what)
        # the full step
        g = gpu_step(gmap, gmpc, tc.PERIODS - 1, K, max_iter=3)
        for s, o in enumerate(r.last_full):
            assert np.array_equal(g["flags"][s][:3], o["flags"][:3]), (s, g["flags"][s], o["flags"])
            if np.array_equal(g["flags"][s], o["flags"]):
                assert np.abs(g["u"][s] - o["u"]).max() <= 1e-6 and np.abs(g["ref_path"][s] - o["ref_path"]).max() <= 1e-6, s
        knn, edge = np.concatenate([d.reshape(-1) for d in differ["knn"]]), np.concatenate([d.reshape(-1) for d in differ["edge"]])
        print(f"rows on which the two maps hold different point sets: k-NN {knn.mean():.0%}, edge 1-NN {edge.mean():.0%}")
        assert knn.mean() >= 0.25 and edge.mean() >= 0.10
    finally:
        lib.amk__frames_force_wide(0)
        gmap.close(); dmap.close()


@pytest.mark.parametrize("a_first", [True, False])
def test_drone_behind_pts_takes_nanoflanns_tenth_neighbour(a_first):
    from avoid_mpc_amd import capi
    want = {capi.AMK_TIES_NANOFLANN: tc.behind_outcome(a_first, _kfmap.MapOracle), capi.AMK_TIES_LOWEST_INDEX: tc.behind_outcome(a_first, tc.IndexOrderMap)}
    for mode, nk in want.items():
        m = new_map(3, mode, S=1, cap=64, ecap=8)
        try:
            for row in tc.behind_pair(a_first):
                feed(m, [row])
                m.update()
            assert m.state()["n_keyframes"][0] == nk, (a_first, mode, m.state()["n_keyframes"], nk)
        finally:
            m.close()
    if a_first:
        assert want[capi.AMK_TIES_NANOFLANN] != want[capi.AMK_TIES_LOWEST_INDEX]   # the flipped case


def test_a_scene_whose_tree_was_given_up_keeps_the_default_order():
    """The 4200-point frame is built with a two-entry ring of open nodes (amk__exact_set_queue_cap, tests only): its tree is given
    up, its queries get the bucketed index's lists; the scenes fed with the shipped ring are not affected.  The step over that map
    packs the bucketed index's obstacle lists for that scene (its edge tree exists: the snap is nanoflann's) and the oracle's for the
    others; the next period's update tests the given-up keyframe with DroneBehindPts and sweeps it, and the map follows the oracle."""
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import MpcBatch
    from tests import _frames_cases as fc
    from tests.test_step_frames_edges_gpu import assert_P_exact, assert_flags01
    lib = capi.load()
    K, t = 8, 0
    r = tc.run(3, K)
    gmap = new_map(3, capi.AMK_TIES_NANOFLANN)
    gmpc = MpcBatch(tc.prm_of(K).T, tc.prm_of(K).dt, K, tc.S); gmpc.configure(tc.prm_of(K))
    oracles = [tc.new_map(3) for _ in range(tc.S)]
    row = tc.script()[t]
    try:
        for s in range(tc.S):
            assert lib.amk__exact_set_queue_cap(2 if s == tc.BIG_SCENE else 0) == 0
            feed(gmap, [row[s]], first_scene=s)
            torch.cuda.synchronize()
            oracles[s].add_vertex(*row[s]); oracles[s].update()
        lib.amk__exact_set_queue_cap(0)
        gmap.update()
        st = gmap.exact_status()
        assert st["obs"][tc.BIG_SCENE, 0] == capi.AMK_EXACT_GAVE_UP, st["obs"][:, 0]
        assert (np.delete(st["obs"][:, 0], tc.BIG_SCENE) == capi.AMK_EXACT_IN_USE).all() and (st["edge"][:, 0] == capi.AMK_EXACT_IN_USE).all(), st
        q = tc.queries(t)
        out = to_np(gmap.query_nearest(torch.from_numpy(q).cuda(), K))
        nano, index = (mq.expected_batch(tc.frames_of(oracles, False, n), q, K) for n in (True, False))
        assert tc.rows_that_differ(nano, index)[tc.BIG_SCENE].mean() >= 0.25
        for s in range(tc.S):
            exp = index if s == tc.BIG_SCENE else nano
            mq.assert_query_equal({k: v[s:s + 1] for k, v in out.items()}, {k: (v[s:s + 1] if k != "path" else v[s:s + 1]) for k, v in exp.items()},
                                  f"scene {s}")
        # the step: the given-up scene's K-NN rows and its snapped point's re-query keep the bucketed index's lists
        N = tc.prm_of(K).N
        want = [dict(o) for o in r.steps[t]]
        P = np.array(want[tc.BIG_SCENE]["ref_log"][0], dtype=np.float64)
        in_order = tc.step_obstacles(oracles[tc.BIG_SCENE], K, want[tc.BIG_SCENE], nano=False)
        assert not np.array_equal(in_order, fc.split_P(P, N, K)[2]) and not np.array_equal(P[10:13], tc.step_scene(tc.BIG_SCENE, t, K)["ref_path"][0, :3])
        fc.split_P(P, N, K)[2][:] = in_order                      # (a view of P)
        want[tc.BIG_SCENE]["ref_log"] = [P]
        g = gpu_step(gmap, gmpc, t, K)
        assert_flags01(g["flags"], want)
        assert_P_exact(g["P"], want, N, K, "a map with a given-up tree")
        # the next period: DroneBehindPts and the sweep over the keyframe whose tree was given up
        feed(gmap, tc.script()[t + 1])
        gmap.update()
        check_state(gmap.state(), r.summaries[t + 1], "the period after a given-up tree")
        st = gmap.exact_status()
        assert (st["obs"][:, 0] == capi.AMK_EXACT_IN_USE).all() and (st["edge"][:, :2] == capi.AMK_EXACT_IN_USE).all(), st
    finally:
        lib.amk__exact_set_queue_cap(0)
        gmap.close()


def test_errors():
    import torch
    from avoid_mpc_amd import capi
    lib = capi.load()
    m = new_map(3, capi.AMK_TIES_LOWEST_INDEX, S=2, cap=64, ecap=8)
    try:
        assert lib.amk_kfmap_set_tie_order(m.h, 7) == capi.AMK_ERR_UNSUPPORTED
        assert lib.amk_kfmap_set_tie_order(m.h, capi.AMK_TIES_AUTO) == capi.AMK_ERR_UNSUPPORTED
        assert lib.amk_kfmap_set_tie_order(None, capi.AMK_TIES_NANOFLANN) == capi.AMK_ERR_INVALID_ARG
        assert lib.amk_kfmap_exact_status_host(None, None, None) == capi.AMK_ERR_INVALID_ARG
        assert lib.amk_kfmap_set_tie_order(m.h, capi.AMK_TIES_NANOFLANN) == 0
        assert lib.amk_kfmap_set_tie_order(m.h, capi.AMK_TIES_LOWEST_INDEX) == 0      # before the first frame the mode may still change
        assert lib.amk_kfmap_set_tie_order(m.h, capi.AMK_TIES_NANOFLANN) == 0
        feed(m, [tc.behind_pair(True)[0]] * 2)
        assert lib.amk_kfmap_set_tie_order(m.h, capi.AMK_TIES_LOWEST_INDEX) == capi.AMK_ERR_INVALID_ARG
        m.reset(0, 2)
        assert lib.amk_kfmap_set_tie_order(m.h, capi.AMK_TIES_NANOFLANN) == capi.AMK_ERR_INVALID_ARG   # a reset does not re-open the call
    finally:
        m.close()
    # a map whose trees do not fit beside its pools: refused with the figure, the map stays usable in the default mode
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0]
    pts, epts, mf = 1000, 200000, 100                          # mostly edge points: their trees and planes are 4.4 x the pool's bytes
    per_scene, tie_per_scene = C.c_longlong(), C.c_longlong()
    assert lib.amk_kfmap_pool_bytes(1, pts, epts, mf, C.byref(per_scene)) == 0
    assert lib.amk_kfmap_tie_order_bytes(1, pts, epts, mf, C.byref(tie_per_scene)) == 0
    assert tie_per_scene.value > 4 * per_scene.value
    n = max(1, int(0.22 * free / per_scene.value))              # the pools take 22 % of what is free, the trees would need 4 x that: more than the rest
    big = new_map(mf, capi.AMK_TIES_LOWEST_INDEX, S=n, cap=pts, ecap=epts)
    try:
        need = C.c_longlong()
        assert lib.amk_kfmap_tie_order_bytes(n, pts, epts, mf, C.byref(need)) == 0 and need.value > torch.cuda.mem_get_info()[0]
        assert lib.amk_kfmap_set_tie_order(big.h, capi.AMK_TIES_NANOFLANN) == capi.AMK_ERR_UNSUPPORTED
        assert (big.exact_status()["obs"] == capi.AMK_EXACT_OFF).all()
        rng = np.random.default_rng(0)
        cloud = rng.uniform(2, 8, (800, 3)).astype(np.float32)
        T = np.eye(4) @ tc.TBC
        cl, ed, Tw, cn, en = pack([(cloud, cloud[:100], T)], pts, epts)
        big.add_vertex(cl, ed, Tw, counts=cn, edge_counts=en)     # scene 0 only
        big.update()
        assert big.state()["n_keyframes"][0] == 1 and big.state()["frame_sizes"][0, 0] == 800
    finally:
        big.close()


@pytest.mark.parametrize("gang", [1, 2])
def test_a_pipeline_slot_in_the_mode_equals_the_direct_calls(gang):
    """A TASK-mode pipeline with keyframes (max_frame_count 3, cloud frames of the script with d_Twc_cur + camera); the mode is set on
    the slot's map before the first submit.  u, flags and ref_path equal amk_kfmap_add_vertex / update / step on a stand-alone map in
    the mode fed with the host twin of the TASK prologue (avoid_mpc_amd/flight.py: GetInitPath, the clock model), the slot map's
    QueryNearest equals the stand-alone map's and the helper's, bit for bit; afterwards the setter is refused."""
    import torch
    from avoid_mpc_amd import capi, flight as amk_flight
    from avoid_mpc_amd.host import MpcBatch, Pipeline
    K, GS = 8, tc.S
    B = GS // gang
    prm = tc.prm_of(K, max_iter=3)
    cam = capi.FrameCamera(*tc.CAM)
    r = tc.run(3, K)
    st = [amk_flight.initial_state(40 + s, prm) for s in range(GS)]
    ref = np.stack([b for _, b in st])
    pipe = Pipeline(1, B, tc.CAP, tc.ECAP, prm, queue_depth=1, gang=gang,
                    keyframes=dict(max_frame_count=3, th_dist=tc.TH_DIST, th_count=tc.TH_COUNT, depth_min=tc.DEPTH_MIN, Tbc=tc.TBC))
    gmap = new_map(3, capi.AMK_TIES_NANOFLANN)
    gmpc = MpcBatch(prm.T, prm.dt, K, GS); gmpc.configure(prm)
    try:
        pipe.kfmap(0).set_tie_order(capi.AMK_TIES_NANOFLANN)
        for t in range(tc.RESET_BEFORE):                          # (the periods before the script's reset)
            row = tc.script()[t]
            x = np.stack([a for a, _ in st])
            for s in range(GS):
                x[s, :3] = tc.drone(s, t)
            cl, ed, Tw, cn, en = pack(row)
            # the direct calls
            sq, px = amk_flight.period_inputs(x, ref, prm)        # GetInitPath shifts ref in place, as the slot does with its mRefPath
            gmap.add_vertex(cl, ed, Tw, counts=cn, edge_counts=en)
            gmap.update()
            dref = torch.from_numpy(ref.copy()).cuda()
            want = gmap.step(gmpc, prm, torch.from_numpy(sq).cuda(), torch.from_numpy(px).cuda(), dref, cam=cam)
            torch.cuda.synchronize()
            # the pipeline
            keep, tickets = [], []
            for g in range(gang):
                sl = slice(g * B, (g + 1) * B)
                bufs = dict(clouds=cl[sl].contiguous(), edges=ed[sl].contiguous(), cloud_counts=cn[sl].contiguous(), edge_counts=en[sl].contiguous(),
                            Twc_cur=Tw[sl].contiguous(), odom=torch.from_numpy(x[sl]).cuda(), cmd_out=torch.empty((B, 3), dtype=torch.float64, device="cuda"),
                            ref_path_init=torch.from_numpy(np.stack([st[i][1] for i in range(sl.start, sl.stop)])).cuda() if t == 0 else None)
                keep.append(bufs)
                tickets.append(pipe.submit(keep_warm_start=t > 0, cam=cam, **bufs))
            dq = torch.from_numpy(tc.queries(t)).cuda()
            got = to_np(pipe.kfmap_query(0, dq, K, cam=cam))
            torch.cuda.synchronize()
            pipe.wait(tickets[-1])
            o = pipe.outputs(tickets[-1])                          # the gang's outputs: gang x B scenes behind the first position's pointers
            what = f"gang {gang}, period {t}"
            direct = to_np(gmap.query_nearest(dq, K, cam=cam))
            assert all(np.array_equal(got[k].view(np.uint8), direct[k].view(np.uint8)) for k in direct), what
            mq.assert_query_equal(got, r.nano[t]["obs_cam"], what)
            stp = pipe.kfmap(0).exact_status()
            for s in range(GS):
                nf = r.status_frames[t][s]
                assert (stp["obs"][s, :nf] == capi.AMK_EXACT_IN_USE).all() and (stp["obs"][s, nf:] == capi.AMK_EXACT_OFF).all(), (what, s)
            outs = [pipe.outputs(tk) for tk in tickets]
            for name, w in (("u", want["u"].cpu().numpy()), ("flags", want["flags"].cpu().numpy()), ("ref_path", dref.cpu().numpy())):
                g_all = np.concatenate([oo[name] for oo in outs]) if outs[0][name].shape[0] == B else outs[0][name]
                assert np.array_equal(g_all.view(np.uint8), w.view(np.uint8)), (what, name)
            ref = dref.cpu().numpy().copy()
            assert pipe.lib.amk_kfmap_set_tie_order(pipe.kfmap(0).h, capi.AMK_TIES_LOWEST_INDEX) == capi.AMK_ERR_INVALID_ARG
    finally:
        pipe.close()
        gmap.close()
