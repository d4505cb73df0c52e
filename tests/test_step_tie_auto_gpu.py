"""GPU: the single-frame control step (amk_step_batch) with handles in AMK_TIES_AUTO.  Quantised scenes -- ties in the obstacle
queries, the edge query and the edge snap's re-query -- must give the bits of the same step in AMK_TIES_NANOFLANN (the same
traversal and the same solve on the same inputs: no tolerance) and match the step oracle; scenes without ties must give the
bits of the default mode and never get a tree.  Plus: the AUTO step in a HIP graph, and the multi-frame paths' refusal."""
import numpy as np
import pytest

from tests import _oracle
from tests.test_step_gpu import TOL, compare
from avoid_mpc_amd import synth, fsm

pytestmark = pytest.mark.gpu
KEYS = ("u", "x0array", "flags", "ref_path")


def _quantised_scenes(prm):
    """The 16 scenes of test_step_in_nanoflann_tie_order_on_quantised_clouds (tests/test_step_gpu.py): clouds on a 0.25 m lattice,
    reference paths on a 0.125 m lattice; odd scenes force the edge snap onto a six-way tied ring of edge points."""
    scenes = []
    for i in range(16):
        sc = synth.make_scene(3072, 1500 + i, prm)
        sc["cloud"] = (np.round(sc["cloud"] * 4) / 4).astype(np.float32)
        sc["edge"] = (np.round(sc["edge"] * 4) / 4).astype(np.float32)
        sc["ref_path"] = sc["ref_path"].copy(); sc["ref_path"][:, :3] = np.round(sc["ref_path"][:, :3] * 8) / 8
        if i % 2:   # reference point 0 within the safety distance of an obstacle -> snap to a (tied) nearest edge point
            sc["cloud"] = np.concatenate([sc["cloud"], (sc["ref_path"][0, :3] + [0.125, 0, 0])[None].astype(np.float32)])
            e0 = sc["ref_path"][0, :3]
            ring = np.float32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]) * 0.5 + e0
            sc["edge"] = np.concatenate([sc["edge"], ring.astype(np.float32)])
        scenes.append(sc)
    return scenes


def _run_gpu(torch, scenes, prm, tie_order, n_steps):
    """-> (per-step results as tests/test_step_gpu.py's run_both makes them, exact status of the two handles after the last step)"""
    from avoid_mpc_amd.host import KdBatch, MpcBatch, step_batch
    S = len(scenes)
    nmax = max(len(sc["cloud"]) for sc in scenes); emax = max(len(sc["edge"]) for sc in scenes)
    cl = np.zeros((S, nmax, 3), np.float32); ed = np.zeros((S, emax, 3), np.float32)
    cn = np.zeros(S, np.int32); en = np.zeros(S, np.int32)
    for s, sc in enumerate(scenes):
        cl[s, :len(sc["cloud"])] = sc["cloud"]; cn[s] = len(sc["cloud"])
        ed[s, :len(sc["edge"])] = sc["edge"]; en[s] = len(sc["edge"])
    kd_o, kd_e = KdBatch(S, nmax), KdBatch(S, emax)
    kd_o.set_tie_order(tie_order); kd_e.set_tie_order(tie_order)
    kd_o.build(torch.from_numpy(cl).cuda(), torch.from_numpy(cn).cuda())
    kd_e.build(torch.from_numpy(ed).cuda(), torch.from_numpy(en).cuda())
    mpc = MpcBatch(prm.T, prm.dt, prm.K, S); mpc.configure(prm)
    sq = torch.from_numpy(np.stack([_oracle.scene_state_quads(sc, prm) for sc in scenes])).cuda()
    ref = torch.from_numpy(np.stack([sc["ref_path"] for sc in scenes])).cuda()
    pos_x = torch.from_numpy(np.array([sc["pos"][0] for sc in scenes])).cuda()
    res = []
    for _ in range(n_steps):
        out = step_batch(kd_o, kd_e, mpc, prm, sq, pos_x, ref)
        torch.cuda.synchronize()
        res.append(dict(u=out["u"].cpu().numpy().copy(), x0array=out["x0array"].cpu().numpy().copy(),
                        flags=out["flags"].cpu().numpy().copy(), ref_path=ref.cpu().numpy().copy()))
    status = (kd_o.exact_status().cpu().numpy(), kd_e.exact_status().cpu().numpy())
    kd_o.close(); kd_e.close(); mpc.close()
    return res, status


def _oracle_steps(scenes, prm, n_steps):
    sq = np.stack([_oracle.scene_state_quads(sc, prm) for sc in scenes])
    cpu = [[] for _ in range(n_steps)]
    for s, sc in enumerate(scenes):
        ko, ke = _oracle.kd_oracle(sc["cloud"]), _oracle.kd_oracle(sc["edge"])
        m = _oracle.MpcOracle(prm.T, prm.dt, prm.K); m.configure(prm)
        rp = sc["ref_path"].copy()
        for t in range(n_steps):
            r = _oracle.step_oracle(ko, ke, m, prm, sq[s], sc["pos"][0], rp)
            r["ref_path"] = rp.copy()
            cpu[t].append(r)
    return cpu


def test_auto_step_equals_the_nanoflann_step_on_ties_and_the_default_step_without():
    """One batch of 32 scenes, two control steps (warm start carried over), both handles in the same mode; modes 2, 1 and 0.
    Scenes 0-15 (quantised): mode 2 matches the step oracle at the usual tolerance and equals mode 1 in every bit of u, x0array,
    flags and ref_path -- a tied query that AUTO missed would show here; mode 0 differs from the oracle on at least one of them,
    so they do exercise ties.  Scenes 16-31 (plain make_scene): mode 2 equals mode 0 bit for bit and both handles still report
    NOT_NEEDED for them afterwards."""
    import torch
    from avoid_mpc_amd import capi
    assert torch.cuda.is_available()
    prm = synth.MpcParams(T=1.0, K=3)
    quant = _quantised_scenes(prm)
    plain = [synth.make_scene(3072, 2500 + i, prm) for i in range(16)]
    scenes = quant + plain
    Q = slice(0, 16); P = slice(16, 32)
    g2, st2 = _run_gpu(torch, scenes, prm, capi.AMK_TIES_AUTO, 2)
    g1, st1 = _run_gpu(torch, scenes, prm, capi.AMK_TIES_NANOFLANN, 2)
    g0, _ = _run_gpu(torch, scenes, prm, capi.AMK_TIES_LOWEST_INDEX, 2)
    cpu = _oracle_steps(quant, prm, 2)
    w = compare([{k: r[k][Q] for k in KEYS} for r in g2], cpu, tol=TOL)
    for t in range(2):
        for k in KEYS:
            assert np.array_equal(g2[t][k][Q].view(np.int64 if g2[t][k].dtype == np.float64 else g2[t][k].dtype),
                                  g1[t][k][Q].view(np.int64 if g1[t][k].dtype == np.float64 else g1[t][k].dtype)), \
                ("AUTO != NANOFLANN on quantised scenes", t, k, np.argwhere(g2[t][k][Q] != g1[t][k][Q])[:4].tolist())
            assert np.array_equal(g2[t][k][P], g0[t][k][P]), ("AUTO != default on tie-free scenes", t, k)
    differ = sum(np.abs(g0[0]["u"][s] - cpu[0][s]["u"]).max() > 1e-6 or
                 np.abs(g0[0]["ref_path"][s] - cpu[0][s]["ref_path"]).max() > 0 for s in range(16))
    print(f"AUTO step: worst |gpu - oracle| on the quantised scenes = {w:.3e}; default tie policy differs from the reference on "
          f"{differ}/16 of them; status obstacle {st2[0].tolist()} edge {st2[1].tolist()}")
    assert differ >= 1
    for st in st2:
        assert (st[P] == capi.AMK_EXACT_NOT_NEEDED).all(), st
    assert (st2[0][Q] == capi.AMK_EXACT_IN_USE).any() and (st2[1][Q] == capi.AMK_EXACT_IN_USE).any(), st2
    assert set(st2[0].tolist()) <= {capi.AMK_EXACT_IN_USE, capi.AMK_EXACT_NOT_NEEDED}


def test_auto_on_one_handle_only():
    """AUTO on the obstacle handle with the edge handle in NANOFLANN mode, and the other way round, and AUTO beside the default:
    the quantised scenes' step equals the all-NANOFLANN step wherever the pair (2, 1) / (1, 2) is used."""
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import KdBatch, MpcBatch, step_batch
    prm = synth.MpcParams(T=1.0, K=3)
    scenes = _quantised_scenes(prm)
    S = len(scenes)
    nmax = max(len(sc["cloud"]) for sc in scenes); emax = max(len(sc["edge"]) for sc in scenes)
    cl = np.zeros((S, nmax, 3), np.float32); ed = np.zeros((S, emax, 3), np.float32)
    cn = np.zeros(S, np.int32); en = np.zeros(S, np.int32)
    for s, sc in enumerate(scenes):
        cl[s, :len(sc["cloud"])] = sc["cloud"]; cn[s] = len(sc["cloud"])
        ed[s, :len(sc["edge"])] = sc["edge"]; en[s] = len(sc["edge"])
    sq = torch.from_numpy(np.stack([_oracle.scene_state_quads(sc, prm) for sc in scenes])).cuda()
    pos_x = torch.from_numpy(np.array([sc["pos"][0] for sc in scenes])).cuda()
    res = {}
    for mo, me in ((1, 1), (2, 1), (1, 2), (2, 2)):
        kd_o, kd_e = KdBatch(S, nmax), KdBatch(S, emax)
        kd_o.set_tie_order(mo); kd_e.set_tie_order(me)
        kd_o.build(torch.from_numpy(cl).cuda(), torch.from_numpy(cn).cuda())
        kd_e.build(torch.from_numpy(ed).cuda(), torch.from_numpy(en).cuda())
        mpc = MpcBatch(prm.T, prm.dt, prm.K, S); mpc.configure(prm)
        ref = torch.from_numpy(np.stack([sc["ref_path"] for sc in scenes])).cuda()
        out = step_batch(kd_o, kd_e, mpc, prm, sq, pos_x, ref)
        torch.cuda.synchronize()
        res[(mo, me)] = dict(u=out["u"].clone(), x0array=out["x0array"].clone(), flags=out["flags"].clone(), ref_path=ref.clone())
        kd_o.close(); kd_e.close(); mpc.close()
    for pair in ((2, 1), (1, 2), (2, 2)):
        for k in KEYS:
            assert torch.equal(res[pair][k], res[(1, 1)][k]), (pair, k)


def test_auto_step_is_graph_capturable_and_replays_bit_exactly():
    """tests/test_graph_gpu.py with both handles in AMK_TIES_AUTO and clouds that tie (a 0.25 m lattice): both index builds and the
    step -- tie detection, the lazy tree builds, the re-answers -- captured in a HIP graph; the replay returns the bits of the
    direct call.  Nothing in the AUTO step synchronises, allocates or branches on device data on the host."""
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import KdBatch, MpcBatch, step_batch
    S, n = 4, 5000
    prm = synth.MpcParams(T=0.66, K=8)
    dev = torch.device("cuda"); N = prm.N
    clouds, edges = synth.make_clouds_torch(n, S, 4242, dev)
    clouds = (torch.round(clouds * 4) / 4).contiguous(); edges = (torch.round(edges * 4) / 4).contiguous()
    sq = np.zeros((S, prm.max_iter, 10)); ref0 = np.zeros((S, N, 10)); posx = np.zeros(S)
    for s in range(S):
        pos, vel, acc, yaw = synth.make_odom(4242 + s, prm)
        sq[s] = fsm.state_quads(pos, vel, acc, yaw, prm.decay, prm.max_iter)
        ref0[s] = synth.make_ref_path(pos, prm); posx[s] = pos[0]
    ref0[:, :, :3] = np.round(ref0[:, :, :3] * 8) / 8
    sq = torch.from_numpy(sq).to(dev); ref0 = torch.from_numpy(ref0).to(dev); posx = torch.from_numpy(posx).to(dev)
    kd_o, kd_e = KdBatch(S, n), KdBatch(S, n // 10)
    kd_o.set_tie_order(capi.AMK_TIES_AUTO); kd_e.set_tie_order(capi.AMK_TIES_AUTO)
    mpc = MpcBatch(prm.T, prm.dt, prm.K, S); mpc.configure(prm)
    ref = ref0.clone()
    out = dict(u=torch.empty((S, 4), dtype=torch.float64, device=dev),
               x0array=torch.empty((S, N, 14), dtype=torch.float64, device=dev),
               flags=torch.empty((S, 4), dtype=torch.int32, device=dev))
    st = torch.cuda.Stream()

    def step():
        ref.copy_(ref0, non_blocking=True); mpc.reset_warm_start(st)
        kd_o.build(clouds, stream=st); kd_e.build(edges, stream=st)
        step_batch(kd_o, kd_e, mpc, prm, sq, posx, ref, stream=st, out=out)

    with torch.cuda.stream(st):
        step()                                   # allocates the workspaces
        step()
    st.synchronize()
    direct = {k: v.clone() for k, v in out.items()}; ref_direct = ref.clone()
    assert int(direct["flags"][:, 1].min()) >= 1
    with torch.cuda.stream(st):
        status = kd_o.exact_status(stream=st)
    st.synchronize()
    assert bool((status == capi.AMK_EXACT_IN_USE).any()), status      # the captured work includes real tree builds
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        step()
    for v in out.values():
        v.zero_()
    g.replay(); torch.cuda.synchronize()
    assert all(torch.equal(out[k], direct[k]) for k in out) and torch.equal(ref, ref_direct)
    g.replay(); torch.cuda.synchronize()          # and again: the step is a pure function of its inputs
    assert all(torch.equal(out[k], direct[k]) for k in out)
    # the same step with the trees built at every build
    kd_o.set_tie_order(capi.AMK_TIES_NANOFLANN); kd_e.set_tie_order(capi.AMK_TIES_NANOFLANN)
    with torch.cuda.stream(st):
        step()
    st.synchronize()
    assert all(torch.equal(out[k], direct[k]) for k in out) and torch.equal(ref, ref_direct)


def test_multi_frame_step_refuses_auto_handles():
    """amk_step_batch_frames with a frame handle in AMK_TIES_AUTO: AMK_ERR_UNSUPPORTED before anything is launched (outputs and the
    reference path untouched) -- on the current frame or a keyframe, obstacle or edge handle."""
    import ctypes as C
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import KdBatch, MpcBatch, step_batch_frames
    prm = synth.MpcParams(T=0.66, K=8)
    S = 2
    scenes = [synth.make_scene(3000, 77 + i, prm) for i in range(S)]
    N = prm.N

    def handle(key, mode):
        nmax = max(len(sc[key]) for sc in scenes)
        buf = np.zeros((S, nmax, 3), np.float32); cnt = np.zeros(S, np.int32)
        for s, sc in enumerate(scenes):
            buf[s, :len(sc[key])] = sc[key]; cnt[s] = len(sc[key])
        kd = KdBatch(S, nmax); kd.set_tie_order(mode); kd.build(torch.from_numpy(buf).cuda(), torch.from_numpy(cnt).cuda())
        return kd

    mpc = MpcBatch(prm.T, prm.dt, prm.K, S); mpc.configure(prm)
    sq = torch.from_numpy(np.stack([_oracle.scene_state_quads(sc, prm) for sc in scenes])).cuda()
    pos_x = torch.from_numpy(np.array([sc["pos"][0] for sc in scenes])).cuda()
    ref0 = torch.from_numpy(np.stack([sc["ref_path"] for sc in scenes])).cuda()
    sp = capi.StepParams(float(prm.speed), float(prm.safety_distance), int(prm.max_iter), 0)
    for which in ((2, 0, 0, 0), (0, 2, 0, 0), (0, 0, 2, 0), (0, 0, 0, 2)):
        ob = [handle("cloud", which[0]), handle("cloud", which[2])]
        ed = [handle("edge", which[1]), handle("edge", which[3])]
        ref = ref0.clone()
        out = dict(u=torch.full((S, 4), -7.0, dtype=torch.float64, device="cuda"),
                   x0array=torch.full((S, N, 14), -7.0, dtype=torch.float64, device="cuda"),
                   flags=torch.full((S, 4), -7, dtype=torch.int32, device="cuda"))
        oa = (C.c_void_p * 2)(*[k.h for k in ob]); ea = (C.c_void_p * 2)(*[k.h for k in ed])
        rc = capi.load().amk_step_batch_frames(oa, ea, 2, None, None, mpc.h, C.byref(sp), capi.dptr(sq), capi.dptr(pos_x),
                                               capi.dptr(ref), capi.dptr(out["u"]), capi.dptr(out["x0array"]),
                                               capi.dptr(out["flags"]), None)
        torch.cuda.synchronize()
        assert rc == capi.AMK_ERR_UNSUPPORTED, (which, rc)
        assert all(bool((v == -7).all()) for v in out.values()) and torch.equal(ref, ref0), which
        for k in ob + ed:
            k.close()
    # the same frames in the default mode are served
    ob = [handle("cloud", 0), handle("cloud", 0)]; ed = [handle("edge", 0), handle("edge", 0)]
    o = step_batch_frames(ob, ed, mpc, prm, sq, pos_x, ref0.clone())
    torch.cuda.synchronize()
    assert int(o["flags"][:, 1].min()) >= 0


def test_pipeline_honours_auto_without_keyframes_and_refuses_it_with_them():
    """amk_pipeline_*: a slot whose handles (amk_pipeline_kd) are in AMK_TIES_AUTO runs the single-frame step in that mode -- gang 1
    (amk_kd_build_pair) and gang 2 (one build launch for the gang's frames) give the bits of the same pipeline in
    AMK_TIES_NANOFLANN on the quantised scenes.  With keyframe handles in the frame, or with a keyframe map, the slot reports
    AMK_ERR_UNSUPPORTED from its submit / wait / drain."""
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import KdBatch, Pipeline
    prm = synth.MpcParams(T=1.0, K=3)
    scenes = _quantised_scenes(prm)
    S = len(scenes)
    n = max(len(sc["cloud"]) for sc in scenes); ne = max(len(sc["edge"]) for sc in scenes)

    def packed(key, cap):
        buf = np.zeros((S, cap, 3), np.float32); cnt = np.zeros(S, np.int32)
        for s, sc in enumerate(scenes):
            buf[s, :len(sc[key])] = sc[key]; cnt[s] = len(sc[key])
        return torch.from_numpy(buf).cuda(), torch.from_numpy(cnt).cuda()

    cl, cn = packed("cloud", n); ed, en = packed("edge", ne)
    sq = torch.from_numpy(np.stack([_oracle.scene_state_quads(sc, prm) for sc in scenes])).cuda()
    pos_x = torch.from_numpy(np.array([sc["pos"][0] for sc in scenes])).cuda()
    ref0 = torch.from_numpy(np.stack([sc["ref_path"] for sc in scenes])).cuda()
    for gang in (1, 2):
        res = {}
        for mode in (capi.AMK_TIES_NANOFLANN, capi.AMK_TIES_AUTO):
            pl = Pipeline(1, S, n, ne, prm, gang=gang)
            pl.kd(0, 0).set_tie_order(mode); pl.kd(0, 1).set_tie_order(mode)
            ts = [pl.submit(cl, ed, sq, pos_x, ref0, cloud_counts=cn, edge_counts=en) for _ in range(gang)]
            pl.drain()
            res[mode] = [pl.outputs(t) for t in ts]
            if mode == capi.AMK_TIES_AUTO:
                st = pl.kd(0, 0).exact_status().cpu().numpy()
                assert (st[:S] == capi.AMK_EXACT_IN_USE).all(), (gang, st)
            pl.close()
        for a, b in zip(res[capi.AMK_TIES_AUTO], res[capi.AMK_TIES_NANOFLANN]):
            for k in ("u", "flags", "ref_path"):
                assert np.array_equal(a[k], b[k]), (gang, k)
    # keyframe handles in the frame: the multi-frame step is not for this mode
    kd_o, kd_e = KdBatch(S, n), KdBatch(S, ne)
    kd_o.build(cl, cn); kd_e.build(ed, en)
    pl = Pipeline(1, S, n, ne, prm)
    pl.kd(0, 1).set_tie_order(capi.AMK_TIES_AUTO)
    with pytest.raises(capi.AmkError, match="status 4"):
        t = pl.submit(cl, ed, sq, pos_x, ref0, cloud_counts=cn, edge_counts=en, keyframes=[(kd_o, kd_e)])
        pl.wait(t); pl.drain()
    pl.close()
    # a keyframe map
    Tw = torch.from_numpy(np.repeat(np.eye(4)[None], S, 0).copy()).cuda()
    cam = capi.FrameCamera(32.0, 32.0, 32.0, 24.0, 6.0, 64, 48)
    pl = Pipeline(1, S, n, ne, prm, keyframes=dict(max_frame_count=3, th_dist=0.1, th_count=10, depth_min=0.1))
    pl.kd(0, 0).set_tie_order(capi.AMK_TIES_AUTO)
    with pytest.raises(capi.AmkError, match="status 4"):
        t = pl.submit(cl, ed, sq, pos_x, ref0, cloud_counts=cn, edge_counts=en, Twc_cur=Tw, cam=cam)
        pl.wait(t); pl.drain()
    pl.close()
    kd_o.close(); kd_e.close()
