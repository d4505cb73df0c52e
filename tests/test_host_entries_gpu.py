"""GPU: the *_host entry points of one handle, interleaved.  The entries of a handle stage through one block of device memory that
every call lays out afresh and that grows between calls (csrc/host_stage.h), so each case runs several entries on a single handle
and compares every host result BIT FOR BIT with the device-pointer twin of the same call, run on a second handle fed the same data:
the same kernels on the same inputs, no tolerance.  The shapes are the smallest at which staging can go wrong: two scenes, one tile,
a block that grows from one call to the next, outputs nobody asked for, scenes and handles without a point."""
import ctypes as C

import numpy as np
import pytest

from avoid_mpc_amd import synth

pytestmark = pytest.mark.gpu


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def assert_same_bits(got, want, what):
    want = want.cpu().numpy() if hasattr(want, "cpu") else np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), what


# ---------------------------------------------------------------------------------------------------------------- amk_kd
KD_S, KD_CAP = 2, 300   # one tile


def _kd_search_both(host, dev, q, k, what):
    import torch
    h = host.search_host(q, k)
    d = dev.search(torch.from_numpy(q).cuda(), k)
    torch.cuda.synchronize()
    for key in ("indices", "sqdist", "pts", "counts"):
        assert_same_bits(h[key], d[key], f"{what}: {key}")
    return h


@pytest.mark.parametrize("tie", [0, 1], ids=["lowest_index", "nanoflann"])
def test_kd_entries_interleaved_on_one_handle(tie):
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import KdBatch
    rng = np.random.default_rng(11)
    cloud_a = (rng.random((KD_S, KD_CAP, 3)) * [8.0, 6.0, 3.0]).astype(np.float32)
    cloud_b = (rng.random((KD_S, KD_CAP, 3)) * [8.0, 6.0, 3.0] + [1.0, -3.0, 0.5]).astype(np.float32)
    counts = np.array([300, 17], np.int32)
    q1 = rng.random((KD_S, 1, 3)) * [8.0, 6.0, 3.0]
    q9 = rng.random((KD_S, 9, 3)) * [8.0, 6.0, 3.0]
    host, dev = KdBatch(KD_S, KD_CAP), KdBatch(KD_S, KD_CAP)
    lib = host.lib
    try:
        for kd in (host, dev):
            kd.set_tie_order(tie)
        # 1, 2: a build with counts, then two searches of which the second needs a larger block
        host.build_host(cloud_a, counts)
        dev.build(torch.from_numpy(cloud_a).cuda(), torch.from_numpy(counts).cuda())
        _kd_search_both(host, dev, q1, 3, "Q = 1, k = 3")
        first = _kd_search_both(host, dev, q9, 5, "Q = 9, k = 5")
        assert (first["counts"] == 5).all()
        # 3, 4: another cloud from a buffer that ends at the last counted point of the last scene; the searches answer for it
        short = np.ascontiguousarray(cloud_b.reshape(-1)[:(KD_S - 1) * KD_CAP * 3 + int(counts[-1]) * 3])
        capi.check(lib.amk_kd_build_host(host.h, vp(short), 3, KD_CAP * 3, vp(counts)), "amk_kd_build_host, short buffer")
        dev.build(torch.from_numpy(cloud_b).cuda(), torch.from_numpy(counts).cuda())
        second = _kd_search_both(host, dev, q9, 5, "Q = 9, k = 5 after the second build")
        assert not np.array_equal(first["pts"], second["pts"])
        for s in range(KD_S):   # (the answers are points of the new cloud's counted part)
            assert (second["pts"][s] == cloud_b[s][second["indices"][s]]).all() and second["indices"][s].max() < counts[s]
        _kd_search_both(host, dev, q1, 3, "Q = 1, k = 3 in the grown block")
        # 5: the points as the handle holds them
        xyz = np.full((KD_S, KD_CAP, 3), -7.0, np.float32); sizes = np.full(KD_S, -7, np.int32)
        xyz_d = xyz.copy(); sizes_d = sizes.copy()
        capi.check(lib.amk_kd_points_host(host.h, vp(xyz), vp(sizes)), "amk_kd_points_host")
        capi.check(lib.amk_kd_points_host(dev.h, vp(xyz_d), vp(sizes_d)), "amk_kd_points_host, device-built handle")
        assert_same_bits(sizes, counts, "sizes"); assert_same_bits(xyz, xyz_d, "points of the two handles")
        for s in range(KD_S):
            assert_same_bits(xyz[s, :counts[s]], cloud_b[s, :counts[s]], f"points of scene {s}")
            assert (xyz[s, counts[s]:] == -7.0).all()
        # 6: which index answers
        status = np.full(KD_S, -7, np.int32)
        capi.check(lib.amk_kd_exact_status_host(host.h, vp(status)), "amk_kd_exact_status_host")
        assert_same_bits(status, dev.exact_status(), "exact status")
        assert (status == (capi.AMK_EXACT_IN_USE if tie else capi.AMK_EXACT_OFF)).all()
        # a scene without a point, then the searches once more
        counts0 = np.array([0, 300], np.int32)
        host.build_host(cloud_a, counts0)
        dev.build(torch.from_numpy(cloud_a).cuda(), torch.from_numpy(counts0).cuda())
        empty = _kd_search_both(host, dev, q9, 5, "a scene with count 0")
        assert (empty["counts"][0] == 0).all() and (empty["counts"][1] == 5).all()
    finally:
        host.close(); dev.close()


def test_kd_handle_without_capacity():
    """max_points = 0: every slot of the build is empty or a single float, the searches find nothing"""
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import KdBatch
    host, dev = KdBatch(KD_S, 0), KdBatch(KD_S, 0)
    try:
        none = np.zeros((KD_S, 0, 3), np.float32); counts = np.zeros(KD_S, np.int32)
        host.build_host(none, counts)
        capi.check(host.lib.amk_kd_build_host(host.h, None, 3, 0, None), "amk_kd_build_host without a buffer")
        dev.build(torch.from_numpy(none).cuda(), torch.from_numpy(counts).cuda())
        q = np.random.default_rng(5).random((KD_S, 4, 3))
        out = _kd_search_both(host, dev, q, 3, "max_points = 0")
        assert (out["counts"] == 0).all()
        xyz = np.full((1, 3), -7.0, np.float32); sizes = np.full(KD_S, -7, np.int32)
        capi.check(host.lib.amk_kd_points_host(host.h, vp(xyz), vp(sizes)), "amk_kd_points_host")
        assert (sizes == 0).all() and (xyz == -7.0).all()
    finally:
        host.close(); dev.close()


# --------------------------------------------------------------------------------------------------------------- amk_mpc
def _mpc_problem():
    """S = 2 at the smallest horizon and K of the MPC tests (N = 7: the generic kernel; K = 2): evaluation points as
    tests/test_mpc_eval_gpu.py makes them, and two single-frame scenes for the control step"""
    from tests.test_mpc_eval_gpu import _points_at
    prm = synth.MpcParams(T=7 * 0.033 + 1e-4, K=2)
    prm, W, R = _points_at(prm, 2, 3)
    scenes = [synth.make_scene(400, seed, prm) for seed in (21, 22)]
    sq = np.stack([[np.concatenate([sc["pos"] + sc["vel"] * prm.decay * (i + 1), [sc["yaw"]], sc["vel"], sc["acc"]])
                    for i in range(prm.max_iter)] for sc in scenes])
    return prm, W, R, scenes, np.ascontiguousarray(sq)


def test_mpc_entries_interleaved_on_one_handle():
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import KdBatch, MpcBatch, step_batch
    prm, W, R, scenes, sq = _mpc_problem()
    S, N = 2, prm.N
    assert N == 7
    host, dev = MpcBatch(prm.T, prm.dt, prm.K, S), MpcBatch(prm.T, prm.dt, prm.K, S)
    kds = []
    for key in ("cloud", "edge"):
        kd = KdBatch(S, len(scenes[0][key]))
        kd.build(torch.from_numpy(np.stack([sc[key] for sc in scenes])).cuda())
        kds.append(kd)
    lib = host.lib
    nx, ng, np_ = host.nx, lib.amk_mpc_ng(host.h), lib.amk_mpc_np(host.h)
    nj, nh = lib.amk_mpc_jac_nnz(host.h), lib.amk_mpc_hess_nnz(host.h)
    dW, dR = torch.from_numpy(W).cuda(), torch.from_numpy(R).cuda()
    lam_f = np.array([0.5, 2.0]); lam_g = np.random.default_rng(4).normal(size=(S, ng))

    def evals(what, want):
        """amk_mpc_eval_host with the outputs `want` (the others NULL) against amk_mpc_eval with the same ones"""
        shape = dict(f=(S,), grad_f=(S, nx), g=(S, ng), jac_g=(S, nj), hess_l=(S, nh))
        h = {k: np.full(shape[k], -7.0) for k in want}
        lf = lam_f if "hess_l" in want else None
        capi.check(lib.amk_mpc_eval_host(host.h, vp(W), vp(R), vp(lf), *[vp(h.get(k)) for k in ("f", "grad_f", "g", "jac_g", "hess_l")]), what)
        d = dev.eval(dW, dR, torch.from_numpy(lf).cuda() if lf is not None else None, want=want)
        torch.cuda.synchronize()
        for k in want:
            assert_same_bits(h[k], d[k], f"{what}: {k}")

    def solves(what, want_traj, want_info):
        u = np.full((S, 4), -7.0); x0 = np.full((S, N, 14), -7.0) if want_traj else None
        info = np.full((S, 4), -7, np.int32) if want_info else None
        capi.check(lib.amk_mpc_solve_host(host.h, vp(R), vp(u), vp(x0), vp(info), 0), what)
        du, dx0, dinfo = dev.Solve(dR)
        torch.cuda.synchronize()
        assert_same_bits(u, du, f"{what}: u")
        if want_traj:
            assert_same_bits(x0, dx0, f"{what}: x0array")
        if want_info:
            assert_same_bits(info, dinfo, f"{what}: info")
        assert_same_bits(host.get_warm_start().cpu().numpy(), dev.get_warm_start(), f"{what}: warm start")

    try:
        for m in (host, dev):
            m.configure(prm)
        evals("eval, three outputs", ("f", "g", "hess_l"))
        solves("solve, every output", True, True)
        # gamma: grad_x only, then both gradients without lam_f
        gx = np.full((S, nx), -7.0); gp = np.full((S, np_), -7.0)
        dgx = torch.empty((S, nx), dtype=torch.float64, device="cuda"); dgp = torch.empty((S, np_), dtype=torch.float64, device="cuda")
        dlf, dlg = torch.from_numpy(lam_f).cuda(), torch.from_numpy(lam_g).cuda()
        capi.check(lib.amk_mpc_eval_gamma_host(host.h, vp(W), vp(R), vp(lam_f), vp(lam_g), vp(gx), None), "gamma, grad_x")
        capi.check(lib.amk_mpc_eval_gamma(dev.h, capi.dptr(dW), capi.dptr(dR), capi.dptr(dlf), capi.dptr(dlg), capi.dptr(dgx), None,
                                          capi.stream_ptr()), "amk_mpc_eval_gamma")
        assert_same_bits(gx, dgx, "gamma: grad_x")
        capi.check(lib.amk_mpc_eval_gamma_host(host.h, vp(W), vp(R), None, vp(lam_g), vp(gx), vp(gp)), "gamma, both, no lam_f")
        capi.check(lib.amk_mpc_eval_gamma(dev.h, capi.dptr(dW), capi.dptr(dR), None, capi.dptr(dlg), capi.dptr(dgx), capi.dptr(dgp),
                                          capi.stream_ptr()), "amk_mpc_eval_gamma")
        assert_same_bits(gx, dgx, "gamma without lam_f: grad_x"); assert_same_bits(gp, dgp, "gamma without lam_f: grad_p")
        # the control step, without the trajectory
        pos_x = np.array([sc["pos"][0] for sc in scenes]); ref = np.stack([sc["ref_path"] for sc in scenes])
        dref = torch.from_numpy(ref).cuda()
        u = np.full((S, 4), -7.0); flags = np.full((S, 4), -7, np.int32)
        sp = capi.StepParams(float(prm.speed), float(prm.safety_distance), int(prm.max_iter), 0)
        capi.check(lib.amk_step_batch_host(kds[0].h, kds[1].h, host.h, C.byref(sp), vp(sq), vp(pos_x), vp(ref), vp(u), None, vp(flags)),
                   "amk_step_batch_host")
        o = step_batch(kds[0], kds[1], dev, prm, torch.from_numpy(sq).cuda(), torch.from_numpy(pos_x).cuda(), dref)
        torch.cuda.synchronize()
        assert_same_bits(u, o["u"], "step: u"); assert_same_bits(flags, o["flags"], "step: flags"); assert_same_bits(ref, dref, "step: ref_path")
        assert_same_bits(host.ref_states(), dev.ref_states(), "step: P")
        assert (flags[:, 1] >= 1).all()   # every scene solved at least once
        # the first two again, in the block the step left behind, with other outputs
        evals("eval again, every output", ("f", "grad_f", "g", "jac_g", "hess_l"))
        solves("solve again, u alone", False, False)
    finally:
        for h in [host, dev] + kds:
            h.close()


# ------------------------------------------------------------------------------------------------------------- amk_kfmap
def test_kfmap_entries_interleaved_on_one_handle():
    """One map, two add_vertex + update rounds, then its host entries one after the other; a second map fed the same frames answers
    the device-pointer queries."""
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import KfMap
    S, CAP, ECAP, NQ = 2, 64, 16, 5
    Tbc = np.eye(4)
    rng = np.random.default_rng(8)
    maps = [KfMap(S, CAP, ECAP, 3, 0.3, 1, 0.3, Tbc) for _ in range(2)]
    host, dev = maps
    lib = host.lib
    try:
        sizes = []
        for t, d in enumerate((0.0, 0.8)):
            cn = np.array([64, 23], np.int32) - 7 * t; en = np.array([16, 5], np.int32)
            cl = (rng.random((S, CAP, 3)) * [6.0, 6.0, 3.0] + [d + 1.0, -3.0, 0.0]).astype(np.float32)
            ed = (rng.random((S, ECAP, 3)) * [6.0, 6.0, 3.0] + [d + 1.0, -3.0, 0.0]).astype(np.float32)
            Tw = np.stack([np.eye(4)] * S); Tw[:, 0, 3] = d; Tw[:, 2, 3] = 1.5
            for m in maps:
                m.add_vertex(torch.from_numpy(cl).cuda(), torch.from_numpy(ed).cuda(), torch.from_numpy(Tw).cuda(),
                             counts=torch.from_numpy(cn).cuda(), edge_counts=torch.from_numpy(en).cuda())
                m.update()
            sizes.append(cn)
        q = rng.random((S, NQ, 3)) * [8.0, 6.0, 3.0] + [0.0, -3.0, 0.0]
        dq = torch.from_numpy(q).cuda()
        for k, edge in ((1, 0), (4, 0), (4, 1)):
            hp = np.full((S, NQ, k, 3), -7.0, np.float32); hd = np.full((S, NQ, k), -7.0); hf = np.full((S, NQ, k), -7, np.int32)
            hc = np.full((S, NQ), -7, np.int32)
            capi.check(lib.amk_kfmap_query_nearest_host(host.h, None, vp(q), 3, NQ, k, edge, vp(hp), vp(hd), vp(hf), vp(hc)), "query host")
            o = dev.query_nearest(dq, k, edge=bool(edge))
            torch.cuda.synchronize()
            for key, got in (("pts", hp), ("sqdist", hd), ("frame", hf), ("counts", hc)):
                assert_same_bits(got, o[key], f"query_nearest_host k = {k}, edge = {edge}: {key}")
            assert (hf >= 0).all() if not edge else True
        # k = 4 once more with two outputs only (the block holds the layout of the call before)
        hd2 = np.full((S, NQ, 4), -7.0); hc2 = np.full((S, NQ), -7, np.int32)
        capi.check(lib.amk_kfmap_query_nearest_host(host.h, None, vp(q), 3, NQ, 4, 0, None, vp(hd2), None, vp(hc2)), "query host, two outputs")
        o = dev.query_nearest(dq, 4)
        assert_same_bits(hd2, o["sqdist"], "two outputs: sqdist"); assert_same_bits(hc2, o["counts"], "two outputs: counts")
        hdist = np.full((S, NQ), -7.0)
        capi.check(lib.amk_kfmap_nearest_distance_host(host.h, vp(q), 3, NQ, vp(hdist)), "distance host")
        assert_same_bits(hdist, dev.nearest_distance(dq), "nearest_distance_host")
        # the map's state through the read-backs, against the other map's and the frames fed
        st, st_d = host.state(), dev.state()
        for key in st:
            assert_same_bits(st[key], st_d[key], f"state: {key}")
        assert (st["n_query_frames"] >= 1).all() and (st["frame_sizes"][:, 0] == sizes[-1]).all()
        for s in range(S):
            (xyz, sz), (xyz_d, sz_d) = host.points(s), dev.points(s)   # (probe, then fill)
            assert_same_bits(xyz, xyz_d, f"points of scene {s}"); assert_same_bits(sz, sz_d, f"frame sizes of scene {s}")
            assert_same_bits(sz, st["frame_sizes"][s], f"frame sizes of scene {s} against the state's")
            assert len(xyz) == sz[sz > 0].sum()
        ex, ex_d = host.exact_status(), dev.exact_status()
        for key in ex:
            assert_same_bits(ex[key], ex_d[key], f"exact status: {key}")
            assert (ex[key] == capi.AMK_EXACT_OFF).all()
        sl, sl_d = host.slots(), dev.slots()
        for key in sl:
            assert_same_bits(sl[key], sl_d[key], f"slots: {key}")
    finally:
        for m in maps:
            m.close()


def test_kfmap_exact_status_in_the_reference_tie_order():
    """AMK_TIES_NANOFLANN: the status entry launches through the map's block, once per pool, after a query laid it out otherwise"""
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import KfMap
    S, CAP, ECAP = 2, 64, 16
    rng = np.random.default_rng(9)
    m = KfMap(S, CAP, ECAP, 3, 0.3, 1, 0.3, np.eye(4))
    try:
        m.set_tie_order(capi.AMK_TIES_NANOFLANN)
        cl = (rng.random((S, CAP, 3)) * 5.0).astype(np.float32); ed = (rng.random((S, ECAP, 3)) * 5.0).astype(np.float32)
        Tw = np.stack([np.eye(4)] * S)
        m.add_vertex(torch.from_numpy(cl).cuda(), torch.from_numpy(ed).cuda(), torch.from_numpy(Tw).cuda())
        m.update()
        q = rng.random((S, 3, 3)) * 5.0; hd = np.zeros((S, 3, 2))
        capi.check(m.lib.amk_kfmap_query_nearest_host(m.h, None, vp(q), 3, 3, 2, 0, None, vp(hd), None, None), "query host")
        ex = m.exact_status()
        nq = m.state()["n_query_frames"]
        for key in ("obs", "edge"):
            for s in range(S):
                assert (ex[key][s, :nq[s]] == capi.AMK_EXACT_IN_USE).all() and (ex[key][s, nq[s]:] == capi.AMK_EXACT_OFF).all(), (key, s, ex[key][s])
    finally:
        m.close()


# ----------------------------------------------------------------------------------------------------------------- depth
def test_depth_host_entries_equal_their_device_calls():
    """amk_depth_to_edge_cloud_host and amk_depth_to_clouds_host had no comparison of their outputs in Python (the C++ adapters call them);
    amk_depth_to_cloud_host beside them.  Two 60 x 80 frames at scale 2, two pixel types."""
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import depth_params, depth_to_cloud, depth_to_clouds
    lib = capi.load()
    S, rows, cols = 2, 60, 80
    rng = np.random.default_rng(2)
    yy, xx = np.mgrid[0:rows, 0:cols]
    base = 2.0 + 0.02 * xx + (xx // 16 % 2) * 1.5 + (yy // 20) * 0.5
    Twb = np.stack([np.eye(4)] * S); Twb[1, :3, 3] = [1.0, -2.0, 1.5]
    Twc = Twb.copy(); Twc[:, 0, 3] -= 0.25
    for dtype, kind, p2m in ((np.float32, capi.AMK_DEPTH_F32, 1.0), (np.uint16, capi.AMK_DEPTH_U16, 0.001)):
        img = np.stack([base, base[::-1] + 0.3]) + rng.random((S, rows, cols)) * 0.01
        img = np.ascontiguousarray((img / p2m).astype(dtype))
        p = depth_params(pixel2meter=p2m, depth_min=0.1, depth_max=20.0, resize_scale=2.0, fx=40.0, fy=40.0, cx=40.0, cy=30.0)
        dimg = torch.from_numpy(img.view(np.int16) if dtype == np.uint16 else img).cuda()
        dTwb, dTwc = torch.from_numpy(Twb).cuda(), torch.from_numpy(Twc).cuda()
        cap = 40 * 30
        new = lambda: (np.zeros((S, cap, 3), np.float32), np.full(S, -7, np.int32))
        for fn, edge, T, dT in ((lib.amk_depth_to_cloud_host, False, Twb, dTwb), (lib.amk_depth_to_edge_cloud_host, True, Twc, dTwc)):
            cloud, cnt = new()
            capi.check(fn(vp(img), kind, rows, cols, rows * cols, S, C.byref(p), vp(T), vp(cloud), 3, cap * 3, vp(cnt)), "one cloud, host")
            dcloud, dcnt = depth_to_cloud(dimg, p, dT, edge=edge)
            torch.cuda.synchronize()
            assert_same_bits(cnt, dcnt, f"edge = {edge}: counts"); assert (cnt > 0).all()
            for s in range(S):
                assert_same_bits(cloud[s, :cnt[s]], dcloud[s, :cnt[s]], f"edge = {edge}: cloud of scene {s}")
        (cloud, cnt), (ecloud, ecnt) = new(), new()
        capi.check(lib.amk_depth_to_clouds_host(vp(img), kind, rows, cols, rows * cols, S, C.byref(p), vp(Twb), vp(Twc), vp(cloud), cap * 3,
                                                vp(cnt), vp(ecloud), cap * 3, vp(ecnt), 3), "amk_depth_to_clouds_host")
        dcloud, dcnt, decloud, decnt = depth_to_clouds(dimg, p, dTwb, dTwc)
        torch.cuda.synchronize()
        assert_same_bits(cnt, dcnt, "both clouds: counts"); assert_same_bits(ecnt, decnt, "both clouds: edge counts")
        assert (cnt > 0).all() and (ecnt > 0).all()
        for s in range(S):
            assert_same_bits(cloud[s, :cnt[s]], dcloud[s, :cnt[s]], f"both clouds: cloud of scene {s}")
            assert_same_bits(ecloud[s, :ecnt[s]], decloud[s, :ecnt[s]], f"both clouds: edge cloud of scene {s}")
