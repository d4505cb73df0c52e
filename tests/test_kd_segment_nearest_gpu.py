"""GPU: amk_kd_segment_nearest (kd_segment_nearest_kernel / grid_segment_knn, csrc/kd_segment_nearest.hip + csrc/kd_grid.h) against
the numpy brute force of tests/_segment_nearest.py, sentence by sentence of the header's contract.  Every comparison is bit for
bit: counts, indices, squared distances, t, points.  Sizes are the smallest that reach the mechanism named in each test."""
import ctypes as C

import numpy as np
import pytest

from tests import _segment_nearest as N

pytestmark = pytest.mark.gpu

DBL_MAX = N.DBL_MAX
KEYS = ("counts", "indices", "sqdist", "t", "pts")


def pack(clouds, cap=None):
    S = len(clouds)
    cap = cap or max(1, max(len(c) for c in clouds))
    xyz = np.zeros((S, cap, 3), np.float32)
    counts = np.zeros(S, np.int32)
    for s, c in enumerate(clouds):
        xyz[s, :len(c)] = np.asarray(c, np.float32).reshape(-1, 3)
        counts[s] = len(c)
    return xyz, counts, cap


def nearest(clouds, path, k, host=False, segment_inf=False, knn_at=None):
    """clouds: one raw cloud per scene (ragged); path float64 [S, P, >= 3] -> numpy dict of the device (or _host) answer.
    segment_inf: KdBatch.segment_search(path, inf, k) on the same index instead; knn_at: queries [S, Q, 3] -> KdBatch.search"""
    import torch
    from avoid_mpc_amd.host import KdBatch
    xyz, counts, cap = pack(clouds)
    kd = KdBatch(len(clouds), cap)
    try:
        kd.build(torch.from_numpy(xyz).cuda(), torch.from_numpy(counts).cuda())
        if host:
            return kd.segment_nearest_host(path, k)
        if knn_at is not None:
            out = kd.search(torch.from_numpy(np.ascontiguousarray(knn_at[:, :, :3])).cuda(), k)
            torch.cuda.synchronize()
            return {key: v.cpu().numpy() for key, v in out.items()}
        dpath = torch.from_numpy(np.ascontiguousarray(path)).cuda()
        out = kd.segment_search(dpath, float("inf"), k) if segment_inf else kd.segment_nearest(dpath, k)
        torch.cuda.synchronize()
        return {key: (v.cpu().numpy() if v is not None else None) for key, v in out.items()}
    finally:
        kd.close()


def check(clouds, path, k, what="", **kw):
    got = nearest(clouds, path, k, **kw)
    want = N.expected_batch([[c] for c in clouds], path, k)
    N.assert_bitwise(got, want, KEYS, what)
    return got, want


def test_a_case_done_by_hand():
    """where the answer is known without any program: a unit leg along x, points beside its ends and its middle"""
    cloud = np.array([[-1.0, 0.0, 0.0], [0.25, 1.0, 0.0], [3.0, 0.0, 2.0], [0.5, 0.0, 0.0]], np.float32)
    path = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]])
    got, _ = check([cloud], path, 4, "by hand, k 4")
    assert got["counts"].tolist() == [[4]] and got["indices"][0, 0].tolist() == [3, 0, 1, 2]
    assert got["sqdist"][0, 0].tolist() == [0.0, 1.0, 1.0, 8.0] and got["t"][0, 0].tolist() == [0.5, 0.0, 0.25, 1.0]
    assert got["pts"][0, 0, 0].tolist() == [0.5, 0.0, 0.0]
    got, _ = check([cloud], path, 2, "by hand, k 2")
    assert got["counts"].tolist() == [[2]] and got["indices"][0, 0].tolist() == [3, 0]   # the tie 0 / 1 at the list's end: the lower index
    got, _ = check([cloud], path, 8, "by hand, k 8")
    assert got["counts"].tolist() == [[4]] and got["indices"][0, 0].tolist() == [3, 0, 1, 2, -1, -1, -1, -1]
    assert (got["sqdist"][0, 0, 4:] == DBL_MAX).all() and (got["t"][0, 0, 4:] == 0).all() and (got["pts"][0, 0, 4:] == 0).all()


@pytest.fixture(scope="module")
def slab():
    """the segment tests' slab: 4 133 points with continuous coordinates, a grid of 1 x 10 x 10 cells in two tiles; a short leg in
    its middle and a leg across it"""
    cloud = (np.random.default_rng(7).random((4133, 3)) * [1.0, 12.0, 12.0]).astype(np.float32)
    g, nt = N.grid_dims(cloud)
    assert tuple(g) == (1, 10, 10) and nt == 2
    a = np.array([0.4, 5.0, 5.0])
    short = np.stack([a, a + [0.33, 0.02, 0.01]])[None]
    across = np.array([[[0.5, 1.0, 1.0], [0.5, 11.0, 11.0]]])
    return cloud, short, across


@pytest.mark.parametrize("k", [1, 8, 63, 64])
def test_the_short_leg_is_neither_endpoint(slab, k):
    cloud, short, _ = slab
    got, _ = check([cloud], short, k, f"short leg, k {k}")
    assert got["counts"][0, 0] == k
    if k == 8:
        a, b = short[0, 0], short[0, 1]
        assert set(got["indices"][0, 0].tolist()) == {189, 932, 936, 1228, 1377, 1882, 2456, 3684}
        ea = set(N.nearest_brute(cloud, a, a, 8)["indices"].tolist()); eb = set(N.nearest_brute(cloud, b, b, 8)["indices"].tolist())
        assert {2821, 3364} <= ea and 3370 in eb                       # a kNN at either endpoint answers something else
        t = got["t"][0, 0]
        assert (t == 1).any() and ((t > 0) & (t < 1)).any()


def test_a_thin_capsule_in_a_wide_box(slab):
    """the leg's box spans 100 rows x 2 tiles: a second batch of items runs, and a stop rule or row cull that is eager loses points"""
    cloud, _, across = slab
    got, _ = check([cloud], across, 64, "across")
    t = got["t"][0, 0]
    assert got["counts"][0, 0] == 64 and ((t > 0) & (t < 1)).sum() == 62
    assert 0.0496 < got["sqdist"][0, 0, 63] < 0.0498


def cells_of(cloud):
    """cell coordinates of every point in the index's grid over the cloud (tests/_radius.grid_dims' geometry)"""
    c = cloud.astype(np.float64)
    lo, ext = c.min(axis=0), c.max(axis=0) - c.min(axis=0)
    e = np.maximum(ext, max(ext.max() * 1e-6, 1e-30))
    h = np.cbrt(e.prod() / min(max(len(c) / 64.0, 1.0), 1024.0))
    for _ in range(64):
        g = np.clip(np.ceil(e / h), 1, 1024).astype(int)
        if g.prod() <= 1024:
            break
        h *= 1.26
    return np.clip(np.floor((c - lo) / h), 0, g - 1).astype(int), g, lo, h


def test_empty_shells():
    """a hole in the slab: shells 0 and 1 around the leg hold no point, the eight nearest all lie in shell 2"""
    cloud = (np.random.default_rng(7).random((4133, 3)) * [1.0, 12.0, 12.0]).astype(np.float32)
    y, z = cloud[:, 1], cloud[:, 2]
    cloud = cloud[~((y > 3) & (y < 9) & (z > 3) & (z < 9))]
    g, nt = N.grid_dims(cloud)
    assert len(cloud) == 3114 and tuple(g) == (1, 9, 9) and nt == 1
    path = np.array([[[0.5, 5.9, 6.0], [0.5, 6.2, 6.1]]])
    cell, g2, lo, h = cells_of(cloud)
    assert tuple(g2) == tuple(g)
    clo = np.floor((path[0].min(axis=0) - lo) / h).astype(int); chi = np.floor((path[0].max(axis=0) - lo) / h).astype(int)
    cheb = np.maximum(np.maximum(clo - cell, cell - chi), 0).max(axis=1)     # the shell of every point's cell
    assert (cheb <= 1).sum() == 0 and (cheb == 2).sum() > 8
    got, _ = check([cloud], path, 8, "empty shells")
    assert got["counts"][0, 0] == 8 and 7.95 < got["sqdist"][0, 0, 0] < 7.96
    assert (cheb[got["indices"][0, 0]] == 2).all()


@pytest.fixture(scope="module")
def lattice():
    """the 10 x 10 x 10 integer lattice, 4 133 points: every site is held four or five times"""
    site = np.arange(4133) % 1000
    return np.stack([site % 10, site // 10 % 10, site // 100], axis=1).astype(np.float32)


@pytest.mark.parametrize("k", [1, 8, 64])
def test_runs_of_equal_distances_on_the_lattice(lattice, k):
    path = np.array([[[2.0, 5.0, 3.0], [6.0, 5.0, 3.0], [6.0, 9.0, 3.0], [6.5, 9.0, 8.0]]])
    got, _ = check([lattice], path, k, f"lattice, k {k}")
    # on legs 0 and 1 every k cuts through a run of equal distances and index order decides; on leg 2 only k = 1 does (every site is
    # held four times, so the nearest distance itself occurs four times)
    for leg, cut in ((0, True), (1, True), (2, k == 1)):
        d = np.sort(N.seg_dists(lattice, path[0, leg], path[0, leg + 1])[0])
        assert (d[k - 1] == d[k]) == cut, (leg, k)
    idx, dd = got["indices"][0], got["sqdist"][0]
    assert all(dd[l, i] < dd[l, i + 1] or (dd[l, i] == dd[l, i + 1] and idx[l, i] < idx[l, i + 1]) for l in range(3) for i in range(k - 1))
    # a lone leg (n_points = 2) answers like the same leg inside a path
    lone, _ = check([lattice], path[:, 1:3], k, "lone leg")
    for key in KEYS:
        assert np.array_equal(lone[key][0, 0], got[key][0, 1]), key


def test_points_the_sampled_bounding_box_missed():
    """outliers the bounding-box sample does not read are clamped into boundary cells: no boundary face may bound or stop the walk"""
    cloud = (np.random.default_rng(3).random((20000, 3)) * [30.0, 16.0, 4.0]).astype(np.float32)
    unread = np.flatnonzero((np.arange(20000) // 64) % 16 != 0)[::40][:400]
    assert len(unread) == 400
    rng = np.random.default_rng(4)
    cloud[unread[:200], 0] = (-4.0 + 3.0 * rng.random(200)).astype(np.float32)
    cloud[unread[200:], 1] = (16.5 + 2.0 * rng.random(200)).astype(np.float32)
    out = np.zeros(20000, bool); out[unread] = True
    sampled = cloud[(np.arange(20000) // 64) % 16 == 0]
    assert sampled[:, 0].min() >= 0 and sampled[:, 1].max() <= 16 and cloud[:, 0].min() < -3.9 and cloud[:, 1].max() > 18.4
    path = np.array([[[-3.5, 8.0, 2.0], [-3.2, 8.3, 2.0], [0.1, 8.0, 2.0], [0.4, 8.1, 2.1],
                      [-0.5, 15.9, 2.0], [0.6, 16.8, 2.0], [15.0, 17.5, 1.0], [15.3, 17.6, 1.2]]])
    got, _ = check([cloud], path, 8, "sampled box")
    clamped = out[got["indices"][0]].sum(axis=1)
    assert got["counts"][0].tolist() == [8] * 7
    assert clamped[0] == 8 and clamped[2] == 0 and 0 < clamped[4] < 8 and clamped[6] == 8


def test_fewer_points_than_k_and_no_size_rule():
    rng = np.random.default_rng(19)
    k = 8
    clouds = [(rng.random((n, 3)) * 3.0).astype(np.float32) for n in (0, 1, 5, k, k + 1)]
    path = np.tile((rng.random((3, 3)) * 3.0)[None], (5, 1, 1))
    got, _ = check(clouds, path, k, "few points")
    assert got["counts"].tolist() == [[0, 0], [1, 1], [5, 5], [8, 8], [8, 8]]      # exactly k points: all k, where amk_kd_search gives none
    assert (got["indices"][0] == -1).all() and (got["indices"][2, :, 5:] == -1).all() and (got["sqdist"][2, :, 5:] == DBL_MAX).all()


def test_a_degenerate_leg_is_the_knn_at_its_point(slab, lattice):
    """identity 2: a == b answers with the distances, indices and points of amk_kd_search(k) at a"""
    p = np.random.default_rng(29).random((3, 3)) * [1.0, 12.0, 12.0]
    path = np.stack([p[0], p[0], p[1], p[1], p[2], p[2]])[None]             # legs 0, 2 and 4 have a == b
    for cl, pa in ((slab[0], path), (lattice, np.round(path))):
        got, _ = check([cl], pa, 16, "degenerate")
        knn = nearest([cl], None, 16, knn_at=pa[:, 0::2])
        for key in ("indices", "sqdist", "pts"):
            assert np.array_equal(got[key][:, 0::2], knn[key]), key
        assert (got["t"][:, 0::2] == 0.0).all() and (got["counts"][:, 0::2] == 16).all()


def test_the_lists_are_the_segment_search_without_a_radius(slab, lattice):
    """identity 1, on the device: amk_kd_segment_search(radius_sq = +inf, max_results = k)"""
    rng = np.random.default_rng(31)
    path = rng.random((2, 7, 3)) * [1.0, 12.0, 12.0]
    path[1] = np.round(path[1] * [9.0, 0.75, 0.75])
    for k in (1, 8, 64):
        got = nearest([slab[0], lattice], path, k)
        seg = nearest([slab[0], lattice], path, k, segment_inf=True)
        N.assert_bitwise(got, seg, ("indices", "sqdist", "t", "pts"), f"k {k}")
        assert np.array_equal(got["counts"], np.minimum(seg["counts"], k)) and (seg["counts"] == 4133).all()


def test_non_finite_path_points_and_cloud_points():
    rng = np.random.default_rng(11)
    nan, inf = float("nan"), float("inf")
    clean = (rng.random((3000, 3)) * 6.0).astype(np.float32)
    bad = clean.copy()
    bad[5::50, 0] = nan      # dropped by the build: the indices shift
    bad[7::60, 1] = nan      # kept in the index space, never counted
    bad[9::70, 2] = inf
    bad[11::500, 0] = -inf
    one = clean[:1]
    path = np.tile((rng.random((12, 3)) * 6.0)[None], (3, 1, 1))
    path[:, 2, 0] = nan      # legs 1 and 2
    path[:, 5, 1] = inf      # legs 4 and 5
    path[:, 8, 2] = 1e200    # legs 7 and 8: both endpoints finite, L2 overflows
    spoiled, sound = [1, 2, 4, 5, 7, 8], [0, 3, 6, 9, 10]
    usable = int(np.isfinite(N.kept(bad)).all(axis=1).sum())
    assert len(N.kept(bad)) < 3000 and usable < len(N.kept(bad))
    for k in (16, 64):
        got, _ = check([bad, clean[:0], one], path, k, f"poisoned, k {k}")
        assert (got["counts"][:, spoiled] == 0).all() and (got["indices"][:, spoiled] == -1).all()
        assert (got["sqdist"][:, spoiled] == DBL_MAX).all() and (got["t"][:, spoiled] == 0).all() and (got["pts"][:, spoiled] == 0).all()
        assert (got["counts"][1] == 0).all() and (got["indices"][1] == -1).all()         # the empty scene
        assert (got["counts"][0, sound] == min(k, usable)).all() and (got["counts"][2, sound] == 1).all() and np.isfinite(got["pts"]).all()
        # the other scenes of the batch: bit-identical to a batch without the poisoned scene
        ref = nearest([clean, clean[:0], one], path, k)
        for key in KEYS:
            assert np.array_equal(got[key][1:], ref[key][1:]), key
        assert not np.array_equal(got["indices"][0], ref["indices"][0])                  # (the shift is visible)


def test_point_strides_and_the_host_variant():
    rng = np.random.default_rng(13)
    cloud = (rng.random((2, 1500, 3)) * 5.0).astype(np.float32)
    base = None
    for stride in (3, 10, 14):
        path = rng.normal(size=(2, 6, stride)) * 50.0
        path[:, :, :3] = np.random.default_rng(17).random((2, 6, 3)) * 5.0
        got, _ = check(list(cloud), path, 8, f"stride {stride}")
        base = base or got
        N.assert_bitwise(got, base, KEYS, f"stride {stride} against 3")
        N.assert_bitwise(nearest(list(cloud), path, 8, host=True), got, KEYS, f"host, stride {stride}")
    assert (base["counts"] == 8).all()


def test_translated_by_4096_m():
    """cloud and path translated by 4096 m: float32 spacing (2^-11 m) at work, and the slack's absolute terms"""
    rng = np.random.default_rng(5)
    box = (rng.random((900, 3)) * [4.0, 3.0, 2.0]).astype(np.float32)
    path = np.array([[[-1.0, 1.0, 1.0], [1.0, 1.2, 0.9], [-0.3, 1.0, 1.0], [-0.3, 2.0, 1.2], [100.0, 100.0, 100.0], [101.0, 100.0, 100.5]]])
    for k in (1, 8):
        near, _ = check([box], path, k, f"box, k {k}")
        assert (near["counts"] == k).all()
        far = (box.astype(np.float64) + 4096.0).astype(np.float32)
        got, _ = check([far], path + [4096.0, 4096.0, 4096.0], k, f"translated, k {k}")
        assert (got["counts"] == k).all()


def test_errors_leave_the_outputs_untouched():
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import KdBatch
    lib = capi.load()
    S, P, k = 2, 4, 4
    L = P - 1
    kd = KdBatch(S, 64)
    try:
        kd.build(torch.rand((S, 64, 3), device="cuda"))
        path = torch.rand((S, P, 3), dtype=torch.float64, device="cuda")
        idx = torch.full((S, L, k), -7, dtype=torch.int32, device="cuda"); d2 = torch.full((S, L, k), -7.0, dtype=torch.float64, device="cuda")
        tt = torch.full((S, L, k), -7.0, dtype=torch.float64, device="cuda")
        pts = torch.full((S, L, k, 3), -7.0, dtype=torch.float32, device="cuda"); cnt = torch.full((S, L), -7, dtype=torch.int32, device="cuda")
        p = capi.dptr
        hq = np.zeros((S, P, 3)); hidx = np.full((S, L, k), -7, np.int32); hcnt = np.full((S, L), -7, np.int32)
        hp = lambda a: a.ctypes.data_as(C.c_void_p)

        def call(kdh=kd.h, pa=path, stride=3, npts=P, kk=k, outs=True):
            return lib.amk_kd_segment_nearest(kdh, p(pa), stride, npts, kk, p(idx) if outs else None, p(d2) if outs else None,
                                              p(tt) if outs else None, p(pts) if outs else None, p(cnt) if outs else None, None)

        def hcall(pa=hq, stride=3, npts=P, kk=k, outs=True):
            return lib.amk_kd_segment_nearest_host(kd.h, hp(pa) if pa is not None else None, stride, npts, kk, hp(hidx) if outs else None,
                                                   None, None, None, hp(hcnt) if outs else None)

        INV, UNS = capi.AMK_ERR_INVALID_ARG, capi.AMK_ERR_UNSUPPORTED
        assert call(npts=1) == INV and call(npts=0) == INV
        assert call(kk=0) == INV and call(kk=-1) == INV and call(kk=capi.AMK_MAX_K + 1) == UNS
        assert call(stride=2) == INV and call(pa=None) == INV and call(kdh=None) == INV and call(outs=False) == INV
        assert hcall(npts=1) == INV and hcall(kk=0) == INV and hcall(kk=capi.AMK_MAX_K + 1) == UNS
        assert hcall(stride=2) == INV and hcall(pa=None) == INV and hcall(outs=False) == INV
        capi.check(lib.amk__kd_set_mode(kd.h, 1), "scan mode")
        assert call() == UNS and hcall() == UNS
        capi.check(lib.amk__kd_set_mode(kd.h, 0), "index mode")
        torch.cuda.synchronize()
        for t in (idx, d2, tt, pts, cnt):
            assert (t == -7).all()
        assert (hidx == -7).all() and (hcnt == -7).all()
        # and the calls the rules allow: only d_sqdist wanted, only d_t wanted
        want = kd.segment_nearest(path, k)
        assert lib.amk_kd_segment_nearest(kd.h, p(path), 3, P, k, None, p(d2), None, None, None, None) == capi.AMK_OK
        torch.cuda.synchronize()
        assert torch.equal(d2, want["sqdist"]) and (tt == -7).all() and (idx == -7).all()
        assert lib.amk_kd_segment_nearest(kd.h, p(path), 3, P, k, None, None, p(tt), None, None, None) == capi.AMK_OK
        torch.cuda.synchronize()
        assert torch.equal(tt, want["t"]) and (idx == -7).all() and (cnt == -7).all() and (want["counts"] == k).all()
    finally:
        kd.close()
