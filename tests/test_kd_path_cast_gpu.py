"""GPU: amk_kd_path_cast (kd_path_cast_kernel / path_cast_scene, csrc/kd_path_cast.hip + csrc/kd_path_cast.h) against the numpy
restatement of tests/_path_cast.py AND against the reduction of KdBatch.segment_cast's own per-leg outputs (the identity the header
states).  Every comparison is bit for bit: stop, leg, t, free, indices, points.  Sizes are the smallest that reach the mechanism
named in each test: a round of the kernel holds 4 legs (8 in the experiments' build), so paths of 2, 5, 6, 9, 10 and 21 points are
a lone leg, fill a round exactly, go one leg beyond it, and reach a third and a sixth round."""
import ctypes as C

import numpy as np
import pytest

from tests import _path_cast as P

pytestmark = pytest.mark.gpu

INF = float("inf")
SEG_KEYS = ("hit", "t", "indices", "pts")


def pack(clouds, cap=None):
    S = len(clouds)
    cap = cap or max(1, max(len(c) for c in clouds))
    xyz = np.zeros((S, cap, 3), np.float32)
    counts = np.zeros(S, np.int32)
    for s, c in enumerate(clouds):
        xyz[s, :len(c)] = np.asarray(c, np.float32).reshape(-1, 3)
        counts[s] = len(c)
    return xyz, counts, cap


def device(clouds, fn):
    """fn(kd, torch) on a KdBatch built over one raw cloud per scene (ragged); its dicts as numpy"""
    import torch
    from avoid_mpc_amd.host import KdBatch
    xyz, counts, cap = pack(clouds)
    kd = KdBatch(len(clouds), cap)
    try:
        kd.build(torch.from_numpy(xyz).cuda(), torch.from_numpy(counts).cuda())
        outs = fn(kd, torch)
        torch.cuda.synchronize()
        return [{key: (v.cpu().numpy() if hasattr(v, "cpu") else v) for key, v in out.items() if v is not None} for out in outs]
    finally:
        kd.close()


def both(clouds, path, r2, host=False):
    """-> (path cast, segment cast) of the same handle on the same path"""
    def run(kd, torch):
        dp = torch.from_numpy(np.ascontiguousarray(path)).cuda()
        return [kd.path_cast_host(path, r2) if host else kd.path_cast(dp, r2), kd.segment_cast(dp, r2)]
    return device(clouds, run)


def check(clouds, path, r2, what="", **kw):
    got, legs = both(clouds, path, r2, **kw)
    want = P.expected_batch([[c] for c in clouds], path, r2)
    P.assert_bitwise(got, want, P.KEYS, what + ": specification")
    P.assert_bitwise(got, P.reduce_legs(legs, path), P.KEYS, what + ": reduction of the segment cast")
    return got, want


EXAMPLE = np.array([[2.0, 0.375, 0.0], [6.0, 0.0, 0.0], [9.0, 5.0, 5.0]], np.float32)
EXAMPLE_PATH = np.array([[[-3.0, 0.0, 0.0], [0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [20.0, 0.0, 0.0]]])


def test_by_hand():
    got, _ = check([EXAMPLE], EXAMPLE_PATH, 0.25, "example")
    t = (20.0 - np.sqrt(400.0 - 389.0625)) * (1.0 / 100.0)
    assert got["stop"].tolist() == [1] and got["leg"].tolist() == [1] and got["indices"].tolist() == [0]
    assert got["t"][0] == t and got["free"][0] == 3.0 + t * 10.0 and got["pts"][0].tolist() == [2.0, 0.375, 0.0]


def slab_cloud():
    cloud = (np.random.default_rng(41).random((3000, 3)) * [30.0, 16.0, 4.0]).astype(np.float32)
    g, nt = P.K.grid_dims(cloud)
    assert tuple(g) == (9, 5, 2) and nt == 1
    return cloud


def wander(seed=43, S=12, n=21):
    """S paths of n points, 0.33 m apart, each a slowly turning walk from a start inside the slab"""
    r = np.random.default_rng(seed)
    a = r.random((S, 3)) * [20.0, 12.0, 3.0] + [2.0, 2.0, 0.5]
    d = r.normal(size=(S, 3))
    d[:, 2] *= 0.2
    d /= np.linalg.norm(d, axis=1)[:, None]
    path = np.zeros((S, n, 3))
    for s in range(S):
        p, dd = a[s].copy(), d[s].copy()
        for i in range(n):
            path[s, i] = p
            dd = dd + 0.05 * r.normal(size=3)
            dd /= np.linalg.norm(dd)
            p = p + 0.33 * dd
    return path


@pytest.fixture(scope="module")
def fixture():
    return slab_cloud(), wander()


STOPS = {0.0625: [6, 6, -1, 7, 6, 11, 7, 6, 6, 0, 10, 4], 0.25: [0, 3, 5, 2, 0, 3, 0, 0, 1, 0, 0, 0], 0.0025: [-1] * 12}


@pytest.mark.parametrize("r2", [0.0625, 0.25, 0.0025])
def test_the_fixture(fixture, r2):
    """one free path, a stop at t = 0 on leg 0, stops inside the first round and in later rounds; every path free at the least radius"""
    cloud, path = fixture
    got, want = check([cloud] * 12, path, r2, f"fixture, r2 {r2}")
    assert want["leg"].tolist() == STOPS[r2]
    total = P.leg_lengths(path)
    if r2 == 0.0625:
        assert want["stop"].tolist().count(0) == 1 and want["t"][9] == 0.0 and want["leg"][9] == 0
    if r2 == 0.25:
        inner = (want["t"] > 0) & (want["t"] < 1)
        assert (inner & (want["leg"] < 4)).sum() >= 4       # stops at 0 < t < 1 inside the first round, of 4 legs or of 8
    if r2 == 0.0025:
        assert (want["stop"] == 0).all() and (want["t"] == 1.0).all() and (want["indices"] == -1).all()
        for s in range(12):
            acc = np.float64(0.0)
            for v in total[s]:
                acc = acc + v
            assert got["free"][s] == acc


@pytest.mark.parametrize("n_points", [2, 5, 6, 9, 10])
def test_ragged_scenes_and_round_edges(fixture, n_points):
    """scenes of 0, 1 and 3000 points; a lone leg is the segment cast; the last round partly filled, exactly filled, one leg beyond"""
    cloud, path = fixture
    clouds = [cloud[:0], cloud[7:8], cloud, cloud]
    sub = np.ascontiguousarray(path[[1, 3, 5, 11], :n_points])
    sub[1, 0] = cloud[7].astype(np.float64) + [0.05, 0.0, 0.0]     # the one-point scene: inside at the start of leg 0
    for r2 in (0.0625, 0.25):
        got, want = check(clouds, sub, r2, f"{n_points} points, r2 {r2}")
        assert got["stop"][0] == 0 and got["leg"][0] == -1 and got["indices"][0] == -1 and got["t"][0] == 1.0
        assert got["stop"][1] == 1 and got["leg"][1] == 0 and got["t"][1] == 0.0 and got["indices"][1] == 0
    if n_points == 2:
        got, legs = both(clouds, sub, 0.25)
        assert np.array_equal(got["stop"], legs["hit"][:, 0]) and np.array_equal(got["t"], legs["t"][:, 0])
        assert np.array_equal(got["indices"], legs["indices"][:, 0]) and np.array_equal(got["pts"], legs["pts"][:, 0])


def test_point_strides_and_the_host_variant(fixture):
    cloud, path = fixture
    rng = np.random.default_rng(13)
    base = None
    for stride in (3, 7, 14):
        wide = rng.normal(size=(12, 21, stride)) * 50.0
        wide[:, :, :3] = path
        got, _ = check([cloud] * 12, wide, 0.0625, f"stride {stride}")
        base = base or got
        P.assert_bitwise(got, base, P.KEYS, f"stride {stride} against 3")
        host, _ = both([cloud] * 12, wide, 0.0625, host=True)
        P.assert_bitwise(host, got, P.KEYS, f"host, stride {stride}")
    assert sorted(set(base["stop"].tolist())) == [0, 1]


def test_non_finite_path_points_and_cloud_points(fixture):
    """NaN in path point 3 spoils legs 2 and 3: stop 2 at leg 2 unless an earlier leg stops; free leaves the bad leg out"""
    cloud, path = fixture
    nan, inf = float("nan"), float("inf")
    bad = cloud.copy()
    bad[5::50, 0] = nan      # dropped by the build: the indices shift
    bad[7::60, 1] = nan      # kept in the index space, never touched
    bad[9::70, 2] = inf
    bad[11::500, 0] = -inf
    for value, col in ((nan, 0), (inf, 1), (-inf, 2), (1e200, 2)):
        p = path.copy()
        p[:, 3, col] = value
        got, want = check([bad] * 12, p, 0.0625, f"path point 3 = {value}")
        early = np.array(STOPS[0.0625])
        assert (want["stop"] == 2).any() and (want["stop"] == 1).any()
        two = want["stop"] == 2
        assert (want["leg"][two] == 2).all() and (want["t"][two] == 0.0).all() and (want["indices"][two] == -1).all() and (want["pts"][two] == 0).all()
        lens = P.leg_lengths(path)
        assert np.array_equal(want["free"][two], lens[two, 0] + lens[two, 1])
        assert (want["leg"][~two] < 2).all() and early[9] == 0 and not two[9]      # (an earlier leg stops: the NaN is never reached)
    # +inf radius: every usable point is inside at the start of leg 0 -- the lowest usable index, behind the dropped and unusable ones
    got, want = check([bad, cloud[:0]], path[:2], INF, "every usable point inside")
    usable = np.flatnonzero(np.isfinite(P.K.kept(bad)).all(axis=1))
    assert got["stop"].tolist() == [1, 0] and got["leg"].tolist() == [0, -1] and got["indices"][0] == usable[0] and got["free"][0] == 0.0


def test_a_point_whose_distance_overflows_is_not_touched():
    """q >= DBL_MAX needs a path far away: from 1e160 m every stored point is unusable and the path is free"""
    cloud = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], np.float32)
    path = np.array([[[1e160, 0.0, 0.0], [1e160, 1.0, 0.0], [1e160, 2.0, 0.0]], [[-1.0, 0.0, 0.0], [0.5, 0.0, 0.0], [3.0, 0.0, 0.0]]])
    got, want = check([cloud, cloud], path, INF, "overflow")
    assert got["stop"].tolist() == [0, 1] and got["free"][0] == 2.0 and got["t"][1] == 0.0


def test_translated_by_4096_m(fixture):
    """cloud and paths translated by 4096 m: float32 spacing (2^-11 m) at work, and the slack's absolute terms"""
    cloud, path = fixture
    far = (cloud.astype(np.float64) + 4096.0).astype(np.float32)
    for r2 in (0.0625, 0.25):
        got, want = check([far] * 12, path + 4096.0, r2, f"translated, r2 {r2}")
        assert (want["stop"] == 1).sum() >= 6


def test_stops_that_the_sampled_bounding_box_misses():
    """the clamped-outlier cloud of the segment cast's test, each 12 m ray as a path of 3 points"""
    cloud = (np.random.default_rng(3).random((20000, 3)) * [30.0, 16.0, 4.0]).astype(np.float32)
    unread = np.flatnonzero((np.arange(20000) // 64) % 16 != 0)[::40][:400]
    rng = np.random.default_rng(4)
    cloud[unread[:200], 0] = (-4.0 + 3.0 * rng.random(200)).astype(np.float32)
    cloud[unread[200:], 1] = (16.5 + 2.0 * rng.random(200)).astype(np.float32)
    out = np.zeros(20000, bool); out[unread] = True
    d = np.array([[1.0, 0.1, 0.02], [-1.0, 0.2, 0.05], [0.3, 1.0, 0.0], [0.2, -1.0, 0.1], [1.0, 1.0, 0.1]])
    d = 6.0 * d / np.linalg.norm(d, axis=1)[:, None]
    a = np.array([[-8.0, 8.0, 2.0], [6.0, 6.0, 2.0], [12.0, 9.0, 1.0], [15.0, 22.0, 2.0], [-7.0, 3.0, 2.0]])
    path = np.stack([a, a + d, a + 2.0 * d], axis=1)
    for r2 in (0.04, 9.0):
        got, want = check([cloud] * 5, path, r2, f"sampled box, r2 {r2}")
        assert (want["stop"] == 1).all()
        first = want["indices"]
        assert out[first].any() and not out[first].all()      # a clamped outlier is met first; elsewhere a point inside the box is


def test_errors_leave_the_outputs_untouched():
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import KdBatch
    lib = capi.load()
    S, NP = 2, 4
    kd = KdBatch(S, 64)
    try:
        kd.build(torch.rand((S, 64, 3), device="cuda"))
        path = torch.rand((S, NP, 3), dtype=torch.float64, device="cuda")
        i32 = lambda: torch.full((S,), -7, dtype=torch.int32, device="cuda")
        f64 = lambda: torch.full((S,), -7.0, dtype=torch.float64, device="cuda")
        stop, leg, idx, tt, free = i32(), i32(), i32(), f64(), f64()
        pts = torch.full((S, 3), -7.0, dtype=torch.float32, device="cuda")
        p = capi.dptr
        hq = np.zeros((S, NP, 3)); hstop = np.full(S, -7, np.int32); hfree = np.full(S, -7.0)
        hp = lambda a: a.ctypes.data_as(C.c_void_p)

        def call(kdh=kd.h, pa=path, stride=3, npts=NP, r2=0.25, outs=True):
            o = [p(stop), p(leg), p(tt), p(free), p(pts), p(idx)] if outs else [None] * 6
            return lib.amk_kd_path_cast(kdh, p(pa), stride, npts, r2, *o, None)

        def hcall(pa=hq, stride=3, npts=NP, r2=0.25, outs=True):
            return lib.amk_kd_path_cast_host(kd.h, hp(pa) if pa is not None else None, stride, npts, r2, hp(hstop) if outs else None, None,
                                             None, hp(hfree) if outs else None, None, None)

        INV, UNS = capi.AMK_ERR_INVALID_ARG, capi.AMK_ERR_UNSUPPORTED
        assert call(npts=1) == INV and call(npts=0) == INV and call(r2=-1.0) == INV and call(r2=float("nan")) == INV
        assert call(stride=2) == INV and call(pa=None) == INV and call(kdh=None) == INV and call(outs=False) == INV
        assert hcall(npts=1) == INV and hcall(r2=-1.0) == INV and hcall(r2=float("nan")) == INV
        assert hcall(stride=2) == INV and hcall(pa=None) == INV and hcall(outs=False) == INV
        capi.check(lib.amk__kd_set_mode(kd.h, 1), "scan mode")
        assert call() == UNS and hcall() == UNS
        capi.check(lib.amk__kd_set_mode(kd.h, 0), "index mode")
        torch.cuda.synchronize()
        for t in (stop, leg, idx, tt, free, pts):
            assert (t == -7).all()
        assert (hstop == -7).all() and (hfree == -7).all()
        # and the calls the rules allow: radius 0, only d_free wanted
        assert call(r2=0.0) == capi.AMK_OK
        want = kd.path_cast(path, 0.25)
        for t in (stop, leg, idx):
            t.fill_(-7)
        tt.fill_(-7.0); pts.fill_(-7.0)
        assert lib.amk_kd_path_cast(kd.h, p(path), 3, NP, 0.25, None, None, None, p(free), None, None, None) == capi.AMK_OK
        torch.cuda.synchronize()
        assert torch.equal(free, want["free"]) and (stop == -7).all() and (tt == -7).all() and (pts == -7).all()
    finally:
        kd.close()
