"""GPU: amk_kd_segment_cast (kd_segment_cast_kernel / grid_cast, csrc/kd_segment_cast.hip + csrc/kd_grid.h) against the numpy brute
force of tests/_cast.py, sentence by sentence of the header's contract.  Every comparison is bit for bit: hit, t, indices, points.
Sizes are the smallest that reach the mechanism named in each test."""
import ctypes as C

import numpy as np
import pytest

from tests import _cast as K
from tests._segment import seg_dists

pytestmark = pytest.mark.gpu

KEYS = ("hit", "t", "indices", "pts")
INF = float("inf")


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
    """fn(kd, torch) on a KdBatch built over one raw cloud per scene (ragged); its dict as numpy"""
    import torch
    from avoid_mpc_amd.host import KdBatch
    xyz, counts, cap = pack(clouds)
    kd = KdBatch(len(clouds), cap)
    try:
        kd.build(torch.from_numpy(xyz).cuda(), torch.from_numpy(counts).cuda())
        out = fn(kd, torch)
        torch.cuda.synchronize()
        return {key: (v.cpu().numpy() if hasattr(v, "cpu") else v) for key, v in out.items() if v is not None}
    finally:
        kd.close()


def cast(clouds, path, r2, host=False):
    if host:
        return device(clouds, lambda kd, torch: kd.segment_cast_host(path, r2))
    return device(clouds, lambda kd, torch: kd.segment_cast(torch.from_numpy(np.ascontiguousarray(path)).cuda(), r2))


def check(clouds, path, r2, what="", **kw):
    got = cast(clouds, path, r2, **kw)
    want = K.expected_batch([[c] for c in clouds], path, r2)
    K.assert_bitwise(got, want, KEYS, what)
    return got, want


EXAMPLE = np.array([[2.0, 0.375, 0.0], [6.0, 0.0, 0.0], [9.0, 5.0, 5.0]], np.float32)
ALONG_X = np.array([[[0.0, 0.0, 0.0], [10.0, 0.0, 0.0]]])


def test_first_is_not_closest():
    """the point closest to the line stands behind the one the vehicle reaches first"""
    got, want = check([EXAMPLE], ALONG_X, 0.25, "example")
    assert want["hit"].tolist() == [[1]] and want["indices"].tolist() == [[0]]
    # by hand: q = 4 + 0.140625, dot = 20, L2 = 100, c = 3.890625, disc = 400 - 389.0625
    assert want["t"][0, 0] == (20.0 - np.sqrt(400.0 - 100.0 * 3.890625)) * (1.0 / 100.0)
    assert abs(want["t"][0, 0] - 0.16692810861169263) < 1e-15 and got["pts"][0, 0].tolist() == [2.0, 0.375, 0.0]
    near = device([EXAMPLE], lambda kd, torch: kd.segment_nearest(torch.from_numpy(ALONG_X).cuda(), 1))
    assert near["indices"][0, 0].tolist() == [1] and near["t"][0, 0, 0] == 60.0 * (1.0 / 100.0)     # segment nearest answers the other point


def test_every_test_is_strict():
    pair = np.array([[3.0, 0.5, 0.0], [7.0, 0.5, 0.0]], np.float32)
    got, _ = check([pair], ALONG_X, 0.25, "grazing")
    assert got["hit"].tolist() == [[0]] and got["t"].tolist() == [[1.0]] and got["indices"].tolist() == [[-1]] and (got["pts"] == 0).all()
    got, _ = check([pair], ALONG_X, 0.265625, "just wider")
    assert got["hit"].tolist() == [[1]] and got["indices"].tolist() == [[0]] and 0 < got["t"][0, 0] < 0.3
    got, _ = check([np.array([[10.5, 0.0, 0.0]], np.float32)], ALONG_X, 0.25, "contact at b")
    assert got["hit"].tolist() == [[0]] and got["t"].tolist() == [[1.0]]
    on = np.array([[0.5, 0.0, 0.0]], np.float32)     # the start lies on the sphere's surface
    got, _ = check([on], ALONG_X, 0.25, "heading in")
    assert got["hit"].tolist() == [[1]] and got["t"].tolist() == [[0.0]]
    got, _ = check([on], -ALONG_X, 0.25, "heading out")
    assert got["hit"].tolist() == [[0]] and got["t"].tolist() == [[1.0]]


def grid_of(cloud):
    """the index's grid over a cloud whose bounding box the build sees whole: (cells per axis, bbmin, h)"""
    c = K.kept(cloud).astype(np.float64)
    g, _ = K.grid_dims(cloud)
    lo, ext = c.min(axis=0), c.max(axis=0) - c.min(axis=0)
    e = np.maximum(ext, max(ext.max() * 1e-6, 1e-30))
    h = np.cbrt(e.prod() / min(max(len(c) / 64.0, 1.0), 1024.0))
    while (np.clip(np.ceil(e / h), 1, 1024).astype(int) != g).any():
        h *= 1.26
    return g, lo, h


@pytest.fixture(scope="module")
def slab():
    """3000 points in 30 x 16 x 4 m, a grid of 9 x 5 x 2 cells in one tile; scenes of 0, 1 and 3000 points; a path whose even legs
    are 0.33, 3 and 12 m long in random directions (some start or end outside the cloud's box, leg 0 lies wholly outside), its
    odd legs whatever joins them"""
    rng = np.random.default_rng(41)
    cloud = (rng.random((3000, 3)) * [30.0, 16.0, 4.0]).astype(np.float32)
    g, nt = K.grid_dims(cloud)
    assert tuple(g) == (9, 5, 2) and nt == 1
    M = 36
    a = rng.random((M, 3)) * [34.0, 20.0, 8.0] - [2.0, 2.0, 2.0]
    d = rng.normal(size=(M, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    length = np.tile([0.33, 3.0, 12.0], M // 3)
    a[0], d[0] = [-9.0, -6.0, 9.0], [0.0, 0.0, 1.0]
    b = a + length[:, None] * d
    path = np.stack([a, b], axis=1).reshape(1, 2 * M, 3)
    lo, hi = cloud.min(axis=0), cloud.max(axis=0)
    inside = lambda p: ((p >= lo) & (p <= hi)).all(axis=-1)
    assert (inside(a) & ~inside(b)).any() and (~inside(a) & inside(b)).any() and not inside(a[0]) and not inside(b[0])
    _, bb, h = grid_of(cloud)
    cell = lambda p: np.clip(np.floor((p - bb) / h), 0, g - 1).astype(int)
    long_legs = np.flatnonzero(length == 12.0)
    assert (np.abs(cell(a[long_legs]) - cell(b[long_legs])).max(axis=1) >= 2).any()      # a 12 m leg spans more than one slab
    clouds = [cloud[:0], cloud[7:8], cloud]
    return clouds, np.tile(path, (3, 1, 1))


@pytest.mark.parametrize("r2", [0.0, 0.0025, 0.25, 1.0, 16.0, INF])
def test_random_slab(slab, r2):
    """legs shorter than a cell, longer than three, radii from nothing to wider than two cells and to everything"""
    clouds, path = slab
    got, want = check(clouds, path, r2, f"slab, r2 {r2}")
    assert (got["hit"][0] == 0).all() and (got["t"][0] == 1.0).all() and (got["indices"][0] == -1).all()
    hit = want["hit"][2]
    if 0 < r2 < INF:
        assert 0 < hit.sum() < hit.size and ((want["t"][2] > 0) & (want["t"][2] < 1)).any()
    if r2 == INF:
        assert hit.all() and (want["t"][2] == 0).all() and (want["indices"][2] == 0).all() and want["hit"][1].all()


@pytest.mark.parametrize("r2", [0.0025, 0.25, 1.0])
def test_a_cast_hits_where_the_segment_search_counts(slab, r2):
    """in exact arithmetic hit == (count > 0); in fp64 wherever the nearest point is not within 1e-9 r2 of the radius"""
    clouds, path = slab
    got = cast(clouds, path, r2)
    cnt = device(clouds, lambda kd, torch: kd.segment_search(torch.from_numpy(path).cuda(), r2, 0))["counts"]
    dmin = np.array([seg_dists(clouds[2], path[2, j], path[2, j + 1])[0].min() for j in range(path.shape[1] - 1)])
    clear = np.abs(dmin - r2) > 1e-9 * r2
    assert clear.mean() >= 0.95
    assert np.array_equal(got["hit"][2][clear] > 0, cnt[2][clear] > 0) and (cnt[2] > 0).any() and (cnt[2] == 0).any()
    assert np.array_equal(got["hit"][:2] > 0, cnt[:2] > 0)


def test_the_early_stop_loses_no_point():
    """12 m rays through a cloud whose outliers the bounding-box sample missed: they sit clamped in boundary cells, no boundary
    face may bound or stop the walk, and a stop that trusts the cells' geometry loses them"""
    cloud = (np.random.default_rng(3).random((20000, 3)) * [30.0, 16.0, 4.0]).astype(np.float32)
    unread = np.flatnonzero((np.arange(20000) // 64) % 16 != 0)[::40][:400]
    rng = np.random.default_rng(4)
    cloud[unread[:200], 0] = (-4.0 + 3.0 * rng.random(200)).astype(np.float32)
    cloud[unread[200:], 1] = (16.5 + 2.0 * rng.random(200)).astype(np.float32)
    out = np.zeros(20000, bool); out[unread] = True
    sampled = cloud[(np.arange(20000) // 64) % 16 == 0]
    assert sampled[:, 0].min() >= 0 and sampled[:, 1].max() <= 16 and cloud[:, 0].min() < -3.9 and cloud[:, 1].max() > 18.4
    d = np.array([[1.0, 0.1, 0.02], [-1.0, 0.2, 0.05], [0.3, 1.0, 0.0], [0.2, -1.0, 0.1], [1.0, 1.0, 0.1]])
    d = 12.0 * d / np.linalg.norm(d, axis=1)[:, None]
    a = np.array([[-8.0, 8.0, 2.0], [6.0, 6.0, 2.0], [12.0, 9.0, 1.0], [15.0, 22.0, 2.0], [-7.0, 3.0, 2.0]])
    path = np.stack([a, a + d], axis=1).reshape(1, 10, 3)
    for r2 in (0.04, 9.0):
        got, want = check([cloud], path, r2, f"sampled box, r2 {r2}")
        first = want["indices"][0, 0::2]
        assert (want["hit"][0, 0::2] == 1).all() and (want["t"][0, 0::2] > 0).any()
        assert out[first].any() and not out[first].all()      # a clamped outlier is met first; elsewhere a point inside the box is


@pytest.fixture(scope="module")
def lattice():
    """the 10 x 10 x 10 integer lattice, 4 133 points: every site is held four or five times"""
    site = np.arange(4133) % 1000
    return np.stack([site % 10, site // 10 % 10, site // 100], axis=1).astype(np.float32)


@pytest.mark.parametrize("r2", [0.25, 0.5])
def test_equal_t_on_the_lattice(lattice, r2):
    legs = np.array([[[-1.0, 3.0, 3.0], [11.0, 3.0, 3.0]],       # along a row of sites
                     [[-1.0, 3.5, 3.0], [11.0, 3.5, 3.0]],       # between two rows, 0.5 from each
                     [[2.0, 2.0, 11.0], [2.0, 2.0, -1.0]],       # down a column
                     [[-1.0, -1.0, -1.0], [11.0, 11.0, 11.0]],   # the diagonal
                     [[9.5, 9.0, 0.5], [-1.0, 0.0, 3.5]]])       # skew
    path = legs.reshape(1, 10, 3)
    got, want = check([lattice], path, r2, f"lattice, r2 {r2}")
    for j in (0, 2, 4, 6, 8):
        hit, t = K.contacts(lattice, path[0, j], path[0, j + 1], r2)
        if not hit.any():
            continue
        first = np.flatnonzero(hit & (t == t[hit].min()))
        assert len(first) >= 4 and got["indices"][0, j] == first.min()       # every site four or five times: the lowest index
    assert got["hit"][0, 0] == 1 and got["indices"][0, 0] == 330 and got["hit"][0, 4] == 1 and got["indices"][0, 4] == 922
    # at exactly distance r from both rows: a miss at r2 = 0.25; at 0.5 the rows y = 3 and y = 4 are met at the same t
    hit, t = K.contacts(lattice, path[0, 2], path[0, 3], r2)
    if r2 == 0.25:
        assert got["hit"][0, 2] == 0 and not hit.any()
    else:
        first = np.flatnonzero(hit & (t == t[hit].min()))
        assert {tuple(p) for p in lattice[first].tolist()} == {(0.0, 3.0, 3.0), (0.0, 4.0, 3.0)} and got["indices"][0, 2] == 330


def test_a_degenerate_leg_is_the_radius_search_at_its_point(slab, lattice):
    rng = np.random.default_rng(29)
    for cl, p in ((slab[0][2], rng.random((6, 3)) * [30.0, 16.0, 4.0]), (lattice, np.round(rng.random((6, 3)) * 9.0))):
        path = np.repeat(p, 2, axis=0)[None]                                # legs 0, 2, ... have a == b
        for r2 in (0.25, 1.0, 4.0):
            got, _ = check([cl], path, r2, "degenerate")
            cnt = device([cl], lambda kd, torch: kd.radius_search(torch.from_numpy(p[None]).cuda(), r2, 0))["counts"]
            assert np.array_equal(got["hit"][0, 0::2] > 0, cnt[0] > 0) and (got["t"][0, 0::2][cnt[0] > 0] == 0).all()
            c = cl.astype(np.float64)
            for i in range(6):
                q = ((c[:, 0] - p[i, 0]) ** 2 + (c[:, 1] - p[i, 1]) ** 2) + (c[:, 2] - p[i, 2]) ** 2
                inside = np.flatnonzero(q < r2)
                assert got["indices"][0, 2 * i] == (inside.min() if len(inside) else -1)   # the lowest index, not the nearest point
        assert (got["hit"][0, 0::2] == 1).any()


def test_non_finite_path_points_and_cloud_points():
    rng = np.random.default_rng(11)
    nan, inf = float("nan"), float("inf")
    clean = (rng.random((3000, 3)) * 6.0).astype(np.float32)
    bad = clean.copy()
    bad[5::50, 0] = nan      # dropped by the build: the indices shift
    bad[7::60, 1] = nan      # kept in the index space, never touched
    bad[9::70, 2] = inf
    bad[11::500, 0] = -inf
    one = clean[:1]
    path = np.tile((rng.random((12, 3)) * 6.0)[None], (3, 1, 1))
    path[:, 2, 0] = nan      # legs 1 and 2
    path[:, 5, 1] = inf      # legs 4 and 5
    path[:, 8, 2] = 1e200    # legs 7 and 8: both endpoints finite, L2 overflows
    spoiled, sound = [1, 2, 4, 5, 7, 8], [0, 3, 6, 9, 10]
    for r2 in (0.04, INF):
        got, want = check([bad, clean[:0], one], path, r2, f"poisoned, r2 {r2}")
        assert (got["hit"][:, spoiled] == 0).all() and (got["t"][:, spoiled] == 1.0).all() and (got["indices"][:, spoiled] == -1).all()
        assert (got["hit"][1] == 0).all() and (got["indices"][1] == -1).all() and (got["pts"][1] == 0).all()      # the empty scene
        assert (got["hit"][0, sound] == 1).all() and np.isfinite(got["pts"]).all()
        ref = cast([clean, clean[:0], one], path, r2)
        for key in KEYS:
            assert np.array_equal(got[key][1:], ref[key][1:]), key
        if r2 == INF:    # every usable point is inside at the start: the lowest usable index, behind the dropped and the unusable ones
            usable = np.flatnonzero(np.isfinite(K.kept(bad)).all(axis=1))
            assert (got["indices"][0, sound] == usable[0]).all() and (got["t"][0, sound] == 0).all() and (got["hit"][2, sound] == 1).all()
        else:
            assert not np.array_equal(got["indices"][0], ref["indices"][0])                  # (the shift is visible)


def test_point_strides_a_lone_leg_and_the_host_variant():
    rng = np.random.default_rng(13)
    cloud = (rng.random((2, 1500, 3)) * 5.0).astype(np.float32)
    base = None
    for stride in (3, 10, 14):
        path = rng.normal(size=(2, 6, stride)) * 50.0
        path[:, :, :3] = np.random.default_rng(17).random((2, 6, 3)) * 7.0 - 1.0
        got, _ = check(list(cloud), path, 0.01, f"stride {stride}")
        base = base or got
        K.assert_bitwise(got, base, KEYS, f"stride {stride} against 3")
        K.assert_bitwise(cast(list(cloud), path, 0.01, host=True), got, KEYS, f"host, stride {stride}")
        lone, _ = check(list(cloud), path[:, 2:4], 0.01, "lone leg")
        for key in KEYS:
            assert np.array_equal(lone[key][:, 0], got[key][:, 2]), key
    assert 0 < base["hit"].sum() < base["hit"].size


def test_translated_by_4096_m():
    """cloud and path translated by 4096 m: float32 spacing (2^-11 m) at work, and the slack's absolute terms"""
    rng = np.random.default_rng(5)
    box = (rng.random((900, 3)) * [4.0, 3.0, 2.0]).astype(np.float32)
    path = np.array([[[-1.0, 1.0, 1.0], [1.0, 1.2, 0.9], [-0.3, 1.0, 1.0], [-0.3, 2.0, 1.2], [100.0, 100.0, 100.0], [101.0, 100.0, 100.5],
                      [5.0, 1.5, 1.0], [-8.0, 1.4, 1.1]]])
    for r2 in (0.01, 0.09):
        near, _ = check([box], path, r2, f"box, r2 {r2}")
        assert near["hit"][0, 4] == 0 and near["hit"][0, 6] == 1
        far = (box.astype(np.float64) + 4096.0).astype(np.float32)
        got, _ = check([far], path + [4096.0, 4096.0, 4096.0], r2, f"translated, r2 {r2}")
        assert got["hit"][0, 4] == 0 and got["hit"][0, 6] == 1


def test_errors_leave_the_outputs_untouched():
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import KdBatch
    lib = capi.load()
    S, P = 2, 4
    L = P - 1
    kd = KdBatch(S, 64)
    try:
        kd.build(torch.rand((S, 64, 3), device="cuda"))
        path = torch.rand((S, P, 3), dtype=torch.float64, device="cuda")
        hit = torch.full((S, L), -7, dtype=torch.int32, device="cuda"); tt = torch.full((S, L), -7.0, dtype=torch.float64, device="cuda")
        pts = torch.full((S, L, 3), -7.0, dtype=torch.float32, device="cuda"); idx = torch.full((S, L), -7, dtype=torch.int32, device="cuda")
        p = capi.dptr
        hq = np.zeros((S, P, 3)); hhit = np.full((S, L), -7, np.int32); ht = np.full((S, L), -7.0)
        hp = lambda a: a.ctypes.data_as(C.c_void_p)

        def call(kdh=kd.h, pa=path, stride=3, npts=P, r2=0.25, outs=True):
            return lib.amk_kd_segment_cast(kdh, p(pa), stride, npts, r2, p(hit) if outs else None, p(tt) if outs else None,
                                           p(pts) if outs else None, p(idx) if outs else None, None)

        def hcall(pa=hq, stride=3, npts=P, r2=0.25, outs=True):
            return lib.amk_kd_segment_cast_host(kd.h, hp(pa) if pa is not None else None, stride, npts, r2, hp(hhit) if outs else None,
                                                hp(ht) if outs else None, None, None)

        INV, UNS = capi.AMK_ERR_INVALID_ARG, capi.AMK_ERR_UNSUPPORTED
        assert call(npts=1) == INV and call(npts=0) == INV and call(r2=-1.0) == INV and call(r2=float("nan")) == INV
        assert call(stride=2) == INV and call(pa=None) == INV and call(kdh=None) == INV and call(outs=False) == INV
        assert hcall(npts=1) == INV and hcall(r2=-1.0) == INV and hcall(r2=float("nan")) == INV
        assert hcall(stride=2) == INV and hcall(pa=None) == INV and hcall(outs=False) == INV
        capi.check(lib.amk__kd_set_mode(kd.h, 1), "scan mode")
        assert call() == UNS and hcall() == UNS
        capi.check(lib.amk__kd_set_mode(kd.h, 0), "index mode")
        torch.cuda.synchronize()
        for t in (hit, tt, pts, idx):
            assert (t == -7).all()
        assert (hhit == -7).all() and (ht == -7).all()
        # and the calls the rules allow: radius 0, only d_t wanted, only d_hit wanted
        assert call(r2=0.0) == capi.AMK_OK
        want = kd.segment_cast(path, 0.25)
        hit.fill_(-7); idx.fill_(-7); pts.fill_(-7.0)
        assert lib.amk_kd_segment_cast(kd.h, p(path), 3, P, 0.25, None, p(tt), None, None, None) == capi.AMK_OK
        torch.cuda.synchronize()
        assert torch.equal(tt, want["t"]) and (hit == -7).all() and (idx == -7).all() and (pts == -7).all()
        tt.fill_(-7.0)
        assert lib.amk_kd_segment_cast(kd.h, p(path), 3, P, 0.25, p(hit), None, None, None, None) == capi.AMK_OK
        torch.cuda.synchronize()
        assert torch.equal(hit, want["hit"]) and (tt == -7).all() and (idx == -7).all()
    finally:
        kd.close()
