"""GPU: the radius search and the four leg walks (grid_radius, grid_segment, grid_segment_knn, grid_cast and the path cast over it;
csrc/kd_grid.h) on every index layout a build can leave -- the table of tests/_index_layouts.py, which tests/test_index_layouts.py
proves on the CPU to reach what it names.  Each case builds the handle as its layout says and runs the five single-handle queries,
device and _host forms, against the existing brute forces (tests/_radius.py, _segment.py, _segment_nearest.py, _cast.py,
_path_cast.py).  Every comparison is bit for bit; there is no tolerance anywhere."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from tests import _index_layouts as IL
from tests import _path_cast as PC
from tests._radius import assert_bitwise

pytestmark = pytest.mark.gpu

RADIUS_KEYS = ("counts", "indices", "sqdist", "pts")
SEGMENT_KEYS = ("counts", "indices", "sqdist", "t", "pts")
CAST_KEYS = ("hit", "t", "indices", "pts")
LEG = IL.LEG


def to_np(out):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items() if v is not None}


def pack(clouds, cap, stride=3):
    """[S, cap, stride] float32 (columns past the third hold something to ignore) and the counts"""
    xyz = np.full((len(clouds), cap, stride), 7.5, np.float32)
    counts = np.zeros(len(clouds), np.int32)
    for s, c in enumerate(clouds):
        xyz[s, :len(c), :3] = np.asarray(c, np.float32).reshape(-1, 3)
        counts[s] = len(c)
    return xyz, counts


def build(kd, clouds, stride=3):
    import torch
    xyz, counts = pack(clouds, kd.max_points, stride)
    kd.build(torch.from_numpy(xyz).cuda(), torch.from_numpy(counts).cuda())


def read_back(kd):
    """amk_kd_points_host: the handle's clouds, one float32 [n, 3] per scene"""
    from avoid_mpc_amd import capi
    pts = np.zeros((kd.S, kd.max_points, 3), np.float32); sizes = np.zeros(kd.S, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    capi.check(kd.lib.amk_kd_points_host(kd.h, vp(pts), vp(sizes)), "amk_kd_points_host")
    return [pts[s, :sizes[s]] for s in range(kd.S)]


def swept_handle(stack):
    """the keyframe handle after the sweep of tests/_index_layouts.swept(), checked against the numpy sweep point for point"""
    import torch
    from avoid_mpc_amd.host import KdBatch
    sw = IL.swept()
    kf, cur = KdBatch(3, IL.SWEEP_CAP), KdBatch(3, IL.SWEEP_CAP)
    stack.callback(kf.close); stack.callback(cur.close)
    build(kf, sw["keyframe"]); build(cur, sw["current"])
    outl, reb = kf.keyframe_sweep(cur, IL.SWEEP_TH, IL.SWEEP_COUNT)
    torch.cuda.synchronize()
    assert outl.cpu().tolist() == sw["outliers"] and reb.cpu().tolist() == sw["rebuilt"]
    assert kf.sizes().tolist() == [len(a) for a in sw["after"]]
    for s, (got, want) in enumerate(zip(read_back(kf), sw["after"])):
        assert got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32)), s
    return kf


def rebuilt_handle(stack, first, second, path):
    """a handle that answered for `first` and was then built again with `second`"""
    import torch
    from avoid_mpc_amd.host import KdBatch
    kd = KdBatch(len(first), IL.REBUILT_CAP)
    stack.callback(kd.close)
    build(kd, first)
    before = to_np(kd.segment_cast(torch.from_numpy(path).cuda(), IL.INF))
    assert before["hit"].all()                                                  # the first index is in use: every scene holds points
    build(kd, second)
    return kd


@contextlib.contextmanager
def handle_of(lay):
    import torch
    from avoid_mpc_amd.host import KdBatch
    with contextlib.ExitStack() as stack:
        if lay.how == "sweep":
            kd = swept_handle(stack)
        elif lay.how == "rebuild":
            kd = rebuilt_handle(stack, IL.rebuilt()[0], lay.clouds, lay.path)
        else:
            kd = KdBatch(len(lay.clouds), lay.cap)
            stack.callback(kd.close)
            if lay.ties:
                kd.set_tie_order(lay.ties)
            build(kd, lay.clouds, lay.stride)
            if lay.ties == 2:                                                   # AMK_TIES_AUTO: tied queries first, so that the lazy trees exist
                kd.search(torch.from_numpy(np.ascontiguousarray(lay.path)).cuda(), 8)
                torch.cuda.synchronize()
                assert 0 in kd.exact_status().cpu().tolist()
        assert kd.sizes().tolist() == [int((~np.isnan(np.asarray(c)[:, 0])).sum()) for c in lay.clouds]
        yield kd


@pytest.mark.parametrize("name", IL.NAMES)
def test_the_five_queries_on_every_layout(name):
    import torch
    lay = IL.layouts()[name]
    path = lay.path
    with handle_of(lay) as kd:
        dpath = torch.from_numpy(np.ascontiguousarray(path)).cuda()
        casts, counts = {}, {}
        for r2 in IL.RADII:
            for k in IL.RADIUS_K:
                keys = RADIUS_KEYS if k else ("counts",)
                want = IL.want_radius(lay.ref, r2, k)
                assert_bitwise(to_np(kd.radius_search(dpath, r2, k)), want, keys, f"{name}: radius, r2 {r2}, k {k}")
                assert_bitwise(kd.radius_search_host(path, r2, k), want, keys, f"{name}: radius host, r2 {r2}, k {k}")
                keys = SEGMENT_KEYS if k else ("counts",)
                want = IL.want_segment(lay.ref, r2, k)
                got = to_np(kd.segment_search(dpath, r2, k))
                assert_bitwise(got, want, keys, f"{name}: segment, r2 {r2}, k {k}")
                assert_bitwise(kd.segment_search_host(path, r2, k), want, keys, f"{name}: segment host, r2 {r2}, k {k}")
                counts[r2] = got["counts"]
            want = IL.want_cast(lay.ref, r2)
            casts[r2] = to_np(kd.segment_cast(dpath, r2))
            assert_bitwise(casts[r2], want, CAST_KEYS, f"{name}: cast, r2 {r2}")
            assert_bitwise(kd.segment_cast_host(path, r2), want, CAST_KEYS, f"{name}: cast host, r2 {r2}")
            for window in IL.WINDOWS:
                i, n = window
                sub = np.ascontiguousarray(path[:, i:i + n])
                dsub = torch.from_numpy(sub).cuda()
                want = IL.want_path_cast(lay.ref, r2, window)
                got = to_np(kd.path_cast(dsub, r2))
                assert_bitwise(got, want, PC.KEYS, f"{name}: path cast, r2 {r2}, points {i}..{i + n - 1}")
                assert_bitwise(kd.path_cast_host(sub, r2), want, PC.KEYS, f"{name}: path cast host, r2 {r2}, points {i}..{i + n - 1}")
                assert_bitwise(got, PC.reduce_legs(to_np(kd.segment_cast(dsub, r2)), sub), PC.KEYS, f"{name}: path cast as a reduction, r2 {r2}")
        for k in IL.NEAREST_K:
            want = IL.want_nearest(lay.ref, k)
            assert_bitwise(to_np(kd.segment_nearest(dpath, k)), want, SEGMENT_KEYS, f"{name}: nearest, k {k}")
            assert_bitwise(kd.segment_nearest_host(path, k), want, SEGMENT_KEYS, f"{name}: nearest host, k {k}")
        # in exact arithmetic hit == (count > 0); in fp64 wherever the nearest point is not within 1e-9 r2 of the radius
        for r2 in (0.0625, 4.0):
            clear = IL.clear_legs(lay, r2)
            assert clear.mean() >= 0.95
            assert np.array_equal(casts[r2]["hit"][clear] > 0, counts[r2][clear] > 0), (name, r2)


@pytest.mark.parametrize("name", ["line", "same"])
def test_a_degenerate_leg_is_the_radius_search_and_the_knn_at_its_point(name):
    import torch
    lay = IL.layouts()[name]
    j = LEG["on_point"]
    leg = np.ascontiguousarray(lay.path[:, j:j + 2])
    assert (leg[:, 0] == leg[:, 1]).all()
    with handle_of(lay) as kd:
        dleg, dq = torch.from_numpy(leg).cuda(), torch.from_numpy(np.ascontiguousarray(leg[:, :1])).cuda()
        for r2 in IL.RADII:
            for k in (8, 64):
                seg, rad = to_np(kd.segment_search(dleg, r2, k)), to_np(kd.radius_search(dq, r2, k))
                assert_bitwise(seg, rad, RADIUS_KEYS, f"{name}: r2 {r2}, k {k}")
                assert (seg["t"] == 0).all()
            cast = to_np(kd.segment_cast(dleg, r2))
            assert np.array_equal(cast["hit"] > 0, rad["counts"] > 0) and (cast["t"][cast["hit"] > 0] == 0).all()
            if name == "same":
                assert (cast["indices"][cast["hit"] > 0] == 0).all()                # coincident points: the lowest index
        assert rad["counts"].min() > 0
        for k in (8, 64):
            near, knn = to_np(kd.segment_nearest(dleg, k)), to_np(kd.search(dq, k))
            assert_bitwise(near, knn, ("indices", "sqdist", "pts"), f"{name}: k {k}")
            assert (near["t"] == 0).all() and (near["counts"] == k).all()


def test_the_frame_lists_on_mixed_layouts():
    """one list of three handles -- a plane cloud built once, the swept keyframe (every record in tile 0), a handle built twice --
    through the five list forms: grid_cast's tcap hand-over and the list folds of csrc/map_query.hip on tables of both builders"""
    import torch
    from avoid_mpc_amd.host import (KdBatch, path_cast_frames, radius_search_frames, segment_cast_frames, segment_nearest_frames,
                                    segment_search_frames)
    fl = IL.frame_list()
    path = fl["path"]
    with contextlib.ExitStack() as stack:
        plane = KdBatch(IL.FRAME_SCENES, 6000)
        stack.callback(plane.close)
        build(plane, fl["plane"])
        hs = [plane, swept_handle(stack), rebuilt_handle(stack, fl["first"], fl["second"], path)]
        dpath = torch.from_numpy(np.ascontiguousarray(path)).cuda()
        for r2 in IL.FRAME_RADII:
            for k in IL.FRAME_K:
                lists = ("pts", "sqdist", "frame") if k else ()
                assert_bitwise(to_np(radius_search_frames(hs, dpath, r2, k)), IL.want_frames("radius", r2, k), ("counts",) + lists,
                               f"frames: radius, r2 {r2}, k {k}")
                assert_bitwise(to_np(segment_search_frames(hs, dpath, r2, k)), IL.want_frames("segment", r2, k),
                               ("counts",) + lists + (("t",) if k else ()), f"frames: segment, r2 {r2}, k {k}")
            assert_bitwise(to_np(segment_cast_frames(hs, dpath, r2)), IL.want_frames("cast", r2), ("hit", "t", "pts", "frame"),
                           f"frames: cast, r2 {r2}")
            for window in IL.WINDOWS:
                i, n = window
                sub = np.ascontiguousarray(path[:, i:i + n])
                dsub = torch.from_numpy(sub).cuda()
                got = to_np(path_cast_frames(hs, dsub, r2))
                assert_bitwise(got, IL.want_frames("path_cast", r2, window), PC.KEYS_FRAMES, f"frames: path cast, r2 {r2}, from {i}")
                assert_bitwise(got, PC.reduce_legs(to_np(segment_cast_frames(hs, dsub, r2)), sub), PC.KEYS_FRAMES,
                               f"frames: path cast as a reduction, r2 {r2}")
        for k in IL.NEAREST_K:
            assert_bitwise(to_np(segment_nearest_frames(hs, dpath, k)), IL.want_frames("nearest", k),
                           ("counts", "pts", "sqdist", "t", "frame"), f"frames: nearest, k {k}")
