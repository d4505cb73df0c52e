"""Thin Python objects over the C ABI (include/avoid_mpc_amd.h) used by tests and bench.py.

torch is plumbing here (device buffers, streams); every computation happens in the HIP library.
The reference-shaped C++ adapters (KDTreeTwo<double>, FrameKDMap, ObstacleAvoidanceMPC) live in
include/avoid_mpc_amd/*.hpp; these classes are their batched Python twins:

  KdBatch   <- S x KDTreeTwo<double>          AM/include/kd_tree_two.h:53-144
  MpcBatch  <- S x ObstacleAvoidanceMPC       AM/include/HighLvlMpc.h:4-33
  step_batch<- TASK branch of Step            AM/src/AvoidanceStateMachine.cpp:322-355
"""
import ctypes as C

import numpy as np
import torch

from . import capi


def _dev():
    if not torch.cuda.is_available():
        raise capi.AmkError("no GPU visible: the hot path has no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


class KdBatch:
    def __init__(self, n_scenes, max_points, handle=None):
        """handle: a borrowed amk_kd* (a pipeline slot's); it is then not destroyed by this object."""
        self.lib = capi.load()
        self.S, self.max_points = int(n_scenes), int(max_points)
        self.owned = handle is None
        if handle is None:
            handle = C.c_void_p()
            capi.check(self.lib.amk_kd_create(self.S, self.max_points, C.byref(handle)), "amk_kd_create")
        self.h = handle if isinstance(handle, C.c_void_p) else C.c_void_p(handle)

    def close(self):
        if getattr(self, "h", None):
            if self.owned:
                self.lib.amk_kd_destroy(self.h)
            self.h = None

    __del__ = close

    def set_tie_order(self, mode):
        """capi.AMK_TIES_LOWEST_INDEX (default), capi.AMK_TIES_NANOFLANN (the reference's tree for every scene at every build) or
        capi.AMK_TIES_AUTO (the same answers; the tree is built on the device only for scenes where a query ties, and only tied
        queries go through it; search k + 1 <= AMK_MAX_K, single-frame step only).  Takes effect at the next build."""
        capi.check(self.lib.amk_kd_set_tie_order(self.h, int(mode)), "amk_kd_set_tie_order")

    def exact_status(self, stream=None):
        """amk_kd_exact_status: int32 device tensor [S] -- -1 mode off / 0 the reference-shaped tree answers / 1 its build gave up /
        2 deeper than the traversal stack (1, 2: the bucketed index answers) / 3 (AMK_TIES_AUTO only) no query of the scene has tied
        since the last build, so it has no tree and the bucketed index has given the reference's answers."""
        st = torch.empty(self.S, dtype=torch.int32, device="cuda")
        capi.check(self.lib.amk_kd_exact_status(self.h, capi.dptr(st), capi.stream_ptr(stream)), "amk_kd_exact_status")
        return st

    def build(self, xyz, counts=None, stream=None):
        """InitializeNew: xyz float32 device tensor [S, max_points, 3|4]; counts int32 [S] or None."""
        assert xyz.dtype == torch.float32 and xyz.dim() == 3 and xyz.shape[0] == self.S
        assert xyz.shape[1] >= self.max_points or self.max_points == 0
        if counts is not None:
            assert counts.dtype == torch.int32 and counts.numel() == self.S
        capi.check(self.lib.amk_kd_build(self.h, capi.dptr(xyz), int(xyz.shape[2]),
                                         int(xyz.shape[1] * xyz.shape[2]), capi.dptr(counts),
                                         capi.stream_ptr(stream)), "amk_kd_build")

    def sizes(self, stream=None):
        out = np.zeros(self.S, np.int32)
        capi.check(self.lib.amk_kd_sizes(self.h, out.ctypes.data_as(C.c_void_p), capi.stream_ptr(stream)),
                   "amk_kd_sizes")
        return out

    def search(self, queries, k, want_pts=True, stream=None, out=None):
        """SearchForNearest for queries float64 [S, Q, 3] -> dict(indices, sqdist, pts, counts)."""
        assert queries.dtype == torch.float64 and queries.shape[0] == self.S and queries.shape[2] == 3
        Q = int(queries.shape[1])
        dev = queries.device
        if out is None:
            out = dict(indices=torch.empty((self.S, Q, k), dtype=torch.int32, device=dev),
                       sqdist=torch.empty((self.S, Q, k), dtype=torch.float64, device=dev),
                       pts=torch.empty((self.S, Q, k, 3), dtype=torch.float32, device=dev) if want_pts else None,
                       counts=torch.empty((self.S, Q), dtype=torch.int32, device=dev))
        capi.check(self.lib.amk_kd_search(self.h, capi.dptr(queries), Q, int(k), capi.dptr(out["indices"]),
                                          capi.dptr(out["sqdist"]), capi.dptr(out["pts"]),
                                          capi.dptr(out["counts"]), capi.stream_ptr(stream)), "amk_kd_search")
        return out

    def radius_search(self, queries, radius_sq, max_results, want_pts=True, stream=None, out=None):
        """amk_kd_radius_search: nanoflann's radiusSearch for queries float64 [S, Q, >= 3] (the first three of every row are read).
        radius_sq: a SQUARED distance, the test is strict (d2 < radius_sq); counts [S, Q] is the full number of usable points within
        the radius whatever max_results; the lists hold the nearest max_results of them, ascending, ties by cloud index, empty slots
        -1 / DBL_MAX / 0.  max_results = 0: the pure count (no lists).  -> dict(indices, sqdist, pts, counts)"""
        Q, stride = _check_queries(queries, self.S)
        k, dev = int(max_results), queries.device
        if out is None:
            lists = k > 0
            out = dict(indices=torch.empty((self.S, Q, k), dtype=torch.int32, device=dev) if lists else None,
                       sqdist=torch.empty((self.S, Q, k), dtype=torch.float64, device=dev) if lists else None,
                       pts=torch.empty((self.S, Q, k, 3), dtype=torch.float32, device=dev) if lists and want_pts else None,
                       counts=torch.empty((self.S, Q), dtype=torch.int32, device=dev))
        capi.check(self.lib.amk_kd_radius_search(self.h, capi.dptr(queries), stride, Q, float(radius_sq), k, capi.dptr(out["indices"]),
                                                 capi.dptr(out["sqdist"]), capi.dptr(out["pts"]), capi.dptr(out["counts"]),
                                                 _stream_arg(stream)), "amk_kd_radius_search")
        return out

    def keyframe_sweep(self, current, th_dist, th_count, stream=None):
        """KeyframeThreadWorker's sweep: self = last keyframe, rebuilt from its outliers w.r.t. `current`.
        -> (outliers int32 [S], rebuilt int32 [S]) device tensors"""
        dev = _dev()
        outl = torch.empty(self.S, dtype=torch.int32, device=dev)
        reb = torch.empty(self.S, dtype=torch.int32, device=dev)
        capi.check(self.lib.amk_kd_keyframe_sweep(self.h, current.h, float(th_dist), int(th_count), capi.dptr(outl),
                                                  capi.dptr(reb), capi.stream_ptr(stream)), "amk_kd_keyframe_sweep")
        return outl, reb

    # host-buffer conveniences ---------------------------------------------------------------
    def build_host(self, xyz, counts=None):
        xyz = np.ascontiguousarray(xyz, np.float32)
        assert xyz.ndim == 3 and xyz.shape[0] == self.S
        cp = None
        if counts is not None:
            counts = np.ascontiguousarray(counts, np.int32)
            cp = counts.ctypes.data_as(C.c_void_p)
        capi.check(self.lib.amk_kd_build_host(self.h, xyz.ctypes.data_as(C.c_void_p), int(xyz.shape[2]),
                                              int(xyz.shape[1] * xyz.shape[2]), cp), "amk_kd_build_host")

    def search_host(self, queries, k):
        q = np.ascontiguousarray(queries, np.float64)
        assert q.ndim == 3 and q.shape[0] == self.S and q.shape[2] == 3
        Q = q.shape[1]
        idx = np.zeros((self.S, Q, k), np.int32); d2 = np.zeros((self.S, Q, k), np.float64)
        pts = np.zeros((self.S, Q, k, 3), np.float32); cnt = np.zeros((self.S, Q), np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        capi.check(self.lib.amk_kd_search_host(self.h, vp(q), Q, int(k), vp(idx), vp(d2), vp(pts), vp(cnt)),
                   "amk_kd_search_host")
        return dict(indices=idx, sqdist=d2, pts=pts, counts=cnt)


    def radius_search_host(self, queries, radius_sq, max_results):
        """amk_kd_radius_search_host: radius_search with numpy buffers (queries [S, Q, >= 3]); synchronises."""
        q = np.ascontiguousarray(queries, np.float64)
        assert q.ndim == 3 and q.shape[0] == self.S and q.shape[2] >= 3
        Q, k = q.shape[1], int(max_results)
        idx = np.zeros((self.S, Q, k), np.int32); d2 = np.zeros((self.S, Q, k), np.float64)
        pts = np.zeros((self.S, Q, k, 3), np.float32); cnt = np.zeros((self.S, Q), np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        lst = (lambda a: vp(a)) if k > 0 else (lambda a: None)   # max_results = 0 is the pure count: no list pointers
        capi.check(self.lib.amk_kd_radius_search_host(self.h, vp(q), int(q.shape[2]), Q, float(radius_sq), k, lst(idx), lst(d2), lst(pts),
                                                      vp(cnt)), "amk_kd_radius_search_host")
        return dict(indices=idx, sqdist=d2, pts=pts, counts=cnt)

    def segment_search(self, path, radius_sq, max_results, want_pts=True, stream=None, out=None):
        """amk_kd_segment_search: the points within a radius of every leg of a path, float64 [S, n_points >= 2, >= 3] (the first
        three of every row are read; leg j runs from point j to point j + 1).  radius_sq: a SQUARED distance, the test is strict;
        counts [S, n_legs] is the full number whatever max_results; the lists hold the nearest max_results, ascending, ties by cloud
        index, t = where along the leg (0 .. 1) each comes closest, empty slots -1 / DBL_MAX / 0.  max_results = 0: the pure count
        (no lists).  -> dict(indices, sqdist, t, pts, counts)"""
        P, stride = _check_path(path, self.S)
        k, dev, L = int(max_results), path.device, P - 1
        if out is None:
            lists = k > 0
            out = dict(indices=torch.empty((self.S, L, k), dtype=torch.int32, device=dev) if lists else None,
                       sqdist=torch.empty((self.S, L, k), dtype=torch.float64, device=dev) if lists else None,
                       t=torch.empty((self.S, L, k), dtype=torch.float64, device=dev) if lists else None,
                       pts=torch.empty((self.S, L, k, 3), dtype=torch.float32, device=dev) if lists and want_pts else None,
                       counts=torch.empty((self.S, L), dtype=torch.int32, device=dev))
        capi.check(self.lib.amk_kd_segment_search(self.h, capi.dptr(path), stride, P, float(radius_sq), k, capi.dptr(out["indices"]),
                                                  capi.dptr(out["sqdist"]), capi.dptr(out["t"]), capi.dptr(out["pts"]),
                                                  capi.dptr(out["counts"]), _stream_arg(stream)), "amk_kd_segment_search")
        return out

    def segment_search_host(self, path, radius_sq, max_results):
        """amk_kd_segment_search_host: segment_search with numpy buffers (path [S, n_points, >= 3]); synchronises."""
        p = np.ascontiguousarray(path, np.float64)
        assert p.ndim == 3 and p.shape[0] == self.S and p.shape[2] >= 3
        L, k = p.shape[1] - 1, int(max_results)
        idx = np.zeros((self.S, L, k), np.int32); d2 = np.zeros((self.S, L, k), np.float64); t = np.zeros((self.S, L, k), np.float64)
        pts = np.zeros((self.S, L, k, 3), np.float32); cnt = np.zeros((self.S, L), np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        lst = (lambda a: vp(a)) if k > 0 else (lambda a: None)   # max_results = 0 is the pure count: no list pointers
        capi.check(self.lib.amk_kd_segment_search_host(self.h, vp(p), int(p.shape[2]), int(p.shape[1]), float(radius_sq), k, lst(idx),
                                                       lst(d2), lst(t), lst(pts), vp(cnt)), "amk_kd_segment_search_host")
        return dict(indices=idx, sqdist=d2, t=t, pts=pts, counts=cnt)

    def segment_nearest(self, path, k, want_pts=True, stream=None, out=None):
        """amk_kd_segment_nearest: the k usable points closest to every leg of a path, float64 [S, n_points >= 2, >= 3], no radius:
        ascending, ties by cloud index, t = where along the leg (0 .. 1) each comes closest; counts [S, n_legs] = min(k, usable
        points of the scene), empty slots -1 / DBL_MAX / 0.  The lists are those of segment_search(path, inf, k), bit for bit.
        -> dict(indices, sqdist, t, pts, counts)"""
        P, stride = _check_path(path, self.S)
        k, dev, L = int(k), path.device, P - 1
        if out is None:
            out = dict(indices=torch.empty((self.S, L, k), dtype=torch.int32, device=dev),
                       sqdist=torch.empty((self.S, L, k), dtype=torch.float64, device=dev),
                       t=torch.empty((self.S, L, k), dtype=torch.float64, device=dev),
                       pts=torch.empty((self.S, L, k, 3), dtype=torch.float32, device=dev) if want_pts else None,
                       counts=torch.empty((self.S, L), dtype=torch.int32, device=dev))
        capi.check(self.lib.amk_kd_segment_nearest(self.h, capi.dptr(path), stride, P, k, capi.dptr(out["indices"]),
                                                   capi.dptr(out["sqdist"]), capi.dptr(out["t"]), capi.dptr(out["pts"]),
                                                   capi.dptr(out["counts"]), _stream_arg(stream)), "amk_kd_segment_nearest")
        return out

    def segment_nearest_host(self, path, k):
        """amk_kd_segment_nearest_host: segment_nearest with numpy buffers (path [S, n_points, >= 3]); synchronises."""
        p = np.ascontiguousarray(path, np.float64)
        assert p.ndim == 3 and p.shape[0] == self.S and p.shape[2] >= 3
        L, k = p.shape[1] - 1, int(k)
        idx = np.zeros((self.S, L, k), np.int32); d2 = np.zeros((self.S, L, k), np.float64); t = np.zeros((self.S, L, k), np.float64)
        pts = np.zeros((self.S, L, k, 3), np.float32); cnt = np.zeros((self.S, L), np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        capi.check(self.lib.amk_kd_segment_nearest_host(self.h, vp(p), int(p.shape[2]), int(p.shape[1]), k, vp(idx), vp(d2), vp(t),
                                                        vp(pts), vp(cnt)), "amk_kd_segment_nearest_host")
        return dict(indices=idx, sqdist=d2, t=t, pts=pts, counts=cnt)

    def segment_cast(self, path, radius_sq, want_pts=True, stream=None, out=None):
        """amk_kd_segment_cast: the first contact of a sphere of SQUARED radius radius_sq whose centre moves along every leg of a
        path, float64 [S, n_points >= 2, >= 3]: hit [S, n_legs] 1 / 0, t where along the leg the contact begins (1.0 without one, so
        t * |ab| is the free distance), the point touched and its cloud index (-1 / (0,0,0) without one); the least t, ties by
        cloud index.  -> dict(hit, t, pts, indices)"""
        P, stride = _check_path(path, self.S)
        dev, L = path.device, P - 1
        if out is None:
            out = _cast_out(self.S, L, dev, "indices", want_pts)
        capi.check(self.lib.amk_kd_segment_cast(self.h, capi.dptr(path), stride, P, float(radius_sq), capi.dptr(out["hit"]),
                                                capi.dptr(out["t"]), capi.dptr(out["pts"]), capi.dptr(out["indices"]),
                                                _stream_arg(stream)), "amk_kd_segment_cast")
        return out

    def segment_cast_host(self, path, radius_sq):
        """amk_kd_segment_cast_host: segment_cast with numpy buffers (path [S, n_points, >= 3]); synchronises."""
        p = np.ascontiguousarray(path, np.float64)
        assert p.ndim == 3 and p.shape[0] == self.S and p.shape[2] >= 3
        L = p.shape[1] - 1
        hit = np.zeros((self.S, L), np.int32); t = np.zeros((self.S, L), np.float64)
        pts = np.zeros((self.S, L, 3), np.float32); idx = np.zeros((self.S, L), np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        capi.check(self.lib.amk_kd_segment_cast_host(self.h, vp(p), int(p.shape[2]), int(p.shape[1]), float(radius_sq), vp(hit), vp(t),
                                                     vp(pts), vp(idx)), "amk_kd_segment_cast_host")
        return dict(hit=hit, t=t, pts=pts, indices=idx)

    def path_cast(self, path, radius_sq, want_pts=True, stream=None, out=None):
        """amk_kd_path_cast: ONE answer per scene for a whole path float64 [S, n_points >= 2, >= 3] -- the first leg that cannot be
        passed: stop [S] 0 free / 1 contact / 2 unjudgeable (non-finite) leg, leg (-1 when free), t on that leg, free = the free
        distance along the path, the point touched and its cloud index.  The reduction of segment_cast's per-leg answers, bit for
        bit; legs behind the stop leg are not walked.  -> dict(stop, leg, t, free, pts, indices)"""
        P, stride = _check_path(path, self.S)
        if out is None:
            out = _path_cast_out(self.S, path.device, "indices", want_pts)
        capi.check(self.lib.amk_kd_path_cast(self.h, capi.dptr(path), stride, P, float(radius_sq), capi.dptr(out["stop"]),
                                             capi.dptr(out["leg"]), capi.dptr(out["t"]), capi.dptr(out["free"]), capi.dptr(out["pts"]),
                                             capi.dptr(out["indices"]), _stream_arg(stream)), "amk_kd_path_cast")
        return out

    def path_cast_host(self, path, radius_sq):
        """amk_kd_path_cast_host: path_cast with numpy buffers (path [S, n_points, >= 3]); synchronises."""
        p = np.ascontiguousarray(path, np.float64)
        assert p.ndim == 3 and p.shape[0] == self.S and p.shape[2] >= 3
        stop = np.zeros(self.S, np.int32); leg = np.zeros(self.S, np.int32); idx = np.zeros(self.S, np.int32)
        t = np.zeros(self.S, np.float64); free = np.zeros(self.S, np.float64); pts = np.zeros((self.S, 3), np.float32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        capi.check(self.lib.amk_kd_path_cast_host(self.h, vp(p), int(p.shape[2]), int(p.shape[1]), float(radius_sq), vp(stop), vp(leg),
                                                  vp(t), vp(free), vp(pts), vp(idx)), "amk_kd_path_cast_host")
        return dict(stop=stop, leg=leg, t=t, free=free, pts=pts, indices=idx)


def _path_cast_out(S, dev, which, want_pts=True):
    """outputs of the path casts, one result per scene; which: "indices" (one handle) or "frame" (a map, a list of handles)"""
    i32 = lambda: torch.empty((S,), dtype=torch.int32, device=dev)
    f64 = lambda: torch.empty((S,), dtype=torch.float64, device=dev)
    return {"stop": i32(), "leg": i32(), "t": f64(), "free": f64(),
            "pts": torch.empty((S, 3), dtype=torch.float32, device=dev) if want_pts else None, which: i32()}


def _cast_out(S, L, dev, which, want_pts=True):
    """outputs of the segment casts, one result per leg; which: "indices" (one handle) or "frame" (a map, a list of handles)"""
    return {"hit": torch.empty((S, L), dtype=torch.int32, device=dev), "t": torch.empty((S, L), dtype=torch.float64, device=dev),
            "pts": torch.empty((S, L, 3), dtype=torch.float32, device=dev) if want_pts else None,
            which: torch.empty((S, L), dtype=torch.int32, device=dev)}


def kd_build_pair(kd_obstacle, xyz, kd_edge, edge_xyz, counts=None, edge_counts=None, stream=None):
    """amk_kd_build_pair: FrameKDMap::AddVertex's two InitializeNew calls as one launch (clouds packed [S, max_points, 3|4])."""
    assert xyz.dtype == torch.float32 and edge_xyz.dtype == torch.float32 and xyz.shape[2] == edge_xyz.shape[2]
    assert xyz.shape[1] == kd_obstacle.max_points and edge_xyz.shape[1] == kd_edge.max_points
    capi.check(capi.load().amk_kd_build_pair(kd_obstacle.h, capi.dptr(xyz), capi.dptr(counts), kd_edge.h, capi.dptr(edge_xyz),
                                             capi.dptr(edge_counts), int(xyz.shape[2]), capi.stream_ptr(stream)), "amk_kd_build_pair")


def kd_tie_flags(kd, queries, k, query_stride=3, stream=None):
    """amk_kd_tie_flags: int32 [S, n_queries], 1 where the k nearest (or the k-th and the best rejected) hold an exact tie."""
    S = kd.S if hasattr(kd, "S") else queries.shape[0]
    nq = int(queries.shape[1])
    out = torch.empty((S, nq), dtype=torch.int32, device=queries.device)
    capi.check(capi.load().amk_kd_tie_flags(kd.h, capi.dptr(queries), int(query_stride), nq, int(k), capi.dptr(out),
                                            capi.stream_ptr(stream)), "amk_kd_tie_flags")
    return out


class MpcBatch:
    def __init__(self, T, dt, nearest_point_num, n_scenes, handle=None):
        """handle: a borrowed amk_mpc* (a pipeline slot's); it is then not destroyed by this object."""
        self.lib = capi.load()
        self.owned = handle is None
        if handle is None:
            handle = C.c_void_p()
            capi.check(self.lib.amk_mpc_create(float(T), float(dt), int(nearest_point_num), int(n_scenes),
                                               C.byref(handle)), "amk_mpc_create")
        h = handle if isinstance(handle, C.c_void_p) else C.c_void_p(handle)
        self.h = h
        self.S, self.K = int(n_scenes), int(nearest_point_num)
        self.N = self.lib.amk_mpc_horizon(h)
        self.nx = self.lib.amk_mpc_nx(h)
        self.ref_len = self.lib.amk_mpc_ref_len(h)

    def close(self):
        if getattr(self, "h", None):
            if self.owned:
                self.lib.amk_mpc_destroy(self.h)
            self.h = None

    __del__ = close

    def _arr(self, v, n):
        a = np.ascontiguousarray(v, np.float64)
        assert a.size == n
        return a.ctypes.data_as(C.c_void_p), a

    def SetupWeights(self, w):
        p, _k = self._arr(w, 25); capi.check(self.lib.amk_mpc_setup_weights(self.h, p), "SetupWeights")

    def SetupTau(self, tau):
        p, _k = self._arr(tau, 4); capi.check(self.lib.amk_mpc_setup_tau(self.h, p), "SetupTau")

    def SetupGains(self, g):
        p, _k = self._arr(g, 4); capi.check(self.lib.amk_mpc_setup_gains(self.h, p), "SetupGains")

    def SetDroneRadius(self, r):
        capi.check(self.lib.amk_mpc_set_drone_radius(self.h, float(r)), "SetDroneRadius")

    def SetDragCoefficient(self, kx, ky=None, kz=None):
        """v' = a - k .* v (the generator's use_drag_coefficient switch read as matrix products: include/avoid_mpc_amd.h); one value = isotropic."""
        ky = kx if ky is None else ky; kz = kx if kz is None else kz
        capi.check(self.lib.amk_mpc_set_drag_coefficient(self.h, float(kx), float(ky), float(kz)), "SetDragCoefficient")

    def SetDroneAccelLimits(self, aMinZ, aMaxZ, aMaxXy, aMaxYawDot):
        capi.check(self.lib.amk_mpc_set_drone_accel_limits(self.h, float(aMinZ), float(aMaxZ), float(aMaxXy),
                                                           float(aMaxYawDot)), "SetDroneAccelLimits")

    def set_solver_options(self, tol=1e-4, max_iter=capi.AMK_MPC_DEFAULT_MAX_ITER):
        capi.check(self.lib.amk_mpc_set_solver_options(self.h, float(tol), int(max_iter)), "set_solver_options")

    def set_solve_budget(self, budget, budget_rounds=0):
        """amk_mpc_set_solve_budget: interior-point iterations per solve LAUNCH inside amk_step_batch (0: off); unfinished solves
        pause and are resumed inside the next round's launch.  A scheduling knob: results are unchanged bit for bit."""
        capi.check(self.lib.amk_mpc_set_solve_budget(self.h, int(budget), int(budget_rounds)), "set_solve_budget")

    def set_precision(self, bits):
        """64 (default) or 32: arithmetic of the solve (BASELINE config C5's fp32 tolerance check)."""
        capi.check(self.lib.amk_mpc_set_precision(self.h, int(bits)), "set_precision")

    def configure(self, prm):
        """SetupMPC (AvoidanceStateMachine.cpp:55-70) from a synth.MpcParams."""
        self.SetupWeights(prm.weights); self.SetupTau(prm.tau); self.SetupGains(prm.gain)
        self.SetDroneAccelLimits(prm.a_min_z, prm.a_max_z, prm.a_max_xy, prm.a_max_yaw_dot)
        self.SetDroneRadius(prm.radius)
        self.SetDragCoefficient(*getattr(prm, "drag", (0.0, 0.0, 0.0)))   # always: a handle configured before may carry another drag

    def Solve(self, ref_states, faster=False, stream=None, want_traj=True):
        assert ref_states.dtype == torch.float64 and tuple(ref_states.shape) == (self.S, self.ref_len)
        dev = ref_states.device
        u = torch.empty((self.S, 4), dtype=torch.float64, device=dev)
        x0 = torch.empty((self.S, self.N, 14), dtype=torch.float64, device=dev) if want_traj else None
        info = torch.empty((self.S, 4), dtype=torch.int32, device=dev)
        capi.check(self.lib.amk_mpc_solve(self.h, capi.dptr(ref_states), capi.dptr(u), capi.dptr(x0),
                                          capi.dptr(info), int(bool(faster)), capi.stream_ptr(stream)),
                   "amk_mpc_solve")
        return u, x0, info

    def eval(self, w, ref_states, lam_f=None, stream=None, want=("f", "grad_f", "g", "jac_g", "hess_l")):
        """amk_mpc_eval: the plugin's nlp_f / nlp_grad_f / nlp_g / nlp_jac_g / nlp_hess_l at w [S, nx] -> dict of tensors."""
        assert w.dtype == torch.float64 and tuple(w.shape) == (self.S, self.nx)
        assert ref_states.dtype == torch.float64 and tuple(ref_states.shape) == (self.S, self.ref_len)
        dev = w.device
        shp = dict(f=(self.S,), grad_f=(self.S, self.nx), g=(self.S, self.lib.amk_mpc_ng(self.h)),
                   jac_g=(self.S, self.lib.amk_mpc_jac_nnz(self.h)), hess_l=(self.S, self.lib.amk_mpc_hess_nnz(self.h)))
        out = {k: torch.empty(shp[k], dtype=torch.float64, device=dev) for k in want}
        capi.check(self.lib.amk_mpc_eval(self.h, capi.dptr(w), capi.dptr(ref_states), capi.dptr(lam_f),
                                         *[capi.dptr(out.get(k)) for k in ("f", "grad_f", "g", "jac_g", "hess_l")],
                                         capi.stream_ptr(stream)), "amk_mpc_eval")
        return out

    def sparsity(self, which):
        """CCS pattern ('jac_g' or 'hess_l') -> (colind int32 [nx + 1], row int32 [nnz])."""
        nnz = (self.lib.amk_mpc_jac_nnz if which == "jac_g" else self.lib.amk_mpc_hess_nnz)(self.h)
        colind = np.zeros(self.nx + 1, np.int32); row = np.zeros(nnz, np.int32)
        fn = self.lib.amk_mpc_jac_sparsity if which == "jac_g" else self.lib.amk_mpc_hess_sparsity
        capi.check(fn(self.h, colind.ctypes.data_as(C.c_void_p), row.ctypes.data_as(C.c_void_p)), which + " sparsity")
        return colind, row

    def get_warm_start(self, stream=None):
        w = torch.empty((self.S, self.nx), dtype=torch.float64, device=_dev())
        capi.check(self.lib.amk_mpc_get_warm_start(self.h, capi.dptr(w), capi.stream_ptr(stream)), "get_warm_start")
        return w

    def set_warm_start(self, w, stream=None):
        assert w.dtype == torch.float64 and tuple(w.shape) == (self.S, self.nx)
        capi.check(self.lib.amk_mpc_set_warm_start(self.h, capi.dptr(w), capi.stream_ptr(stream)), "set_warm_start")

    def reset_warm_start(self, stream=None):
        capi.check(self.lib.amk_mpc_reset_warm_start(self.h, capi.stream_ptr(stream)), "reset_warm_start")

    def ref_states(self):
        """(tests) float64 [S, ref_len]: the P vectors the newest pass of the last control step handed to the solve (synchronises)."""
        P = np.zeros((self.S, self.ref_len))
        capi.check(self.lib.amk__mpc_ref_states(self.h, P.ctypes.data_as(C.c_void_p), P.size), "amk__mpc_ref_states")
        return P


def _stream_arg(stream):
    """A torch stream, None (torch's current stream) or a raw hipStream_t (int / c_void_p, e.g. amk_pipeline_stream)."""
    if isinstance(stream, C.c_void_p):
        return stream
    if isinstance(stream, int):
        return C.c_void_p(stream)
    return capi.stream_ptr(stream)


def _check_queries(queries, S):
    assert queries.dtype == torch.float64 and queries.dim() == 3 and queries.shape[0] == S and queries.shape[2] >= 3 and queries.shape[1] >= 1
    return int(queries.shape[1]), int(queries.shape[2])


def _query_out(S, Q, k, dev):
    return dict(pts=torch.empty((S, Q, k, 3), dtype=torch.float32, device=dev), sqdist=torch.empty((S, Q, k), dtype=torch.float64, device=dev),
                frame=torch.empty((S, Q, k), dtype=torch.int32, device=dev), counts=torch.empty((S, Q), dtype=torch.int32, device=dev))


def query_frames(handles, queries, k, Twc=None, cam=None, stream=None, out=None):
    """amk_kd_query_frames: FrameKDMap::QueryNearest over a list of KdBatch handles (obstacle OR edge, index 0 = current frame).
    queries float64 [S, Q, >= 3]; Twc float64 [S, 4, 4] or None; cam: capi.FrameCamera.  -> dict(pts, sqdist, frame, counts)"""
    F, S = len(handles), handles[0].S
    Q, stride = _check_queries(queries, S)
    if out is None:
        out = _query_out(S, Q, int(k), queries.device)
    ha = (C.c_void_p * F)(*[h.h for h in handles])
    capi.check(capi.load().amk_kd_query_frames(ha, F, capi.dptr(Twc), C.byref(cam) if cam is not None else None, capi.dptr(queries), stride,
                                               Q, int(k), capi.dptr(out["pts"]), capi.dptr(out["sqdist"]), capi.dptr(out["frame"]),
                                               capi.dptr(out["counts"]), _stream_arg(stream)), "amk_kd_query_frames")
    return out


def nearest_distance_frames(handles, queries, stream=None, out=None):
    """amk_kd_nearest_distance_frames: FrameKDMap::GetNearestDistance over a list of KdBatch handles -> float64 [S, Q]"""
    F, S = len(handles), handles[0].S
    Q, stride = _check_queries(queries, S)
    if out is None:
        out = torch.empty((S, Q), dtype=torch.float64, device=queries.device)
    ha = (C.c_void_p * F)(*[h.h for h in handles])
    capi.check(capi.load().amk_kd_nearest_distance_frames(ha, F, capi.dptr(queries), stride, Q, capi.dptr(out), _stream_arg(stream)),
               "amk_kd_nearest_distance_frames")
    return out


def _radius_out(S, Q, k, dev):
    """outputs of the multi-frame radius searches; max_results = 0 is the pure count: no lists"""
    out = _query_out(S, Q, k, dev)
    return out if k > 0 else dict(pts=None, sqdist=None, frame=None, counts=out["counts"])


def radius_search_frames(handles, queries, radius_sq, max_results, stream=None, out=None):
    """amk_kd_radius_search_frames: the radius search over a list of KdBatch handles (obstacle OR edge, index 0 = current frame);
    counts sum over the frames, the lists merge by (squared distance, frame, cloud index).  -> dict(pts, sqdist, frame, counts)"""
    F, S = len(handles), handles[0].S
    Q, stride = _check_queries(queries, S)
    if out is None:
        out = _radius_out(S, Q, int(max_results), queries.device)
    ha = (C.c_void_p * F)(*[h.h for h in handles])
    capi.check(capi.load().amk_kd_radius_search_frames(ha, F, capi.dptr(queries), stride, Q, float(radius_sq), int(max_results),
                                                       capi.dptr(out["pts"]), capi.dptr(out["sqdist"]), capi.dptr(out["frame"]),
                                                       capi.dptr(out["counts"]), _stream_arg(stream)), "amk_kd_radius_search_frames")
    return out


def _check_path(path, S):
    assert path.dtype == torch.float64 and path.dim() == 3 and path.shape[0] == S and path.shape[2] >= 3 and path.shape[1] >= 1
    return int(path.shape[1]), int(path.shape[2])


def _segment_out(S, L, k, dev):
    """outputs of the multi-frame segment searches, a row per leg; max_results = 0 is the pure count: no lists"""
    out = _radius_out(S, L, k, dev)
    out["t"] = torch.empty((S, L, k), dtype=torch.float64, device=dev) if k > 0 else None
    return out


def segment_search_frames(handles, path, radius_sq, max_results, stream=None, out=None):
    """amk_kd_segment_search_frames: the segment search over a list of KdBatch handles (obstacle OR edge, index 0 = current frame);
    counts sum over the frames, the lists merge by (squared distance, frame, cloud index).  -> dict(pts, sqdist, t, frame, counts)"""
    F, S = len(handles), handles[0].S
    P, stride = _check_path(path, S)
    if out is None:
        out = _segment_out(S, P - 1, int(max_results), path.device)
    ha = (C.c_void_p * F)(*[h.h for h in handles])
    capi.check(capi.load().amk_kd_segment_search_frames(ha, F, capi.dptr(path), stride, P, float(radius_sq), int(max_results),
                                                        capi.dptr(out["pts"]), capi.dptr(out["sqdist"]), capi.dptr(out["t"]),
                                                        capi.dptr(out["frame"]), capi.dptr(out["counts"]), _stream_arg(stream)),
               "amk_kd_segment_search_frames")
    return out


def segment_nearest_frames(handles, path, k, stream=None, out=None):
    """amk_kd_segment_nearest_frames: segment nearest over a list of KdBatch handles (obstacle OR edge, index 0 = current frame):
    per leg the k nearest of all frames by (squared distance, frame, cloud index), counts = min(k, usable points over the frames).
    -> dict(pts, sqdist, t, frame, counts)"""
    F, S = len(handles), handles[0].S
    P, stride = _check_path(path, S)
    if out is None:
        out = _segment_out(S, P - 1, int(k), path.device)
    ha = (C.c_void_p * F)(*[h.h for h in handles])
    capi.check(capi.load().amk_kd_segment_nearest_frames(ha, F, capi.dptr(path), stride, P, int(k), capi.dptr(out["pts"]),
                                                         capi.dptr(out["sqdist"]), capi.dptr(out["t"]), capi.dptr(out["frame"]),
                                                         capi.dptr(out["counts"]), _stream_arg(stream)),
               "amk_kd_segment_nearest_frames")
    return out


def segment_cast_frames(handles, path, radius_sq, stream=None, out=None):
    """amk_kd_segment_cast_frames: the segment cast over a list of KdBatch handles (obstacle OR edge, index 0 = current frame): per
    leg the first contact over all frames by (t, frame, cloud index).  -> dict(hit, t, pts, frame)"""
    F, S = len(handles), handles[0].S
    P, stride = _check_path(path, S)
    if out is None:
        out = _cast_out(S, P - 1, path.device, "frame")
    ha = (C.c_void_p * F)(*[h.h for h in handles])
    capi.check(capi.load().amk_kd_segment_cast_frames(ha, F, capi.dptr(path), stride, P, float(radius_sq), capi.dptr(out["hit"]),
                                                      capi.dptr(out["t"]), capi.dptr(out["pts"]), capi.dptr(out["frame"]),
                                                      _stream_arg(stream)), "amk_kd_segment_cast_frames")
    return out


def path_cast_frames(handles, path, radius_sq, stream=None, out=None):
    """amk_kd_path_cast_frames: the path cast over a list of KdBatch handles (obstacle OR edge, index 0 = current frame): per scene
    the first leg that cannot be passed, a leg's contact the least (t, frame, cloud index).  -> dict(stop, leg, t, free, pts, frame)"""
    F, S = len(handles), handles[0].S
    P, stride = _check_path(path, S)
    if out is None:
        out = _path_cast_out(S, path.device, "frame")
    ha = (C.c_void_p * F)(*[h.h for h in handles])
    capi.check(capi.load().amk_kd_path_cast_frames(ha, F, capi.dptr(path), stride, P, float(radius_sq), capi.dptr(out["stop"]),
                                                   capi.dptr(out["leg"]), capi.dptr(out["t"]), capi.dptr(out["free"]),
                                                   capi.dptr(out["pts"]), capi.dptr(out["frame"]), _stream_arg(stream)),
               "amk_kd_path_cast_frames")
    return out


class KfMap:
    """amk_kfmap: FrameKDMap's keyframe list for S scenes on the device (FrameKDMap.cpp:29-74,233-252,428-488)."""

    def __init__(self, n_scenes, max_points, max_edge_points, max_frame_count, th_dist, th_count, depth_min, Tbc, handle=None):
        """handle: a borrowed amk_kfmap* (a pipeline slot's); it is then not destroyed by this object."""
        self.lib = capi.load()
        self.owned = handle is None
        if handle is not None:
            self.h = handle if isinstance(handle, C.c_void_p) else C.c_void_p(handle)
            self.S, self.F = self.lib.amk_kfmap_scenes(self.h), self.lib.amk_kfmap_frames(self.h)
            self.max_points, self.max_edge_points = int(max_points), int(max_edge_points)
            return
        p = capi.KfmapParams(int(max_frame_count), int(th_count), float(th_dist), float(depth_min),
                             (C.c_double * 16)(*[float(v) for v in np.asarray(Tbc, np.float64).reshape(-1)]))
        h = C.c_void_p()
        capi.check(self.lib.amk_kfmap_create(int(n_scenes), int(max_points), int(max_edge_points), C.byref(p), C.byref(h)), "amk_kfmap_create")
        self.h, self.S, self.F = h, int(n_scenes), int(max_frame_count) + 1
        self.max_points, self.max_edge_points = int(max_points), int(max_edge_points)

    def close(self):
        if getattr(self, "h", None):
            if self.owned:
                self.lib.amk_kfmap_destroy(self.h)
            self.h = None

    __del__ = close

    def add_vertex(self, clouds, edges, Twc, counts=None, edge_counts=None, first_scene=0, stream=None):
        """clouds [n, max_points, 3|4] f32, edges likewise, Twc [n, 4, 4] f64 = Twb * Tbc of the frame; counts int32 [n] or None."""
        assert clouds.dtype == torch.float32 and edges.dtype == torch.float32 and Twc.dtype == torch.float64
        assert clouds.shape[1] == self.max_points and edges.shape[1] == self.max_edge_points and clouds.shape[2] == edges.shape[2]
        capi.check(self.lib.amk_kfmap_add_vertex(self.h, int(first_scene), int(clouds.shape[0]), capi.dptr(clouds), capi.dptr(counts),
                                                 capi.dptr(edges), capi.dptr(edge_counts), int(clouds.shape[2]), capi.dptr(Twc),
                                                 capi.stream_ptr(stream)), "amk_kfmap_add_vertex")

    def update(self, stream=None):
        capi.check(self.lib.amk_kfmap_update(self.h, capi.stream_ptr(stream)), "amk_kfmap_update")

    def step(self, mpc, prm, state_quad, pos_x, ref_path, cam=None, stream=None, out=None):
        """amk_kfmap_step; ref_path is refilled in place.  -> dict(u, x0array, flags)"""
        S, N = self.S, mpc.N
        dev = _dev()
        if out is None:
            out = dict(u=torch.empty((S, 4), dtype=torch.float64, device=dev), x0array=torch.empty((S, N, 14), dtype=torch.float64, device=dev),
                       flags=torch.empty((S, 4), dtype=torch.int32, device=dev))
        sp = capi.StepParams(float(prm.speed), float(prm.safety_distance), int(prm.max_iter), 0)
        capi.check(self.lib.amk_kfmap_step(self.h, C.byref(cam) if cam is not None else None, mpc.h, C.byref(sp), capi.dptr(state_quad),
                                           capi.dptr(pos_x), capi.dptr(ref_path), capi.dptr(out["u"]), capi.dptr(out["x0array"]),
                                           capi.dptr(out["flags"]), capi.stream_ptr(stream)), "amk_kfmap_step")
        return out

    def query_nearest(self, queries, k, cam=None, edge=False, stream=None, out=None):
        """amk_kfmap_query_nearest: FrameKDMap::QueryNearest for queries float64 [S, Q, 3 | 10 | 14 ...] (the first three of every
        row are read) over each scene's own query vector, from the map as it stands.  cam: capi.FrameCamera or None (every query
        counts as inside the current frame); edge: the edge clouds.  stream: a torch stream or a raw hipStream_t (int).
        -> dict(pts [S,Q,k,3] f32, sqdist [S,Q,k] f64, frame [S,Q,k] i32 (position in the query vector, -1 empty), counts [S,Q] i32)"""
        Q, stride = _check_queries(queries, self.S)
        if out is None:
            out = _query_out(self.S, Q, int(k), queries.device)
        capi.check(self.lib.amk_kfmap_query_nearest(self.h, C.byref(cam) if cam is not None else None, capi.dptr(queries), stride, Q, int(k),
                                                    int(bool(edge)), capi.dptr(out["pts"]), capi.dptr(out["sqdist"]), capi.dptr(out["frame"]),
                                                    capi.dptr(out["counts"]), _stream_arg(stream)), "amk_kfmap_query_nearest")
        return out

    def radius_search(self, queries, radius_sq, max_results, edge=False, stream=None, out=None):
        """amk_kfmap_radius_search: nanoflann's radiusSearch for queries float64 [S, Q, >= 3] over every frame each scene's query
        vector holds (no fast path, no frustum test, no size rule).  radius_sq is a squared distance, the test is strict; counts is
        the full number over the frames; the lists hold the nearest max_results, ordered by (squared distance, frame, cloud index).
        -> dict(pts [S,Q,k,3] f32, sqdist [S,Q,k] f64, frame [S,Q,k] i32, counts [S,Q] i32); max_results = 0: counts only"""
        Q, stride = _check_queries(queries, self.S)
        if out is None:
            out = _radius_out(self.S, Q, int(max_results), queries.device)
        capi.check(self.lib.amk_kfmap_radius_search(self.h, capi.dptr(queries), stride, Q, float(radius_sq), int(max_results), int(bool(edge)),
                                                    capi.dptr(out["pts"]), capi.dptr(out["sqdist"]), capi.dptr(out["frame"]),
                                                    capi.dptr(out["counts"]), _stream_arg(stream)), "amk_kfmap_radius_search")
        return out

    def segment_search(self, path, radius_sq, max_results, edge=False, stream=None, out=None):
        """amk_kfmap_segment_search: the points within a radius of every leg of a path float64 [S, n_points >= 2, >= 3], over every
        frame each scene's query vector holds (no fast path, no frustum test, no size rule).  radius_sq is a squared distance, the test
        is strict; counts is the full number over the frames; the lists hold the nearest max_results by (squared distance, frame,
        cloud index) with t, the position of the closest approach along the leg.
        -> dict(pts [S,L,k,3] f32, sqdist, t [S,L,k] f64, frame [S,L,k] i32, counts [S,L] i32), L = n_points - 1; max_results = 0:
        counts only"""
        P, stride = _check_path(path, self.S)
        if out is None:
            out = _segment_out(self.S, P - 1, int(max_results), path.device)
        capi.check(self.lib.amk_kfmap_segment_search(self.h, capi.dptr(path), stride, P, float(radius_sq), int(max_results), int(bool(edge)),
                                                     capi.dptr(out["pts"]), capi.dptr(out["sqdist"]), capi.dptr(out["t"]),
                                                     capi.dptr(out["frame"]), capi.dptr(out["counts"]), _stream_arg(stream)),
                   "amk_kfmap_segment_search")
        return out

    def segment_nearest(self, path, k, edge=False, stream=None, out=None):
        """amk_kfmap_segment_nearest: the k points closest to every leg of a path float64 [S, n_points >= 2, >= 3], over every frame
        each scene's query vector holds (no radius, no fast path, no frustum test, no size rule): the nearest k by (squared distance,
        frame, cloud index) with t, the position of the closest approach along the leg; counts = min(k, usable points over the frames).
        -> dict(pts [S,L,k,3] f32, sqdist, t [S,L,k] f64, frame [S,L,k] i32, counts [S,L] i32), L = n_points - 1"""
        P, stride = _check_path(path, self.S)
        if out is None:
            out = _segment_out(self.S, P - 1, int(k), path.device)
        capi.check(self.lib.amk_kfmap_segment_nearest(self.h, capi.dptr(path), stride, P, int(k), int(bool(edge)), capi.dptr(out["pts"]),
                                                      capi.dptr(out["sqdist"]), capi.dptr(out["t"]), capi.dptr(out["frame"]),
                                                      capi.dptr(out["counts"]), _stream_arg(stream)), "amk_kfmap_segment_nearest")
        return out

    def segment_cast(self, path, radius_sq, edge=False, stream=None, out=None):
        """amk_kfmap_segment_cast: the first contact of a sphere of SQUARED radius radius_sq moving along every leg of a path float64
        [S, n_points >= 2, >= 3], over every frame each scene's query vector holds: the least (t, frame, cloud index); t = 1.0 and
        frame -1 without a contact.  -> dict(hit [S,L] i32, t [S,L] f64, pts [S,L,3] f32, frame [S,L] i32), L = n_points - 1"""
        P, stride = _check_path(path, self.S)
        if out is None:
            out = _cast_out(self.S, P - 1, path.device, "frame")
        capi.check(self.lib.amk_kfmap_segment_cast(self.h, capi.dptr(path), stride, P, float(radius_sq), int(bool(edge)),
                                                   capi.dptr(out["hit"]), capi.dptr(out["t"]), capi.dptr(out["pts"]),
                                                   capi.dptr(out["frame"]), _stream_arg(stream)), "amk_kfmap_segment_cast")
        return out

    def path_cast(self, path, radius_sq, edge=False, stream=None, out=None):
        """amk_kfmap_path_cast: per scene the first leg of a path float64 [S, n_points >= 2, >= 3] that cannot be passed, over every
        frame the scene's query vector holds; a leg's contact is the least (t, frame, cloud index).
        -> dict(stop [S] i32, leg [S] i32, t [S] f64, free [S] f64, pts [S,3] f32, frame [S] i32)"""
        P, stride = _check_path(path, self.S)
        if out is None:
            out = _path_cast_out(self.S, path.device, "frame")
        capi.check(self.lib.amk_kfmap_path_cast(self.h, capi.dptr(path), stride, P, float(radius_sq), int(bool(edge)),
                                                capi.dptr(out["stop"]), capi.dptr(out["leg"]), capi.dptr(out["t"]), capi.dptr(out["free"]),
                                                capi.dptr(out["pts"]), capi.dptr(out["frame"]), _stream_arg(stream)), "amk_kfmap_path_cast")
        return out

    def nearest_distance(self, queries, stream=None, out=None):
        """amk_kfmap_nearest_distance: FrameKDMap::GetNearestDistance -> float64 [S, Q] (sqrt(DBL_MAX) where no frame answers)."""
        Q, stride = _check_queries(queries, self.S)
        if out is None:
            out = torch.empty((self.S, Q), dtype=torch.float64, device=queries.device)
        capi.check(self.lib.amk_kfmap_nearest_distance(self.h, capi.dptr(queries), stride, Q, capi.dptr(out), _stream_arg(stream)),
                   "amk_kfmap_nearest_distance")
        return out

    def points(self, scene):
        """amk_kfmap_points_host: FrameKDMap::GetPtCloud for one scene -> (xyz float32 [n, 3] in query-vector order, frame_sizes int32 [F],
        -1 behind the scene's last frame) (synchronises)"""
        sz = np.zeros(self.F, np.int32); n = C.c_longlong(0)
        capi.check(self.lib.amk_kfmap_points_host(self.h, int(scene), None, 0, sz.ctypes.data_as(C.c_void_p), C.byref(n)),
                   "amk_kfmap_points_host")   # the size probe
        xyz = np.zeros((n.value, 3), np.float32)
        if n.value:
            capi.check(self.lib.amk_kfmap_points_host(self.h, int(scene), xyz.ctypes.data_as(C.c_void_p), n.value, sz.ctypes.data_as(C.c_void_p),
                                                      C.byref(n)), "amk_kfmap_points_host")
        return xyz, sz

    def state(self):
        """-> dict(n_keyframes [S], n_query_frames [S], last_outliers [S], frame_sizes [S, F]) (synchronises)"""
        nk = np.zeros(self.S, np.int32); nq = np.zeros(self.S, np.int32); out = np.zeros(self.S, np.int32)
        sz = np.zeros((self.S, self.F), np.int32)
        capi.check(self.lib.amk_kfmap_state_host(self.h, nk.ctypes.data_as(C.c_void_p), nq.ctypes.data_as(C.c_void_p),
                                                 out.ctypes.data_as(C.c_void_p), sz.ctypes.data_as(C.c_void_p)), "amk_kfmap_state_host")
        return dict(n_keyframes=nk, n_query_frames=nq, last_outliers=out, frame_sizes=sz)

    def set_tie_order(self, mode):
        """amk_kfmap_set_tie_order: capi.AMK_TIES_LOWEST_INDEX (default) or capi.AMK_TIES_NANOFLANN, before the map's first frame."""
        capi.check(self.lib.amk_kfmap_set_tie_order(self.h, int(mode)), "amk_kfmap_set_tie_order")

    def exact_status(self):
        """amk_kfmap_exact_status_host -> dict(obs [S, F], edge [S, F]) int32: amk_kd_exact_status's codes per query frame,
        capi.AMK_EXACT_OFF for an absent frame or a map in the default mode (synchronises)"""
        obs = np.zeros((self.S, self.F), np.int32); edge = np.zeros((self.S, self.F), np.int32)
        capi.check(self.lib.amk_kfmap_exact_status_host(self.h, obs.ctypes.data_as(C.c_void_p), edge.ctypes.data_as(C.c_void_p)),
                   "amk_kfmap_exact_status_host")
        return dict(obs=obs, edge=edge)

    def reset(self, first_scene, n_scenes, stream=None):
        capi.check(self.lib.amk_kfmap_reset(self.h, int(first_scene), int(n_scenes), capi.stream_ptr(stream)), "amk_kfmap_reset")

    def slots(self):
        """Internal (tests): the raw bookkeeping -> dict(cur_slot [S], kf_n [S], kf_slots [S, P], fmap [F, S], need [S]) (synchronises)"""
        S, F = self.S, self.F
        a = dict(cur_slot=np.zeros(S, np.int32), kf_n=np.zeros(S, np.int32), kf_slots=np.zeros((S, F + 1), np.int32),
                 fmap=np.zeros((F, S), np.int32), need=np.zeros(S, np.int32))
        capi.check(self.lib.amk__kfmap_slots_host(self.h, *[a[k].ctypes.data_as(C.c_void_p) for k in ("cur_slot", "kf_n", "kf_slots", "fmap", "need")]),
                   "amk__kfmap_slots_host")
        return a


class Pipeline:
    """amk_pipeline: n_slots launches in flight, each slot = {HIP stream, obstacle + edge index, MPC batch, outputs};
    gang = frames (of n_scenes scenes) that share one set of launches -- the slot's handles then hold gang * n_scenes scenes."""

    def __init__(self, n_slots, n_scenes, max_points, max_edge_points, prm, queue_depth=0, gang=0, farest_point=500.0,
                 slow_down_kp=0.3, slow_down_kd=0.3, iter_time=0.0, use_odom_est=True, depth=None, task="forward", keyframes=None):
        """keyframes: dict(max_frame_count, th_dist, th_count, depth_min[, Tbc]) -> every slot keeps a keyframe map (amk_kfmap)."""
        self.lib = capi.load()
        task = capi.TaskParams(float(prm.decay), float(iter_time), float(farest_point), float(prm.height), float(slow_down_kp),
                               float(slow_down_kd), float(prm.a_max_xy), float(prm.a_max_z), int(bool(use_odom_est)),
                               {"forward": 0, "global_goal": 1}[task])
        cfg = capi.PipelineConfig(int(n_slots), int(n_scenes), int(max_points), int(max_edge_points), float(prm.T), float(prm.dt),
                                  int(prm.K), int(queue_depth), int(gang),
                                  capi.StepParams(float(prm.speed), float(prm.safety_distance), int(prm.max_iter), 0), task,
                                  depth if depth is not None else capi.DepthParams(),
                                  self._kfmap_params(keyframes))
        h = C.c_void_p()
        capi.check(self.lib.amk_pipeline_create(C.byref(cfg), C.byref(h)), "amk_pipeline_create")
        self.h, self.n_slots, self.S, self.prm = h, int(n_slots), int(n_scenes), prm
        self.N = self.lib.amk_mpc_horizon(self.lib.amk_pipeline_mpc(h, 0))
        self.gang = self.lib.amk_pipeline_gang(h)
        self._events = []
        self._max_points = (int(max_points), int(max_edge_points))
        hs = n_scenes * self.gang   # scenes of a slot's handles
        self._mpc = [MpcBatch(prm.T, prm.dt, prm.K, hs, handle=self.lib.amk_pipeline_mpc(h, i)) for i in range(n_slots)]
        self._kd = [(KdBatch(hs, max_points, handle=self.lib.amk_pipeline_kd(h, i, 0)),
                     KdBatch(hs, max_edge_points, handle=self.lib.amk_pipeline_kd(h, i, 1))) for i in range(n_slots)]
        for m in self._mpc:
            m.configure(prm)

    @staticmethod
    def _kfmap_params(keyframes):
        """amk_kfmap_params of the configuration; keyframes["Tbc"] (4 x 4, optional) is mParamTbc -- absent: the depth configuration's."""
        if not keyframes:
            return capi.KfmapParams()
        kp = capi.KfmapParams(int(keyframes["max_frame_count"]), int(keyframes["th_count"]), float(keyframes["th_dist"]),
                              float(keyframes["depth_min"]))
        if keyframes.get("Tbc") is not None:
            T = np.asarray(keyframes["Tbc"], np.float64).reshape(16)
            for i in range(16):
                kp.Tbc[i] = float(T[i])
        return kp

    def kfmap_state(self, slot):
        """State of the slot's keyframe map (amk_kfmap_state_host): dict(n_keyframes, n_query_frames, last_outliers, frame_sizes)."""
        h = self.lib.amk_pipeline_kfmap(self.h, int(slot))
        assert h, "the pipeline was created without keyframes"
        S = self.S * self.gang
        F = self.lib.amk_kfmap_frames(h)
        nk = np.zeros(S, np.int32); nq = np.zeros(S, np.int32); out = np.zeros(S, np.int32); sz = np.zeros((S, F), np.int32)
        capi.check(self.lib.amk_kfmap_state_host(h, nk.ctypes.data_as(C.c_void_p), nq.ctypes.data_as(C.c_void_p),
                                                 out.ctypes.data_as(C.c_void_p), sz.ctypes.data_as(C.c_void_p)), "amk_kfmap_state_host")
        return dict(n_keyframes=nk, n_query_frames=nq, last_outliers=out, frame_sizes=sz)

    def kfmap(self, slot):
        """The slot's keyframe map as a KfMap that borrows the handle (amk_pipeline_kfmap)."""
        h = self.lib.amk_pipeline_kfmap(self.h, int(slot))
        assert h, "the pipeline was created without keyframes"
        return KfMap(0, self._max_points[0], self._max_points[1], 0, 0, 0, 0, None, handle=h)

    def kfmap_query(self, slot, queries, k=None, cam=None, edge=False, after_wait=False):
        """QueryNearest (k given) or GetNearestDistance (k None) on the slot's keyframe map, over its gang x n_scenes scenes.
        Enqueued on the SLOT's stream, behind every launch the slot has been given so far (frames staged in an open gang are not in the
        map yet: wait() first); torch's current stream is ordered on both sides -- the slot reads `queries` after the work queued on it
        so far, and work queued on it afterwards sees the results.  after_wait=True: the caller has waited for the slot (wait / drain)
        and the query runs on torch's current stream instead.  The slot's next launch must not overlap the query: order the next
        submit's input_ready behind it (the default order_after_current_stream does)."""
        m = self.kfmap(slot)
        Q = int(queries.shape[1])   # (the outputs belong to torch's current stream, which waits for the slot below before it reuses them)
        out = torch.empty((m.S, Q), dtype=torch.float64, device=queries.device) if k is None else _query_out(m.S, Q, int(k), queries.device)
        run = (lambda st: m.nearest_distance(queries, stream=st, out=out)) if k is None else \
              (lambda st: m.query_nearest(queries, k, cam=cam, edge=edge, stream=st, out=out))
        if after_wait:
            return run(None)
        raw = self.lib.amk_pipeline_stream(self.h, int(slot))
        ext = torch.cuda.ExternalStream(int(raw))
        ext.wait_stream(torch.cuda.current_stream())
        run(int(raw))
        torch.cuda.current_stream().wait_stream(ext)
        return out

    def kfmap_points(self, slot, scene):
        """GetPtCloud of one scene of the slot's keyframe map (synchronises the device) -> (xyz [n, 3], frame_sizes [F])."""
        return self.kfmap(slot).points(scene)

    def queue_mode(self, slot):
        """amk_pipeline_queue_mode: how the slot's stream was really created (capi.AMK_QUEUES_POOLED / _PRIORITY)."""
        return self.lib.amk_pipeline_queue_mode(self.h, int(slot))

    def mpc(self, slot):
        return self._mpc[slot]

    def kd(self, slot, which):
        return self._kd[slot][which]

    def close(self):
        if getattr(self, "h", None):
            self.lib.amk_pipeline_destroy(self.h)
            self.h = None

    __del__ = close

    def submit(self, clouds, edges, state_quad=None, pos_x=None, ref_path_init=None, cloud_counts=None, edge_counts=None, u_out=None,
               keep_warm_start=False, order_after_current_stream=True, odom=None, odom_age=0.0, cmd_out=None, depth=None, Twb=None,
               keyframes=None, Twc_cur=None, cam=None, global_goal=None):
        """One fresh frame + control step on the next slot; returns its ticket at once (blocks only when that slot's queue
        is full).  ticket % n_slots = slot; with a gang the frame is staged until the gang is full (or wait / drain).
        All tensors are device tensors that must stay alive until the frame finished.  A slot runs on its own stream: by default
        an event recorded on torch's current stream is handed over (amk_pipeline_frame.input_ready) so that the slot reads the
        inputs only after the work queued on that stream so far -- like every other entry point of this module, which run ON the
        current stream.  order_after_current_stream=False: the caller guarantees the inputs are complete (bench.py: frames made
        once, synchronised).
        TASK mode: odom float64 [S, 10] = [mPos, yaw, mVel, mAcc] instead of state_quad / pos_x; the slot then runs GetInitPath on
        its own mRefPath (ref_path_init, when given, re-initialises it first), the clock model, the step and PubCmd /
        PubSlowDownCmd (cmd_out float64 [S, 3])."""
        opt = lambda t: t.data_ptr() if t is not None else None
        dinfo = (None, 0, 0, 0, 0, None)
        if depth is not None:   # a frame that starts at the raw depth image: depth [S, rows, cols] uint16 / int16 / float32, Twb [S, 4, 4]
            assert depth.dim() == 3 and depth.is_contiguous() and Twb.dtype == torch.float64 and Twb.is_contiguous()
            kind = capi.AMK_DEPTH_F32 if depth.dtype == torch.float32 else capi.AMK_DEPTH_U16
            dinfo = (depth.data_ptr(), kind, int(depth.shape[1]), int(depth.shape[2]), 0, Twb.data_ptr())
        else:
            assert clouds.dtype == torch.float32 and edges.dtype == torch.float32 and clouds.shape[2] == edges.shape[2]
        self._kf_keep = (None, None, cam)
        kinfo = (None, None, 0, 0, opt(Twc_cur), C.cast(C.pointer(cam), C.c_void_p) if cam is not None else None)
        if keyframes:   # [(KdBatch obstacle, KdBatch edge), ...]: the multi-frame map [this frame, keyframes ...] (gang 1 only)
            ko = (C.c_void_p * len(keyframes))(*[k[0].h for k in keyframes]); ke = (C.c_void_p * len(keyframes))(*[k[1].h for k in keyframes])
            self._kf_keep = (ko, ke, cam)
            kinfo = (C.cast(ko, C.c_void_p), C.cast(ke, C.c_void_p), len(keyframes), 0) + kinfo[4:]
        ev_ptr = None
        if order_after_current_stream:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            ev_ptr = ev.cuda_event
            self._events.append(ev)                      # alive until the frame has been launched: keep the newest ones
            if len(self._events) > 4 * self.n_slots * self.gang + 8:
                del self._events[:len(self._events) // 2]
        fr = capi.PipelineFrame(opt(clouds), opt(cloud_counts), opt(edges), opt(edge_counts),
                                int(clouds.shape[2]) if clouds is not None else 3, int(bool(keep_warm_start)), opt(state_quad), opt(pos_x),
                                opt(ref_path_init), opt(u_out), opt(odom), float(odom_age), opt(cmd_out), *dinfo, *kinfo, ev_ptr,
                                opt(global_goal))
        slot = C.c_int(-1)
        capi.check(self.lib.amk_pipeline_submit(self.h, C.byref(fr), C.byref(slot)), "amk_pipeline_submit")
        return slot.value

    def wait_stream(self, ticket, stream=None):
        """Device-side wait (amk_pipeline_wait_stream): work queued on `stream` (default: torch's current stream) after this call
        runs after the frame's step; the host does not block."""
        capi.check(self.lib.amk_pipeline_wait_stream(self.h, int(ticket), capi.stream_ptr(stream)), "amk_pipeline_wait_stream")

    def output_tensors(self, ticket):
        """The frame's results as torch tensors ALIASING the slot's buffers (no copy, no synchronisation): valid to read on a
        stream that waited for the frame (wait / wait_stream) until the slot's next launch overwrites them.
        -> dict(u [S,4], x0array [S,N,14], flags [S,4] int32, ref_path [S,N,10])"""
        ptr = [C.c_void_p() for _ in range(4)]
        capi.check(self.lib.amk_pipeline_outputs(self.h, int(ticket), *[C.byref(p) for p in ptr]), "amk_pipeline_outputs")
        S, N = self.S, self.N
        return dict(u=capi.tensor_from_ptr(ptr[0].value, (S, 4), torch.float64), x0array=capi.tensor_from_ptr(ptr[1].value, (S, N, 14), torch.float64),
                    flags=capi.tensor_from_ptr(ptr[2].value, (S, 4), torch.int32), ref_path=capi.tensor_from_ptr(ptr[3].value, (S, N, 10), torch.float64))

    def set_path_audit(self, mode, radius, n_legs=0):
        """amk_pipeline_set_path_audit: the trajectory audit between the step and the command -- mode capi.AMK_AUDIT_OFF / _REPORT /
        _SLOW_DOWN, radius in metres, n_legs 0 = all N - 1.  Only while nothing is staged or in flight (before the first submit,
        after drain)."""
        capi.check(self.lib.amk_pipeline_set_path_audit(self.h, int(mode), float(radius), int(n_legs)), "amk_pipeline_set_path_audit")

    def audit_outputs(self, ticket):
        """Host copies of the frame's audit answers (after wait): dict(stop [S], leg [S], t [S], free [S], pts [S,3], src [S]);
        src is the cloud index of the point touched, the frame for a slot with a keyframe map."""
        ptr = [C.c_void_p() for _ in range(6)]
        capi.check(self.lib.amk_pipeline_audit_outputs(self.h, int(ticket), *[C.byref(p) for p in ptr]), "amk_pipeline_audit_outputs")
        S = self.S
        shapes = [("stop", (S,), np.int32), ("leg", (S,), np.int32), ("t", (S,), np.float64), ("free", (S,), np.float64),
                  ("pts", (S, 3), np.float32), ("src", (S,), np.int32)]
        out = {}
        for p, (name, shp, dt) in zip(ptr, shapes):
            a = np.empty(shp, dt)
            capi.check_hip(capi.hip_memcpy_dtoh(a, p.value), name)
            out[name] = a
        return out

    def wait(self, ticket):
        capi.check(self.lib.amk_pipeline_wait(self.h, int(ticket)), "amk_pipeline_wait")

    def drain(self):
        capi.check(self.lib.amk_pipeline_drain(self.h), "amk_pipeline_drain")

    def outputs(self, ticket):
        """Host copies of the frame's results (after wait): dict(u [S,4], x0array [S,N,14], flags [S,4], ref_path [S,N,10])."""
        ptr = [C.c_void_p() for _ in range(4)]
        capi.check(self.lib.amk_pipeline_outputs(self.h, int(ticket), *[C.byref(p) for p in ptr]), "amk_pipeline_outputs")
        S, N = self.S, self.N
        shapes = [((S, 4), np.float64), ((S, N, 14), np.float64), ((S, 4), np.int32), ((S, N, 10), np.float64)]
        out = {}
        for name, p, (shp, dt) in zip(("u", "x0array", "flags", "ref_path"), ptr, shapes):
            a = np.empty(shp, dt)
            capi.check_hip(capi.hip_memcpy_dtoh(a, p.value), name)
            out[name] = a
        return out


class Shard:
    """amk_shard: one process per GPU, RCCL bound by the library (ncclCommInitRank / ncclAllGather / ncclAllReduce)."""

    def __init__(self, rank, world, unique_id):
        self.lib = capi.load()
        h = C.c_void_p()
        capi.check(self.lib.amk_shard_create(unique_id, int(rank), int(world), C.byref(h)), "amk_shard_create")
        self.h, self.rank, self.world = h, int(rank), int(world)

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        capi.check(capi.load().amk_shard_unique_id(buf), "amk_shard_unique_id")
        return buf.raw

    def gather(self, local, out, stream=None):
        """out[r * n : (r + 1) * n] = rank r's `local` (float64 device tensors, n = local.numel())."""
        assert local.dtype == torch.float64 and out.dtype == torch.float64 and out.numel() == local.numel() * self.world
        capi.check(self.lib.amk_shard_gather(self.h, capi.dptr(local), int(local.numel()), capi.dptr(out),
                                             capi.stream_ptr(stream)), "amk_shard_gather")
        return out

    def max(self, values, stream=None):
        capi.check(self.lib.amk_shard_max(self.h, capi.dptr(values), int(values.numel()), capi.stream_ptr(stream)), "amk_shard_max")
        return values

    def wait(self, stream=None, timeout_s=120.0):
        """amk_shard_wait: the watchdog of the exchange step -- returns capi.AMK_OK or capi.AMK_ERR_TIMEOUT (a hung collective)."""
        return self.lib.amk_shard_wait(self.h, capi.stream_ptr(stream), float(timeout_s))

    @staticmethod
    def rccl_info():
        """-> dict(path, version, was_loaded) of the RCCL the library bound, or None when no librccl can be loaded."""
        buf = C.create_string_buffer(1024); ver = C.c_int(0); was = C.c_int(0)
        if capi.load().amk_shard_rccl_info(buf, 1024, C.byref(ver), C.byref(was)) != capi.AMK_OK:
            return None
        return dict(path=buf.value.decode(), version=ver.value, loaded_before_amk=bool(was.value))

    def close(self):
        if getattr(self, "h", None):
            self.lib.amk_shard_destroy(self.h)
            self.h = None

    __del__ = close


def step_batch(kd_obstacle, kd_edge, mpc, prm, state_quad, pos_x, ref_path, stream=None, out=None):
    """One control step for every scene (amk_step_batch).  ref_path is updated in place."""
    S, N = mpc.S, mpc.N
    assert state_quad.dtype == torch.float64 and tuple(state_quad.shape) == (S, prm.max_iter, 10)
    assert ref_path.dtype == torch.float64 and tuple(ref_path.shape) == (S, N, 10)
    assert pos_x.dtype == torch.float64 and pos_x.numel() == S
    dev = ref_path.device
    if out is None:
        out = dict(u=torch.empty((S, 4), dtype=torch.float64, device=dev),
                   x0array=torch.empty((S, N, 14), dtype=torch.float64, device=dev),
                   flags=torch.empty((S, 4), dtype=torch.int32, device=dev))
    sp = capi.StepParams(float(prm.speed), float(prm.safety_distance), int(prm.max_iter), 0)
    capi.check(capi.load().amk_step_batch(kd_obstacle.h, kd_edge.h, mpc.h, C.byref(sp), capi.dptr(state_quad),
                                          capi.dptr(pos_x), capi.dptr(ref_path), capi.dptr(out["u"]),
                                          capi.dptr(out["x0array"]), capi.dptr(out["flags"]),
                                          capi.stream_ptr(stream)), "amk_step_batch")
    return out


def step_batch_frames(kd_obstacle_frames, kd_edge_frames, mpc, prm, state_quad, pos_x, ref_path, Twc=None, cam=None,
                      stream=None, out=None):
    """amk_step_batch_frames: the control step over a multi-frame map.  kd_*_frames: lists of KdBatch, index 0 = current
    frame; Twc float64 [S, 4, 4] (or None); cam: capi.FrameCamera."""
    S, N = mpc.S, mpc.N
    F = len(kd_obstacle_frames)
    assert F == len(kd_edge_frames) and F >= 1
    dev = ref_path.device
    if out is None:
        out = dict(u=torch.empty((S, 4), dtype=torch.float64, device=dev),
                   x0array=torch.empty((S, N, 14), dtype=torch.float64, device=dev),
                   flags=torch.empty((S, 4), dtype=torch.int32, device=dev))
    sp = capi.StepParams(float(prm.speed), float(prm.safety_distance), int(prm.max_iter), 0)
    oa = (C.c_void_p * F)(*[k.h for k in kd_obstacle_frames]); ea = (C.c_void_p * F)(*[k.h for k in kd_edge_frames])
    capi.check(capi.load().amk_step_batch_frames(oa, ea, F, capi.dptr(Twc), C.byref(cam) if cam is not None else None, mpc.h,
                                                 C.byref(sp), capi.dptr(state_quad), capi.dptr(pos_x), capi.dptr(ref_path),
                                                 capi.dptr(out["u"]), capi.dptr(out["x0array"]), capi.dptr(out["flags"]),
                                                 capi.stream_ptr(stream)), "amk_step_batch_frames")
    return out


def depth_params(pixel2meter=1.0, depth_min=0.1, depth_max=100.0, resize_scale=10.0, fx=320.0, fy=320.0, cx=320.0,
                 cy=240.0, Tbc=None):
    """amk_depth_params with the defaults of AM/config/mpc_parameters.yaml:59-66."""
    p = capi.DepthParams(float(pixel2meter), float(depth_min), float(depth_max), float(resize_scale), float(fx),
                         float(fy), float(cx), float(cy))
    T = np.eye(4) if Tbc is None else np.asarray(Tbc, np.float64).reshape(4, 4)
    for i in range(16):
        p.Tbc[i] = float(T.flat[i])
    return p


def _depth_batch(depth, params, poses):
    """What depth_to_cloud and depth_to_clouds start with: the checked shapes of a batch and the library's answer about its
    down-scaled size -> (lib, S, rows, cols, capacity of a cloud in points, AMK_DEPTH_* of the pixels)."""
    assert depth.dim() == 3 and depth.dtype in (torch.uint16, torch.int16, torch.float32) and depth.is_contiguous()
    S, rows, cols = (int(v) for v in depth.shape)
    for T in poses:
        assert T.dtype == torch.float64 and tuple(T.shape) == (S, 4, 4) and T.is_contiguous()
    lib = capi.load()
    w, h = C.c_int(), C.c_int()
    capi.check(lib.amk_depth_out_size(rows, cols, params.resize_scale, C.byref(w), C.byref(h)), "amk_depth_out_size")
    return lib, S, rows, cols, w.value * h.value, capi.AMK_DEPTH_F32 if depth.dtype == torch.float32 else capi.AMK_DEPTH_U16


def depth_to_cloud(depth, params, Twb, point_stride=3, stream=None, edge=False):
    """FrameKDMap::ProcessDepth (edge=True: FrameKDMap::BuildEdgeCloud, Twb then = mCurFrame.Twc) for a batch: depth [S, rows, cols] uint16 / float32 device tensor, Twb [S, 4, 4]
    float64 -> (cloud float32 [S, W*H, point_stride], counts int32 [S]); the cloud feeds KdBatch.build(cloud, counts)."""
    lib, S, rows, cols, cap, kind = _depth_batch(depth, params, (Twb,))
    cloud = torch.zeros((S, cap, point_stride), dtype=torch.float32, device=depth.device)
    counts = torch.empty(S, dtype=torch.int32, device=depth.device)
    fn = lib.amk_depth_to_edge_cloud if edge else lib.amk_depth_to_cloud
    capi.check(fn(capi.dptr(depth), kind, rows, cols, rows * cols, S, C.byref(params), capi.dptr(Twb), capi.dptr(cloud),
                  int(point_stride), cap * point_stride, capi.dptr(counts), capi.stream_ptr(stream)),
               "amk_depth_to_edge_cloud" if edge else "amk_depth_to_cloud")
    return cloud, counts


def depth_to_clouds(depth, params, Twb, Twc, point_stride=3, stream=None):
    """AddVertex's image half for a batch, FrameKDMap::ProcessDepth followed by FrameKDMap::BuildEdgeCloud, in one call and for
    down-scaled images of any size (amk_depth_to_clouds): depth [S, rows, cols] uint16 / float32 device tensor, Twb and Twc
    (mCurFrame.Twc: the previous frame's Twb * Tbc) [S, 4, 4] float64 -> (cloud, counts, edge, edge_counts), clouds float32
    [S, W*H, point_stride] of which the first counts[s] points of a scene are written, counts int32 [S]."""
    lib, S, rows, cols, cap, kind = _depth_batch(depth, params, (Twb, Twc))
    nbytes = C.c_longlong()
    capi.check(lib.amk_depth_clouds_work_bytes(rows, cols, params.resize_scale, S, C.byref(nbytes)), "amk_depth_clouds_work_bytes")
    cloud = torch.zeros((S, cap, point_stride), dtype=torch.float32, device=depth.device)
    edge = torch.zeros((S, cap, point_stride), dtype=torch.float32, device=depth.device)
    counts = torch.empty(S, dtype=torch.int32, device=depth.device)
    edge_counts = torch.empty(S, dtype=torch.int32, device=depth.device)
    work = torch.empty((nbytes.value + 7) // 8, dtype=torch.int64, device=depth.device)
    if stream is not None:
        work.record_stream(stream)   # dropped at return: its memory must not be reused before the launches on `stream` are through
    capi.check(lib.amk_depth_to_clouds(capi.dptr(depth), kind, rows, cols, rows * cols, S, C.byref(params), capi.dptr(Twb), capi.dptr(Twc),
                                       capi.dptr(cloud), cap * point_stride, capi.dptr(counts), capi.dptr(edge), cap * point_stride,
                                       capi.dptr(edge_counts), int(point_stride), capi.dptr(work), work.numel() * 8,
                                       capi.stream_ptr(stream)), "amk_depth_to_clouds")
    return cloud, counts, edge, edge_counts


def sim_render_depth(cyl, Twb, params, rows, cols, counts=None, z_top=4.0, max_range=60.0, dtype=torch.uint16, out=None, stream=None):
    """amk_sim_render_depth: the depth frames a camera at Twb * params.Tbc sees in worlds of vertical cylinders on the ground plane.
    cyl float64 [S, max_cyl, 3] = (cx, cy, r), counts int32 [S] or None (max_cyl in every scene), Twb float64 [S, 4, 4]
    -> depth [S, rows, cols] of `dtype` (torch.uint16 / int16: AMK_DEPTH_U16, torch.float32: AMK_DEPTH_F32), 0 = no return; it feeds
    depth_to_clouds and Pipeline.submit(depth=...).  dtype torch.float64 is the test-only fp64 ray parameter (amk__sim_render_t).
    Stream-ordered on torch's current stream (or `stream`); `out` re-uses a buffer."""
    assert cyl.dtype == torch.float64 and cyl.dim() == 3 and cyl.shape[2] == 3 and cyl.is_contiguous()
    S, max_cyl = int(cyl.shape[0]), int(cyl.shape[1])
    assert Twb.dtype == torch.float64 and tuple(Twb.shape) == (S, 4, 4) and Twb.is_contiguous()
    assert counts is None or (counts.dtype == torch.int32 and tuple(counts.shape) == (S,) and counts.is_contiguous())
    if out is None:
        out = torch.empty((S, int(rows), int(cols)), dtype=dtype, device=Twb.device)
    assert tuple(out.shape) == (S, int(rows), int(cols)) and out.is_contiguous()
    lib = capi.load()
    head = (capi.dptr(cyl) if max_cyl else None, capi.dptr(counts), max_cyl, S, float(z_top), float(max_range), C.byref(params), int(rows),
            int(cols), capi.dptr(Twb), capi.dptr(out))
    if out.dtype == torch.float64:
        capi.check(lib.amk__sim_render_t(*head, capi.stream_ptr(stream)), "amk__sim_render_t")
    else:
        kind = capi.AMK_DEPTH_F32 if out.dtype == torch.float32 else capi.AMK_DEPTH_U16
        assert kind == capi.AMK_DEPTH_F32 or out.dtype in (torch.uint16, torch.int16)
        capi.check(lib.amk_sim_render_depth(*head, kind, capi.stream_ptr(stream)), "amk_sim_render_depth")
    return out


def sim_vehicle_step(ABc, cmd, x, Twb=None, pose_quantum=0.0, stream=None):
    """amk_sim_vehicle_step: x <- A x + B (cmd, 0) + c in place for every scene, and Twb = [Rz(yaw) | rint(p q) / q] of the new state.
    ABc: numpy float64 [150] on the HOST (A [10][10], B [10][4], c [10]; plant_model() makes it), cmd float64 [S, 3], x float64 [S, 10]
    (the layout of Pipeline.submit's odom), Twb float64 [S, 4, 4] or None; pose_quantum 1e6 rounds the pose to a micrometre."""
    ABc = np.ascontiguousarray(ABc, np.float64).reshape(-1)
    assert ABc.size == 150
    S = int(x.shape[0])
    assert x.dtype == torch.float64 and tuple(x.shape) == (S, 10) and cmd.dtype == torch.float64 and tuple(cmd.shape) == (S, 3)
    assert Twb is None or (Twb.dtype == torch.float64 and tuple(Twb.shape) == (S, 4, 4))
    capi.check(capi.load().amk_sim_vehicle_step(ABc.ctypes.data_as(C.c_void_p), capi.dptr(cmd), capi.dptr(x), capi.dptr(Twb), S,
                                                float(pose_quantum), capi.stream_ptr(stream)), "amk_sim_vehicle_step")
    return x


def sim_render_world(cyl, box, Twb, params, rows, cols, cyl_counts=None, box_counts=None, z_top=4.0, max_range=60.0, dtype=torch.uint16,
                     out=None, stream=None):
    """amk_sim_render_world: sim_render_depth in worlds that also hold boxes.  cyl float64 [S, max_cyl, 3], box float64 [S, max_box, 8]
    = (cx, cy, hx, hy, c, s, z0, z1), cyl_counts / box_counts int32 [S] or None (the maximum in every scene), Twb float64 [S, 4, 4]
    -> depth [S, rows, cols] of `dtype`, as sim_render_depth; dtype torch.float64 is the test-only fp64 ray parameter
    (amk__sim_render_world_t).  Stream-ordered on torch's current stream (or `stream`); `out` re-uses a buffer."""
    assert cyl.dtype == torch.float64 and cyl.dim() == 3 and cyl.shape[2] == 3 and cyl.is_contiguous()
    S, max_cyl, max_box = int(cyl.shape[0]), int(cyl.shape[1]), int(box.shape[1])
    assert box.dtype == torch.float64 and tuple(box.shape) == (S, max_box, 8) and box.is_contiguous()
    assert Twb.dtype == torch.float64 and tuple(Twb.shape) == (S, 4, 4) and Twb.is_contiguous()
    for counts in (cyl_counts, box_counts):
        assert counts is None or (counts.dtype == torch.int32 and tuple(counts.shape) == (S,) and counts.is_contiguous())
    if out is None:
        out = torch.empty((S, int(rows), int(cols)), dtype=dtype, device=Twb.device)
    assert tuple(out.shape) == (S, int(rows), int(cols)) and out.is_contiguous()
    lib = capi.load()
    head = (capi.dptr(cyl) if max_cyl else None, capi.dptr(cyl_counts), max_cyl, capi.dptr(box) if max_box else None, capi.dptr(box_counts),
            max_box, S, float(z_top), float(max_range), C.byref(params), int(rows), int(cols), capi.dptr(Twb), capi.dptr(out))
    if out.dtype == torch.float64:
        capi.check(lib.amk__sim_render_world_t(*head, capi.stream_ptr(stream)), "amk__sim_render_world_t")
    else:
        kind = capi.AMK_DEPTH_F32 if out.dtype == torch.float32 else capi.AMK_DEPTH_U16
        assert kind == capi.AMK_DEPTH_F32 or out.dtype in (torch.uint16, torch.int16)
        capi.check(lib.amk_sim_render_world(*head, kind, capi.stream_ptr(stream)), "amk_sim_render_world")
    return out


def sim_noise_params(params=None, **fields):
    """amk_sim_noise_params from flight.noise_params' fields (a dict, an object with those attributes, or keywords); everything
    not given is off."""
    from . import flight
    p = flight.noise_params(params, **fields)
    return capi.SimNoiseParams(int(p.seed), *[float(getattr(p, name)) for name in flight.NOISE_FIELDS[1:]])


def sim_depth_noise(depth, params, pixel2meter, frame, scene_id0=0, out=None, stream=None):
    """amk_sim_depth_noise: the frames a depth camera makes of perfect ones -- missing returns and flying pixels at depth
    discontinuities, dropouts, axial noise, disparity steps, the sensor's range -- every draw a pure function of (params.seed,
    scene_id0 + s, frame, pixel).  depth [S, rows, cols] uint16 / int16 / float32 device tensor (sim_render_world's) -> a tensor of the
    same shape and dtype, never `depth` itself; it feeds depth_to_clouds and Pipeline.submit(depth=...).  params: capi.SimNoiseParams,
    or what sim_noise_params takes.  Stream-ordered on torch's current stream (or `stream`); `out` re-uses a buffer."""
    assert depth.dim() == 3 and depth.dtype in (torch.uint16, torch.int16, torch.float32) and depth.is_contiguous()
    S, rows, cols = (int(v) for v in depth.shape)
    if out is None:
        out = torch.empty_like(depth)
    assert tuple(out.shape) == (S, rows, cols) and out.is_contiguous() and out.dtype == depth.dtype
    if not isinstance(params, capi.SimNoiseParams):
        params = sim_noise_params(params)
    kind = capi.AMK_DEPTH_F32 if depth.dtype == torch.float32 else capi.AMK_DEPTH_U16
    capi.check(capi.load().amk_sim_depth_noise(capi.dptr(depth), capi.dptr(out), kind, rows, cols, rows * cols, S, float(pixel2meter),
                                               C.byref(params), int(scene_id0), int(frame), capi.stream_ptr(stream)), "amk_sim_depth_noise")
    return out


def sim_vehicle_step_att(ABc, cmd, x, Twb=None, pose_quantum=0.0, attitude=capi.AMK_SIM_ATT_ACCEL, gz=9.81, stream=None):
    """amk_sim_vehicle_step_att: sim_vehicle_step, with Twb's rotation chosen by `attitude`: capi.AMK_SIM_ATT_YAW is sim_vehicle_step
    bit for bit, capi.AMK_SIM_ATT_ACCEL tilts the vehicle into its thrust a + (0, 0, gz) (acc2rotmat on the new state)."""
    ABc = np.ascontiguousarray(ABc, np.float64).reshape(-1)
    assert ABc.size == 150
    S = int(x.shape[0])
    assert x.dtype == torch.float64 and tuple(x.shape) == (S, 10) and cmd.dtype == torch.float64 and tuple(cmd.shape) == (S, 3)
    assert Twb is None or (Twb.dtype == torch.float64 and tuple(Twb.shape) == (S, 4, 4))
    capi.check(capi.load().amk_sim_vehicle_step_att(ABc.ctypes.data_as(C.c_void_p), capi.dptr(cmd), capi.dptr(x), capi.dptr(Twb), S,
                                                    float(pose_quantum), int(attitude), float(gz), capi.stream_ptr(stream)),
               "amk_sim_vehicle_step_att")
    return x


def sim_body_params(con_dt=None, params=None, **fields):
    """amk_sim_body_params from flight.body_params' fields (a dict, an object with those attributes, or keywords) for a control period of
    con_dt seconds; what is not given takes flight.body_params' defaults.  con_dt may be None when `h` is given."""
    from . import flight
    if con_dt is None:
        assert "h" in fields or (params is not None and (("h" in params) if isinstance(params, dict) else hasattr(params, "h")))
        con_dt = 0.0
    p = flight.body_params(con_dt, params, **fields)
    return capi.SimBodyParams(float(p.h), int(p.n_sub), float(p.gz), float(p.k_att), float(p.rate_max), float(p.k_rate), float(p.k_thrust),
                              float(p.f_min), float(p.f_max), (C.c_double * 3)(*p.drag), float(p.yaw_cs), float(p.yaw_sn), int(p.cog_window),
                              (C.c_double * capi.AMK_SIM_COG_MAX)(*[float(v) for v in p.cog_weight]))


def sim_body_reset(body, gz=9.81, stream=None):
    """amk_sim_body_reset: body float64 [S, 64] <- level, at rest, hovering (f = gz), an empty IMU window (flight.body_state0)."""
    S = int(body.shape[0])
    assert body.dtype == torch.float64 and tuple(body.shape) == (S, capi.AMK_SIM_BODY_DOUBLES) and body.is_contiguous()
    capi.check(capi.load().amk_sim_body_reset(capi.dptr(body), S, float(gz), capi.stream_ptr(stream)), "amk_sim_body_reset")
    return body


def sim_vehicle_step_body(params, cmd, x, body, Twb=None, pose_quantum=0.0, stream=None):
    """amk_sim_vehicle_step_body: the rigid-body vehicle over one control period, in place -- cmd float64 [S, 3] (a thrust acceleration,
    gravity inside), x float64 [S, 10] (p and v advance, x[:, 7:10] becomes the filtered IMU acceleration, the yaw is not written),
    body float64 [S, 64] the hidden state (sim_body_reset), Twb float64 [S, 4, 4] or None <- [R | rint(p q) / q].  params:
    capi.SimBodyParams, or what sim_body_params takes as `params` (then `h` must be among it).  Stream-ordered."""
    S = int(x.shape[0])
    assert x.dtype == torch.float64 and tuple(x.shape) == (S, 10) and cmd.dtype == torch.float64 and tuple(cmd.shape) == (S, 3)
    assert body.dtype == torch.float64 and tuple(body.shape) == (S, capi.AMK_SIM_BODY_DOUBLES)
    assert x.is_contiguous() and cmd.is_contiguous() and body.is_contiguous()
    assert Twb is None or (Twb.dtype == torch.float64 and tuple(Twb.shape) == (S, 4, 4) and Twb.is_contiguous())
    if not isinstance(params, capi.SimBodyParams):
        params = sim_body_params(None, params)
    capi.check(capi.load().amk_sim_vehicle_step_body(C.byref(params), capi.dptr(cmd), capi.dptr(x), capi.dptr(body), capi.dptr(Twb), S,
                                                     float(pose_quantum), capi.stream_ptr(stream)), "amk_sim_vehicle_step_body")
    return x


def _sim_world_head(cyl, box, cyl_counts, box_counts, z_top):
    """The leading arguments of the ground-truth queries: amk_sim_render_world's world, checked as sim_render_world checks it"""
    assert cyl.dtype == torch.float64 and cyl.dim() == 3 and cyl.shape[2] == 3 and cyl.is_contiguous()
    S, max_cyl, max_box = int(cyl.shape[0]), int(cyl.shape[1]), int(box.shape[1])
    assert box.dtype == torch.float64 and tuple(box.shape) == (S, max_box, 8) and box.is_contiguous()
    for counts in (cyl_counts, box_counts):
        assert counts is None or (counts.dtype == torch.int32 and tuple(counts.shape) == (S,) and counts.is_contiguous())
    return S, (capi.dptr(cyl) if max_cyl else None, capi.dptr(cyl_counts), max_cyl, capi.dptr(box) if max_box else None,
               capi.dptr(box_counts), max_box, S, float(z_top))


def _sim_points(pts, S):
    assert pts.dtype == torch.float64 and pts.dim() == 3 and pts.shape[0] == S and pts.shape[2] >= 3 and pts.is_contiguous()
    return int(pts.shape[1]), int(pts.shape[2])


def sim_clearance(cyl, box, pts, cyl_counts=None, box_counts=None, z_top=4.0, out=None, stream=None):
    """amk_sim_clearance: the signed distance from every point to the nearest TRUE solid of sim_render_world's world (negative: inside)
    and which solid it is.  pts float64 [S, P, >= 3] (x, y, z lead every row; a [S, 1, 10] view of the odometry goes in as it is)
    -> dict(dist float64 [S, P], kind int32 [S, P] 0 ground / 1 cylinder / 2 box, index int32 [S, P], -1 for the ground).
    Stream-ordered on torch's current stream (or `stream`); `out` re-uses the buffers, an entry None is not written."""
    S, head = _sim_world_head(cyl, box, cyl_counts, box_counts, z_top)
    P, stride = _sim_points(pts, S)
    if out is None:
        out = {"dist": torch.empty((S, P), dtype=torch.float64, device=pts.device),
               "kind": torch.empty((S, P), dtype=torch.int32, device=pts.device), "index": torch.empty((S, P), dtype=torch.int32, device=pts.device)}
    capi.check(capi.load().amk_sim_clearance(*head, capi.dptr(pts), stride, P, capi.dptr(out["dist"]), capi.dptr(out["kind"]),
                                             capi.dptr(out["index"]), capi.stream_ptr(stream)), "amk_sim_clearance")
    return out


def sim_segment_cast(cyl, box, path, radius, cyl_counts=None, box_counts=None, z_top=4.0, out=None, stream=None):
    """amk_sim_segment_cast: per leg of path float64 [S, n_points >= 2, >= 3], the first contact of a sphere of `radius` with the world's
    solids inflated by it -> dict(hit int32 [S, L], t float64 [S, L] (1.0 without contact), kind, index int32 [S, L], -1 / -1 without).
    A leg that starts inside a solid touches it at t = 0."""
    S, head = _sim_world_head(cyl, box, cyl_counts, box_counts, z_top)
    P, stride = _sim_points(path, S)
    L = P - 1
    if out is None:
        i32 = lambda: torch.empty((S, L), dtype=torch.int32, device=path.device)
        out = {"hit": i32(), "t": torch.empty((S, L), dtype=torch.float64, device=path.device), "kind": i32(), "index": i32()}
    capi.check(capi.load().amk_sim_segment_cast(*head, capi.dptr(path), stride, P, float(radius), capi.dptr(out["hit"]), capi.dptr(out["t"]),
                                                capi.dptr(out["kind"]), capi.dptr(out["index"]), capi.stream_ptr(stream)),
               "amk_sim_segment_cast")
    return out


def sim_path_cast_out(S, dev):
    """outputs of sim_path_cast, one result per scene (the layout of KdBatch.path_cast's, pts in float64, kind and index for the id)"""
    i32 = lambda: torch.empty((S,), dtype=torch.int32, device=dev)
    f64 = lambda *shape: torch.empty((S, *shape), dtype=torch.float64, device=dev)
    return {"stop": i32(), "leg": i32(), "t": f64(), "free": f64(), "pts": f64(3), "kind": i32(), "index": i32()}


def sim_path_cast(cyl, box, path, radius, cyl_counts=None, box_counts=None, z_top=4.0, out=None, stream=None):
    """amk_sim_path_cast: ONE verdict per scene for a whole path, laid out like KdBatch.path_cast's: stop [S] 0 free / 1 contact /
    2 unjudgeable leg, leg (-1 when free), t, free (the free distance along the path), pts float64 [S, 3] the sphere's centre at the
    contact, kind / index of the solid touched.  The reduction of sim_segment_cast's per-leg answers, bit for bit.  path must be a
    contiguous [S, n_points, stride] tensor: Pipeline.output_tensors()["x0array"] itself (n_points = N), or a copy of its leading
    n_legs + 1 rows per scene."""
    S, head = _sim_world_head(cyl, box, cyl_counts, box_counts, z_top)
    P, stride = _sim_points(path, S)
    if out is None:
        out = sim_path_cast_out(S, path.device)
    capi.check(capi.load().amk_sim_path_cast(*head, capi.dptr(path), stride, P, float(radius), capi.dptr(out["stop"]), capi.dptr(out["leg"]),
                                             capi.dptr(out["t"]), capi.dptr(out["free"]), capi.dptr(out["pts"]), capi.dptr(out["kind"]),
                                             capi.dptr(out["index"]), capi.stream_ptr(stream)), "amk_sim_path_cast")
    return out


def plant_model(tau, con_dt, drag=(0.0, 0.0, 0.0)):
    """h_ABc of sim_vehicle_step: the MPC's own model at the control period con_dt (the library's host-side amk__mpc_dynamics; no
    device) -> numpy float64 [150] = A [10][10], B [10][4], c [10]."""
    tau4 = np.zeros(4); tau4[:min(4, len(tau))] = np.asarray(tau, np.float64)[:4]   # (tau_yaw, when given, is not in the model)
    tau, drag = tau4, np.ascontiguousarray(drag, np.float64)
    ABc = np.zeros(150)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    capi.check(capi.load().amk__mpc_dynamics(vp(tau), vp(drag), float(con_dt), vp(ABc[:100]), vp(ABc[100:140]), vp(ABc[140:]), None),
               "amk__mpc_dynamics")
    return ABc
