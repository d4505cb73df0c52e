// Internal helpers shared by the HIP translation units of libavoid_mpc_amd.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/avoid_mpc_amd.h"

namespace amk {

extern thread_local int g_last_hip_error;

inline int hip_fail(hipError_t e) {
    g_last_hip_error = (int)e;
    return AMK_ERR_HIP;
}

#define AMK_HIP(expr)                                   \
    do {                                                \
        hipError_t _e = (expr);                         \
        if (_e != hipSuccess) return amk::hip_fail(_e); \
    } while (0)

constexpr int kWave = 64;  // CDNA4 wavefront

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// A device buffer that frees itself (handles own their storage; no allocation on the hot path).
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    hipError_t alloc(size_t count) {
        release();
        n = count;
        if (count == 0) return hipSuccess;
        return hipMalloc((void **)&p, count * sizeof(T));
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    ~DevBuf() { release(); }
};

// value of lane `src` (wave-uniform) broadcast to every lane through scalar registers
__device__ __forceinline__ double readlane_f64(double v, int src) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, src);
    hi = __builtin_amdgcn_readlane(hi, src);
    return __hiloint2double(hi, lo);
}

// ---- optional per-kernel-class timing with HIP events on the launch stream (bench.py's roofline leg).
// Off by default; internal (amk__timing_* are not part of the C ABI in include/avoid_mpc_amd.h).
enum KernelClass { KC_COMPACT = 0, KC_SCAN_OBS, KC_SCAN_EDGE, KC_PLAN, KC_PACK, KC_SOLVE, KC_BEGIN, KC_GRID, KC_COUNT };
struct Timing;
Timing &timing();
struct TimedLaunch {  // RAII: records an event before and after the enclosed launch when enabled
    TimedLaunch(int kclass, hipStream_t stream);
    ~TimedLaunch();
    int slot;
    hipStream_t stream;
};

}  // namespace amk

#include "host_stage.h"

struct amk_kd;
struct amk_mpc;
// kd_index.hip, for kd_sweep.hip and kd_exact.hip: the index-ordered planes made valid on `stream`
int ensure_soa(amk_kd *kd, hipStream_t stream);
extern "C" int amk__kd_ensure_soa(amk_kd *kd, void *stream);   // ensure_soa for step.hip (internal: not in include/avoid_mpc_amd.h)

// ---- kd_exact.hip: the reference-shaped tree (AMK_TIES_NANOFLANN, AMK_TIES_AUTO, the keyframe map's tie order) -- everything the
// other translation units call.  The tree's C ABI (amk_kd_set_tie_order, amk_kd_exact_status*, amk__kd_exact_*,
// amk__exact_set_queue_cap) lives there too.
// the trees of every scene of a handle in AMK_TIES_NANOFLANN, from its index-ordered planes (made on demand): two launches
int exact_build(amk_kd *kd, hipStream_t stream);
// what every index build of a handle ends with: AUTO's per-scene words cleared for the new cloud, exact_build in AMK_TIES_NANOFLANN
int exact_after_index_build(amk_kd *kd, hipStream_t stream);
// nanoflann's own traversal over the results of the bucketed search launched before it on `stream`: every row of every scene whose
// tree is available, or (kd->auto_on()) the rows the search flagged in the scenes whose tree is built.  One launch.
int exact_search(amk_kd *kd, const double *d_queries, int n_queries, int k, int *d_indices, double *d_sqdist, float *d_pts,
                 int *d_counts, hipStream_t stream);
namespace amk {
// AMK_TIES_AUTO: the lazy build of the trees of up to two handles (null: none) in two launches -- a workgroup returns at once
// unless its scene's `need` word is raised and its tree is not built yet (see amk_kd::au_state)
int kd_auto_build(amk_kd *a, amk_kd *b, hipStream_t stream);
// The keyframe map in AMK_TIES_NANOFLANN (amk_kfmap_set_tie_order): the trees of a pool's scenes.
// _bytes: what _reserve allocates (host arithmetic); _build: two launches behind a mapped build (both pools, d_gate null) or a
// sweep (obstacle pool, edge_pool null, d_gate = the sweep's rebuilt flags) -- row i builds pool scene d_rows[i] unless that is < 0
// or its gate word is 0, decided on the device
long long kd_pool_exact_bytes(long long scenes, int max_points, bool with_planes);
int kd_pool_exact_reserve(amk_kd *pool);
int kd_pool_exact_build(amk_kd *obs_pool, amk_kd *edge_pool, int n_rows, const int *d_rows, const int *d_gate, hipStream_t stream);
int kd_pool_exact_status(amk_kd *pool, int *d_status, hipStream_t stream);   // amk_kd_exact_status's codes for every pool scene

struct ExactPtrs;   // kd_exact.h
// The tree's device arrays for the scenes of one handle: all of them or none.  ONE description (kArrays) gives every array's element
// size and extent; alloc and bytes both read it.
struct ExactStore {
    enum Id { VIND, SA, SB, PC, LEFT, RIGHT, FEAT, CHILD, LOW, HIGH, NBBOX, ROOT, NN, kCount };
    enum Extent { kPerPoint, kPerNode, kPerScene };   // x (scenes * cap), x (scenes * max_nodes), x scenes
    struct Array { int bytes; Extent per; };
    static constexpr Array kArrays[kCount] = {
        {4, kPerPoint}, {4, kPerPoint}, {4, kPerPoint},   // VIND vAcc_ | SA, SB planeSplit's lists of misplaced positions
        {12, kPerPoint},                                  // PC [3][S][cap] the coordinates in vAcc_ order (leaves are contiguous runs)
        {4, kPerNode}, {4, kPerNode}, {4, kPerNode}, {4, kPerNode},   // LEFT, RIGHT node range in vAcc_ | FEAT divfeat | CHILD child1
        {8, kPerNode}, {8, kPerNode}, {48, kPerNode},     // LOW divlow | HIGH divhigh | NBBOX the box divideTree hands down
        {48, kPerScene}, {4, kPerScene},                  // ROOT root_bbox_ | NN number of nodes, -1: the tree is not available
    };
    static long long nodes_for(long long cap) { return cap / 2 + 64; }   // ~0.29 nodes per point with 10-point leaves; more = pathological data
    static long long array_bytes(Id i, long long scenes, long long cap) {
        const Extent e = kArrays[i].per;
        return kArrays[i].bytes * scenes * (e == kPerPoint ? cap : e == kPerNode ? nodes_for(cap) : 1);
    }
    static long long bytes(long long scenes, long long cap) {
        long long b = 0;
        for (int i = 0; i < kCount; ++i) b += array_bytes((Id)i, scenes, cap);
        return b;
    }
    DevBuf<unsigned char> buf[kCount];
    int max_nodes = 0;
    int alloc(int scenes, int cap);   // AMK_OK when they exist already; a failure part way through frees what it got
    void release() { for (auto &b : buf) b.release(); }
    bool allocated() const { return buf[VIND].p != nullptr; }
    template <typename T> T *at(Id i) const { return reinterpret_cast<T *>(buf[i].p); }
    int *n_nodes() const { return at<int>(NN); }
    // the batch pointers over the handle's index-ordered planes x / y / z (kd_exact.h)
    ExactPtrs ptrs(const float *x, const float *y, const float *z, int cap, int scenes) const;
};

// kd_index.hip: the frames of a pipeline gang built by one launch (see there)
int kd_build_gang(amk_kd *obstacle, amk_kd *edge, int n_frames, int frame_scenes, const float *const *d_xyz,
                  const int *const *d_counts, const float *const *d_edge_xyz, const int *const *d_edge_counts, int point_stride,
                  hipStream_t stream, const int *const *d_keep_if_zero = nullptr);
// kd_index.hip / kd_sweep.hip, for the keyframe map (kfmap.hip): builds and sweeps on a POOL handle (scene = physical slot * S + scene)
int pool_planes(amk_kd *kd);   // kd_sweep.hip: allocates a handle's index-ordered planes where it has none (every pool build writes them)
int kd_build_mapped(amk_kd *obs_pool, amk_kd *edge_pool, int n_in, const float *d_xyz, const int *d_counts, const float *d_edge_xyz,
                    const int *d_edge_counts, int point_stride, const int *d_out_scene, hipStream_t stream);
int kd_pool_reserve(amk_kd *pool, int n_rows);
int kd_build_mapped_gang(amk_kd *obs_pool, amk_kd *edge_pool, int n_frames, int frame_scenes, const float *const *d_xyz,
                         const int *const *d_counts, const float *const *d_edge_xyz, const int *const *d_edge_counts, int point_stride,
                         const int *d_out_scene, hipStream_t stream);
int kd_sweep_mapped(amk_kd *pool, int n_rows, const int *d_kf_list, const int *d_cur_list, double th_dist, int th_count,
                    int *d_outliers, int *d_rebuilt, hipStream_t stream);
// step_frames.hip, for kfmap.hip: the control step over a keyframe map -- every frame of every scene in the two pool handles, frame f
// of scene s = pool scene d_fmap[f * S + s] (< 0: absent); n_frames = 1 + max_frame_count of the map, <= AMK_MAX_MAP_FRAMES
int step_batch_map(amk_kd *obs_pool, amk_kd *edge_pool, int n_frames, const int *d_fmap, const double *d_Twc,
                   const amk_frame_camera *cam, amk_mpc *mpc, const amk_step_params *prm, const double *d_state_quad,
                   const double *d_pos_x, double *d_ref_path, double *d_u, double *d_x0array, int *d_flags, hipStream_t stream,
                   bool exact);
// map_query.hip, for kfmap.hip: QueryNearest / GetNearestDistance over a pool
int map_query_nearest(amk_kd *pool, int n_frames, const int *d_fmap, int S, const double *d_Twc, const amk_frame_camera *cam,
                      const double *d_queries, int query_stride, int n_queries, int k, float *d_pts, double *d_sqdist, int *d_frame,
                      int *d_counts, hipStream_t stream, bool exact);
int map_nearest_distance(amk_kd *pool, int n_frames, const int *d_fmap, int S, const double *d_queries, int query_stride,
                         int n_queries, double *d_dist, hipStream_t stream);
inline bool query_args_ok(const double *queries, int query_stride, int n_queries) { return queries && query_stride >= 3 && n_queries >= 1; }
// kd_radius.hip / map_query.hip: the argument rules every radius search shares (include/avoid_mpc_amd.h), checked before anything
// is staged or launched.  any_list: a list output was given; any_out: an output at all
inline int radius_args_status(const double *queries, int query_stride, int n_queries, double radius_sq, int max_results, bool any_list,
                              bool any_out) {
    if (!query_args_ok(queries, query_stride, n_queries) || !(radius_sq >= 0.0) || max_results < 0 || !any_out) return AMK_ERR_INVALID_ARG;
    if (max_results > AMK_MAX_K) return AMK_ERR_UNSUPPORTED;
    if (max_results == 0 && any_list) return AMK_ERR_INVALID_ARG;
    return AMK_OK;
}
inline double radius_clamped(double radius_sq) { return radius_sq < DBL_MAX ? radius_sq : DBL_MAX; }   // +inf: every usable point
// map_query.hip, for kfmap.hip: the radius search over a pool
int map_radius_search(amk_kd *pool, int n_frames, const int *d_fmap, int S, const double *d_queries, int query_stride, int n_queries,
                      double radius_sq, int max_results, float *d_pts, double *d_sqdist, int *d_frame, int *d_counts, hipStream_t stream);
// Their *_host variants and amk_kd_query_frames_host: queries (and poses) staged through `stage`, launch(d) -- the entry's device
// call, d[i] = MapQuerySlot i, null where the host pointer is -- enqueued on the null stream between two device-wide waits (a
// build or an update enqueued on any stream is seen), results copied back.  A convenience for single-robot hosts and tests,
// not a hot path.  Any output may be NULL.  map_stage_call is that staging, the tail of every one of them.
template <class Launch>
int map_stage_call(HostStage &stage, std::initializer_list<HostCopy> slots, Launch &&launch) {
    return stage.call(slots, [&](const HostStage::Dev *d) { AMK_HIP(hipDeviceSynchronize()); return launch(d); }, hipDeviceSynchronize);
}
// the doubles a batch of queries or path points spans in host memory: n_points of `stride` doubles per scene, the last one 3 long
inline size_t points_extent(size_t S, int n_points, int stride) { return (S * n_points - 1) * stride + 3; }
enum MapQuerySlot { MQ_QUERIES, MQ_TWC, MQ_PTS, MQ_SQDIST, MQ_FRAME, MQ_COUNTS, MQ_DIST };
template <class Launch>
int map_query_host(HostStage &stage, int S, const double *h_queries, int query_stride, int n_queries, int k, const double *h_Twc,
                   float *h_pts, double *h_sqdist, int *h_frame, int *h_counts, double *h_dist, Launch &&launch) {
    if (S < 1 || !query_args_ok(h_queries, query_stride, n_queries) || k < 1) return AMK_ERR_INVALID_ARG;
    if (k > AMK_MAX_K) return AMK_ERR_UNSUPPORTED;
    const size_t rows = (size_t)S * n_queries;
    return map_stage_call(stage,
                          {to_device(h_queries, sizeof(double) * points_extent(S, n_queries, query_stride)),
                           if_given(to_device(h_Twc, sizeof(double) * S * 16)), if_given(to_host(h_pts, sizeof(float) * rows * k * 3)),
                           if_given(to_host(h_sqdist, sizeof(double) * rows * k)), if_given(to_host(h_frame, sizeof(int) * rows * k)),
                           if_given(to_host(h_counts, sizeof(int) * rows)), if_given(to_host(h_dist, sizeof(double) * rows))},
                          launch);
}
// The *_host variants of the map's radius searches: the same staging (slots MQ_QUERIES, MQ_PTS ... MQ_COUNTS) under the radius
// search's argument rules
template <class Launch>
int map_radius_host(HostStage &stage, int S, const double *h_queries, int query_stride, int n_queries, double radius_sq, int max_results,
                    float *h_pts, double *h_sqdist, int *h_frame, int *h_counts, Launch &&launch) {
    if (S < 1) return AMK_ERR_INVALID_ARG;
    if (const int st = radius_args_status(h_queries, query_stride, n_queries, radius_sq, max_results, h_pts || h_sqdist || h_frame,
                                          h_pts || h_sqdist || h_frame || h_counts);
        st != AMK_OK)
        return st;
    const size_t rows = (size_t)S * n_queries, k = (size_t)max_results;
    return map_stage_call(stage,
                          {to_device(h_queries, sizeof(double) * points_extent(S, n_queries, query_stride)), scratch(0),
                           if_given(to_host(h_pts, sizeof(float) * rows * k * 3)), if_given(to_host(h_sqdist, sizeof(double) * rows * k)),
                           if_given(to_host(h_frame, sizeof(int) * rows * k)), if_given(to_host(h_counts, sizeof(int) * rows))},
                          launch);
}
// kd_segment.hip / map_query.hip: the argument rules every segment search shares (include/avoid_mpc_amd.h, "Segment search"),
// checked before anything is staged or launched: a path is n_points >= 2 positions, the rest as for the radius searches
inline int segment_args_status(const double *path, int point_stride, int n_points, double radius_sq, int max_results, bool any_list,
                               bool any_out) {
    if (n_points < 2) return AMK_ERR_INVALID_ARG;
    return radius_args_status(path, point_stride, n_points, radius_sq, max_results, any_list, any_out);
}
// map_query.hip, for kfmap.hip: the segment search over a pool
int map_segment_search(amk_kd *pool, int n_frames, const int *d_fmap, int S, const double *d_path, int point_stride, int n_points,
                       double radius_sq, int max_results, float *d_pts, double *d_sqdist, double *d_t, int *d_frame, int *d_counts,
                       hipStream_t stream);
// The *_host variants of the map's segment searches: map_radius_host's staging with the path in MQ_QUERIES and t in MQ_DIST; the
// outputs have a row per LEG
template <class Launch>
int map_segment_host(HostStage &stage, int S, const double *h_path, int point_stride, int n_points, double radius_sq, int max_results,
                     float *h_pts, double *h_sqdist, double *h_t, int *h_frame, int *h_counts, Launch &&launch) {
    if (S < 1) return AMK_ERR_INVALID_ARG;
    if (const int st = segment_args_status(h_path, point_stride, n_points, radius_sq, max_results, h_pts || h_sqdist || h_t || h_frame,
                                           h_pts || h_sqdist || h_t || h_frame || h_counts);
        st != AMK_OK)
        return st;
    const size_t rows = (size_t)S * (n_points - 1), k = (size_t)max_results;
    return map_stage_call(stage,
                          {to_device(h_path, sizeof(double) * points_extent(S, n_points, point_stride)), scratch(0),
                           if_given(to_host(h_pts, sizeof(float) * rows * k * 3)), if_given(to_host(h_sqdist, sizeof(double) * rows * k)),
                           if_given(to_host(h_frame, sizeof(int) * rows * k)), if_given(to_host(h_counts, sizeof(int) * rows)),
                           if_given(to_host(h_t, sizeof(double) * rows * k))},
                          launch);
}
// kd_segment_nearest.hip / map_query.hip / kfmap.hip: the argument rules all six segment-nearest entries share
// (include/avoid_mpc_amd.h, "Segment nearest"), checked before anything is staged or launched.  any_out: an output at all
inline int segment_nearest_args_status(const double *path, int point_stride, int n_points, int k, bool any_out) {
    if (n_points < 2 || !query_args_ok(path, point_stride, n_points) || k < 1 || !any_out) return AMK_ERR_INVALID_ARG;
    if (k > AMK_MAX_K) return AMK_ERR_UNSUPPORTED;
    return AMK_OK;
}
// map_query.hip, for kfmap.hip: segment nearest over a pool
int map_segment_nearest(amk_kd *pool, int n_frames, const int *d_fmap, int S, const double *d_path, int point_stride, int n_points, int k,
                        float *d_pts, double *d_sqdist, double *d_t, int *d_frame, int *d_counts, hipStream_t stream);
// The *_host variants of the map's segment-nearest queries: map_segment_host as it is, k in place of max_results and every
// usable point in place of the radius, under the rules above
template <class Launch>
int map_segment_nearest_host(HostStage &stage, int S, const double *h_path, int point_stride, int n_points, int k, float *h_pts,
                             double *h_sqdist, double *h_t, int *h_frame, int *h_counts, Launch &&launch) {
    if (const int st = segment_nearest_args_status(h_path, point_stride, n_points, k, h_pts || h_sqdist || h_t || h_frame || h_counts);
        st != AMK_OK)
        return st;
    return map_segment_host(stage, S, h_path, point_stride, n_points, DBL_MAX, k, h_pts, h_sqdist, h_t, h_frame, h_counts, launch);
}
// kd_segment_cast.hip / map_query.hip / kfmap.hip: the argument rules all six segment-cast entries share
// (include/avoid_mpc_amd.h, "Segment cast"), checked before anything is staged or launched: the segment search's path and radius
// rules, no max_results.  any_out: an output at all
inline int segment_cast_args_status(const double *path, int point_stride, int n_points, double radius_sq, bool any_out) {
    if (n_points < 2 || !query_args_ok(path, point_stride, n_points) || !(radius_sq >= 0.0) || !any_out) return AMK_ERR_INVALID_ARG;
    return AMK_OK;
}
// map_query.hip, for kfmap.hip: the segment cast over a pool
int map_segment_cast(amk_kd *pool, int n_frames, const int *d_fmap, int S, const double *d_path, int point_stride, int n_points,
                     double radius_sq, int *d_hit, double *d_t, float *d_pts, int *d_frame, hipStream_t stream);
// The *_host variants of the map's segment casts: map_segment_host as it is with one result per leg -- hit in MQ_COUNTS, t in
// MQ_DIST, no squared distance -- under the rules above
template <class Launch>
int map_segment_cast_host(HostStage &stage, int S, const double *h_path, int point_stride, int n_points, double radius_sq, int *h_hit,
                          double *h_t, float *h_pts, int *h_frame, Launch &&launch) {
    if (const int st = segment_cast_args_status(h_path, point_stride, n_points, radius_sq, h_hit || h_t || h_pts || h_frame);
        st != AMK_OK)
        return st;
    return map_segment_host(stage, S, h_path, point_stride, n_points, radius_sq, 1, h_pts, nullptr, h_t, h_frame, h_hit, launch);
}
// Path cast (include/avoid_mpc_amd.h, "Path cast"; kd_path_cast.hip / map_query.hip / kfmap.hip): the outputs, a row per SCENE,
// each null where it is not wanted
struct PathCastOut {
    int *stop, *leg;
    double *t, *free;
    float *pts;
    int *id;   // cloud index (one handle) or frame (a map, a list of handles)
    bool any() const { return stop || leg || t || free || pts || id; }
};
// The entries behind the six calls, which the pipeline's audit stage uses as well: the leading n_scenes scenes of the handle (the
// map), scene s's path at path + s * scene_stride doubles.  The public calls pass every scene and n_points * point_stride.
int kd_path_cast_scenes(amk_kd *kd, int n_scenes, const double *d_path, int point_stride, long long scene_stride, int n_points,
                        double radius_sq, const PathCastOut &out, hipStream_t stream);
int map_path_cast(amk_kd *pool, int n_frames, const int *d_fmap, int S, int n_scenes, const double *d_path, int point_stride,
                  long long scene_stride, int n_points, double radius_sq, const PathCastOut &out, hipStream_t stream);
int kfmap_path_cast_scenes(amk_kfmap *m, int n_scenes, const double *d_path, int point_stride, long long scene_stride, int n_points,
                           double radius_sq, int query_edge, const PathCastOut &out, hipStream_t stream);
// The *_host variants of the map's path casts: the segment cast's staging (device-wide waits around a launch on the null stream)
// with one result per scene
enum PathCastSlot { PC_PATH, PC_STOP, PC_LEG, PC_T, PC_FREE, PC_PTS, PC_ID };
template <class Launch>
int map_path_cast_host(HostStage &stage, int S, const double *h_path, int point_stride, int n_points, double radius_sq, int *h_stop,
                       int *h_leg, double *h_t, double *h_free, float *h_pts, int *h_frame, Launch &&launch) {
    if (S < 1) return AMK_ERR_INVALID_ARG;
    if (const int st = segment_cast_args_status(h_path, point_stride, n_points, radius_sq, h_stop || h_leg || h_t || h_free || h_pts || h_frame);
        st != AMK_OK)
        return st;
    const size_t rows = (size_t)S;
    return map_stage_call(stage,
                          {to_device(h_path, sizeof(double) * points_extent(S, n_points, point_stride)),
                           if_given(to_host(h_stop, sizeof(int) * rows)), if_given(to_host(h_leg, sizeof(int) * rows)),
                           if_given(to_host(h_t, sizeof(double) * rows)), if_given(to_host(h_free, sizeof(double) * rows)),
                           if_given(to_host(h_pts, sizeof(float) * rows * 3)), if_given(to_host(h_frame, sizeof(int) * rows))},
                          launch);
}
// kfmap.hip, for pipeline.hip: AddVertex for the frames of a gang (see there)
int kfmap_add_vertex_gang(amk_kfmap *m, int n_frames, int frame_scenes, const float *const *d_xyz, const int *const *d_counts,
                          const float *const *d_edge_xyz, const int *const *d_edge_counts, int point_stride, const double *const *d_Twc,
                          hipStream_t stream);
}  // namespace amk

// ------------------------------------------------------------------------------------------------
// handle layouts (shared between kd_index.hip, kd_exact.hip, mpc_solve.hip and step.hip)
// ------------------------------------------------------------------------------------------------
struct amk_kd {
    int n_scenes = 0;
    int max_points = 0;
    int cap = 0;  // per-scene SoA capacity, multiple of 256 with >= 1024 floats of NaN padding
    amk::DevBuf<float> x, y, z;  // [S][cap] filtered points (order preserved), NaN padded -- made ON DEMAND from the
                                 // bucket records (ensure_soa, kd_index.hip): the build does not write them
    int soa_valid = 0;           // host flag: x/y/z match the current index
    amk::DevBuf<int> size;       // [S] cloud.pts.size() after the NaN-x filter
    amk::DevBuf<float> pmax;     // [S] max |coordinate| of the kept points (bounds the fp32 pre-filter error)
    // bucketed index (kd_grid.h): bucket-contiguous copy of the points, their cloud indices, bucket starts
    amk::DevBuf<float4> gpt;         // [S][cap]  (x, y, z, cloud index)
    amk::DevBuf<float> bbox;         // [S][6]    min xyz, max xyz of the finite points
    amk::DevBuf<int> cell_start;     // [S][ntiles][kGridMaxCells + 2]  bucket starts of every tile of the record array (kd_grid.h)
    int ntiles = 1;                  // ceil(max_points / kTilePoints)
    amk::DevBuf<double> gparams;     // [S][8]
    int mode = 0;                    // 0: grid search (default), 1: streaming scan (cross-check)
    // opt-in "nanoflann tie order" (amk_kd_set_tie_order, kd_exact.h): the reference's own tree, built beside the bucketed index
    int tie_order = 0;
    int ex_valid = 0;   // host flag: the exact tree was built from the cloud the bucketed index currently holds
    int pool_exact = 0; // host flag, a keyframe map's pool only: the map is in AMK_TIES_NANOFLANN -- every pool scene that holds a frame holds
                        // its tree (kd_pool_exact_build), and the mapped build writes this pool's index-ordered planes too
    amk::ExactStore exact;   // the tree's arrays (kd_exact.hip allocates them: the two modes and the keyframe map's pools)
    // AMK_TIES_AUTO: the same tree, built on the device for the scenes where a query tied, by the searches that saw the tie.
    // Every index build clears au_state on its stream, so a tree never answers for a cloud it was not built from.
    int au_active = 0;            // host flag: the last index build ran in AMK_TIES_AUTO and cleared au_state for the cloud held
    amk::DevBuf<int> au_state;    // [3][S] need (a query of the scene tied), built (its tree belongs to the cloud held), requery_tied
                                  // (the control step's re-query of the snapped reference point tied in this pass)
    amk::DevBuf<int> au_rowflag;  // [S][AMK_MAX_QUERIES] tie flag of every (scene, query) row of the search / step pass in flight
    int *au_need() const { return au_state.p; }
    int *au_built() const { return au_state.p + n_scenes; }
    int *au_requery() const { return au_state.p + 2 * (size_t)n_scenes; }
    bool auto_on() const { return tie_order == AMK_TIES_AUTO && au_active && mode == 0; }
    amk::DevBuf<unsigned char> flags; // [S][cap] keyframe sweep: 1 = outlier
    amk::DevBuf<int> sweep_cnt;       // [S][2]   {outliers, rebuilt}
    // the keyframe map's pool only (kd_sweep_mapped): the sweep's target, per sweep ROW -- the current frame's points once more, sorted
    // into a fine hashed grid (cells of 2.5 th), rebuilt before every sweep
    // Two generations (this sweep's and the one before: a row's newest keyframe is usually the frame it swept against last period,
    // and its points are then taken in that grid's order -- the lanes of a wavefront ask for the same few buckets)
    amk::DevBuf<float4> sw_gpt;       // [2][rows][cap]         records, bucket by bucket
    amk::DevBuf<int> sw_cs;           // [2][rows][buckets + 1] bucket starts; the last entry = points with finite coordinates
    amk::DevBuf<int> sw_src;          // [2 + 1][rows]          pool scene the row's grid was built from, -1: none (row 2: always -1)
    int sw_rows = 0, sw_flip = 0;
    double sw_inv_h = 0.0;            // the lattice of the grids held (1 / cell edge)
    // staging of the *_host conveniences.  amk_kd_search_host goes through the pinned block and the private stream, so that a
    // single-query SearchForNearest costs one small H2D copy, one launch, one D2H copy and a wait on THAT stream only (a device-wide
    // synchronisation would stall every other stream of the process: a ROS node calls this ~100 times per control period)
    amk::HostStage stage;
    int async_pending = 0;  // a stream-ordered build / sweep was enqueued since the last synchronisation
};
