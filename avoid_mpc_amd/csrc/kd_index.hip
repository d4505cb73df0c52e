// KD index of the Avoid-MPC hot path for gfx950 (MI355X): batch of KDTreeTwo<double> objects.
//
// Replaces (AM = roswrapper/ros/src/avoid_mpc in the reference tree):
//   amk_kd_build   <- KDTreeTwo::InitializeNew      AM/include/kd_tree_two.h:76-78,88-106
//                     (+ nanoflann buildIndex       AM/include/nanoflann_two.hpp:1518-1541)
//   amk_kd_search  <- KDTreeTwo::SearchForNearest   AM/include/kd_tree_two.h:108-133
//                     (+ nanoflann findNeighbors    AM/include/nanoflann_two.hpp:1563-1586)
//
// Design: only the RESULTS of a search must equal the reference's, the
// tree shape is free.  build = one launch, one 512-thread block per scene, reading the caller's AoS cloud directly:
// sampled bounding box, histogram pass (which also applies the NaN-x filter by ballot/popcount), scan, scatter of one
// 16-byte record (x, y, z, cloud index) per point into a bucketed grid (kd_grid.h).  search = one wavefront per
// (scene, query) walking Chebyshev rings of grid cells with nanoflann's branch-and-bound stop rule.  The streaming scan
// of index-ordered SoA planes (kd_device.h; the first correct path) is kept as a cross-check (amk__kd_set_mode) and
// makes its planes on demand.  The opt-in reference-shaped tree beside the index (tie orders AMK_TIES_NANOFLANN / AMK_TIES_AUTO) is
// kd_exact.hip, the keyframe sweep kd_sweep.hip; what this file calls of the tree is the block "kd_exact.hip" of amk_common.h.
#include "kd_exact.h"

#include <cstring>

namespace amk {
thread_local int g_last_hip_error = 0;

struct Timing {
    int mode = 0;  // 0 off, 1 KC_SOLVE and KC_GRID (the dominant kernel and the HBM-heavy one), 2 every kernel class
    struct Rec { int kclass; hipEvent_t a, b; };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    hipEvent_t get() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e;
        (void)hipEventCreate(&e);
        return e;
    }
};
Timing &timing() { static Timing t; return t; }

TimedLaunch::TimedLaunch(int kclass, hipStream_t s) : slot(-1), stream(s) {
    Timing &t = timing();
    if (t.mode == 0 || (t.mode == 1 && kclass != KC_SOLVE && kclass != KC_GRID)) return;
    Timing::Rec r{kclass, t.get(), t.get()};
    (void)hipEventRecord(r.a, stream);
    slot = (int)t.recs.size();
    t.recs.push_back(r);
}
TimedLaunch::~TimedLaunch() {
    if (slot >= 0) (void)hipEventRecord(timing().recs[slot].b, stream);
}
}  // namespace amk

extern "C" void amk__timing_enable(int mode) { amk::timing().mode = mode; }
// Waits for the recorded events; adds elapsed milliseconds / launch counts per kernel class; resets.
extern "C" int amk__timing_collect(double *ms, int *counts) {
    amk::Timing &t = amk::timing();
    for (int i = 0; i < amk::KC_COUNT; ++i) { ms[i] = 0.0; counts[i] = 0; }
    for (auto &r : t.recs) {
        float f = 0.f;
        if (hipEventSynchronize(r.b) != hipSuccess || hipEventElapsedTime(&f, r.a, r.b) != hipSuccess) return AMK_ERR_HIP;
        ms[r.kclass] += f;
        counts[r.kclass] += 1;
        t.pool.push_back(r.a);
        t.pool.push_back(r.b);
    }
    t.recs.clear();
    return AMK_OK;
}

// Like amk__timing_collect, but keeps every launch: class, start and end in milliseconds after the first recorded launch
// (tools/experiments/burst_timeline.py: who runs when, without a tracer slowing the host down).  Returns the number of launches.
extern "C" int amk__timing_timeline(int max_recs, int *kclass, double *start_ms, double *end_ms) {
    amk::Timing &t = amk::timing();
    int n = 0;
    for (auto &r : t.recs) {
        float fa = 0.f, fb = 0.f;
        if (hipEventSynchronize(r.b) != hipSuccess || hipEventElapsedTime(&fa, t.recs[0].a, r.a) != hipSuccess ||
            hipEventElapsedTime(&fb, t.recs[0].a, r.b) != hipSuccess)
            return AMK_ERR_HIP;
        if (n < max_recs) { kclass[n] = r.kclass; start_ms[n] = fa; end_ms[n] = fb; ++n; }
    }
    for (auto &r : t.recs) { t.pool.push_back(r.a); t.pool.push_back(r.b); }
    t.recs.clear();
    return n;
}

using amk::kWave;

// ------------------------------------------------------------------------------------------------
// build: order-preserving compaction of the points whose x is not NaN (kd_tree_two.h:96-101)
// ------------------------------------------------------------------------------------------------
using amk::kCompactThreads;   // (kd_grid.h: 512, and why not 1024)

// Pre-pass of the index build: bounding box of a SAMPLE of the caller's cloud (of a large cloud: runs of 64 consecutive
// points, one run in 16; finite points whose x is not NaN).  The grid geometry only needs a box that holds most points: a
// point outside is clamped into a boundary cell (kd_grid.h), so 1/16 of the cloud is read here instead of all of it.
__device__ __forceinline__ void sample_bbox_scene(int s, const float *__restrict__ src, int point_stride, int n,
                                                  float *__restrict__ bbox_out) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    constexpr int NW = kCompactThreads / kWave;
    __shared__ float wave_bb[6][NW];
#ifndef AMK_BBOX_STEP
#define AMK_BBOX_STEP 16
#endif
    const int step = n >= 16384 ? AMK_BBOX_STEP : 1;
    float bmn[3] = {3.0e38f, 3.0e38f, 3.0e38f}, bmx[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    // the sample: runs of 64 consecutive points, one run in `step` (lines of the cloud are fetched whole, so a point in 16
    // cost 2/3 of a full pass in traffic; a run in 16 costs 1/16)
    for (int t = tid;; t += kCompactThreads) {
        const long long i = (long long)(t >> 6) * (64 * step) + (t & 63);
        if (i >= n) break;
        const float *p = src + (size_t)i * point_stride;
        const float px = p[0], py = p[1], pz = p[2];
        if (amk::boxable3(px, py, pz)) {
            bmn[0] = fminf(bmn[0], px); bmx[0] = fmaxf(bmx[0], px);
            bmn[1] = fminf(bmn[1], py); bmx[1] = fmaxf(bmx[1], py);
            bmn[2] = fminf(bmn[2], pz); bmx[2] = fmaxf(bmx[2], pz);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            bmn[a] = fminf(bmn[a], __shfl_xor(bmn[a], off));
            bmx[a] = fmaxf(bmx[a], __shfl_xor(bmx[a], off));
        }
    if (lane == 0)
#pragma unroll
        for (int a = 0; a < 3; ++a) { wave_bb[a][w] = bmn[a]; wave_bb[3 + a][w] = bmx[a]; }
    __syncthreads();
    if (tid < 6) {
        float v = wave_bb[tid][0];
        for (int j = 1; j < NW; ++j) v = tid < 3 ? fminf(v, wave_bb[tid][j]) : fmaxf(v, wave_bb[tid][j]);
        bbox_out[6 * s + tid] = v;
    }
    __threadfence_block();
    __syncthreads();  // read back by the index build below
}

// InitializeNew for scene s = blockIdx.x in one launch: the sampled bounding box, then the bucketed index straight
// from the caller's cloud in ONE pass over it (grid_build_tiles_scene: the cloud in tiles of 4096 points, each loaded once,
// its records written into the tile's own window).  The index-ordered SoA planes are NOT written: whoever needs them
// (scan-mode searches, amk_kd_points_host, the keyframe sweep) gets them from the records on demand (ensure_soa).
struct BuildArgs {   // one tree's InitializeNew
    const float *xyz;
    int point_stride;
    long long scene_stride;
    const int *counts;
    int max_points, cap;
    int *size_out;
    float *pmax_out, *bbox_out;
    float4 *GP;
    int *cell_start;
    int ntiles;
    double *gparams;
    const int *keep_if_zero;   // [S] or null: scene s keeps its previous index when keep_if_zero[s] == 0 (FrameKDMap::AddVertex
                               // returns before BOTH InitializeNew calls when the frame's obstacle cloud is empty, FrameKDMap.cpp:39-41)
    float *soa_x, *soa_y, *soa_z;   // or null: the index-ordered planes of the handle's first scene of this entry, written by the build
    const int *out_scene;      // [S] or null: input scene s is built into scene out_scene[s] of the handle (< 0: not built) -- the
                               // keyframe map's pool, where every scene's current frame lives in a physical slot of its own (kfmap.hip)
};
// grid = (scenes, trees): blockIdx.y selects the tree.  FrameKDMap::AddVertex builds TWO trees per depth frame (obstacle +
// edge cloud, FrameKDMap.cpp:44-47): amk_kd_build_pair issues them as one launch, so the small edge build (24 us alone,
// mostly latency) runs in the shadow of the obstacle build instead of behind it.
constexpr int kBuildMaxEntries = 2 * AMK_PIPELINE_MAX_GANG;   // (tree, frame) pairs of one launch
struct BuildArgs2 { BuildArgs t[kBuildMaxEntries]; };
__global__ __launch_bounds__(kCompactThreads, 4) void kd_build_kernel(const BuildArgs2 args) {   // 4 waves per SIMD = two blocks per CU: <= 128 VGPRs
    const BuildArgs &a = args.t[blockIdx.y];   // a scalar load from the kernel-argument segment
    const int s_in = blockIdx.x;
    if (a.keep_if_zero && a.keep_if_zero[s_in] == 0) return;   // (block-uniform)
    const int s = a.out_scene ? a.out_scene[s_in] : s_in;      // where the index goes
    if (s < 0) return;
    const float *src = a.xyz + (long long)s_in * a.scene_stride;
    int n = a.counts ? a.counts[s_in] : a.max_points;
    n = n < 0 ? 0 : (n > a.max_points ? a.max_points : n);
    sample_bbox_scene(s, src, a.point_stride, n, a.bbox_out);
    const size_t so = (size_t)s * a.cap;
    amk::grid_build_tiles_scene(s, src, a.point_stride, a.cap, n, a.bbox_out, a.GP, a.cell_start, a.ntiles, a.gparams,
                                a.size_out + s, a.pmax_out + s, a.soa_x ? a.soa_x + so : nullptr, a.soa_y ? a.soa_y + so : nullptr,
                                a.soa_z ? a.soa_z + so : nullptr);
}
// so: first scene of the handle this entry writes (a gang launch builds frame f into scenes [f * S, (f + 1) * S) of the handle)
static BuildArgs build_args(amk_kd *kd, const float *d_xyz, int point_stride, long long scene_stride, const int *d_counts,
                            size_t so = 0) {
    return BuildArgs{d_xyz, point_stride, scene_stride, d_counts, kd->max_points, kd->cap,
                     kd->size.p + so, kd->pmax.p + so, kd->bbox.p + so * 6, kd->gpt.p + so * kd->cap,
                     kd->cell_start.p + so * kd->ntiles * (amk::kGridMaxCells + 2), kd->ntiles,
                     kd->gparams.p + so * amk::kGridParamDoubles, nullptr, nullptr, nullptr, nullptr, nullptr};
}
// A handle in nanoflann tie order builds its tree from the index-ordered planes right after the index: the build kernel
// writes them itself (coalesced) instead of kd_records_to_soa_kernel scattering them from the records afterwards.  Returns
// whether `a` now asks for them (false: allocation failed or not wanted -- ensure_soa makes them on demand as before).
static bool build_writes_soa(amk_kd *kd, BuildArgs &a, size_t so = 0) {
    if (kd->tie_order != AMK_TIES_NANOFLANN || kd->cap <= 0) return false;   // (AMK_TIES_AUTO makes them per scene, on demand)
    if (!kd->x.p || !kd->y.p || !kd->z.p) {   // (a failed allocation leaves what it got: ensure_soa retries the rest)
        const size_t tot = (size_t)kd->n_scenes * kd->cap;
        if ((!kd->x.p && kd->x.alloc(tot) != hipSuccess) || (!kd->y.p && kd->y.alloc(tot) != hipSuccess) ||
            (!kd->z.p && kd->z.alloc(tot) != hipSuccess))
            return false;
    }
    a.soa_x = kd->x.p + so * kd->cap; a.soa_y = kd->y.p + so * kd->cap; a.soa_z = kd->z.p + so * kd->cap;
    return true;
}

namespace amk {
// FrameKDMap::AddVertex's two InitializeNew calls (FrameKDMap.cpp:44-47) for the G frames of a pipeline gang in ONE launch
// (grid.y = 2 G trees): frame f's scenes are built into the pool scenes d_out_scene[f * frame_scenes + s] (< 0: that scene gets no
// new frame); the obstacle pool's planes are written along.  (One add_vertex per gang position was 2 G launches per period: the
// map's periods at the reference's 3072-point frames are bound by their launch count.)
int kd_build_mapped_gang(amk_kd *obs_pool, amk_kd *edge_pool, int n_frames, int frame_scenes, const float *const *d_xyz,
                         const int *const *d_counts, const float *const *d_edge_xyz, const int *const *d_edge_counts, int point_stride,
                         const int *d_out_scene, hipStream_t stream) {
    if (!obs_pool || !edge_pool || n_frames < 1 || n_frames > AMK_PIPELINE_MAX_GANG || frame_scenes < 1 || !d_out_scene || point_stride < 3)
        return AMK_ERR_INVALID_ARG;
    const int st = pool_planes(obs_pool);
    if (st != AMK_OK) return st;
    BuildArgs2 args{};
    for (int f = 0; f < n_frames; ++f) {
        if (!d_xyz[f] || !d_edge_xyz[f]) return AMK_ERR_INVALID_ARG;
        BuildArgs a = build_args(obs_pool, d_xyz[f], point_stride, (long long)obs_pool->max_points * point_stride, d_counts[f]);
        BuildArgs b = build_args(edge_pool, d_edge_xyz[f], point_stride, (long long)edge_pool->max_points * point_stride, d_edge_counts[f]);
        a.out_scene = b.out_scene = d_out_scene + (size_t)f * frame_scenes;
        a.soa_x = obs_pool->x.p; a.soa_y = obs_pool->y.p; a.soa_z = obs_pool->z.p;
        if (edge_pool->pool_exact) { b.soa_x = edge_pool->x.p; b.soa_y = edge_pool->y.p; b.soa_z = edge_pool->z.p; }   // (the edge trees are built from them)
        args.t[2 * f] = a; args.t[2 * f + 1] = b;
    }
    {
        amk::TimedLaunch tg(amk::KC_GRID, stream);
        hipLaunchKernelGGL(kd_build_kernel, dim3(frame_scenes, 2 * n_frames), dim3(kCompactThreads), 0, stream, args);
    }
    AMK_HIP(hipGetLastError());
    for (amk_kd *kd : {obs_pool, edge_pool}) { kd->soa_valid = 0; kd->ex_valid = 0; kd->async_pending = 1; }
    return AMK_OK;
}
// one frame of n_in scenes: a gang of one
int kd_build_mapped(amk_kd *obs_pool, amk_kd *edge_pool, int n_in, const float *d_xyz, const int *d_counts,
                    const float *d_edge_xyz, const int *d_edge_counts, int point_stride, const int *d_out_scene,
                    hipStream_t stream) {
    return kd_build_mapped_gang(obs_pool, edge_pool, 1, n_in, &d_xyz, &d_counts, &d_edge_xyz, &d_edge_counts, point_stride,
                                d_out_scene, stream);
}
}  // namespace amk

// index-ordered planes from the bucket records (position -> cloud index), NaN padding behind them
__global__ __launch_bounds__(256) void kd_records_to_soa_kernel(const float4 *__restrict__ GP, const int *__restrict__ sizes,
                                                                float *__restrict__ X, float *__restrict__ Y,
                                                                float *__restrict__ Z, int cap) {
    const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= cap) return;
    const size_t base = (size_t)s * cap;
    if (i < sizes[s]) {
        const float4 r = GP[base + i];
        const int idx = __float_as_int(r.w);
        X[base + idx] = r.x; Y[base + idx] = r.y; Z[base + idx] = r.z;
    } else {
        const float qnan = __builtin_nanf("");
        X[base + i] = qnan; Y[base + i] = qnan; Z[base + i] = qnan;
    }
}

// makes the SoA planes of `kd` valid on `stream` (no-op when they already are)
int ensure_soa(amk_kd *kd, hipStream_t stream) {
    if (kd->soa_valid) return AMK_OK;
    if (const int st = amk::pool_planes(kd); st != AMK_OK) return st;
    if (kd->cap > 0)
        hipLaunchKernelGGL(kd_records_to_soa_kernel, dim3((kd->cap + 255) / 256, kd->n_scenes), dim3(256), 0, stream,
                           kd->gpt.p, kd->size.p, kd->x.p, kd->y.p, kd->z.p, kd->cap);
    AMK_HIP(hipGetLastError());
    kd->soa_valid = 1;
    return AMK_OK;
}
extern "C" int amk__kd_ensure_soa(amk_kd *kd, void *stream) { return kd ? ensure_soa(kd, (hipStream_t)stream) : AMK_ERR_INVALID_ARG; }

// ------------------------------------------------------------------------------------------------
// search: one wavefront per (scene, group of QPW queries); device scan in kd_device.h
// ------------------------------------------------------------------------------------------------
template <int QPW>
__global__ __launch_bounds__(512) void kd_scan_kernel(
    const float *__restrict__ X, const float *__restrict__ Y, const float *__restrict__ Z, int cap,
    const int *__restrict__ sizes, const float *__restrict__ pmaxs, int n_scenes,
    const double *__restrict__ queries, int n_queries, int k, int *__restrict__ out_idx,
    double *__restrict__ out_d2, float *__restrict__ out_pts, int *__restrict__ out_cnt) {
    // One wavefront per (scene, group of QPW queries); the waves of a block are consecutive groups of
    // ONE scene, so they stream the same tiles at the same pace (wave_slot, kd_device.h).
    const int groups = (n_queries + QPW - 1) / QPW;
    const int wpb = blockDim.x >> 6;
    const amk::WaveSlot m = amk::wave_slot(groups, wpb);
    const int s = m.s, w = m.w, g = m.unit, lane = m.lane;
    if (s >= n_scenes || g >= groups) return;
    const int size = sizes[s];
    const float *xs = X + (size_t)s * cap, *ys = Y + (size_t)s * cap, *zs = Z + (size_t)s * cap;

    extern __shared__ __attribute__((aligned(16))) unsigned char scan_smem[];
    amk::ScanLds<QPW> *ws = reinterpret_cast<amk::ScanLds<QPW> *>(scan_smem) + w;
    double *qt = reinterpret_cast<double *>(reinterpret_cast<amk::ScanLds<QPW> *>(scan_smem) + wpb) + w * QPW * 3;
    const int q0 = g * QPW;
    const int nvalid = n_queries - q0 < QPW ? n_queries - q0 : QPW;
    // stage this group's queries (a ragged tail group pads with copies of its last query; not stored)
    if (lane < QPW * 3) {
        const int qq = lane / 3 < nvalid ? lane / 3 : nvalid - 1;
        qt[lane] = queries[((size_t)s * n_queries + q0 + qq) * 3 + lane % 3];
    }
    amk::scan_cloud<QPW>(xs, ys, zs, size, pmaxs[s], qt, 3, k, ws);

    const int cnt = amk::adaptor_count(size, k);
    for (int qq = 0; qq < nvalid; ++qq) {
        const int li = ws->li[qq][lane];
        amk::store_search_row(out_idx, out_d2, out_pts, out_cnt, (size_t)s * n_queries + q0 + qq, k, lane, cnt, li != amk::kNoIndex, li,
                              ws->ld[qq][lane], [&](int c) { return (c == 0 ? xs : c == 1 ? ys : zs)[li]; });
    }
}

// search over the bucketed index: one wavefront per (scene, query), four queries of a scene per block.
// AUTO (kd_grid_search_auto_kernel, AMK_TIES_AUTO): one more candidate and the tie test on the k + 1 -- the first k are stored as
// without it (the k + 1 nearest in (distance, index) order begin with the k nearest in that order), the row's flag says whether
// nanoflann's list may differ, and a flagged row raises its scene's `need` word for the lazy build behind the launch.
template <bool AUTO>
__device__ __forceinline__ void grid_search_row(const amk::GridPtrs &gpt, const int *sizes, int n_scenes, const double *queries,
    int n_queries, int k, int *out_idx, double *out_d2, float *out_pts, int *out_cnt, int *rowflag, int *need) {
    __shared__ amk::GridWaveLds wl[4];
    const amk::WaveSlot m = amk::wave_slot(n_queries);
    const int s = m.s, q = m.unit, lane = m.lane;
    if (s >= n_scenes || q >= n_queries) return;
    const size_t row = (size_t)s * n_queries + q;
    const double *qp = queries + row * 3;
    double ld;
    int li, lpos;
    const amk::GridScene gs = gpt.scene(s);
    amk::grid_knn(gs, qp[0], qp[1], qp[2], AUTO ? k + 1 : k, ld, li, lpos, &wl[m.w]);
    const int cnt = amk::adaptor_count(sizes[s], k);
    if constexpr (AUTO) {
        const bool any = amk::wave_tie(ld, li, lane, cnt);
        if (lane == 0) {
            rowflag[row] = any;
            if (any) need[s] = 1;   // (every wavefront that raises it stores the same value)
        }
    }
    const float4 rec = gs.pt[lpos];  // lpos = 0 for empty slots: a valid address
    amk::store_search_row(out_idx, out_d2, out_pts, out_cnt, row, k, lane, cnt, li != amk::kNoIndex, li, ld,
                          [&](int c) { return c == 0 ? rec.x : c == 1 ? rec.y : rec.z; });
}
__global__ __launch_bounds__(256) void kd_grid_search_kernel(amk::GridPtrs gpt, const int *__restrict__ sizes, int n_scenes,
    const double *__restrict__ queries, int n_queries, int k, int *__restrict__ out_idx, double *__restrict__ out_d2,
    float *__restrict__ out_pts, int *__restrict__ out_cnt) {
    grid_search_row<false>(gpt, sizes, n_scenes, queries, n_queries, k, out_idx, out_d2, out_pts, out_cnt, nullptr, nullptr);
}
__global__ __launch_bounds__(256) void kd_grid_search_auto_kernel(amk::GridPtrs gpt, const int *__restrict__ sizes, int n_scenes,
    const double *__restrict__ queries, int n_queries, int k, int *__restrict__ out_idx, double *__restrict__ out_d2,
    float *__restrict__ out_pts, int *__restrict__ out_cnt, int *__restrict__ rowflag, int *__restrict__ need) {
    grid_search_row<true>(gpt, sizes, n_scenes, queries, n_queries, k, out_idx, out_d2, out_pts, out_cnt, rowflag, need);
}

// Tie visibility (amk_kd_tie_flags): wave_tie on the k + 1 nearest of every query, among what SearchForNearest(k) returns.
// (Not an instantiation of grid_search_row: it stores nothing else, raises no `need` and reads its queries at a stride.)
__global__ __launch_bounds__(256) void kd_tie_flags_kernel(amk::GridPtrs gpt, const int *__restrict__ sizes, int n_scenes,
    const double *__restrict__ queries, int query_stride, int n_queries, int k, int *__restrict__ out_flags) {
    __shared__ amk::GridWaveLds wl[4];
    const amk::WaveSlot m = amk::wave_slot(n_queries);
    if (m.s >= n_scenes || m.unit >= n_queries) return;
    const size_t row = (size_t)m.s * n_queries + m.unit;
    const double *qp = queries + row * query_stride;
    double ld;
    int li, lpos;
    amk::grid_knn(gpt.scene(m.s), qp[0], qp[1], qp[2], k + 1, ld, li, lpos, &wl[m.w]);
    const bool any = amk::wave_tie(ld, li, m.lane, amk::adaptor_count(sizes[m.s], k));
    if (m.lane == 0) out_flags[row] = any;
}

extern "C" int amk_kd_points_host(amk_kd *kd, float *h_xyz, int *h_sizes) {
    if (!kd || !h_xyz || !h_sizes) return AMK_ERR_INVALID_ARG;
    AMK_HIP(hipDeviceSynchronize());
    if (const int st = ensure_soa(kd, nullptr); st != AMK_OK) return st;
    int st = amk::read_back({{h_sizes, kd->size.p, sizeof(int) * kd->n_scenes}});
    for (int s = 0; s < kd->n_scenes && st == AMK_OK; ++s) {
        const size_t at = (size_t)s * kd->cap;
        st = amk::planes_to_xyz(kd->x.p + at, kd->y.p + at, kd->z.p + at, h_sizes[s], h_xyz + (size_t)s * kd->max_points * 3);
    }
    return st;
}

// internal (tests / benchmarks): 0 = bucketed index (default), 1 = streaming scan
extern "C" int amk__kd_set_mode(amk_kd *kd, int mode) {
    if (!kd) return AMK_ERR_INVALID_ARG;
    kd->mode = mode;
    return AMK_OK;
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

int amk_version(void) { return 100; }

const char *amk_status_string(int status) {
    switch (status) {
        case AMK_OK: return "ok";
        case AMK_ERR_INVALID_ARG: return "invalid argument";
        case AMK_ERR_HIP: return "HIP runtime error";
        case AMK_ERR_NO_DEVICE: return "no HIP device (this library has no CPU fallback)";
        case AMK_ERR_UNSUPPORTED: return "unsupported size";
        case AMK_ERR_TIMEOUT: return "timed out waiting for a collective (amk_shard_wait)";
        default: return "unknown status";
    }
}

int amk_last_hip_error(void) { return amk::g_last_hip_error; }

int amk_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int amk_kd_create(int n_scenes, int max_points, amk_kd **out) {
    if (!out || n_scenes <= 0 || max_points < 0) return AMK_ERR_INVALID_ARG;
    *out = nullptr;
    if (amk_device_count() <= 0) return AMK_ERR_NO_DEVICE;
    amk_kd *kd = new amk_kd();
    kd->n_scenes = n_scenes;
    kd->max_points = max_points;
    kd->cap = amk::round_up(max_points, 256) + 1024;  // NaN padding: full vector loads + 3-tile look-ahead
    const size_t tot = (size_t)n_scenes * kd->cap;
    hipError_t e;
    // the index-ordered planes x/y/z are allocated by ensure_soa, the first time something asks for them
    if ((e = kd->size.alloc(n_scenes)) != hipSuccess ||
        (e = kd->pmax.alloc(n_scenes)) != hipSuccess || (e = hipMemset(kd->pmax.p, 0, sizeof(float) * n_scenes)) != hipSuccess) {
        delete kd;
        return amk::hip_fail(e);
    }
    if ((e = hipMemset(kd->size.p, 0, sizeof(int) * n_scenes)) != hipSuccess ||
        (e = kd->gpt.alloc(tot)) != hipSuccess || (e = kd->bbox.alloc((size_t)n_scenes * 6)) != hipSuccess ||
        (e = kd->cell_start.alloc((size_t)n_scenes * (kd->ntiles = amk::grid_tiles(max_points)) * (amk::kGridMaxCells + 2))) != hipSuccess ||
        (e = kd->gparams.alloc((size_t)n_scenes * amk::kGridParamDoubles)) != hipSuccess ||
        (e = hipMemset(kd->cell_start.p, 0, sizeof(int) * (size_t)n_scenes * kd->ntiles * (amk::kGridMaxCells + 2))) != hipSuccess ||
        (e = hipMemset(kd->gparams.p, 0, sizeof(double) * (size_t)n_scenes * amk::kGridParamDoubles)) != hipSuccess) {
        delete kd;
        return amk::hip_fail(e);
    }
    *out = kd;
    return AMK_OK;
}

int amk_kd_destroy(amk_kd *kd) {
    if (!kd) return AMK_ERR_INVALID_ARG;
    delete kd;
    return AMK_OK;
}

int amk_kd_build(amk_kd *kd, const float *d_xyz, int point_stride, long long scene_stride,
                 const int *d_counts, void *stream) {
    if (!kd || (!d_xyz && kd->max_points > 0) || point_stride < 3 || scene_stride < 0) return AMK_ERR_INVALID_ARG;
    {
        amk::TimedLaunch tg(amk::KC_GRID, (hipStream_t)stream);
        BuildArgs a = build_args(kd, d_xyz, point_stride, scene_stride, d_counts);
        const bool soa = build_writes_soa(kd, a);
        BuildArgs2 args{};
        args.t[0] = a;
        hipLaunchKernelGGL(kd_build_kernel, dim3(kd->n_scenes, 1), dim3(kCompactThreads), 0, (hipStream_t)stream, args);
        kd->soa_valid = soa ? 1 : 0;
        kd->ex_valid = 0;   // the exact tree (if any) describes the previous cloud until exact_build has run
        kd->async_pending = 1;
    }
    AMK_HIP(hipGetLastError());
    return exact_after_index_build(kd, (hipStream_t)stream);
}

int amk_kd_build_pair(amk_kd *obstacle, const float *d_xyz, const int *d_counts, amk_kd *edge, const float *d_edge_xyz,
                      const int *d_edge_counts, int point_stride, void *stream) {
    if (!obstacle || !edge || (!d_xyz && obstacle->max_points > 0) || (!d_edge_xyz && edge->max_points > 0)) return AMK_ERR_INVALID_ARG;
    return amk::kd_build_gang(obstacle, edge, 1, obstacle->n_scenes, &d_xyz, &d_counts, &d_edge_xyz, &d_edge_counts, point_stride,
                              (hipStream_t)stream);   // (a gang of one frame: the same launch, dim3(S, 2))
}

// Internal (csrc/pipeline.hip, gang > 1): the frames of a gang in ONE launch -- frame f's two clouds are built into scenes
// [f * frame_scenes, (f + 1) * frame_scenes) of the two handles (which hold n_frames * frame_scenes scenes); grid.y = (tree, frame).
}  // extern "C"
namespace amk {
int kd_build_gang(amk_kd *obstacle, amk_kd *edge, int n_frames, int frame_scenes, const float *const *d_xyz,
                  const int *const *d_counts, const float *const *d_edge_xyz, const int *const *d_edge_counts, int point_stride,
                  hipStream_t stream, const int *const *d_keep_if_zero) {
    if (!obstacle || !edge || n_frames < 1 || n_frames > AMK_PIPELINE_MAX_GANG || point_stride < 3 ||
        obstacle->n_scenes < n_frames * frame_scenes || edge->n_scenes != obstacle->n_scenes)
        return AMK_ERR_INVALID_ARG;
    {
        amk::TimedLaunch tg(amk::KC_GRID, stream);
        BuildArgs2 args{};
        for (int f = 0; f < n_frames; ++f) {
            const size_t so = (size_t)f * frame_scenes;
            args.t[2 * f] = build_args(obstacle, d_xyz[f], point_stride, (long long)obstacle->max_points * point_stride, d_counts[f], so);
            args.t[2 * f + 1] = build_args(edge, d_edge_xyz[f], point_stride, (long long)edge->max_points * point_stride, d_edge_counts[f], so);
            if (d_keep_if_zero) args.t[2 * f].keep_if_zero = args.t[2 * f + 1].keep_if_zero = d_keep_if_zero[f];
        }
        // (a scene that keeps its previous index keeps planes that may predate the tie-order mode: ensure_soa remakes them all)
        bool soa_o = !d_keep_if_zero, soa_e = !d_keep_if_zero;
        for (int f = 0; f < n_frames; ++f) {
            soa_o = soa_o && build_writes_soa(obstacle, args.t[2 * f], (size_t)f * frame_scenes);
            soa_e = soa_e && build_writes_soa(edge, args.t[2 * f + 1], (size_t)f * frame_scenes);
        }
        if (!soa_o) for (int f = 0; f < n_frames; ++f) args.t[2 * f].soa_x = args.t[2 * f].soa_y = args.t[2 * f].soa_z = nullptr;
        if (!soa_e) for (int f = 0; f < n_frames; ++f) args.t[2 * f + 1].soa_x = args.t[2 * f + 1].soa_y = args.t[2 * f + 1].soa_z = nullptr;
        hipLaunchKernelGGL(kd_build_kernel, dim3(frame_scenes, 2 * n_frames), dim3(kCompactThreads), 0, stream, args);
        obstacle->soa_valid = soa_o ? 1 : 0; edge->soa_valid = soa_e ? 1 : 0;
        for (amk_kd *kd : {obstacle, edge}) {
            kd->ex_valid = 0;
            kd->async_pending = 1;
        }
    }
    AMK_HIP(hipGetLastError());
    for (amk_kd *kd : {obstacle, edge})
        if (const int st = exact_after_index_build(kd, stream); st != AMK_OK) return st;
    return AMK_OK;
}
}  // namespace amk
extern "C" {
int amk_kd_sizes(amk_kd *kd, int *h_sizes, void *stream) {
    if (!kd || !h_sizes) return AMK_ERR_INVALID_ARG;
    AMK_HIP(hipMemcpyAsync(h_sizes, kd->size.p, sizeof(int) * kd->n_scenes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    AMK_HIP(hipStreamSynchronize((hipStream_t)stream));
    return AMK_OK;
}

int amk_kd_search(amk_kd *kd, const double *d_queries, int n_queries, int k, int *d_indices, double *d_sqdist,
                  float *d_pts, int *d_counts, void *stream) {
    if (!kd || !d_queries || n_queries <= 0 || k <= 0) return AMK_ERR_INVALID_ARG;
    if (k > AMK_MAX_K || n_queries > AMK_MAX_QUERIES) return AMK_ERR_UNSUPPORTED;
    if (kd->mode == 0 && kd->tie_order == AMK_TIES_AUTO && k + 1 > AMK_MAX_K) return AMK_ERR_UNSUPPORTED;   // (amk_kd_tie_flags' rule)
    if (kd->auto_on()) {
        // bucketed search with tie detection, lazy build, re-answer of the tied rows: four launches whatever the data holds
        hipLaunchKernelGGL(kd_grid_search_auto_kernel, dim3((unsigned)amk::search_blocks(kd->n_scenes, n_queries)), dim3(256), 0, (hipStream_t)stream, grid_ptrs(kd), kd->size.p,
                           kd->n_scenes, d_queries, n_queries, k, d_indices, d_sqdist, d_pts, d_counts, kd->au_rowflag.p, kd->au_need());
        AMK_HIP(hipGetLastError());
        if (const int st = amk::kd_auto_build(kd, nullptr, (hipStream_t)stream); st != AMK_OK) return st;
        return exact_search(kd, d_queries, n_queries, k, d_indices, d_sqdist, d_pts, d_counts, (hipStream_t)stream);
    }
    if (kd->mode == 0) {
        hipLaunchKernelGGL(kd_grid_search_kernel, dim3((unsigned)amk::search_blocks(kd->n_scenes, n_queries)), dim3(256), 0, (hipStream_t)stream, grid_ptrs(kd), kd->size.p,
                           kd->n_scenes, d_queries, n_queries, k, d_indices, d_sqdist, d_pts, d_counts);
        AMK_HIP(hipGetLastError());
        if (kd->tie_order == AMK_TIES_NANOFLANN && kd->ex_valid)   // nanoflann's own traversal where its tree is available (and current)
            return exact_search(kd, d_queries, n_queries, k, d_indices, d_sqdist, d_pts, d_counts, (hipStream_t)stream);
        return AMK_OK;
    }
    {   // the streaming scan reads the index-ordered planes
        const int st = ensure_soa(kd, (hipStream_t)stream);
        if (st != AMK_OK) return st;
    }
    int qpw, groups, wpb;
    amk::scan_geometry(n_queries, qpw, groups, wpb);
    const unsigned blocks = (unsigned)amk::search_blocks(kd->n_scenes, groups, wpb);
#define AMK_LAUNCH_SCAN(Q)                                                                                      \
    hipLaunchKernelGGL(kd_scan_kernel<Q>, dim3(blocks), dim3(wpb * kWave), amk::scan_lds_bytes<Q>(wpb),          \
                       (hipStream_t)stream, kd->x.p, kd->y.p, kd->z.p, kd->cap, kd->size.p, kd->pmax.p,          \
                       kd->n_scenes, d_queries, n_queries, k, d_indices, d_sqdist, d_pts, d_counts)
    if (qpw == 1) AMK_LAUNCH_SCAN(1);
    else AMK_LAUNCH_SCAN(5);
#undef AMK_LAUNCH_SCAN
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

int amk_kd_tie_flags(amk_kd *kd, const double *d_queries, int query_stride, int n_queries, int k, int *d_tie_flags,
                     void *stream) {
    if (!kd || !d_queries || !d_tie_flags || n_queries <= 0 || k <= 0 || query_stride < 3) return AMK_ERR_INVALID_ARG;
    if (k + 1 > AMK_MAX_K || n_queries > AMK_MAX_QUERIES) return AMK_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(kd_tie_flags_kernel, dim3((unsigned)amk::search_blocks(kd->n_scenes, n_queries)), dim3(256), 0, (hipStream_t)stream, grid_ptrs(kd), kd->size.p, kd->n_scenes,
                       d_queries, query_stride, n_queries, k, d_tie_flags);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

int amk_kd_build_host(amk_kd *kd, const float *h_xyz, int point_stride, long long scene_stride, const int *h_counts) {
    if (!kd || (!h_xyz && kd->max_points > 0) || point_stride < 3) return AMK_ERR_INVALID_ARG;
    const long long min_stride = (long long)kd->max_points * point_stride;
    if (scene_stride < min_stride && kd->n_scenes > 1) return AMK_ERR_INVALID_ARG;
    const size_t S = kd->n_scenes, tot = (S - 1) * scene_stride + (size_t)min_stride;
    for (size_t s = 0; h_counts && s < S; ++s)
        if (h_counts[s] < 0 || h_counts[s] > kd->max_points) return AMK_ERR_INVALID_ARG;
    enum { XYZ, COUNTS };
    // with counts, only the points every scene holds go over (the caller's buffer need not extend to the capacity): the launch copies them
    const int st = kd->stage.call(
        {!h_counts && tot > 0 ? amk::to_device(h_xyz, sizeof(float) * tot) : amk::scratch(sizeof(float) * (tot > 0 ? tot : 1)),
         amk::if_given(amk::to_device(h_counts, sizeof(int) * S))},
        [&](const amk::HostStage::Dev *d) {
            float *d_xyz = d[XYZ];
            for (size_t s = 0; h_counts && s < S; ++s)
                if (const size_t nf = (size_t)h_counts[s] * point_stride)
                    AMK_HIP(hipMemcpy(d_xyz + s * scene_stride, h_xyz + s * scene_stride, nf * sizeof(float), hipMemcpyHostToDevice));
            return amk_kd_build(kd, d_xyz, point_stride, scene_stride, d[COUNTS], nullptr);
        },
        hipDeviceSynchronize);
    if (st == AMK_OK) kd->async_pending = 0;
    return st;
}

int amk_kd_search_host(amk_kd *kd, const double *h_queries, int n_queries, int k, int *h_indices, double *h_sqdist,
                       float *h_pts, int *h_counts) {
    if (!kd || !h_queries || n_queries <= 0 || k <= 0) return AMK_ERR_INVALID_ARG;
    if (k > AMK_MAX_K || n_queries > AMK_MAX_QUERIES) return AMK_ERR_UNSUPPORTED;
    if (kd->mode == 0 && kd->tie_order == AMK_TIES_AUTO && k + 1 > AMK_MAX_K) return AMK_ERR_UNSUPPORTED;   // (before anything is staged)
    if (const int st = amk::kd_order_behind_pending(kd); st != AMK_OK) return st;
    const size_t rows = (size_t)kd->n_scenes * n_queries;
    enum { QUERIES, SQDIST, INDICES, COUNTS, PTS };
    return kd->stage.call_pinned({amk::to_device(h_queries, rows * 3 * sizeof(double)), amk::to_host(h_sqdist, rows * k * sizeof(double)),
                                  amk::to_host(h_indices, rows * k * sizeof(int)), amk::to_host(h_counts, rows * sizeof(int)),
                                  amk::to_host(h_pts, rows * k * 3 * sizeof(float))},
                                 [&](const amk::HostStage::Dev *d, hipStream_t stream) {
                                     return amk_kd_search(kd, d[QUERIES], n_queries, k, d[INDICES], d[SQDIST], d[PTS], d[COUNTS], stream);
                                 });
}

// Internal (not in include/avoid_mpc_amd.h; tests/test_host_stage.py), host only, needs no device: where HostStage puts n slots of
// bytes[i] -- offsets[n], and total = the block that holds them
int amk__stage_layout(const long long *bytes, int n, long long *offsets, long long *total) {
    if (n < 0 || !total || (n > 0 && (!bytes || !offsets))) return AMK_ERR_INVALID_ARG;
    size_t end = 0;
    for (int i = 0; i < n; ++i) {
        if (bytes[i] < 0) return AMK_ERR_INVALID_ARG;
        offsets[i] = (long long)amk::stage_next(end, (size_t)bytes[i]);
    }
    *total = (long long)end;
    return AMK_OK;
}

}  // extern "C"
