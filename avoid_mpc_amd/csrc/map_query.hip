// FrameKDMap's own queries over a MULTI-FRAME map, for a batch of scenes on gfx950, outside any control step:
//   QueryNearest (AM/src/FrameKDMap.cpp:254-376)       amk_kfmap_query_nearest / amk_kd_query_frames
//   GetNearestDistance (:378-427)                       amk_kfmap_nearest_distance / amk_kd_nearest_distance_frames
// The rules are the ones the step applies to its reference points (step_frames.hip; written out in
// include/avoid_mpc_amd.h, "The map's own queries"), answered here for any points, any k <= AMK_MAX_K and any
// number of queries, from the map as it stands -- no amk_mpc, no staging of per-frame rows, no workspace.
//
// map_query_kernel: one wavefront per (scene, query).  It decides fast path or merge from the numbers the step uses (size of
// frame 0, PtIsInFrame with contraction off), walks the frames its scene holds, runs grid_knn in every frame that contributes and
// folds that frame's sorted k-list into a running sorted k-list held one entry per lane (distance, point, frame).  The fold is the
// insertion grid_knn itself uses: the frame's entries are offered best first, an entry ranks behind every kept entry at the same or
// a smaller distance (kept entries came from an earlier frame or are earlier neighbours of this one: the tie rule), and the
// fold of a frame ends at its first entry that ranks behind the k-th kept one -- every later one is no nearer.  On a map whose
// running list is full of near points a frame that holds nothing nearer costs ONE rank (a ballot and a population count).
#include "step_common.h"
#include "kd_path_cast.h"

using namespace amk;

namespace {

struct QueryFrames {  // kernel argument: the frames of ONE kind of cloud (obstacle or edge)
    GridPtrs g[AMK_MAX_FRAMES];
    const int *size[AMK_MAX_FRAMES];
    FrameMap map;  // a keyframe map: the pool is g[0] / size[0]
};

__device__ __forceinline__ float wave_shr1_f32(float v) { return __int_as_float(wave_shr1_i32(__float_as_int(v))); }

// One frame's sorted k-list for the fold (lane i < k: squared distance nd, DBL_MAX where there is none, and the point).
// EXACT (a keyframe map in AMK_TIES_NANOFLANN): nanoflann's list from the pool scene's tree; a scene without a tree (given up,
// too deep) keeps the bucketed index's, as a plain handle does.
template <bool EXACT>
__device__ __forceinline__ void frame_list(const GridScene &gs, const ExactPtrs &ex, int m, double qx, double qy, double qz, int k, int lane,
                                           GridWaveLds *wl, double &nd, float4 &rec) {
    if constexpr (EXACT) {
        __shared__ ExactWaveStack xst[4];
        const ExactTree T = ex.scene(m);
        double xd;
        int xi;
        const int got = exact_knn_wave(T, qx, qy, qz, k, xd, xi, &xst[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)]);
        if (got >= 0) {   // (wave-uniform)
            const bool ok = lane < got;
            nd = ok ? xd : DBL_MAX;
            rec = ok ? make_float4(T.x[xi], T.y[xi], T.z[xi], 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
            return;
        }
    }
    double ld;
    int li, lpos;
    grid_knn(gs, qx, qy, qz, k, ld, li, lpos, wl);
    rec = gs.pt[lpos];   // (lpos = 0 for empty slots: a valid address)
    nd = (lane < k && li != kNoIndex) ? ld : DBL_MAX;
}

// Folds one frame's sorted list (frame_list's nd / rec, frame number f) into the running list held one entry per lane < k: the
// frame's entries are offered best first, an entry ranks behind every kept one at the same or a smaller distance (kept entries came
// from an earlier frame or are earlier neighbours of this one: the tie rule), and the fold ends at the first entry that ranks
// behind the k-th kept one.  WITH_T (the segment search): every entry carries a further payload, its t (nt in the frame's list, rt
// in the running one); without it the two are never touched.
template <bool WITH_T = false>
__device__ __forceinline__ void fold_frame_list(double nd, const float4 &rec, int f, int k, int lane, double &rd, float &rx, float &ry,
                                                float &rz, int &rf, double nt = 0.0, double *rt = nullptr) {
    for (int e = 0; e < k; ++e) {     // this frame's entries, best first
        const double dc = readlane_f64(nd, e);
        if (!(dc < DBL_MAX)) break;
        // rank among the kept entries: behind every one at the same or a smaller distance
        const int pos = __popcll(__ballot((lane < k) & (rd <= dc)));
        if (pos >= k) break;          // (the entries behind it are no nearer)
        const float cx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rec.x), e));
        const float cy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rec.y), e));
        const float cz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rec.z), e));
        const double up_d = wave_shr1_f64(rd);
        const float up_x = wave_shr1_f32(rx), up_y = wave_shr1_f32(ry), up_z = wave_shr1_f32(rz);
        const int up_f = wave_shr1_i32(rf);
        const bool above = lane > pos, here = lane == pos;   // selects, not branches
        rd = here ? dc : (above ? up_d : rd);
        rx = here ? cx : (above ? up_x : rx);
        ry = here ? cy : (above ? up_y : ry);
        rz = here ? cz : (above ? up_z : rz);
        rf = here ? f : (above ? up_f : rf);
        if constexpr (WITH_T) {
            const double ct = readlane_f64(nt, e), up_t = wave_shr1_f64(*rt);
            *rt = here ? ct : (above ? up_t : *rt);
        }
    }
}

// The frame walk every kernel below shares.  frames_held: one past the last frame scene s holds -- asked ONCE per wavefront, by all
// of its lanes, ahead of any lane-dependent branch and of the walk (the path cast walks once per leg and asks once per block).
// for_each_frame: the frames below F that the scene holds, in order: visit(f, m, gs) -- frame f, which scene m of its handle it is
// (MAP, a keyframe map: of the pool; a frame the scene's map does not hold is passed over) and that scene's index -- for as long
// as more() holds, asked ahead of every frame (the casts: nothing can begin earlier than a contact at t = 0).
template <bool MAP>
__device__ __forceinline__ int frame_scene(const QueryFrames &qf, int f, int s) { return MAP ? qf.map.pool_scene(f, s) : s; }   // (< 0: absent)
template <bool MAP>
__device__ __forceinline__ int frames_held(const QueryFrames &qf, int s, int lane) { return MAP ? qf.map.held(s, lane) : qf.map.n; }
struct EveryFrame { __device__ bool operator()() const { return true; } };
template <bool MAP, class Visit, class More = EveryFrame>
__device__ __forceinline__ void for_each_frame(const QueryFrames &qf, int s, int F, Visit &&visit, More &&more = More{}) {
    const GridPtrs pool = qf.g[0];   // (map mode: one set of pool pointers stays live over the loop)
    for (int f = 0; f < F && more(); ++f) {
        const int m = frame_scene<MAP>(qf, f, s);
        if (m < 0) continue;         // (map mode: this scene's map has no frame f)
        visit(f, m, (MAP ? pool : qf.g[f]).scene(m));
    }
}

// DIST: GetNearestDistance -- the same walk with k = 1 and no fast path; out_dist = sqrt of the best squared distance
template <bool MAP, bool DIST, bool EXACT>
__device__ __forceinline__ void map_query_row(const QueryFrames &qf, const ExactPtrs &ex, int n_scenes, const double *__restrict__ queries,
                                              int query_stride, int n_queries, int k_in,
                                              const double *__restrict__ Twc, const amk_frame_camera &cam,
                                              float *__restrict__ out_pts, double *__restrict__ out_d2,
                                              int *__restrict__ out_frame, int *__restrict__ out_cnt,
                                              double *__restrict__ out_dist) {
    __shared__ GridWaveLds wl[4];
    const RowSlot r = row_slot(queries, query_stride, n_queries, n_queries);
    const int s = r.ws.s, w = r.ws.w, lane = r.ws.lane;
    if (!r.in(n_scenes)) return;
    const int k = DIST ? 1 : k_in;
    const double qx = r.p[0], qy = r.p[1], qz = r.p[2];
    const int F = frames_held<MAP>(qf, s, lane);
    auto size_of = [&](int f, int m) { return (MAP ? qf.size[0] : qf.size[f])[m]; };

    double rd = DBL_MAX;             // the running list: lane i < k holds the i-th best (distance, point, frame) so far
    float rx = 0.f, ry = 0.f, rz = 0.f;
    int rf = -1, cnt = 0;
    bool fast = false;
    if (!DIST && F > 0) {            // QueryNearestWithCurFrame (:254-275, 339-345)
        const int m0 = frame_scene<MAP>(qf, 0, s);
        const int n0 = m0 < 0 ? 0 : size_of(0, m0);
        fast = n0 >= k && (!Twc || pt_in_frame(Twc + (size_t)s * 16, cam, qx, qy, qz));
        if (fast) {
            const GridScene gs = qf.g[0].scene(m0);
            cnt = adaptor_count(n0, k);   // (n0 >= k here: k, or nothing from a cloud of exactly k points)
            if constexpr (EXACT) {
                double nd;
                float4 rec;
                frame_list<true>(gs, ex, m0, qx, qy, qz, k, lane, &wl[w], nd, rec);
                if (lane < cnt && nd < DBL_MAX) { rd = nd; rx = rec.x; ry = rec.y; rz = rec.z; rf = 0; }
            } else {
                double ld;
                int li, lpos;
                grid_knn(gs, qx, qy, qz, k, ld, li, lpos, &wl[w]);
                if (lane < cnt && li != kNoIndex) {
                    const float4 rec = gs.pt[lpos];
                    rd = ld; rx = rec.x; ry = rec.y; rz = rec.z; rf = 0;
                }
            }
        }
    }
    if (!fast) {                     // QueryNearestThreadWorker over mVecQueryVector (:276-321) + sort by distance (:371-375)
        for_each_frame<MAP>(qf, s, F, [&](int f, int m, const GridScene &gs) {
            if (size_of(f, m) <= k) return;   // k' = min(k, size_f) results exist iff size_f > k'
            double nd;
            float4 rec;
            frame_list<EXACT>(gs, ex, m, qx, qy, qz, k, lane, &wl[w], nd, rec);
            fold_frame_list(nd, rec, f, k, lane, rd, rx, ry, rz, rf);
        });
        cnt = __popcll(__ballot((lane < k) & (rd < DBL_MAX)));
    }
    if (DIST) {
        if (lane == 0) out_dist[r.row] = sqrt(rd);   // (no frame answered: sqrt(DBL_MAX), :381,426)
        return;
    }
    write_list_row<false>(r.row, k, lane, cnt, rd < DBL_MAX, rd, 0.0, [&] { return make_float4(rx, ry, rz, 0.f); }, rf, out_cnt, out_d2,
                          nullptr, out_frame, out_pts);
}
template <bool MAP, bool DIST>
__global__ __launch_bounds__(256) void map_query_kernel(QueryFrames qf, int n_scenes, const double *__restrict__ queries,
                                                        int query_stride, int n_queries, int k_in,
                                                        const double *__restrict__ Twc, amk_frame_camera cam,
                                                        float *__restrict__ out_pts, double *__restrict__ out_d2,
                                                        int *__restrict__ out_frame, int *__restrict__ out_cnt,
                                                        double *__restrict__ out_dist) {
    map_query_row<MAP, DIST, false>(qf, ExactPtrs{}, n_scenes, queries, query_stride, n_queries, k_in, Twc, cam, out_pts, out_d2, out_frame,
                                    out_cnt, out_dist);
}
// QueryNearest over a keyframe map in AMK_TIES_NANOFLANN: every contributing frame's list by nanoflann's traversal of its tree
__global__ __launch_bounds__(256) void map_query_exact_kernel(QueryFrames qf, ExactPtrs ex, int n_scenes, const double *__restrict__ queries,
                                                              int query_stride, int n_queries, int k_in,
                                                              const double *__restrict__ Twc, amk_frame_camera cam,
                                                              float *__restrict__ out_pts, double *__restrict__ out_d2,
                                                              int *__restrict__ out_frame, int *__restrict__ out_cnt) {
    map_query_row<true, false, true>(qf, ex, n_scenes, queries, query_stride, n_queries, k_in, Twc, cam, out_pts, out_d2, out_frame,
                                     out_cnt, nullptr);
}

template <bool DIST>
int launch_query(const QueryFrames &qf, int S, const double *d_queries, int query_stride, int n_queries, int k, const double *d_Twc,
                 const amk_frame_camera *cam, float *d_pts, double *d_sqdist, int *d_frame, int *d_counts, double *d_dist,
                 hipStream_t stream, const ExactPtrs *ex = nullptr) {
    const long long blocks = search_blocks(S, n_queries);
    if (blocks > 0x7fffffffll) return AMK_ERR_UNSUPPORTED;
    amk_frame_camera c{};
    if (cam) c = *cam;
    if (ex) {   // (a keyframe map in AMK_TIES_NANOFLANN; never GetNearestDistance: a distance does not depend on the order of ties)
        hipLaunchKernelGGL(map_query_exact_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, qf, *ex, S, d_queries, query_stride, n_queries,
                           k, d_Twc, c, d_pts, d_sqdist, d_frame, d_counts);
        AMK_HIP(hipGetLastError());
        return AMK_OK;
    }
    auto kernel = qf.map.fmap ? map_query_kernel<true, DIST> : map_query_kernel<false, DIST>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, stream, qf, S, d_queries, query_stride, n_queries, k, d_Twc, c,
                       d_pts, d_sqdist, d_frame, d_counts, d_dist);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

// a caller's list of frame handles -> the kernel's argument and the scenes, or a status (the header's rules, before anything is
// launched).  default_ties_only: the multi-frame kNN queries and casts answer in the default tie order only; the list queries'
// results have no tie-order modes
struct HandleFrames {
    int status;
    QueryFrames qf;
    int S;
};
HandleFrames frames_of_handles(amk_kd *const *frames, int n_frames, bool default_ties_only = true) {
    HandleFrames h{AMK_OK, QueryFrames{}, 0};
    auto refused = [&](int status) { h.status = status; return h; };
    if (!frames || n_frames < 1) return refused(AMK_ERR_INVALID_ARG);
    if (n_frames > AMK_MAX_FRAMES) return refused(AMK_ERR_UNSUPPORTED);
    for (int f = 0; f < n_frames; ++f)
        if (!frames[f] || frames[f]->n_scenes != frames[0]->n_scenes) return refused(AMK_ERR_INVALID_ARG);
    h.S = frames[0]->n_scenes;
    h.qf.map = FrameMap{n_frames, nullptr, h.S};
    for (int f = 0; f < n_frames; ++f) {
        if (frames[f]->mode != 0 || (default_ties_only && frames[f]->tie_order != AMK_TIES_LOWEST_INDEX)) return refused(AMK_ERR_UNSUPPORTED);
        h.qf.g[f] = grid_ptrs(frames[f]);
        h.qf.size[f] = frames[f]->size.p;
    }
    return h;
}
// The *_frames_host entries: host(stage, S) stages through a block of its own, freed at return -- these frames belong to no one handle
template <class Host>
int frames_host(amk_kd *const *frames, int n_frames, bool default_ties_only, Host &&host) {
    const HandleFrames h = frames_of_handles(frames, n_frames, default_ties_only);
    if (h.status != AMK_OK) return h.status;
    amk::HostStage stage;
    return host(stage, h.S);
}

bool pool_args_ok(const amk_kd *pool, const int *d_fmap, int n_frames, int S) { return pool && d_fmap && n_frames >= 1 && S >= 1; }
QueryFrames frames_of_pool(amk_kd *pool, int n_frames, const int *d_fmap, int S) {
    QueryFrames qf{};
    qf.map = FrameMap{n_frames, d_fmap, S};
    qf.g[0] = grid_ptrs(pool);
    qf.size[0] = pool->size.p;
    return qf;
}

// The launch of a kernel with one wavefront per (scene, unit) (wave_slot): its keyframe-map or its list-of-handles instantiation,
// whichever qf describes, with (qf, S, args...)
template <class Kernel, class... Args>
int launch_rows(Kernel map_kernel, Kernel handles_kernel, const QueryFrames &qf, int S, int units, hipStream_t stream, Args... args) {
    const long long blocks = search_blocks(S, units);
    if (blocks > 0x7fffffffll) return AMK_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(qf.map.fmap ? map_kernel : handles_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, qf, S, args...);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

// Radius search over the frames (amk_kfmap_radius_search / amk_kd_radius_search_frames): one wavefront per (scene, query) walks
// every frame its scene holds -- no fast path, no PtIsInFrame, no size rule: those belong to QueryNearest -- with grid_radius; the
// counts add up, each frame's list is folded into the running list as above (equal distances keep the earlier frame, then the
// lower index within a frame).
template <bool MAP>
__global__ __launch_bounds__(256) void map_radius_kernel(QueryFrames qf, int n_scenes, const double *__restrict__ queries,
                                                         int query_stride, int n_queries, double r2, int k,
                                                         float *__restrict__ out_pts, double *__restrict__ out_d2,
                                                         int *__restrict__ out_frame, int *__restrict__ out_cnt) {
    __shared__ GridWaveLds wl[4];
    const RowSlot r = row_slot(queries, query_stride, n_queries, n_queries);
    const int s = r.ws.s, w = r.ws.w, lane = r.ws.lane;
    if (!r.in(n_scenes)) return;
    const double qx = r.p[0], qy = r.p[1], qz = r.p[2];
    const int F = frames_held<MAP>(qf, s, lane);
    double rd = DBL_MAX;             // the running list: lane i < k holds the i-th best (distance, point, frame) so far
    float rx = 0.f, ry = 0.f, rz = 0.f;
    int rf = -1, cnt = 0;
    for_each_frame<MAP>(qf, s, F, [&](int f, int, const GridScene &gs) {
        double ld;
        int li, lpos;
        cnt += grid_radius(gs, qx, qy, qz, r2, k, ld, li, lpos, &wl[w]);
        if (k > 0) {
            const float4 rec = gs.pt[lpos];   // (lpos = 0 for empty slots: a valid address)
            fold_frame_list((lane < k && li != kNoIndex) ? ld : DBL_MAX, rec, f, k, lane, rd, rx, ry, rz, rf);
        }
    });
    write_list_row<false>(r.row, k, lane, cnt, rd < DBL_MAX, rd, 0.0, [&] { return make_float4(rx, ry, rz, 0.f); }, rf, out_cnt, out_d2,
                          nullptr, out_frame, out_pts);
}

// Segment search over the frames (amk_kfmap_segment_search / amk_kd_segment_search_frames): one wavefront per (scene, leg) walks
// every frame its scene holds with grid_segment, as map_radius_kernel does with grid_radius -- the counts add up, each frame's list
// is folded into the running list with its t (equal distances keep the earlier frame, then the lower index within a frame).
template <bool MAP>
__global__ __launch_bounds__(256) void map_segment_kernel(QueryFrames qf, int n_scenes, const double *__restrict__ path,
                                                          int point_stride, int n_points, double r2, int k,
                                                          float *__restrict__ out_pts, double *__restrict__ out_d2,
                                                          double *__restrict__ out_t, int *__restrict__ out_frame,
                                                          int *__restrict__ out_cnt) {
    __shared__ GridWaveLds wl[4];
    const RowSlot r = row_slot(path, point_stride, n_points, n_points - 1);
    const int s = r.ws.s, w = r.ws.w, lane = r.ws.lane;
    if (!r.in(n_scenes)) return;
    const SegLeg leg = seg_leg(r.p, r.p + point_stride);
    const int F = frames_held<MAP>(qf, s, lane);
    double rd = DBL_MAX, rt = 0.0;   // the running list: lane i < k holds the i-th best (distance, t, point, frame) so far
    float rx = 0.f, ry = 0.f, rz = 0.f;
    int rf = -1, cnt = 0;
    for_each_frame<MAP>(qf, s, F, [&](int f, int, const GridScene &gs) {
        double ld, lt;
        int li, lpos;
        cnt += grid_segment(gs, leg, r2, k, ld, li, lpos, lt, &wl[w]);
        if (k > 0) {
            const float4 rec = gs.pt[lpos];   // (lpos = 0 for empty slots: a valid address)
            fold_frame_list<true>((lane < k && li != kNoIndex) ? ld : DBL_MAX, rec, f, k, lane, rd, rx, ry, rz, rf, lt, &rt);
        }
    });
    write_list_row<true>(r.row, k, lane, cnt, rd < DBL_MAX, rd, rt, [&] { return make_float4(rx, ry, rz, 0.f); }, rf, out_cnt, out_d2,
                         out_t, out_frame, out_pts);
}

// Segment nearest over the frames (amk_kfmap_segment_nearest / amk_kd_segment_nearest_frames): one wavefront per (scene, leg) walks
// every frame its scene holds with grid_segment_knn and folds each frame's k nearest into the running list with their t, as
// map_segment_kernel does (equal distances keep the earlier frame, then the lower index within a frame).  Every frame's walk
// starts unbounded: the k nearest of all frames are among the frames' own k nearest, whatever the other frames hold.  The count is
// min(k, sum of the frames' kept entries) = min(k, sum of their usable points).
template <bool MAP>
__global__ __launch_bounds__(256) void map_segment_nearest_kernel(QueryFrames qf, int n_scenes, const double *__restrict__ path,
                                                                  int point_stride, int n_points, int k, float *__restrict__ out_pts,
                                                                  double *__restrict__ out_d2, double *__restrict__ out_t,
                                                                  int *__restrict__ out_frame, int *__restrict__ out_cnt) {
    __shared__ GridWaveLds wl[4];
    const RowSlot r = row_slot(path, point_stride, n_points, n_points - 1);
    const int s = r.ws.s, w = r.ws.w, lane = r.ws.lane;
    if (!r.in(n_scenes)) return;
    const SegLeg leg = seg_leg(r.p, r.p + point_stride);
    const int F = frames_held<MAP>(qf, s, lane);
    double rd = DBL_MAX, rt = 0.0;   // the running list: lane i < k holds the i-th best (distance, t, point, frame) so far
    float rx = 0.f, ry = 0.f, rz = 0.f;
    int rf = -1, cnt = 0;
    for_each_frame<MAP>(qf, s, F, [&](int f, int, const GridScene &gs) {
        double ld, lt;
        int li, lpos;
        cnt += grid_segment_knn(gs, leg, k, ld, li, lpos, lt, &wl[w]);
        const float4 rec = gs.pt[lpos];   // (lpos = 0 for empty slots: a valid address)
        fold_frame_list<true>((lane < k && li != kNoIndex) ? ld : DBL_MAX, rec, f, k, lane, rd, rx, ry, rz, rf, lt, &rt);
    });
    write_list_row<true>(r.row, k, lane, min(cnt, k), rd < DBL_MAX, rd, rt, [&] { return make_float4(rx, ry, rz, 0.f); }, rf, out_cnt, out_d2,
                         out_t, out_frame, out_pts);
}

// One leg's cast over the frames scene s holds, for map_segment_cast_kernel and map_path_cast_kernel: the least (t, frame, index)
// -- a plain minimum, no list to fold.  Unlike segment nearest the running best bounds the next frame's walk: grid_cast takes it
// as tcap, counts only contacts strictly below it (an equal t keeps the earlier frame) and ends that frame's walk where nothing
// can begin earlier; after a contact at t = 0 the remaining frames are not walked at all.  True: a contact, in rt (wave-uniform;
// 1.0 without one), its frame rf (-1) and the point touched (left as the caller set it: zeros).
template <bool MAP>
__device__ __forceinline__ bool cast_frames(const QueryFrames &qf, int s, int F, const SegLeg &leg, double r2, GridWaveLds *wl,
                                            double &rt, int &rf, float &rx, float &ry, float &rz) {
    rt = 1.0;   // the first contact so far
    rf = -1;
    for_each_frame<MAP>(qf, s, F, [&](int f, int, const GridScene &gs) {
        double bt;
        int bi, bpos;
        if (grid_cast(gs, leg, r2, rt, bt, bi, bpos, wl)) {   // (wave-uniform)
            const float4 rec = gs.pt[bpos];
            rt = bt; rx = rec.x; ry = rec.y; rz = rec.z; rf = f;
        }
    }, [&] { return rt > 0.0; });
    return rf >= 0;
}

// Segment cast over the frames (amk_kfmap_segment_cast / amk_kd_segment_cast_frames): one wavefront per (scene, leg), cast_frames
template <bool MAP>
__global__ __launch_bounds__(256) void map_segment_cast_kernel(QueryFrames qf, int n_scenes, const double *__restrict__ path,
                                                               int point_stride, int n_points, double r2, int *__restrict__ out_hit,
                                                               double *__restrict__ out_t, float *__restrict__ out_pts,
                                                               int *__restrict__ out_frame) {
    __shared__ GridWaveLds wl[4];
    const RowSlot r = row_slot(path, point_stride, n_points, n_points - 1);
    if (!r.in(n_scenes)) return;
    const SegLeg leg = seg_leg(r.p, r.p + point_stride);
    double rt;
    float rx = 0.f, ry = 0.f, rz = 0.f;
    int rf;
    const bool hit = cast_frames<MAP>(qf, r.ws.s, frames_held<MAP>(qf, r.ws.s, r.ws.lane), leg, r2, &wl[r.ws.w], rt, rf, rx, ry, rz);
    write_cast_row(r.row, r.ws.lane, hit, rt, rx, ry, rz, rf, out_hit, out_t, out_frame, out_pts);
}

// Path cast over the frames (amk_kfmap_path_cast / amk_kd_path_cast_frames): kd_path_cast_kernel's block per scene and rounds
// (path_cast_scene, kd_path_cast.h, with the barrier rules; the only return before it is the whole-block one), a leg's wave
// folding the frames exactly as map_segment_cast_kernel does, inside the per-leg call.
template <bool MAP, int W>
__global__ __launch_bounds__(64 * W) void map_path_cast_kernel(QueryFrames qf, int n_scenes, const double *__restrict__ path,
                                                               int point_stride, long long scene_stride, int n_points, double r2,
                                                               PathCastOut out) {
    __shared__ PathCastLds<W> lds;
    const int s = blockIdx.x;
    if (s >= n_scenes) return;   // (the whole block)
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int F = frames_held<MAP>(qf, s, lane);   // (once, ahead of the rounds)
    path_cast_scene<W>(s, path + (size_t)s * scene_stride, point_stride, n_points - 1, lds, out,
                       [&](const SegLeg &leg, double &rt, int &rf, float &rx, float &ry, float &rz) {
                           return cast_frames<MAP>(qf, s, F, leg, r2, &lds.wl[w], rt, rf, rx, ry, rz);
                       });
}

int launch_path_cast(const QueryFrames &qf, int n_scenes, const double *d_path, int point_stride, long long scene_stride, int n_points,
                     double radius_sq, const PathCastOut &out, hipStream_t stream) {
    auto kernel = qf.map.fmap ? map_path_cast_kernel<true, kPathCastWaves> : map_path_cast_kernel<false, kPathCastWaves>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_scenes), dim3(64 * kPathCastWaves), 0, stream, qf, n_scenes, d_path, point_stride,
                       scene_stride, n_points, radius_clamped(radius_sq), out);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

}  // namespace

namespace amk {
// The path cast over a pool (kfmap.hip, pipeline.hip): the leading n_scenes scenes of a map of S
int map_path_cast(amk_kd *pool, int n_frames, const int *d_fmap, int S, int n_scenes, const double *d_path, int point_stride,
                  long long scene_stride, int n_points, double radius_sq, const PathCastOut &out, hipStream_t stream) {
    if (!pool_args_ok(pool, d_fmap, n_frames, S) || n_scenes < 1 || n_scenes > S || scene_stride < 0) return AMK_ERR_INVALID_ARG;
    if (const int st = segment_cast_args_status(d_path, point_stride, n_points, radius_sq, out.any()); st != AMK_OK) return st;
    return launch_path_cast(frames_of_pool(pool, n_frames, d_fmap, S), n_scenes, d_path, point_stride, scene_stride, n_points, radius_sq,
                            out, stream);
}
// The two queries over a keyframe map's pool (kfmap.hip): frame f of scene s = pool scene d_fmap[f * S + s] (< 0: absent).
int map_query_nearest(amk_kd *pool, int n_frames, const int *d_fmap, int S, const double *d_Twc, const amk_frame_camera *cam,
                      const double *d_queries, int query_stride, int n_queries, int k, float *d_pts, double *d_sqdist, int *d_frame,
                      int *d_counts, hipStream_t stream, bool exact) {
    if (!pool_args_ok(pool, d_fmap, n_frames, S) || !query_args_ok(d_queries, query_stride, n_queries) || k < 1) return AMK_ERR_INVALID_ARG;
    if (d_Twc && !cam) return AMK_ERR_INVALID_ARG;
    if (k > AMK_MAX_K) return AMK_ERR_UNSUPPORTED;
    ExactPtrs ex;
    if (exact) {
        if (!pool->exact.allocated()) return AMK_ERR_INVALID_ARG;   // (amk_kfmap_set_tie_order allocated the trees)
        ex = amk_exact_ptrs(pool);
    }
    return launch_query<false>(frames_of_pool(pool, n_frames, d_fmap, S), S, d_queries, query_stride, n_queries, k, d_Twc, cam, d_pts,
                               d_sqdist, d_frame, d_counts, nullptr, stream, exact ? &ex : nullptr);
}

int map_nearest_distance(amk_kd *pool, int n_frames, const int *d_fmap, int S, const double *d_queries, int query_stride,
                         int n_queries, double *d_dist, hipStream_t stream) {
    if (!pool_args_ok(pool, d_fmap, n_frames, S) || !query_args_ok(d_queries, query_stride, n_queries) || !d_dist) return AMK_ERR_INVALID_ARG;
    return launch_query<true>(frames_of_pool(pool, n_frames, d_fmap, S), S, d_queries, query_stride, n_queries, 1, nullptr, nullptr,
                              nullptr, nullptr, nullptr, nullptr, d_dist, stream);
}
int map_radius_search(amk_kd *pool, int n_frames, const int *d_fmap, int S, const double *d_queries, int query_stride, int n_queries,
                      double radius_sq, int max_results, float *d_pts, double *d_sqdist, int *d_frame, int *d_counts, hipStream_t stream) {
    if (!pool_args_ok(pool, d_fmap, n_frames, S)) return AMK_ERR_INVALID_ARG;
    if (const int st = radius_args_status(d_queries, query_stride, n_queries, radius_sq, max_results, d_pts || d_sqdist || d_frame,
                                          d_pts || d_sqdist || d_frame || d_counts);
        st != AMK_OK)
        return st;
    return launch_rows(map_radius_kernel<true>, map_radius_kernel<false>, frames_of_pool(pool, n_frames, d_fmap, S), S, n_queries, stream,
                       d_queries, query_stride, n_queries, radius_clamped(radius_sq), max_results, d_pts, d_sqdist, d_frame, d_counts);
}
int map_segment_search(amk_kd *pool, int n_frames, const int *d_fmap, int S, const double *d_path, int point_stride, int n_points,
                       double radius_sq, int max_results, float *d_pts, double *d_sqdist, double *d_t, int *d_frame, int *d_counts,
                       hipStream_t stream) {
    if (!pool_args_ok(pool, d_fmap, n_frames, S)) return AMK_ERR_INVALID_ARG;
    if (const int st = segment_args_status(d_path, point_stride, n_points, radius_sq, max_results, d_pts || d_sqdist || d_t || d_frame,
                                           d_pts || d_sqdist || d_t || d_frame || d_counts);
        st != AMK_OK)
        return st;
    return launch_rows(map_segment_kernel<true>, map_segment_kernel<false>, frames_of_pool(pool, n_frames, d_fmap, S), S, n_points - 1,
                       stream, d_path, point_stride, n_points, radius_clamped(radius_sq), max_results, d_pts, d_sqdist, d_t, d_frame,
                       d_counts);
}
int map_segment_nearest(amk_kd *pool, int n_frames, const int *d_fmap, int S, const double *d_path, int point_stride, int n_points, int k,
                        float *d_pts, double *d_sqdist, double *d_t, int *d_frame, int *d_counts, hipStream_t stream) {
    if (!pool_args_ok(pool, d_fmap, n_frames, S)) return AMK_ERR_INVALID_ARG;
    if (const int st = segment_nearest_args_status(d_path, point_stride, n_points, k, d_pts || d_sqdist || d_t || d_frame || d_counts);
        st != AMK_OK)
        return st;
    return launch_rows(map_segment_nearest_kernel<true>, map_segment_nearest_kernel<false>, frames_of_pool(pool, n_frames, d_fmap, S), S,
                       n_points - 1, stream, d_path, point_stride, n_points, k, d_pts, d_sqdist, d_t, d_frame, d_counts);
}
int map_segment_cast(amk_kd *pool, int n_frames, const int *d_fmap, int S, const double *d_path, int point_stride, int n_points,
                     double radius_sq, int *d_hit, double *d_t, float *d_pts, int *d_frame, hipStream_t stream) {
    if (!pool_args_ok(pool, d_fmap, n_frames, S)) return AMK_ERR_INVALID_ARG;
    if (const int st = segment_cast_args_status(d_path, point_stride, n_points, radius_sq, d_hit || d_t || d_pts || d_frame); st != AMK_OK)
        return st;
    return launch_rows(map_segment_cast_kernel<true>, map_segment_cast_kernel<false>, frames_of_pool(pool, n_frames, d_fmap, S), S,
                       n_points - 1, stream, d_path, point_stride, n_points, radius_clamped(radius_sq), d_hit, d_t, d_pts, d_frame);
}
}  // namespace amk

extern "C" {

int amk_kd_query_frames(amk_kd *const *frames, int n_frames, const double *d_Twc, const amk_frame_camera *cam,
                        const double *d_queries, int query_stride, int n_queries, int k, float *d_pts, double *d_sqdist,
                        int *d_frame, int *d_counts, void *stream) {
    if (!query_args_ok(d_queries, query_stride, n_queries) || k < 1) return AMK_ERR_INVALID_ARG;
    if (d_Twc && !cam) return AMK_ERR_INVALID_ARG;
    if (k > AMK_MAX_K) return AMK_ERR_UNSUPPORTED;
    const HandleFrames h = frames_of_handles(frames, n_frames);
    if (h.status != AMK_OK) return h.status;
    return launch_query<false>(h.qf, h.S, d_queries, query_stride, n_queries, k, d_Twc, cam, d_pts, d_sqdist, d_frame, d_counts, nullptr,
                               (hipStream_t)stream);
}

int amk_kd_nearest_distance_frames(amk_kd *const *frames, int n_frames, const double *d_queries, int query_stride, int n_queries,
                                   double *d_dist, void *stream) {
    if (!query_args_ok(d_queries, query_stride, n_queries) || !d_dist) return AMK_ERR_INVALID_ARG;
    const HandleFrames h = frames_of_handles(frames, n_frames);
    if (h.status != AMK_OK) return h.status;
    return launch_query<true>(h.qf, h.S, d_queries, query_stride, n_queries, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                              d_dist, (hipStream_t)stream);
}

int amk_kd_query_frames_host(amk_kd *const *frames, int n_frames, const double *h_Twc, const amk_frame_camera *cam,
                             const double *h_queries, int query_stride, int n_queries, int k, float *h_pts, double *h_sqdist,
                             int *h_frame, int *h_counts) {
    if (h_Twc && !cam) return AMK_ERR_INVALID_ARG;
    return frames_host(frames, n_frames, true, [&](amk::HostStage &stage, int S) {
        return amk::map_query_host(stage, S, h_queries, query_stride, n_queries, k, h_Twc, h_pts, h_sqdist, h_frame, h_counts, nullptr,
                                   [&](const amk::HostStage::Dev *d) {
                                       return amk_kd_query_frames(frames, n_frames, d[amk::MQ_TWC], cam, d[amk::MQ_QUERIES], query_stride,
                                                                  n_queries, k, d[amk::MQ_PTS], d[amk::MQ_SQDIST], d[amk::MQ_FRAME],
                                                                  d[amk::MQ_COUNTS], nullptr);
                                   });
    });
}

int amk_kd_radius_search_frames(amk_kd *const *frames, int n_frames, const double *d_queries, int query_stride, int n_queries,
                                double radius_sq, int max_results, float *d_pts, double *d_sqdist, int *d_frame, int *d_counts,
                                void *stream) {
    if (const int st = radius_args_status(d_queries, query_stride, n_queries, radius_sq, max_results, d_pts || d_sqdist || d_frame,
                                          d_pts || d_sqdist || d_frame || d_counts);
        st != AMK_OK)
        return st;
    const HandleFrames h = frames_of_handles(frames, n_frames, false);
    if (h.status != AMK_OK) return h.status;
    return launch_rows(map_radius_kernel<true>, map_radius_kernel<false>, h.qf, h.S, n_queries, (hipStream_t)stream, d_queries,
                       query_stride, n_queries, radius_clamped(radius_sq), max_results, d_pts, d_sqdist, d_frame, d_counts);
}

int amk_kd_radius_search_frames_host(amk_kd *const *frames, int n_frames, const double *h_queries, int query_stride, int n_queries,
                                     double radius_sq, int max_results, float *h_pts, double *h_sqdist, int *h_frame, int *h_counts) {
    return frames_host(frames, n_frames, false, [&](amk::HostStage &stage, int S) {
        return amk::map_radius_host(stage, S, h_queries, query_stride, n_queries, radius_sq, max_results, h_pts, h_sqdist, h_frame, h_counts,
                                    [&](const amk::HostStage::Dev *d) {
                                        return amk_kd_radius_search_frames(frames, n_frames, d[amk::MQ_QUERIES], query_stride, n_queries,
                                                                           radius_sq, max_results, d[amk::MQ_PTS], d[amk::MQ_SQDIST],
                                                                           d[amk::MQ_FRAME], d[amk::MQ_COUNTS], nullptr);
                                    });
    });
}

int amk_kd_segment_search_frames(amk_kd *const *frames, int n_frames, const double *d_path, int point_stride, int n_points,
                                 double radius_sq, int max_results, float *d_pts, double *d_sqdist, double *d_t, int *d_frame,
                                 int *d_counts, void *stream) {
    if (const int st = segment_args_status(d_path, point_stride, n_points, radius_sq, max_results, d_pts || d_sqdist || d_t || d_frame,
                                           d_pts || d_sqdist || d_t || d_frame || d_counts);
        st != AMK_OK)
        return st;
    const HandleFrames h = frames_of_handles(frames, n_frames, false);
    if (h.status != AMK_OK) return h.status;
    return launch_rows(map_segment_kernel<true>, map_segment_kernel<false>, h.qf, h.S, n_points - 1, (hipStream_t)stream, d_path,
                       point_stride, n_points, radius_clamped(radius_sq), max_results, d_pts, d_sqdist, d_t, d_frame, d_counts);
}

int amk_kd_segment_search_frames_host(amk_kd *const *frames, int n_frames, const double *h_path, int point_stride, int n_points,
                                      double radius_sq, int max_results, float *h_pts, double *h_sqdist, double *h_t, int *h_frame,
                                      int *h_counts) {
    return frames_host(frames, n_frames, false, [&](amk::HostStage &stage, int S) {
        return amk::map_segment_host(stage, S, h_path, point_stride, n_points, radius_sq, max_results, h_pts, h_sqdist, h_t, h_frame, h_counts,
                                     [&](const amk::HostStage::Dev *d) {
                                         return amk_kd_segment_search_frames(frames, n_frames, d[amk::MQ_QUERIES], point_stride, n_points,
                                                                             radius_sq, max_results, d[amk::MQ_PTS], d[amk::MQ_SQDIST],
                                                                             d[amk::MQ_DIST], d[amk::MQ_FRAME], d[amk::MQ_COUNTS], nullptr);
                                     });
    });
}

int amk_kd_segment_nearest_frames(amk_kd *const *frames, int n_frames, const double *d_path, int point_stride, int n_points, int k,
                                  float *d_pts, double *d_sqdist, double *d_t, int *d_frame, int *d_counts, void *stream) {
    if (const int st = segment_nearest_args_status(d_path, point_stride, n_points, k, d_pts || d_sqdist || d_t || d_frame || d_counts);
        st != AMK_OK)
        return st;
    const HandleFrames h = frames_of_handles(frames, n_frames, false);
    if (h.status != AMK_OK) return h.status;
    return launch_rows(map_segment_nearest_kernel<true>, map_segment_nearest_kernel<false>, h.qf, h.S, n_points - 1, (hipStream_t)stream,
                       d_path, point_stride, n_points, k, d_pts, d_sqdist, d_t, d_frame, d_counts);
}

int amk_kd_segment_nearest_frames_host(amk_kd *const *frames, int n_frames, const double *h_path, int point_stride, int n_points, int k,
                                       float *h_pts, double *h_sqdist, double *h_t, int *h_frame, int *h_counts) {
    return frames_host(frames, n_frames, false, [&](amk::HostStage &stage, int S) {
        return amk::map_segment_nearest_host(stage, S, h_path, point_stride, n_points, k, h_pts, h_sqdist, h_t, h_frame, h_counts,
                                             [&](const amk::HostStage::Dev *d) {
                                                 return amk_kd_segment_nearest_frames(frames, n_frames, d[amk::MQ_QUERIES], point_stride,
                                                                                      n_points, k, d[amk::MQ_PTS], d[amk::MQ_SQDIST],
                                                                                      d[amk::MQ_DIST], d[amk::MQ_FRAME], d[amk::MQ_COUNTS],
                                                                                      nullptr);
                                             });
    });
}

int amk_kd_segment_cast_frames(amk_kd *const *frames, int n_frames, const double *d_path, int point_stride, int n_points,
                               double radius_sq, int *d_hit, double *d_t, float *d_pts, int *d_frame, void *stream) {
    if (const int st = segment_cast_args_status(d_path, point_stride, n_points, radius_sq, d_hit || d_t || d_pts || d_frame); st != AMK_OK)
        return st;
    const HandleFrames h = frames_of_handles(frames, n_frames);
    if (h.status != AMK_OK) return h.status;
    return launch_rows(map_segment_cast_kernel<true>, map_segment_cast_kernel<false>, h.qf, h.S, n_points - 1, (hipStream_t)stream, d_path,
                       point_stride, n_points, radius_clamped(radius_sq), d_hit, d_t, d_pts, d_frame);
}

int amk_kd_segment_cast_frames_host(amk_kd *const *frames, int n_frames, const double *h_path, int point_stride, int n_points,
                                    double radius_sq, int *h_hit, double *h_t, float *h_pts, int *h_frame) {
    return frames_host(frames, n_frames, true, [&](amk::HostStage &stage, int S) {
        return amk::map_segment_cast_host(stage, S, h_path, point_stride, n_points, radius_sq, h_hit, h_t, h_pts, h_frame,
                                          [&](const amk::HostStage::Dev *d) {
                                              return amk_kd_segment_cast_frames(frames, n_frames, d[amk::MQ_QUERIES], point_stride, n_points,
                                                                                radius_sq, d[amk::MQ_COUNTS], d[amk::MQ_DIST],
                                                                                d[amk::MQ_PTS], d[amk::MQ_FRAME], nullptr);
                                          });
    });
}

int amk_kd_path_cast_frames(amk_kd *const *frames, int n_frames, const double *d_path, int point_stride, int n_points, double radius_sq,
                            int *d_stop, int *d_leg, double *d_t, double *d_free, float *d_pts, int *d_frame, void *stream) {
    const PathCastOut out{d_stop, d_leg, d_t, d_free, d_pts, d_frame};
    if (const int st = segment_cast_args_status(d_path, point_stride, n_points, radius_sq, out.any()); st != AMK_OK) return st;
    const HandleFrames h = frames_of_handles(frames, n_frames);
    if (h.status != AMK_OK) return h.status;
    return launch_path_cast(h.qf, h.S, d_path, point_stride, (long long)n_points * point_stride, n_points, radius_sq, out,
                            (hipStream_t)stream);
}

int amk_kd_path_cast_frames_host(amk_kd *const *frames, int n_frames, const double *h_path, int point_stride, int n_points,
                                 double radius_sq, int *h_stop, int *h_leg, double *h_t, double *h_free, float *h_pts, int *h_frame) {
    return frames_host(frames, n_frames, true, [&](amk::HostStage &stage, int S) {
        return amk::map_path_cast_host(stage, S, h_path, point_stride, n_points, radius_sq, h_stop, h_leg, h_t, h_free, h_pts, h_frame,
                                       [&](const amk::HostStage::Dev *d) {
                                           return amk_kd_path_cast_frames(frames, n_frames, d[amk::PC_PATH], point_stride, n_points,
                                                                          radius_sq, d[amk::PC_STOP], d[amk::PC_LEG], d[amk::PC_T],
                                                                          d[amk::PC_FREE], d[amk::PC_PTS], d[amk::PC_ID], nullptr);
                                       });
    });
}

}  // extern "C"
