// One control step over a MULTI-FRAME map (current frame + keyframes) for a batch of scenes on gfx950.
//
// amk_step_batch (step.hip) covers the map of BASELINE's synthetic configs, mVecQueryVector = [cur].  With keyframes
// FrameKDMap answers a query differently (AM/src/FrameKDMap.cpp):
//   QueryNearest (:322-376)     fast path -- current frame only -- when that frame's cloud holds >= k points AND the query
//                               projects into the current image (PtIsInFrame, :215-231); otherwise every frame f of
//                               mVecQueryVector is searched with k' = min(k, size_f) (:298) and the union is sorted by
//                               squared distance, first k kept (:371-375).  With KDTreeTwo's count rule (kd_tree_two.h:
//                               119-124: size == n -> no result) a frame contributes k points iff it holds MORE than k.
//   GetNearestDistance (:400-427)  min over the frames (non-empty obstacle cloud) of the 1-NN squared distance, sqrt.
// This file is the TASK branch of Step (AM/src/AvoidanceStateMachine.cpp:322-355) on such a map: obstacles remembered only
// through keyframes (already out of the field of view) stay in needReplan, PlanWapionts and P.
//
// Per outer iteration:
//   step_knn_frames_kernel        raw K-NN of the N reference points + edge 1-NN of point 0 in EVERY frame (grid.y = frame)
//   step_merge_plan_pack_kernel   one workgroup (4 wavefronts) per scene: PtIsInFrame per reference point, GetNearestDistance, PlanWapionts
//                                 (snap to the nearest edge point over the frames, re-query), fast path / merge per
//                                 reference point, padding, needReplan, early exit, GetRefStates
//   mpc_solve_kernel              Solve + refill of the reference path (mpc_solve.hip)
// Frames whose handles are in AMK_TIES_NANOFLANN mode are queried by nanoflann's own traversal of its own tree
// (kd_exact.h): step_knn_exact_kernel (step_common.h) overwrites the raw results, the snap re-query follows suit.
// A keyframe map in that mode (amk_kfmap_set_tie_order) holds a tree per pool scene: step_knn_exact_map_kernel and
// step_merge_plan_pack_map_kernel do the same through MapTrees (step_common.h).
#include "step_common.h"

using namespace amk;

namespace {

struct FrameSet {  // kernel argument: where every frame's indices live
    GridPtrs obs[AMK_MAX_FRAMES], edge[AMK_MAX_FRAMES];
    const int *size_obs[AMK_MAX_FRAMES], *size_edge[AMK_MAX_FRAMES];
    int n;
    // Map mode (the keyframe map, kfmap.hip): every frame of every scene lives in ONE pool handle (obs[0] / edge[0] /
    // size_*[0]); frame f of scene s is pool scene fmap[f * S + s], or absent (< 0: this scene's map is shorter) -- an absent
    // frame behaves like an empty cloud, which contributes nothing to any query (FrameKDMap.cpp:298,385-387).  n may then
    // exceed AMK_MAX_FRAMES (the per-frame arrays above are not used beyond [0]).
    const int *fmap;
    int S;
    __device__ __forceinline__ int scene_of(int f, int s) const { return fmap ? fmap[(size_t)f * S + s] : s; }
    __device__ __forceinline__ GridScene obs_scene(int f, int m) const { return (fmap ? obs[0] : obs[f]).scene(m); }
    __device__ __forceinline__ GridScene edge_scene(int f, int m) const { return (fmap ? edge[0] : edge[f]).scene(m); }
    __device__ __forceinline__ int n_obs(int f, int s) const {
        const int m = scene_of(f, s);
        return m < 0 ? 0 : (fmap ? size_obs[0] : size_obs[f])[m];
    }
    __device__ __forceinline__ int n_edge(int f, int s) const {
        const int m = scene_of(f, s);
        return m < 0 ? 0 : (fmap ? size_edge[0] : size_edge[f])[m];
    }
};

// blockIdx.y = the frame (a list of handles: every frame exists) or a chunk of consecutive frames (a keyframe map with room for
// 101 frames holds ~6 on a flight, and a launch of 101 x S x (N + 4) / 4 blocks of which 94 % return at once is mostly dispatch)
template <bool MAP>
__global__ __launch_bounds__(256) void step_knn_frames_kernel(FrameSet fs, int n_scenes, const double *__restrict__ ref_path,
                                                              int N, int K, FrameBufs fb, const int *__restrict__ done, int fc,
                                                              const double *__restrict__ Twc, amk_frame_camera cam) {
    __shared__ GridWaveLds wl[4];
    // map mode: reference point 0 is searched in EVERY frame (GetNearestDistance reads it, the snap may move it) -- one wavefront
    // walking the ~6 frames of a flight's map in turn was the tail of every launch.  Frames 1 .. fc - 1 of the first chunk get a
    // wavefront each: "queries" N + 1 .. N + fc - 1 are reference point 0 in frame q - N.
    const int nq = N + 1, nv = MAP ? fc - 1 : 0;
    const WaveSlot ws = wave_slot(nq + nv);
    const int s = ws.s, w = ws.w, lane = ws.lane;
    int q = ws.unit;
    if (s >= n_scenes || q >= nq + nv || done[s]) return;
    int f_only = -1;
    if (q >= nq) {
        if (blockIdx.y != 0) return;
        f_only = q - N;
        q = 0;
    }
    const bool is_edge = q == N;
    const double *qp = ref_path + ((size_t)s * N + (is_edge ? 0 : q)) * SD;
    const double qx = qp[0], qy = qp[1], qz = qp[2];
    const int k = is_edge ? 1 : K;
    // Frames behind the current one are searched only for the queries that will read them: QueryNearest answers from the current
    // frame alone when that frame holds >= k points and the query projects into the current image (FrameKDMap.cpp:339-345) -- on a
    // flight nearly every reference point does.  The merge kernel takes the same decision from the same numbers (reference point 0
    // may be moved by the snap in between and GetNearestDistance reads its rows in every frame: it is always searched everywhere).
    bool cur_only = false;
    if (q != 0) {
        const int n0 = is_edge ? fs.n_edge(0, s) : fs.n_obs(0, s);
        cur_only = n0 >= k && (!Twc || pt_in_frame(Twc + (size_t)s * 16, cam, qx, qy, qz));
    }
    const GridPtrs pool = is_edge ? fs.edge[0] : fs.obs[0];   // (map mode: one set of pool pointers stays live over the loop)
    // map mode: chunk c = frames [fc (2^c - 1), fc (2^(c+1) - 1)) -- 8, 16, 32, ... of them: a map on a flight holds ~6 frames of its
    // 101, and every chunk beyond the first is a grid of blocks that find nothing to do
    int f_begin = MAP ? fc * ((1 << blockIdx.y) - 1) : blockIdx.y;
    int f_end = MAP ? min(fs.n, fc * ((2 << blockIdx.y) - 1)) : (int)blockIdx.y + 1;
    if (MAP && blockIdx.y == 0) {
        if (f_only >= 0) { f_begin = f_only; f_end = min(f_end, f_only + 1); }
        else if (q == 0) f_end = min(f_end, 1);   // (its other frames of this chunk: the wavefronts above)
    }
    for (int f = f_begin; f < f_end; ++f) {
        if (cur_only && f > 0) break;
        const int m = MAP ? fs.fmap[(size_t)f * fs.S + s] : s;
        if (m < 0) continue;   // (map mode: this scene's map has no frame f; nobody reads its rows -- n_obs / n_edge are 0)
        double ld;
        int li, lpos;
        const GridScene gs = MAP ? pool.scene(m) : (is_edge ? fs.edge[f] : fs.obs[f]).scene(m);
        grid_knn(gs, qx, qy, qz, k, ld, li, lpos, &wl[w]);
        if (lane < k) {
            const bool ok = li != kNoIndex;
            const float4 rec = gs.pt[lpos];
            const size_t o = (size_t)f * n_scenes + s;
            if (is_edge) store_nbr(fb.edge_pt, fb.edge_d2, o, ok, ld, rec.x, rec.y, rec.z);
            else store_nbr(fb.knn_pts, fb.knn_d2, (o * N + q) * K + lane, ok, ld, rec.x, rec.y, rec.z);
        }
    }
}

// A keyframe map in AMK_TIES_NANOFLANN: the raw rows once more, by nanoflann's traversal of the pool scenes' trees, over what
// step_knn_frames_kernel<true> wrote (a pool scene without a tree keeps that).  One wavefront per (scene, query) walks the frames
// the scene HOLDS and skips what that kernel skips: the frames behind the current one for a row that will take the fast path.
// Reference point 0 is read in every frame: as there, frames 1 .. fc - 1 get a wavefront each ("queries" N + 1 .. N + fc - 1).
__global__ __launch_bounds__(256) void step_knn_exact_map_kernel(MapTrees trees, const int *__restrict__ size_obs,
                                                                 const int *__restrict__ size_edge, int n_frames, int n_scenes,
                                                                 const double *__restrict__ ref_path, int N, int K, FrameBufs fb,
                                                                 const int *__restrict__ done, int fc, const double *__restrict__ Twc,
                                                                 amk_frame_camera cam) {
    __shared__ ExactWaveStack stacks[4];
    const int nq = N + 1, nv = fc - 1;
    const WaveSlot ws = wave_slot(nq + nv);
    const int s = ws.s, w = ws.w, lane = ws.lane;
    int q = ws.unit;
    if (s >= n_scenes || q >= nq + nv || done[s]) return;
    int f_only = -1;
    if (q >= nq) { f_only = q - N; q = 0; }
    const bool is_edge = q == N;
    const double *qp = ref_path + ((size_t)s * N + (is_edge ? 0 : q)) * SD;
    const double qx = qp[0], qy = qp[1], qz = qp[2];
    const int k = is_edge ? 1 : K;
    bool cur_only = false;   // step_knn_frames_kernel's decision, from the same numbers
    if (q != 0) {
        const int m0 = trees.fmap[s];
        const int n0 = m0 < 0 ? 0 : (is_edge ? size_edge : size_obs)[m0];
        cur_only = n0 >= k && (!Twc || pt_in_frame(Twc + (size_t)s * 16, cam, qx, qy, qz));
    }
    int F = 0;               // frames this scene's map holds
    for (int f0 = 0; f0 < n_frames; f0 += 64) {
        const int f = f0 + lane;
        const unsigned long long b = __ballot(f < n_frames && trees.fmap[(size_t)f * trees.S + s] >= 0);
        if (b) F = f0 + 64 - __clzll((long long)b);
    }
    int f = 0, f_end = F;
    if (f_only >= 0) { f = f_only; f_end = min(F, f_only + 1); }
    for (; f < f_end; ++f) {
        if (cur_only && f > 0) break;
        if (f_only < 0 && q == 0 && f > 0 && f < fc) continue;   // (the wavefronts above)
        if (!map_frame_present(trees, f, s)) continue;
        const ExactTree T = exact_scene(trees, f, is_edge, s);
        double rd;
        int ri;
        const int got = exact_knn_wave(T, qx, qy, qz, k, rd, ri, &stacks[w]);
        if (got < 0) continue;
        if (lane < k) {
            const bool ok = lane < got;
            const float px = ok ? T.x[ri] : 0.f, py = ok ? T.y[ri] : 0.f, pz = ok ? T.z[ri] : 0.f;
            const size_t o = (size_t)f * n_scenes + s;
            if (is_edge) store_nbr(fb.edge_pt, fb.edge_d2, o, ok, rd, px, py, pz);
            else store_nbr(fb.knn_pts, fb.knn_d2, (o * N + q) * K + lane, ok, rd, px, py, pz);
        }
    }
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    return v;
}

constexpr int kMaxCandPerLane = (AMK_MAX_FRAMES * AMK_MAX_K + 63) / 64;
constexpr int kMaxCandPerLaneMap = 0;   // the keyframe map beyond 64 kMaxCandPerLane candidates (the reference's max_frame_count = 100:
                                        // 101 frames x K): the candidates are re-read every round instead of living in registers

// EXACT (some frame in AMK_TIES_NANOFLANN mode): a template parameter so that the default kernel needs no scratch memory.
// CPL: merge candidates (frame, neighbour) a lane may hold -- F K <= 64 CPL.
template <bool EXACT, int CPL = kMaxCandPerLane>
__global__ __launch_bounds__(4 * kWave) void step_merge_plan_pack_kernel(
    FrameSet fs, const FrameExact *__restrict__ fe, FrameBufs fb, int S, const double *__restrict__ Twc, amk_frame_camera cam, int N, int K, int nref, int iter,
    int max_iter, double speed, double T, double safety_distance, const double *__restrict__ state_quad,
    const double *__restrict__ pos_x, double *__restrict__ ref_path, float *__restrict__ knn_pts,
    double *__restrict__ knn_d2, double *__restrict__ ref_states, int *__restrict__ done, int *__restrict__ flags) {
    constexpr bool kMapTrees = false;
    const MapTrees *trees = nullptr;
#define AMK_STEP_MERGE_PLAN_PACK_BODY   // (the body refuses to be included anywhere else)
#include "step_merge_plan_pack_body.h"
#undef AMK_STEP_MERGE_PLAN_PACK_BODY
}
// the same over a keyframe map in AMK_TIES_NANOFLANN: the snap's re-query through the pool scenes' trees, four wavefronts
// (CPL 4, or 0: the wide merge)
template <int CPL>
__global__ __launch_bounds__(4 * kWave) void step_merge_plan_pack_map_kernel(
    FrameSet fs, MapTrees map_trees, FrameBufs fb, int S, const double *__restrict__ Twc, amk_frame_camera cam, int N, int K, int nref, int iter,
    int max_iter, double speed, double T, double safety_distance, const double *__restrict__ state_quad,
    const double *__restrict__ pos_x, double *__restrict__ ref_path, float *__restrict__ knn_pts,
    double *__restrict__ knn_d2, double *__restrict__ ref_states, int *__restrict__ done, int *__restrict__ flags) {
    constexpr bool EXACT = true, kMapTrees = true;
    const MapTrees *trees = &map_trees;
    const FrameExact *fe = nullptr;
#define AMK_STEP_MERGE_PLAN_PACK_BODY   // (the body refuses to be included anywhere else)
#include "step_merge_plan_pack_body.h"
#undef AMK_STEP_MERGE_PLAN_PACK_BODY
}
}  // namespace

// tests only (tests/test_kfmap_gpu.py): take the wide-map merge (candidates re-read every round) whatever the map's size
static int g_force_wide = 0;
extern "C" void amk__frames_force_wide(int on) { g_force_wide = on; }

// the rounds of the step over a frame set (plain handles or the keyframe map's pool), shared by the two entry points below
static int run_frames(const FrameSet &fs, amk_kd *const *obstacle, amk_kd *const *edge, const double *d_Twc,
                      const amk_frame_camera *cam, amk_mpc *mpc, const amk_step_params *prm, const double *d_state_quad,
                      const double *d_pos_x, double *d_ref_path, double *d_u, double *d_x0array, int *d_flags, hipStream_t stream,
                      const MapTrees *map_trees = nullptr) {
    const int N = mpc->N, K = mpc->K, F = fs.n;
    if (int st = ensure_step_workspace(mpc); st != AMK_OK) return st;
    const int Sall = mpc->S;
    if (mpc->mf_frames < F) {   // sized ONCE for the largest map of its kind (AMK_MAX_FRAMES handles; a keyframe map: its own
        // 1 + max_frame_count): a map that gains a keyframe between two calls must not free a buffer an earlier call's kernels
        // may still be reading
        const size_t FM = F > AMK_MAX_FRAMES ? F : AMK_MAX_FRAMES;
        if (mpc->mf_frames > 0) AMK_HIP(hipDeviceSynchronize());   // (growing: an explicit change of the map's capacity)
        AMK_HIP(mpc->mf_knn_pts.alloc(FM * Sall * N * K * 3));
        AMK_HIP(mpc->mf_knn_d2.alloc(FM * Sall * N * K));
        AMK_HIP(mpc->mf_edge_pt.alloc(FM * Sall * 3));
        AMK_HIP(mpc->mf_edge_d2.alloc(FM * Sall));
        mpc->mf_frames = (int)FM;
    }
    const int S = mpc->launch_scenes();   // (amk_pipeline: a gang that is not full runs its leading scenes only; the per-frame
                                          // rows of this call are laid out with this S, the frame map keeps the handle's: fs.S)
    const FrameBufs fb{mpc->mf_knn_pts.p, mpc->mf_knn_d2.p, mpc->mf_edge_pt.p, mpc->mf_edge_d2.p};
    // frames in AMK_TIES_NANOFLANN mode (their reference-shaped trees were built by amk_kd_build / amk_kd_push_keyframe)
    bool any_exact = false;
    FrameExact *fe_dev = nullptr;
    if (!fs.fmap) {
        std::vector<char> cur(sizeof(FrameExact), 0);
        FrameExact *h = reinterpret_cast<FrameExact *>(cur.data());
        for (int f = 0; f < F; ++f) {
            h->use_obs[f] = obstacle[f]->tie_order == AMK_TIES_NANOFLANN && obstacle[f]->ex_valid;
            h->use_edge[f] = edge[f]->tie_order == AMK_TIES_NANOFLANN && edge[f]->ex_valid;
            // bytewise copies of zero-filled structs: the table is compared bytewise below, padding included
            if (h->use_obs[f]) { const ExactPtrs t = amk_exact_ptrs(obstacle[f]); std::memcpy(&h->obs[f], &t, sizeof t); }
            if (h->use_edge[f]) { const ExactPtrs t = amk_exact_ptrs(edge[f]); std::memcpy(&h->edge[f], &t, sizeof t); }
            any_exact |= h->use_obs[f] || h->use_edge[f];
        }
        if (any_exact) {
            // The table lives in device memory (too large for the kernel-argument segment).  It is uploaded only when the
            // frame list or a frame's mode changed -- a host event (AddVertex / keyframe push) -- and then synchronously after
            // a device-wide wait: earlier calls on other streams may still be reading the old table.  The steady state issues
            // no copy at all, so a step over an unchanged exact-mode map is graph-capturable like the other step paths; the
            // call that follows a change of the map is not.
            if (!mpc->mf_exact.p) AMK_HIP(mpc->mf_exact.alloc(sizeof(FrameExact)));
            if (mpc->mf_exact_host != cur) {
                AMK_HIP(hipDeviceSynchronize());
                AMK_HIP(hipMemcpy(mpc->mf_exact.p, h, sizeof(FrameExact), hipMemcpyHostToDevice));
                mpc->mf_exact_host = cur;
            }
            fe_dev = reinterpret_cast<FrameExact *>(mpc->mf_exact.p);
        }
    }
    amk_frame_camera c{};
    if (cam) c = *cam;
    // the merge keeps ceil(F K / 64) candidates per lane in registers: instantiated for 1 / 2 / 4 / 16 (a 4-frame map with K = 8 needs
    // ONE; the 16-wide instantiation carries 32 key registers and 16 x unrolled selection loops: 204 VGPRs against 70-odd)
    const int need_cpl = (F * K + 63) / 64;
    // a keyframe map beyond 4 candidates per lane takes the wide merge: 61 VGPRs (it runs beside the solves' waves; the 16-wide
    // instantiation cannot), and with the loops bounded by the frames a scene actually holds its re-reads are few
    const bool wide = F * K > 64 * kMaxCandPerLane || (fs.fmap && need_cpl > 4) || (g_force_wide && !any_exact);
    // a keyframe map in AMK_TIES_NANOFLANN: every (max_frame_count, K) of the default map step, by the wide merge or four candidates per lane
    auto map_merge_kernel = wide ? step_merge_plan_pack_map_kernel<kMaxCandPerLaneMap> : step_merge_plan_pack_map_kernel<4>;
    auto merge_kernel = step_merge_plan_pack_kernel<false, kMaxCandPerLane>;
    if (wide) merge_kernel = step_merge_plan_pack_kernel<false, kMaxCandPerLaneMap>;
    else if (any_exact) merge_kernel = step_merge_plan_pack_kernel<true>;
    else if (need_cpl <= 1) merge_kernel = step_merge_plan_pack_kernel<false, 1>;
    else if (need_cpl <= 2) merge_kernel = step_merge_plan_pack_kernel<false, 2>;
    else if (need_cpl <= 4) merge_kernel = step_merge_plan_pack_kernel<false, 4>;
    launch_step_begin(S, mpc->done.p, d_flags, d_u, stream);
    const int fc = 8;   // map mode: frames of the first chunk of search blocks (the chunks double: 8, 16, 32, ...)
    int n_chunks = 1;
    while (fc * ((1 << n_chunks) - 1) < F) ++n_chunks;
    for (int iter = 0; iter < prm->mpc_max_iter; ++iter) {
        if (fs.fmap)
            hipLaunchKernelGGL(step_knn_frames_kernel<true>, dim3((unsigned)search_blocks(S, N + 1 + (fc - 1)), n_chunks), dim3(256), 0, stream, fs, S,
                               d_ref_path, N, K, fb, mpc->done.p, fc, d_Twc, c);
        else
            hipLaunchKernelGGL(step_knn_frames_kernel<false>, dim3((unsigned)search_blocks(S, N + 1), F), dim3(256), 0, stream, fs, S, d_ref_path,
                               N, K, fb, mpc->done.p, 1, d_Twc, c);
        if (any_exact)
            hipLaunchKernelGGL(step_knn_exact_kernel<const FrameExact *>, dim3((S * (N + 1) + 3) / 4, F), dim3(256), 0, stream,
                               fe_dev, S, d_ref_path, N, K, fb, mpc->done.p);
        if (map_trees) {
            hipLaunchKernelGGL(step_knn_exact_map_kernel, dim3((unsigned)search_blocks(S, N + 1 + (fc - 1))), dim3(256), 0, stream, *map_trees,
                               fs.size_obs[0], fs.size_edge[0], F, S, d_ref_path, N, K, fb, mpc->done.p, fc, d_Twc, c);
            hipLaunchKernelGGL(map_merge_kernel, dim3(S), dim3(4 * kWave), 0, stream, fs, *map_trees, fb, S, d_Twc, c, N, K, mpc->nref,
                               iter, prm->mpc_max_iter, prm->speed, mpc->T, prm->safety_distance, d_state_quad, d_pos_x,
                               d_ref_path, mpc->knn_pts.p, mpc->knn_d2.p, mpc->ref_states.p, mpc->done.p, d_flags);
        } else
        hipLaunchKernelGGL(merge_kernel, dim3(S), dim3(any_exact ? kWave : 4 * kWave), 0, stream, fs, fe_dev, fb, S, d_Twc, c, N, K, mpc->nref,
                           iter, prm->mpc_max_iter, prm->speed, mpc->T, prm->safety_distance, d_state_quad, d_pos_x,
                           d_ref_path, mpc->knn_pts.p, mpc->knn_d2.p, mpc->ref_states.p, mpc->done.p, d_flags);
        AMK_HIP(hipGetLastError());
        int st = launch_solve(mpc, mpc->ref_states.p, d_u, d_x0array, nullptr, mpc->done.p, d_ref_path, d_flags, stream);
        if (st != AMK_OK) return st;
    }
    return AMK_OK;
}

extern "C" int amk_step_batch_frames(amk_kd *const *obstacle, amk_kd *const *edge, int n_frames, const double *d_Twc,
                                     const amk_frame_camera *cam, amk_mpc *mpc, const amk_step_params *prm,
                                     const double *d_state_quad, const double *d_pos_x, double *d_ref_path, double *d_u,
                                     double *d_x0array, int *d_flags, void *stream_) {
    if (!obstacle || !edge || !mpc || !prm || !d_state_quad || !d_pos_x || !d_ref_path || !d_u || !d_flags || n_frames < 1)
        return AMK_ERR_INVALID_ARG;
    if (d_Twc && !cam) return AMK_ERR_INVALID_ARG;
    if (n_frames > AMK_MAX_FRAMES) return AMK_ERR_UNSUPPORTED;
    if (!step_params_ok(mpc, prm)) return AMK_ERR_INVALID_ARG;
    const int S = mpc->S, F = n_frames;
    FrameSet fs{};
    fs.n = F;
    fs.fmap = nullptr;
    fs.S = S;
    for (int f = 0; f < F; ++f) {
        if (!obstacle[f] || !edge[f] || obstacle[f]->n_scenes != S || edge[f]->n_scenes != S) return AMK_ERR_INVALID_ARG;
        if (obstacle[f]->mode != 0 || edge[f]->mode != 0) return AMK_ERR_UNSUPPORTED;  // bucketed indices only
        // (no lazily built trees on the multi-frame path -- header)
        if (obstacle[f]->tie_order == AMK_TIES_AUTO || edge[f]->tie_order == AMK_TIES_AUTO) return AMK_ERR_UNSUPPORTED;
        fs.obs[f] = grid_ptrs(obstacle[f]);
        fs.edge[f] = grid_ptrs(edge[f]);
        fs.size_obs[f] = obstacle[f]->size.p;
        fs.size_edge[f] = edge[f]->size.p;
    }
    return run_frames(fs, obstacle, edge, d_Twc, cam, mpc, prm, d_state_quad, d_pos_x, d_ref_path, d_u, d_x0array, d_flags,
                      (hipStream_t)stream_);
}

namespace amk {
// The same step over a keyframe map (kfmap.hip): every frame of every scene in the two pool handles, frame f of scene s = pool
// scene d_fmap[f * S + s] (< 0: absent); n_frames = 1 + max_frame_count of the map, <= AMK_MAX_MAP_FRAMES.
int step_batch_map(amk_kd *obs_pool, amk_kd *edge_pool, int n_frames, const int *d_fmap, const double *d_Twc,
                   const amk_frame_camera *cam, amk_mpc *mpc, const amk_step_params *prm, const double *d_state_quad,
                   const double *d_pos_x, double *d_ref_path, double *d_u, double *d_x0array, int *d_flags, hipStream_t stream,
                   bool exact) {
    if (!obs_pool || !edge_pool || !d_fmap || !mpc || !prm || !d_state_quad || !d_pos_x || !d_ref_path || !d_u || !d_flags || n_frames < 1)
        return AMK_ERR_INVALID_ARG;
    if (d_Twc && !cam) return AMK_ERR_INVALID_ARG;
    if (n_frames > AMK_MAX_MAP_FRAMES || n_frames * mpc->K > 64 * 128) return AMK_ERR_UNSUPPORTED;
    if (!step_params_ok(mpc, prm)) return AMK_ERR_INVALID_ARG;
    FrameSet fs{};
    fs.n = n_frames;
    fs.fmap = d_fmap;
    fs.S = mpc->S;
    fs.obs[0] = grid_ptrs(obs_pool);
    fs.edge[0] = grid_ptrs(edge_pool);
    fs.size_obs[0] = obs_pool->size.p;
    fs.size_edge[0] = edge_pool->size.p;
    MapTrees trees{};
    if (exact) {   // the map is in AMK_TIES_NANOFLANN: amk_kfmap_set_tie_order allocated the trees, every build behind it filled them
        if (!obs_pool->ex_vind.p || !edge_pool->ex_vind.p) return AMK_ERR_INVALID_ARG;
        trees.obs_pool = amk_exact_ptrs(obs_pool);
        trees.edge_pool = amk_exact_ptrs(edge_pool);
        trees.fmap = d_fmap;
        trees.S = mpc->S;
    }
    return run_frames(fs, nullptr, nullptr, d_Twc, cam, mpc, prm, d_state_quad, d_pos_x, d_ref_path, d_u, d_x0array, d_flags, stream,
                      exact ? &trees : nullptr);
}
}  // namespace amk
