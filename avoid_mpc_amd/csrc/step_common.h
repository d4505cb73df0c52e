// What the two control-step paths share: step.hip (one frame per scene) and step_frames.hip (a list of frames or the
// keyframe map's pool).  Each rule of the TASK branch of AvoidanceStateMachine::Step (AM/src/AvoidanceStateMachine.cpp:
// 322-355) that both paths apply is written here once.
#pragma once
#include "kd_exact.h"
#include "mpc_handle.h"

namespace amk {

struct FrameBufs {  // raw query results, frame-major; frame 0 of the single-frame path is the mpc's own workspace
    float *knn_pts;   // [F][S][N][K][3]
    double *knn_d2;   // [F][S][N][K]
    float *edge_pt;   // [F][S][3]
    double *edge_d2;  // [F][S]
};

// Neighbour slot i of a K-NN row (or of the edge 1-NN buffers, same layout): the point, or DBL_MAX and zeros when absent.
__device__ __forceinline__ void store_nbr(float *__restrict__ pts, double *__restrict__ d2, size_t i, bool ok, double d,
                                          float x, float y, float z) {
    d2[i] = ok ? d : DBL_MAX;
    float *o = pts + i * 3;
    o[0] = ok ? x : 0.f;
    o[1] = ok ? y : 0.f;
    o[2] = ok ? z : 0.f;
}

// PtIsInFrame (FrameKDMap.cpp:215-231): Twc rigid, its inverse is [R' | -R' t]
__device__ __forceinline__ bool pt_in_frame(const double *__restrict__ T, const amk_frame_camera &cam, double px, double py,
                                            double pz) {
#pragma clang fp contract(off)   // every kernel that takes this decision for a point (the step's searches skip what its merge will not read; map_query.hip) gets the same bits
    const double dx = px - T[3], dy = py - T[7], dz = pz - T[11];
    const double x = T[0] * dx + T[4] * dy + T[8] * dz;
    const double y = T[1] * dx + T[5] * dy + T[9] * dz;
    const double z = T[2] * dx + T[6] * dy + T[10] * dz;
    if (z > cam.depth_max || z < 0) return false;
    const double u = cam.fx * x / z + cam.cx;
    const double v = cam.fy * y / z + cam.cy;
    if (u < 0 || u >= cam.width || v < 0 || v >= cam.height) return false;
    return true;
}

// The frames of a multi-frame map, for every kernel that walks them (step_frames.hip, map_query.hip).  A list of handles (fmap
// null): frame f of scene s is scene s of handle f, and every frame exists.  A keyframe map (kfmap.hip): every frame of every scene
// lives in ONE pool handle, frame f of scene s is pool scene fmap[f * S + s], or absent (< 0: this scene's map is shorter) -- an
// absent frame behaves like an empty cloud, which contributes nothing to any query (FrameKDMap.cpp:298,385-387).  n may then
// exceed AMK_MAX_FRAMES.
struct FrameMap {
    int n;
    const int *fmap;
    int S;
    __device__ __forceinline__ int pool_scene(int f, int s) const { return fmap[(size_t)f * S + s]; }   // (a keyframe map)
    __device__ __forceinline__ int scene_of(int f, int s) const { return fmap ? pool_scene(f, s) : s; }
    // A keyframe map: one past the last frame scene s holds (frames before it may be absent), asked by a whole wavefront.
    __device__ __forceinline__ int held(int s, int lane) const {
        int hi = 0;
        for (int f0 = 0; f0 < n; f0 += 64) {
            const int f = f0 + lane;
            const unsigned long long b = __ballot(f < n && pool_scene(f, s) >= 0);
            if (b) hi = f0 + 64 - __clzll((long long)b);
        }
        return hi;
    }
};

// Where the AMK_TIES_NANOFLANN trees come from: one frame's two trees by value (the single-frame path: no table to upload,
// its steps stay graph-capturable), or the device table of a frame list (too large for the kernel-argument segment next to
// FrameSet; frame = blockIdx.y).
struct ExactPair {
    ExactPtrs obs, edge;
    int use_obs, use_edge;
};
struct FrameExact {
    ExactPtrs obs[AMK_MAX_FRAMES], edge[AMK_MAX_FRAMES];
    int use_obs[AMK_MAX_FRAMES], use_edge[AMK_MAX_FRAMES];
};
// ... or the two POOLS of a keyframe map in AMK_TIES_NANOFLANN (kfmap.hip), by value: no device table, no host upload.  Which pool
// scene is frame f of scene s says the FrameMap that travels with them.
struct MapTrees {
    ExactPtrs obs_pool, edge_pool;
};
__device__ __forceinline__ bool exact_used(const ExactPair &t, int, bool edge) { return edge ? t.use_edge : t.use_obs; }
__device__ __forceinline__ bool exact_used(const FrameExact *t, int f, bool edge) {
    return edge ? t->use_edge[f] : t->use_obs[f];
}
__device__ __forceinline__ ExactTree exact_scene(const ExactPair &t, int, bool edge, int s) {
    return edge ? t.edge.scene(s) : t.obs.scene(s);
}
__device__ __forceinline__ ExactTree exact_scene(const FrameExact *t, int f, bool edge, int s) {
    return edge ? t->edge[f].scene(s) : t->obs[f].scene(s);
}
// whether row (s, q) of a tree that is used goes through it: every row (step.hip's StepAuto: only the rows that tied)
template <class Trees>
__device__ __forceinline__ bool exact_row_wanted(const Trees &, int, bool, int, int, int) { return true; }

// Handles in AMK_TIES_NANOFLANN mode: the raw results by nanoflann's own traversal of its own tree (kd_exact.h), one
// WAVEFRONT per (frame, scene, query), overwriting what the bucketed search wrote wherever the tree is available.  With exact
// ties (quantised edge clouds) this is what keeps the snapped edge point and the neighbour SET equal to the reference's.
// One body for every source of trees (Trees: ExactPair, const FrameExact *, step.hip's StepAuto); f: the frame.
template <class Trees>
__device__ __forceinline__ void step_knn_exact_row(const Trees &trees, int f, int n_scenes, const double *ref_path,
    int N, int K, const FrameBufs &fb, const int *done) {
    __shared__ ExactWaveStack stacks[4];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)  /* wave-uniform: keeps what derives from it in SGPRs */, lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + w;
    const int nq = N + 1;
    if (t >= n_scenes * nq) return;
    const int s = t / nq, q = t - s * nq;
    if (done[s]) return;
    const bool is_edge = q == N;
    if (!exact_used(trees, f, is_edge) || !exact_row_wanted(trees, f, is_edge, s, q, N)) return;
    const double *qp = ref_path + ((size_t)s * N + (is_edge ? 0 : q)) * SD;
    const ExactTree T = exact_scene(trees, f, is_edge, s);
    const int k = is_edge ? 1 : K;
    double rd;
    int ri;
    const int got = exact_knn_wave(T, qp[0], qp[1], qp[2], k, rd, ri, &stacks[w]);
    if (got < 0) return;
    if (lane < k) {
        const bool ok = lane < got;
        const float px = ok ? T.x[ri] : 0.f, py = ok ? T.y[ri] : 0.f, pz = ok ? T.z[ri] : 0.f;
        const size_t o = (size_t)f * n_scenes + s;
        if (is_edge) store_nbr(fb.edge_pt, fb.edge_d2, o, ok, rd, px, py, pz);
        else store_nbr(fb.knn_pts, fb.knn_d2, (o * N + q) * K + lane, ok, rd, px, py, pz);
    }
}
template <class Trees>
__global__ __launch_bounds__(256) void step_knn_exact_kernel(Trees trees, int n_scenes, const double *__restrict__ ref_path, int N,
    int K, FrameBufs fb, const int *__restrict__ done) {
    step_knn_exact_row(trees, blockIdx.y, n_scenes, ref_path, N, K, fb, done);
}

// AMK_TIES_NANOFLANN: the re-query of the snapped point (ProcessWaypoints queries it next, :210-215) by the reference's
// own traversal, into row `row` of pts / d2 unless the tree declines.  One wavefront per workgroup calls it; lane 0 walks.
__device__ __forceinline__ void exact_requery(const ExactTree &T, double ex, double ey, double ez, int K,
                                              float *__restrict__ pts, double *__restrict__ d2, size_t row) {
    __shared__ double xr[AMK_MAX_K];
    __shared__ int xi[AMK_MAX_K], xgot;
    __shared__ ExactStackStorage xstack;  // LDS, not scratch: one lane walks the tree
    const int lane = threadIdx.x;
    if (lane == 0) xgot = exact_knn_thread(T, ex, ey, ez, K, xr, xi, xstack.view());
    __syncthreads();
    if (xgot >= 0 && lane < K) {
        const bool ok = lane < xgot;
        store_nbr(pts, d2, row * K + lane, ok, xr[lane], ok ? T.x[xi[lane]] : 0.f, ok ? T.y[xi[lane]] : 0.f,
                  ok ? T.z[xi[lane]] : 0.f);
    }
}

// ProcessWaypoints' padding and needReplan (:216-231), the early exit (:333-335) and GetRefStates (:236-257) for scene s,
// by threads tid = 0 .. nthr - 1 of its workgroup (every wavefront takes the same decision).  cnt(i): the neighbours
// QueryNearest gave reference point i; rp: the scene's reference path; is_safety: what PlanWapionts decided.
template <class Count>
__device__ __forceinline__ void pack_ref_states(int tid, int nthr, int s, int N, int K, int nref, int iter, int max_iter,
                                                double speed, double T, double safety_distance, int is_safety, Count cnt,
                                                const double *__restrict__ state_quad, const double *__restrict__ pos_x,
                                                const double *__restrict__ rp, const float *__restrict__ knn_pts,
                                                const double *__restrict__ knn_d2, double *__restrict__ ref_states,
                                                int *__restrict__ done) {
    const int lane = tid & 63;
    bool need = false;
    if (lane < N) need = (cnt(lane) == 0) || (sqrt(knn_d2[((size_t)s * N + lane) * K]) <= safety_distance);
    const bool need_replan = __ballot(need) != 0ull;
    if (!need_replan && iter > 0 && is_safety) {
        if (tid == 0) done[s] = 1;
        return;
    }
    const SceneRecord R{N, K};
    double *P = ref_states + (size_t)s * nref;
    const double *sq = state_quad + ((size_t)s * max_iter + iter) * SD;
    if (tid < SD) P[R.x_init() + tid] = sq[tid];
    for (int e = tid; e < SD * N; e += nthr) P[R.ref() + e] = rp[e];
    for (int e = tid; e < 3 * K * N; e += nthr) {
        const int i = e / (3 * K), j = (e / 3) % K;
        P[R.obs() + e] = (j < cnt(i)) ? (double)knn_pts[(size_t)s * N * K * 3 + e] : 10000.0;  // :223-226
    }
    if (tid < SD) {
        const double *last = rp + (N - 1) * SD;
        double v = last[tid];
        if (tid == 0) {
#pragma clang fp contract(off)   // the product rounded, then the difference, like the oracle's two operations: fused, the target's x differs in its last bit whenever speed * T is inexact
            double dX = speed * T - fmax(0., last[0] - pos_x[s]);
            dX = fmax(0., dX);
            v += dX;
        }
        if (tid == 1) v = 0.;
        P[R.target() + tid] = v;
    }
}

// step.hip: done = 0, flags = {isSafety = 1 (:326), passes 0, -1, 0}, u = 0 for scenes [0, S)
void launch_step_begin(int S, int *done, int *flags, double *u, hipStream_t stream);

}  // namespace amk

// the control step's device workspace, allocated by the first step of either path
inline int ensure_step_workspace(amk_mpc *mpc) {
    if (mpc->done.p) return AMK_OK;
    const size_t S = mpc->S, N = mpc->N, K = mpc->K;
    AMK_HIP(mpc->knn_pts.alloc(S * N * K * 3));
    AMK_HIP(mpc->knn_d2.alloc(S * N * K));
    AMK_HIP(mpc->edge_pt.alloc(S * 3));
    AMK_HIP(mpc->edge_d2.alloc(S));
    AMK_HIP(mpc->ref_states.alloc(S * mpc->nref));
    AMK_HIP(mpc->done.alloc(S));
    return AMK_OK;
}

inline bool step_params_ok(const amk_mpc *mpc, const amk_step_params *prm) {
    return prm->mpc_max_iter >= 1 && prm->mpc_max_iter <= AMK_MAX_OUTER_ITER && mpc->K >= 1;
}
