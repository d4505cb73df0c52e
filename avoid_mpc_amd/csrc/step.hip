// One control step for a batch of scenes on gfx950: the TASK branch of AvoidanceStateMachine::Step
// (AM/src/AvoidanceStateMachine.cpp:322-355) with the single-frame FrameKDMap queries it makes
// (AM/src/FrameKDMap.cpp:254-275,322-427), as a fixed sequence of kernels on one stream -- no host
// round trip between the dual-KD-tree queries, the packing of P and the solves.
//
// Per outer iteration (<= mpc_max_iter):
//   step_knn_grid_kernel   one launch for both trees: the N K-NN queries at the reference points in the obstacle index
//                          (:204-215) and the 1-NN of reference point 0 in the edge index (:270), through the bucketed
//                          indices (step_scan_kernel<5> / <1>: the same through the streaming-scan cross-check path)
//   step_plan_pack_kernel  PlanWapionts: nearest-obstacle test, snap to the edge point, re-query (:259-281), then
//                          ProcessWaypoints padding/needReplan, early exit, GetRefStates      (:216-257,333-335)
//   mpc_solve_kernel       Solve + refill of the reference path                                (:337-342)
// The multi-frame map (keyframes, PtIsInFrame fast path, per-frame merge) is step_frames.hip.
#include <type_traits>

#include "step_common.h"

using namespace amk;

namespace {

__global__ void step_begin_kernel(int S, int *__restrict__ done, int *__restrict__ flags, double *__restrict__ u) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    done[s] = 0;
    flags[4 * s + 0] = 1;   // isSafety = true (:326)
    flags[4 * s + 1] = 0;
    flags[4 * s + 2] = -1;
    flags[4 * s + 3] = 0;
    u[4 * s + 0] = u[4 * s + 1] = u[4 * s + 2] = u[4 * s + 3] = 0.0;
}

// Raw k nearest neighbours (nanoflann's own answer: min(k, size) entries, no adaptor count rule) of
// n_queries reference points per scene; queries are read in place from the reference path
// (stride 10 doubles).  Empty slots: distance DBL_MAX.
template <int QPW>
__global__ __launch_bounds__(512) void step_scan_kernel(const float *__restrict__ X, const float *__restrict__ Y,
                                                        const float *__restrict__ Z, int cap,
                                                        const int *__restrict__ sizes,
                                                        const float *__restrict__ pmaxs, int n_scenes,
                                                        const double *__restrict__ ref_path, int N, int n_queries,
                                                        int k, float *__restrict__ out_pts,
                                                        double *__restrict__ out_d2, const int *__restrict__ done) {
    const int groups = (n_queries + QPW - 1) / QPW;
    const int wpb = blockDim.x >> 6;
    const WaveSlot m = wave_slot(groups, wpb);  // all blocks of a scene share one XCD's L2; its waves one CU's L1
    const int s = m.s, w = m.w, g = m.unit, lane = m.lane;
    if (s >= n_scenes || g >= groups || done[s]) return;
    const int size = sizes[s];
    const float *xs = X + (size_t)s * cap, *ys = Y + (size_t)s * cap, *zs = Z + (size_t)s * cap;
    extern __shared__ __attribute__((aligned(16))) unsigned char scan_smem[];
    ScanLds<QPW> *ws = reinterpret_cast<ScanLds<QPW> *>(scan_smem) + w;
    double *qt = reinterpret_cast<double *>(reinterpret_cast<ScanLds<QPW> *>(scan_smem) + wpb) + w * QPW * 3;
    const int q0 = g * QPW;
    const int nvalid = n_queries - q0 < QPW ? n_queries - q0 : QPW;
    if (lane < QPW * 3) {  // queries = positions of the reference points (stride 10 in mRefPath)
        const int qq = lane / 3 < nvalid ? lane / 3 : nvalid - 1;
        qt[lane] = ref_path[((size_t)s * N + q0 + qq) * SD + lane % 3];
    }
    scan_cloud<QPW>(xs, ys, zs, size, pmaxs[s], qt, 3, k, ws);
    for (int qq = 0; qq < nvalid; ++qq) {
        const size_t row = (size_t)s * n_queries + q0 + qq;
        if (lane < k) {
            const int li = ws->li[qq][lane];
            const bool ok = li != kNoIndex;
            store_nbr(out_pts, out_d2, row * k + lane, ok, ws->ld[qq][lane], ok ? xs[li] : 0.f, ok ? ys[li] : 0.f,
                      ok ? zs[li] : 0.f);
        }
    }
}

// ---- AMK_TIES_AUTO (either handle): the same pass with tie detection in the queries that answer it, the reference-shaped tree
// built lazily on the device for the scenes where something tied, and only the tied rows answered again by its traversal.
// Every launch is unconditional (the host never learns whether anything tied): where nothing did, they return at once.
struct StepAuto {
    int obs, edge;               // the handle is in AMK_TIES_AUTO (and its flags are current)
    int eager_obs, eager_edge;   // the handle is in AMK_TIES_NANOFLANN with a current tree: every row goes through it, as in step_knn_exact_kernel
    ExactPtrs tobs, tedge;
    int *need_obs, *need_edge;
    const int *built_obs, *built_edge;
    int *row_obs;                // [S][N] tie flag of obstacle query (s, q) of this pass
    int *row_edge;               // [S]    tie flag of the edge query
    int *requery_tied;           // [S]    the re-query of the snapped point tied in this pass
};

// Same outputs through the bucketed indices (kd_grid.h), both trees in one launch: wavefront q < N answers
// the K-NN of reference point q in the obstacle index, wavefront q == N the 1-NN of reference point 0 in
// the edge index (the Edge-KD-tree query of PlanWapionts, :270).
// AUTO (step_knn_grid_auto_kernel): one more candidate and the tie test for the handles in AMK_TIES_AUTO (raw results, so every one
// of the k slots counts -- there is no adaptor count rule here).
template <bool AUTO>
__device__ __forceinline__ void step_knn_grid_row(const GridPtrs &gobs, const GridPtrs &gedge, int n_scenes,
    const double *ref_path, int N, int K, float *knn_pts, double *knn_d2,
    float *edge_pt, double *edge_d2, const int *done, const StepAuto &au) {
    __shared__ GridWaveLds wl[4];
    const int nq = N + 1;
    const WaveSlot m = wave_slot(nq);
    const int s = m.s, q = m.unit, lane = m.lane;
    if (s >= n_scenes || q >= nq || done[s]) return;
    const bool is_edge = q == N;
    const double *qp = ref_path + ((size_t)s * N + (is_edge ? 0 : q)) * SD;  // read in place from mRefPath
    const int k = is_edge ? 1 : K;
    const bool detect = AUTO && (is_edge ? au.edge : au.obs);   // (wave-uniform)
    double ld;
    int li, lpos;
    const GridScene gs = is_edge ? gedge.scene(s) : gobs.scene(s);
    grid_knn(gs, qp[0], qp[1], qp[2], detect ? k + 1 : k, ld, li, lpos, &wl[m.w]);
    if (detect) {
        const bool any = wave_tie(ld, li, lane, k);
        if (lane == 0) {
            if (is_edge) au.row_edge[s] = any;
            else au.row_obs[(size_t)s * N + q] = any;
            if (any) (is_edge ? au.need_edge : au.need_obs)[s] = 1;   // (every wavefront that raises it stores the same value)
        }
    }
    if (lane < k) {
        const bool ok = li != kNoIndex;
        const float4 rec = gs.pt[lpos];  // the neighbour's coordinates (lpos = 0 for an empty slot: a valid address)
        if (is_edge) store_nbr(edge_pt, edge_d2, s, ok, ld, rec.x, rec.y, rec.z);
        else store_nbr(knn_pts, knn_d2, ((size_t)s * N + q) * K + lane, ok, ld, rec.x, rec.y, rec.z);
    }
}
// <= 48 VGPRs: a CU that holds its 8 solve waves (2 x 232 registers per SIMD, 142.6 of 160 KB of LDS since round 5) still
// has 48 registers per SIMD and 17 KB of LDS free -- exactly one block of this kernel (one wave per SIMD), which then runs
// in the issue slots the latency-bound solves leave empty instead of waiting for a CU to drain.
__global__ __launch_bounds__(256) void step_knn_grid_kernel(GridPtrs gobs, GridPtrs gedge, int n_scenes,
    const double *__restrict__ ref_path, int N, int K, float *__restrict__ knn_pts, double *__restrict__ knn_d2,
    float *__restrict__ edge_pt, double *__restrict__ edge_d2, const int *__restrict__ done) {
    step_knn_grid_row<false>(gobs, gedge, n_scenes, ref_path, N, K, knn_pts, knn_d2, edge_pt, edge_d2, done, StepAuto{});
}
// (a kernel of its own: the default one keeps its 48 registers)
__global__ __launch_bounds__(256) void step_knn_grid_auto_kernel(GridPtrs gobs, GridPtrs gedge, int n_scenes,
    const double *__restrict__ ref_path, int N, int K, float *__restrict__ knn_pts, double *__restrict__ knn_d2,
    float *__restrict__ edge_pt, double *__restrict__ edge_d2, const int *__restrict__ done, StepAuto au) {
    step_knn_grid_row<true>(gobs, gedge, n_scenes, ref_path, N, K, knn_pts, knn_d2, edge_pt, edge_d2, done, au);
}

// The StepAuto policy of step_knn_exact_row (step_common.h), for a pair of handles of which at least one is in AMK_TIES_AUTO: of
// such a handle only the rows the kernel above flagged, and only where the scene's tree is built; a handle in AMK_TIES_NANOFLANN
// every row, as with ExactPair.
__device__ __forceinline__ bool exact_used(const StepAuto &au, int, bool edge) {
    return edge ? (au.edge || au.eager_edge) : (au.obs || au.eager_obs);
}
__device__ __forceinline__ bool exact_row_wanted(const StepAuto &au, int, bool edge, int s, int q, int N) {
    if (!(edge ? au.edge : au.obs)) return true;   // (AMK_TIES_NANOFLANN)
    if (edge) return au.row_edge[s] && au.built_edge[s];
    return au.row_obs[(size_t)s * N + q] && au.built_obs[s];
}
__device__ __forceinline__ ExactTree exact_scene(const StepAuto &au, int, bool edge, int s) {
    return edge ? au.tedge.scene(s) : au.tobs.scene(s);
}
__global__ __launch_bounds__(256) void step_knn_exact_auto_kernel(StepAuto au, int n_scenes, const double *__restrict__ ref_path,
    int N, int K, FrameBufs fb, const int *__restrict__ done) {
    step_knn_exact_row(au, 0, n_scenes, ref_path, N, K, fb, done);
}

// PlanWapionts (:259-281) for reference point 0; called by the one wavefront that owns scene s.
// AUTO (obstacle handle in AMK_TIES_AUTO mode, GRID only): the re-query of the snapped point asks for K + 1 neighbours and makes
// the tie test (wave_tie) on them (raw results: every slot counts); a tie raises the scene's `need` word for the lazy
// tree build behind this kernel and `requery_tied`, which has step_requery_pack_auto_kernel redo the re-query in that tree.
template <bool EXACT, bool GRID, bool AUTO = false>
__device__ __forceinline__ void plan_scene(int s, GridPtrs gpt, ExactPtrs eobs,
                                                          const float *__restrict__ X, const float *__restrict__ Y,
                                                          const float *__restrict__ Z, int cap,
                                                          const int *__restrict__ sizes_obs,
                                                          const float *__restrict__ pmax_obs,
                                                          const int *__restrict__ sizes_edge, int N, int K,
                                                          double safety_distance, double *__restrict__ ref_path,
                                                          float *__restrict__ knn_pts, double *__restrict__ knn_d2,
                                                          const float *__restrict__ edge_pt,
                                                          const double *__restrict__ edge_d2,
                                                          int *__restrict__ flags, int *__restrict__ need = nullptr,
                                                          int *__restrict__ requery_tied = nullptr) {
    const int lane = threadIdx.x;
    const int size_o = sizes_obs[s];
    // GetNearestDistance (FrameKDMap.cpp:400-427): SearchForNearest(p, 1) -> no result unless the cloud
    // holds more than one point (kd_tree_two.h:119-124); DBL_MAX then.
    const double d2n = (size_o > 1) ? knn_d2[(size_t)s * N * K] : DBL_MAX;
    const double nearest = sqrt(d2n);
    int is_safety = 1;
    if (!(nearest > safety_distance)) {
        // QueryNearest(p1, 1, edgePts, distances, true) (:270): one result iff the edge cloud has > 1 point
        const bool has_edge = sizes_edge[s] > 1 && edge_d2[s] < DBL_MAX;
        if (!has_edge) {
            is_safety = 0;
        } else {
            double *p1 = ref_path + (size_t)s * N * SD;
            const double ex = (double)edge_pt[3 * s + 0], ey = (double)edge_pt[3 * s + 1], ez = (double)edge_pt[3 * s + 2];
            // the snapped point is what ProcessWaypoints queries next (:210-215): redo query 0
            const float *xs = X + (size_t)s * cap, *ys = Y + (size_t)s * cap, *zs = Z + (size_t)s * cap;
            // GRID is a template parameter: the streaming-scan cross-check path (amk__kd_set_mode) brought its registers and
            // LDS into the default kernel (93 VGPRs; 58 without it -- few enough to run beside the solves' waves)
            __shared__ typename std::conditional<GRID, int, ScanLds<1>>::type ws1_store;
            __shared__ typename std::conditional<GRID, GridWaveLds, int>::type wl1_store;
            __shared__ double q1[3];
            double gld = DBL_MAX;
            int gli = kNoIndex, glpos = 0;
            const GridScene gs = gpt.scene(s);
            int sli = kNoIndex;
            double sld = DBL_MAX;
            if constexpr (GRID) {
                grid_knn(gs, ex, ey, ez, AUTO ? K + 1 : K, gld, gli, glpos, &wl1_store);
                if constexpr (AUTO)
                    if (wave_tie(gld, gli, lane, K) && lane == 0) { need[s] = 1; requery_tied[s] = 1; }
            } else {
                ScanLds<1> &ws1 = ws1_store;
                q1[0] = ex; q1[1] = ey; q1[2] = ez;  // every lane stores the same values
                scan_cloud<1>(xs, ys, zs, size_o, pmax_obs[s], q1, 3, K, &ws1);
                if (lane < K) { sli = ws1.li[0][lane]; sld = ws1.ld[0][lane]; }
            }
            if (lane < K) {
                const int li = GRID ? gli : sli;
                const bool ok = li != kNoIndex;
                float nx = 0.f, ny = 0.f, nz = 0.f;
                if (GRID) {
                    const float4 rec = gs.pt[glpos];
                    nx = rec.x; ny = rec.y; nz = rec.z;
                } else if (ok) {
                    nx = xs[li]; ny = ys[li]; nz = zs[li];
                }
                store_nbr(knn_pts, knn_d2, (size_t)s * N * K + lane, ok, GRID ? gld : sld, nx, ny, nz);
            }
            if constexpr (EXACT) exact_requery(eobs.scene(s), ex, ey, ez, K, knn_pts, knn_d2, (size_t)s * N);
            if (lane == 0) {
                p1[0] = ex;
                p1[1] = ey;
                p1[2] = ez;
            }
        }
    }
    if (lane == 0) flags[4 * s + 0] = is_safety;
}

// pack_ref_states (step_common.h) for the one wavefront that owns scene s
__device__ __forceinline__ void pack_scene(int s, const int *__restrict__ sizes_obs, int N, int K, int nref,
                                                          int iter, int max_iter, double speed, double T,
                                                          double safety_distance,
                                                          const double *__restrict__ state_quad,
                                                          const double *__restrict__ pos_x,
                                                          const double *__restrict__ ref_path,
                                                          const float *__restrict__ knn_pts,
                                                          const double *__restrict__ knn_d2,
                                                          double *__restrict__ ref_states, int *__restrict__ done,
                                                          const int *__restrict__ flags) {
    // iter < 0: the scene's own pass counter (the solves it has finished this step, flags[1]) -- with an iteration budget on the
    // solve (amk_mpc_set_solve_budget) the scenes of a launch are no longer in the same pass
    if (iter < 0) iter = flags[4 * s + 1];
    // QueryNearest through either path returns K points iff the cloud holds more than K, else none
    // (FrameKDMap.cpp:298,339-345 + kd_tree_two.h:119-124)
    const int cnt = sizes_obs[s] > K ? K : 0;
    pack_ref_states(threadIdx.x, kWave, s, N, K, nref, iter, max_iter, speed, T, safety_distance, flags[4 * s + 0],
                    [cnt](int) { return cnt; }, state_quad, pos_x, ref_path + (size_t)s * N * SD, knn_pts, knn_d2,
                    ref_states, done);
}

// PlanWapionts, then ProcessWaypoints' bookkeeping + GetRefStates, for scene s = blockIdx.x (one wavefront): the
// second half reads what the first one wrote for this scene only (snapped point, its neighbours, isSafety).
// EXACT (obstacle handle in AMK_TIES_NANOFLANN mode) is a template parameter, not a flag: the traversal's stack lives in
// scratch memory, and a kernel that MAY use scratch makes every hardware queue reserve it (with 32 queues in flight the
// default path ran out of resources when the two shared one kernel).
template <bool EXACT, bool GRID>
__global__ __launch_bounds__(kWave) void step_plan_pack_kernel(
    GridPtrs gpt, ExactPtrs eobs, const float *__restrict__ X, const float *__restrict__ Y, const float *__restrict__ Z,
    int cap, const int *__restrict__ sizes_obs, const float *__restrict__ pmax_obs, const int *__restrict__ sizes_edge,
    int N, int K, int nref, int iter, int max_iter, double speed, double T, double safety_distance,
    const double *__restrict__ state_quad, const double *__restrict__ pos_x, double *__restrict__ ref_path,
    float *__restrict__ knn_pts, double *__restrict__ knn_d2, const float *__restrict__ edge_pt,
    const double *__restrict__ edge_d2, double *__restrict__ ref_states, int *__restrict__ done,
    int *__restrict__ flags) {
    const int s = blockIdx.x;
    if (done[s]) return;
    plan_scene<EXACT, GRID>(s, gpt, eobs, X, Y, Z, cap, sizes_obs, pmax_obs, sizes_edge, N, K, safety_distance, ref_path, knn_pts,
               knn_d2, edge_pt, edge_d2, flags);
    __threadfence_block();
    __syncthreads();
    pack_scene(s, sizes_obs, N, K, nref, iter, max_iter, speed, T, safety_distance, state_quad, pos_x, ref_path, knn_pts,
               knn_d2, ref_states, done, flags);
}

// Obstacle handle in AMK_TIES_AUTO: the two halves of step_plan_pack_kernel as two kernels, because the tree the snapped point's
// re-query may need can only be built between them (the query point is computed by the first half).
__global__ __launch_bounds__(kWave) void step_plan_auto_kernel(
    GridPtrs gpt, const int *__restrict__ sizes_obs, const int *__restrict__ sizes_edge, int N, int K, double safety_distance,
    double *__restrict__ ref_path, float *__restrict__ knn_pts, double *__restrict__ knn_d2, const float *__restrict__ edge_pt,
    const double *__restrict__ edge_d2, const int *__restrict__ done, int *__restrict__ flags, int *__restrict__ need,
    int *__restrict__ requery_tied) {
    const int s = blockIdx.x;
    if (done[s]) return;
    if (threadIdx.x == 0) requery_tied[s] = 0;   // (raised again below by the same lane)
    plan_scene<false, true, true>(s, gpt, ExactPtrs{}, nullptr, nullptr, nullptr, 0, sizes_obs, nullptr, sizes_edge, N, K,
                                  safety_distance, ref_path, knn_pts, knn_d2, edge_pt, edge_d2, flags, need, requery_tied);
}
// ... the second half: where the re-query tied and the scene's tree is built, exact_requery at the snapped point (reference
// point 0, where plan_scene left it), as step_plan_pack_kernel<true, true> makes it for every snap; then pack_scene.
__global__ __launch_bounds__(kWave) void step_requery_pack_auto_kernel(
    ExactPtrs eobs, const int *__restrict__ requery_tied, const int *__restrict__ built, const int *__restrict__ sizes_obs, int N,
    int K, int nref, int iter, int max_iter, double speed, double T, double safety_distance,
    const double *__restrict__ state_quad, const double *__restrict__ pos_x, const double *__restrict__ ref_path,
    float *__restrict__ knn_pts, double *__restrict__ knn_d2, double *__restrict__ ref_states, int *__restrict__ done,
    const int *__restrict__ flags) {
    const int s = blockIdx.x;
    if (done[s]) return;
    if (requery_tied[s] && built[s]) {   // (block-uniform)
        const double *p1 = ref_path + (size_t)s * N * SD;
        exact_requery(eobs.scene(s), p1[0], p1[1], p1[2], K, knn_pts, knn_d2, (size_t)s * N);
        __threadfence_block();
        __syncthreads();
    }
    pack_scene(s, sizes_obs, N, K, nref, iter, max_iter, speed, T, safety_distance, state_quad, pos_x, ref_path, knn_pts,
               knn_d2, ref_states, done, flags);
}

}  // namespace

void amk::launch_step_begin(int S, int *done, int *flags, double *u, hipStream_t stream) {
    hipLaunchKernelGGL(step_begin_kernel, dim3((S + 255) / 256), dim3(256), 0, stream, S, done, flags, u);
}

// Internal (tools/experiments, bench.py AMK_BENCH_SKIP): leave kernel classes out of amk_step_batch to see what each costs
// with the others in flight -- bit 0 queries, bit 1 plan/pack, bit 2 solves.  Results are garbage while set.
static int g_diag_skip = 0;
extern "C" void amk__diag_skip(int mask) { g_diag_skip = mask; }

// Internal (tests): host copy of the packed parameter vectors P the newest pass of the last step -- either path -- handed to the
// solve: the first min(n, S nref) doubles of the workspace, after a device-wide wait.  No step has run yet: AMK_ERR_INVALID_ARG.
extern "C" int amk__mpc_ref_states(amk_mpc *mpc, double *h_out, long long n) {
    if (!mpc || !h_out || n < 0 || !mpc->ref_states.p) return AMK_ERR_INVALID_ARG;
    const long long have = (long long)mpc->S * mpc->nref;
    return read_back({{h_out, mpc->ref_states.p, sizeof(double) * (size_t)(n < have ? n : have)}});
}

extern "C" int amk_step_batch(amk_kd *obstacle, amk_kd *edge, amk_mpc *mpc, const amk_step_params *prm,
                              const double *d_state_quad, const double *d_pos_x, double *d_ref_path, double *d_u,
                              double *d_x0array, int *d_flags, void *stream_) {
    if (!obstacle || !edge || !mpc || !prm || !d_state_quad || !d_pos_x || !d_ref_path || !d_u || !d_flags)
        return AMK_ERR_INVALID_ARG;
    if (obstacle->n_scenes != mpc->S || edge->n_scenes != mpc->S) return AMK_ERR_INVALID_ARG;
    if (!step_params_ok(mpc, prm)) return AMK_ERR_INVALID_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    const int N = mpc->N, K = mpc->K;
    // AMK_TIES_AUTO on the obstacle handle asks the bucketed index for K + 1 neighbours (the rule of amk_kd_tie_flags)
    if (obstacle->mode == 0 && edge->mode == 0 && obstacle->tie_order == AMK_TIES_AUTO && K + 1 > AMK_MAX_K) return AMK_ERR_UNSUPPORTED;
    if (int st = ensure_step_workspace(mpc); st != AMK_OK) return st;
    const int S = mpc->launch_scenes();   // (amk_pipeline: a gang that is not full runs its leading scenes only)
    { TimedLaunch tl(KC_BEGIN, stream);
    launch_step_begin(S, mpc->done.p, d_flags, d_u, stream); }
    int qpw, groups, wpb;
    scan_geometry(N, qpw, groups, wpb);
    const int use_grid = (obstacle->mode == 0 && edge->mode == 0) ? 1 : 0;
    if (!use_grid) {  // the streaming-scan cross-check path reads the index-ordered planes
        int st = amk__kd_ensure_soa(obstacle, stream_);
        if (st == AMK_OK) st = amk__kd_ensure_soa(edge, stream_);
        if (st != AMK_OK) return st;
    }
    const GridPtrs gobs = grid_ptrs(obstacle), gedge = grid_ptrs(edge);
    // handles in AMK_TIES_NANOFLANN mode (their reference-shaped trees were built by amk_kd_build)
    ExactPair ex{};
    ex.use_obs = use_grid && obstacle->tie_order == AMK_TIES_NANOFLANN && obstacle->ex_valid;
    ex.use_edge = use_grid && edge->tie_order == AMK_TIES_NANOFLANN && edge->ex_valid;
    if (ex.use_obs) ex.obs = amk_exact_ptrs(obstacle);
    if (ex.use_edge) ex.edge = amk_exact_ptrs(edge);
    // handles in AMK_TIES_AUTO mode (their trees are built by this step, on the device, where a query ties)
    const bool au_obs = use_grid && obstacle->auto_on(), au_edge = use_grid && edge->auto_on();
    StepAuto au{};
    if (au_obs || au_edge) {
        au.obs = au_obs; au.edge = au_edge; au.eager_obs = ex.use_obs; au.eager_edge = ex.use_edge;
        if (au_obs || ex.use_obs) au.tobs = amk_exact_ptrs(obstacle);
        if (au_edge || ex.use_edge) au.tedge = amk_exact_ptrs(edge);
        if (au_obs) { au.need_obs = obstacle->au_need(); au.built_obs = obstacle->au_built(); au.row_obs = obstacle->au_rowflag.p;
                      au.requery_tied = obstacle->au_requery(); }
        if (au_edge) { au.need_edge = edge->au_need(); au.built_edge = edge->au_built(); au.row_edge = edge->au_rowflag.p; }
    }
    const FrameBufs out{mpc->knn_pts.p, mpc->knn_d2.p, mpc->edge_pt.p, mpc->edge_d2.p};
    // Rounds.  Plain schedule (no budget): round r IS pass r of every scene still in the loop, mpc_max_iter rounds.  With an
    // iteration budget B (amk_mpc_set_solve_budget) a solve launch of the first `budget_rounds` rounds ends after B iterations per
    // scene; a scene that is not finished by then pauses (done[s] = 2), sits out the next round's queries and packing, and is
    // resumed INSIDE that round's solve launch beside the fresh solves of the scenes that moved on.  Every scene still makes its
    // passes in order with the reference's data flow (queries at ITS refilled path, its own pass counter for GetCurStateQuad and
    // the early exit), so the results are the plain schedule's bit for bit; what changes is that a launch no longer lasts as
    // long as its slowest scene.  The rounds behind the budgeted ones run without a budget: a scene that enters them in pass p
    // needs mpc_max_iter - p of them, hence mpc_max_iter catch-up rounds (a round nobody needs is three empty launches).
    const int mi = prm->mpc_max_iter;
    const int budget = (g_diag_skip & 4) ? 0 : mpc->solve_budget;
    const int brounds = budget > 0 ? (mpc->budget_rounds > 0 ? mpc->budget_rounds : mi - 1) : 0;
    const int rounds = budget > 0 && brounds > 0 ? brounds + mi : mi;
    const bool per_scene = rounds != mi;
    for (int iter = 0; iter < rounds; ++iter) {
        if (g_diag_skip & 1) {
        } else if (au_obs || au_edge) {
            TimedLaunch tl(KC_SCAN_OBS, stream);
            hipLaunchKernelGGL(step_knn_grid_auto_kernel, dim3((unsigned)search_blocks(S, N + 1)), dim3(256), 0, stream, gobs, gedge, S,
                               d_ref_path, N, K, mpc->knn_pts.p, mpc->knn_d2.p, mpc->edge_pt.p, mpc->edge_d2.p,
                               mpc->done.p, au);
            if (int st = kd_auto_build(au_obs ? obstacle : nullptr, au_edge ? edge : nullptr, stream); st != AMK_OK) return st;
            hipLaunchKernelGGL(step_knn_exact_auto_kernel, dim3((S * (N + 1) + 3) / 4), dim3(256), 0, stream, au, S, d_ref_path,
                               N, K, out, mpc->done.p);
        } else if (use_grid) {
            TimedLaunch tl(KC_SCAN_OBS, stream);
            hipLaunchKernelGGL(step_knn_grid_kernel, dim3((unsigned)search_blocks(S, N + 1)), dim3(256), 0, stream, gobs, gedge, S,
                               d_ref_path, N, K, mpc->knn_pts.p, mpc->knn_d2.p, mpc->edge_pt.p, mpc->edge_d2.p,
                               mpc->done.p);
            if (ex.use_obs || ex.use_edge)
                hipLaunchKernelGGL(step_knn_exact_kernel<ExactPair>, dim3((S * (N + 1) + 3) / 4), dim3(256), 0, stream, ex, S,
                                   d_ref_path, N, K, out, mpc->done.p);
        } else {
        { TimedLaunch tl(KC_SCAN_OBS, stream);
        hipLaunchKernelGGL(step_scan_kernel<5>, dim3((unsigned)search_blocks(S, groups, wpb)), dim3(wpb * kWave), scan_lds_bytes<5>(wpb), stream,
                           obstacle->x.p, obstacle->y.p, obstacle->z.p, obstacle->cap, obstacle->size.p,
                           obstacle->pmax.p, S, d_ref_path, N, N, K, mpc->knn_pts.p, mpc->knn_d2.p, mpc->done.p); }
        { TimedLaunch tl(KC_SCAN_EDGE, stream);
        hipLaunchKernelGGL(step_scan_kernel<1>, dim3((unsigned)search_blocks(S, 1, 1)), dim3(kWave), scan_lds_bytes<1>(1), stream, edge->x.p,
                           edge->y.p, edge->z.p, edge->cap, edge->size.p, edge->pmax.p, S, d_ref_path, N, 1, 1,
                           mpc->edge_pt.p, mpc->edge_d2.p, mpc->done.p); }
        }
        if (!(g_diag_skip & 2) && au_obs) { TimedLaunch tl(KC_PLAN, stream);
        hipLaunchKernelGGL(step_plan_auto_kernel, dim3(S), dim3(kWave), 0, stream, gobs, obstacle->size.p, edge->size.p, N, K,
                           prm->safety_distance, d_ref_path, mpc->knn_pts.p, mpc->knn_d2.p, mpc->edge_pt.p, mpc->edge_d2.p,
                           mpc->done.p, d_flags, obstacle->au_need(), obstacle->au_requery());
        if (int st = kd_auto_build(obstacle, nullptr, stream); st != AMK_OK) return st;
        hipLaunchKernelGGL(step_requery_pack_auto_kernel, dim3(S), dim3(kWave), 0, stream, au.tobs, obstacle->au_requery(),
                           obstacle->au_built(), obstacle->size.p, N, K, mpc->nref, per_scene ? -1 : iter, prm->mpc_max_iter,
                           prm->speed, mpc->T, prm->safety_distance, d_state_quad, d_pos_x, d_ref_path, mpc->knn_pts.p,
                           mpc->knn_d2.p, mpc->ref_states.p, mpc->done.p, d_flags);
        } else if (!(g_diag_skip & 2)) { TimedLaunch tl(KC_PLAN, stream);
        auto plan_kernel = step_plan_pack_kernel<false, true>;
        if (!use_grid) plan_kernel = step_plan_pack_kernel<false, false>;
        else if (ex.use_obs) plan_kernel = step_plan_pack_kernel<true, true>;
        hipLaunchKernelGGL(plan_kernel, dim3(S), dim3(kWave), 0, stream, gobs, ex.obs, obstacle->x.p,
                           obstacle->y.p, obstacle->z.p, obstacle->cap, obstacle->size.p, obstacle->pmax.p, edge->size.p, N,
                           K, mpc->nref, per_scene ? -1 : iter, prm->mpc_max_iter, prm->speed, mpc->T, prm->safety_distance, d_state_quad,
                           d_pos_x, d_ref_path, mpc->knn_pts.p, mpc->knn_d2.p, mpc->edge_pt.p, mpc->edge_d2.p,
                           mpc->ref_states.p, mpc->done.p, d_flags); }
        AMK_HIP(hipGetLastError());
        if (g_diag_skip & 4) continue;
        int st = launch_solve(mpc, mpc->ref_states.p, d_u, d_x0array, nullptr, mpc->done.p, d_ref_path, d_flags, stream,
                              per_scene && iter < brounds ? budget : 0, per_scene ? mi : 0);
        if (st != AMK_OK) return st;
    }
    return AMK_OK;
}

extern "C" int amk_step_batch_host(amk_kd *obstacle, amk_kd *edge, amk_mpc *mpc, const amk_step_params *prm,
                                   const double *h_state_quad, const double *h_pos_x, double *h_ref_path, double *h_u,
                                   double *h_x0array, int *h_flags) {
    if (!mpc || !prm || !h_state_quad || !h_pos_x || !h_ref_path || !h_u || !h_flags) return AMK_ERR_INVALID_ARG;
    if (!step_params_ok(mpc, prm)) return AMK_ERR_INVALID_ARG;
    const size_t S = mpc->S, N = mpc->N, mi = prm->mpc_max_iter;
    enum { STATE_QUAD, POS_X, REF_PATH, U, X0ARRAY, FLAGS };
    return mpc->stage.call({to_device(h_state_quad, sizeof(double) * S * mi * SD), to_device(h_pos_x, sizeof(double) * S),
                            both_ways(h_ref_path, sizeof(double) * S * N * SD), to_host(h_u, sizeof(double) * S * 4),
                            to_host(h_x0array, sizeof(double) * S * N * 14), to_host(h_flags, sizeof(int) * S * 4)},
                           [&](const HostStage::Dev *d) {
                               return amk_step_batch(obstacle, edge, mpc, prm, d[STATE_QUAD], d[POS_X], d[REF_PATH], d[U], d[X0ARRAY],
                                                     d[FLAGS], nullptr);
                           },
                           hipDeviceSynchronize);
}

#ifdef AMK_KNN_COUNT
extern "C" int amk__knn_counters(unsigned long long *h8, int reset) {   // diagnostics build only: step.hip's copy of grid_knn's counters
    if (hipDeviceSynchronize() != hipSuccess) return AMK_ERR_HIP;
    if (hipMemcpyFromSymbol(h8, HIP_SYMBOL(amk::g_knn_cnt), sizeof(unsigned long long) * 8) != hipSuccess) return AMK_ERR_HIP;
    if (reset) { unsigned long long z[8] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(amk::g_knn_cnt), z, sizeof z) != hipSuccess) return AMK_ERR_HIP; }
    return AMK_OK;
}
#endif
