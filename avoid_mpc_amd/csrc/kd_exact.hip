// The reference-shaped tree of the KD index for gfx950 (kd_exact.h says why it exists): its arrays, its build kernels, its two
// search kernels and the handle's tie-order calls.  Three callers build it, all through ONE kernel pair template (its gate):
//   AMK_TIES_NANOFLANN (exact_build)                 every scene of a handle, behind every index build and keyframe sweep;
//   AMK_TIES_AUTO (amk::kd_auto_build)               the scenes where a query tied, behind every search and step pass;
//   the keyframe map's pools (kd_pool_exact_build)   the pool scenes that the rows of a mapped build or of a sweep name.
// The bucketed index -- build, searches, the rest of the handle's C ABI -- is kd_index.hip.
#include "kd_exact_build.h"

// ---- the tree's arrays (amk_common.h: ExactStore) ------------------------------------------------------------------
int amk::ExactStore::alloc(int scenes, int cap) {
    if (allocated()) return AMK_OK;
    max_nodes = (int)nodes_for(cap);
    for (int i = 0; i < kCount; ++i)
        if (const hipError_t e = buf[i].alloc((size_t)array_bytes((Id)i, scenes, cap)); e != hipSuccess) {
            release();   // all or none: a later call starts over instead of taking what is there for complete
            return amk::hip_fail(e);
        }
    return AMK_OK;
}

// ---- build: one kernel pair, gated per workgroup -------------------------------------------------------------------
// The guard of every build: nanoflann's divideTree compares coordinates against split planes and is undefined on a NaN or an
// infinity (the reference's own header ends with a segmentation fault on most clouds that keep such a point; some build and
// then prune wrongly).  A scene whose bucketed index holds anything in its trash bucket does not start the build: its tree is
// marked unavailable (amk_kd_exact_status: AMK_EXACT_GAVE_UP), the bucketed index answers.  Decided on the device, from
// the index the build kernel has just written on the same stream.  Block-uniform.
__device__ __forceinline__ bool exact_refused(const amk::GridScene &gs, const amk::ExactTree &T) {
    if (amk::grid_trash_count(gs) == 0) return false;
    if (threadIdx.x == 0) *T.n_nodes = -1;   // (exact_build_rest then finds nothing to do and leaves it at -1)
    return true;
}
// grid = (rows, handles <= 2).  Workgroup (i, h) builds a scene of handle h -- which one, and whether at all, is the GATE the pair
// is instantiated with.  Launched unconditionally: the host never learns which workgroups built.
//   kGateNone   scene i                                                (AMK_TIES_NANOFLANN: every scene, one handle)
//   kGateLazy   scene i, unless !need[h][i] || built[h][i]             (AMK_TIES_AUTO: no query tied, or the tree is the cloud's already)
//   kGateRows   scene rows[i], unless that is < 0 or gate && !gate[i]  (the map's pools: no scene, or the sweep did not rebuild it)
// A compile-time gate: one pair that tested rows / gate / need for null at run time kept every resource figure, but its lower kernel
// took 1747 us against 1707 .. 1714 us per 256 x 50 k-point AMK_TIES_NANOFLANN build (profiles/exact_home_ab.txt).
enum ExactGate { kGateNone, kGateLazy, kGateRows };
struct ExactBuildArgs {
    struct Handle {
        amk::ExactPtrs ep;
        amk::GridPtrs grid;
        const int *sizes;
        const int *need;   // kGateLazy only, with:
        int *built;
        const float4 *gp;  //   the bucket records and the index-ordered planes they are scattered into
        float *x, *y, *z;
    } t[2];
    const int *rows, *gate;   // kGateRows only; gate may be null
};
template <int GATE>
__device__ __forceinline__ int exact_build_scene(const ExactBuildArgs &a, const ExactBuildArgs::Handle &t) {   // -1: not built (block-uniform)
    if constexpr (GATE == kGateRows) {
        const int m = a.rows[blockIdx.x];
        return m < 0 || (a.gate && !a.gate[blockIdx.x]) ? -1 : m;
    }
    const int s = blockIdx.x;
    if constexpr (GATE == kGateLazy)
        if (!t.need[s] || t.built[s]) return -1;
    return s;
}
// kGateLazy first makes the scene's index-ordered planes from its bucket records (kd_records_to_soa_kernel for one scene: the
// index build does not write them in this mode, which would be 12 bytes per point stored for nothing on the untied path).
// The scatter is what a tied scene pays over AMK_TIES_NANOFLANN, whose index build writes the planes coalesced: +0.29 ms per
// 256 x 50 k-point build.  (Measured and not kept: the scatter as a kernel of its own -- 12 blocks per scene in dispatch order
// 0.15 ms SLOWER, 16 or 64 blocks per scene pinned to the XCD s % 8 0.09 ms faster, which leaves 0.2 ms and costs every lazy
// build one more launch that returns at once on the untied path: profiles/tie_auto_cost.txt.)
template <int GATE>
__global__ __launch_bounds__(amk::kExactTopThreads) void kd_exact_build_top_kernel(const ExactBuildArgs a) {
    const ExactBuildArgs::Handle &t = a.t[GATE == kGateNone ? 0 : blockIdx.y];   // (scalar loads from the kernel-argument segment)
    const int s = exact_build_scene<GATE>(a, t);
    if (s < 0) return;
    if (exact_refused(t.grid.scene(s), t.ep.scene(s))) return;   // (the rest kernel still marks a lazy scene built: GAVE_UP)
    const int n = t.sizes[s];
    if constexpr (GATE == kGateLazy) {
        const int cap = t.ep.cap;
        const size_t base = (size_t)s * cap;
        const float4 *gp = t.gp + base;
        float *xs = t.x + base, *ys = t.y + base, *zs = t.z + base;
        const float qnan = __builtin_nanf("");
        for (int i = threadIdx.x; i < cap; i += amk::kExactTopThreads) {
            if (i < n) {
                const float4 r = gp[i];
                const int idx = __float_as_int(r.w);   // < n: the padding stores below touch other elements
                xs[idx] = r.x; ys[idx] = r.y; zs[idx] = r.z;
            } else {
                xs[i] = qnan; ys[i] = qnan; zs[i] = qnan;
            }
        }
        __threadfence_block();
        __syncthreads();   // the planes are read back by the tree build
    }
    amk::exact_build_top(t.ep.scene(s), n);
}
// exact_build_rest; a lazy scene's tree now belongs to the cloud held (also a tree that was given up: n_nodes = -1 says so)
template <int GATE>
__global__ __launch_bounds__(amk::kExactThreads) void kd_exact_build_kernel(const ExactBuildArgs a, int qcap) {
    const ExactBuildArgs::Handle &t = a.t[GATE == kGateNone ? 0 : blockIdx.y];   // (scalar loads from the kernel-argument segment)
    const int s = exact_build_scene<GATE>(a, t);
    if (s < 0) return;
    amk::exact_build_rest(t.ep.scene(s), t.sizes[s], qcap);
    if constexpr (GATE == kGateLazy)
        if (threadIdx.x == 0) t.built[s] = 1;
}
// tests only (tests/test_kd_gpu.py): a smaller ring of open nodes, so that the give-up path of exact_build_rest is reachable
// with a cloud that fits a test (0 = the compiled capacity)
static int g_exact_queue_cap = amk::kExactQueue;
extern "C" int amk__exact_set_queue_cap(int cap) {
    if (cap == 0) cap = amk::kExactQueue;
    if (cap < 2 || cap > amk::kExactQueue || (cap & (cap - 1))) return AMK_ERR_INVALID_ARG;
    g_exact_queue_cap = cap;
    return AMK_OK;
}
static ExactBuildArgs::Handle exact_build_handle(const amk_kd *kd, bool lazy) {
    ExactBuildArgs::Handle t{};
    t.ep = amk_exact_ptrs(kd);
    t.grid = grid_ptrs(kd);
    t.sizes = kd->size.p;
    if (lazy) {
        t.need = kd->au_need(); t.built = kd->au_built();
        t.gp = kd->gpt.p; t.x = kd->x.p; t.y = kd->y.p; t.z = kd->z.p;
    }
    return t;
}
// the pair for one handle or two (h1 null: one); d_rows / d_gate: kGateRows only
template <int GATE>
static int exact_build_launch(const amk_kd *h0, const amk_kd *h1, int n_rows, const int *d_rows, const int *d_gate, hipStream_t stream) {
    ExactBuildArgs a{};
    a.t[0] = exact_build_handle(h0, GATE == kGateLazy);
    if (h1) a.t[1] = exact_build_handle(h1, GATE == kGateLazy);
    a.rows = d_rows; a.gate = d_gate;
    const dim3 grid(n_rows, h1 ? 2 : 1);
    hipLaunchKernelGGL(kd_exact_build_top_kernel<GATE>, grid, dim3(amk::kExactTopThreads), 0, stream, a);
    hipLaunchKernelGGL(kd_exact_build_kernel<GATE>, grid, dim3(amk::kExactThreads), 0, stream, a, g_exact_queue_cap);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

// AMK_TIES_NANOFLANN: every scene, from the index-ordered planes (made on demand from the bucket records)
int exact_build(amk_kd *kd, hipStream_t stream) {
    int st = kd->exact.alloc(kd->n_scenes, kd->cap);
    if (st == AMK_OK) st = ensure_soa(kd, stream);
    if (st != AMK_OK) return st;
    st = exact_build_launch<kGateNone>(kd, nullptr, kd->n_scenes, nullptr, nullptr, stream);
    if (st == AMK_OK) kd->ex_valid = 1;
    return st;
}

// AMK_TIES_AUTO: the lazy build behind every search, for up to two handles per launch (the control step passes its obstacle and edge handle)
int amk::kd_auto_build(amk_kd *a, amk_kd *b, hipStream_t stream) {
    if (!a) { a = b; b = nullptr; }
    if (!a) return AMK_OK;
    if (b && b->n_scenes != a->n_scenes) return AMK_ERR_INVALID_ARG;
    return exact_build_launch<kGateLazy>(a, b, a->n_scenes, nullptr, nullptr, stream);
}
// The mode's device memory: everything AMK_TIES_NANOFLANN holds plus the three words per scene and the row flags.  Called by
// amk_kd_set_tie_order(AUTO) -- never by a search or a step.
static int auto_alloc(amk_kd *kd) {
    const size_t S = kd->n_scenes;
    int st = kd->exact.alloc(kd->n_scenes, kd->cap);
    if (st == AMK_OK) st = amk::pool_planes(kd);
    if (st != AMK_OK) return st;
    if (!kd->au_rowflag.p) {
        AMK_HIP(kd->au_rowflag.alloc(S * AMK_MAX_QUERIES));
        AMK_HIP(hipMemset(kd->au_rowflag.p, 0, sizeof(int) * S * AMK_MAX_QUERIES));
    }
    if (!kd->au_state.p) {
        AMK_HIP(kd->au_state.alloc(3 * S));
        AMK_HIP(hipMemset(kd->au_state.p, 0, sizeof(int) * 3 * S));
    }
    return AMK_OK;
}
// Called by EVERY index build of a handle, behind its launch: whatever trees the handle holds describe the previous cloud.
static int auto_reset(amk_kd *kd, hipStream_t stream) {
    kd->au_active = 0;
    if (kd->tie_order != AMK_TIES_AUTO) return AMK_OK;
    if (!kd->au_state.p) return AMK_ERR_INVALID_ARG;   // (amk_kd_set_tie_order allocated it)
    AMK_HIP(hipMemsetAsync(kd->au_state.p, 0, sizeof(int) * 3 * (size_t)kd->n_scenes, stream));
    kd->au_active = 1;
    return AMK_OK;
}
int exact_after_index_build(amk_kd *kd, hipStream_t stream) {
    if (const int st = auto_reset(kd, stream); st != AMK_OK) return st;
    return kd->tie_order == AMK_TIES_NANOFLANN ? exact_build(kd, stream) : AMK_OK;
}

// The keyframe map's pools in AMK_TIES_NANOFLANN (amk_kfmap_set_tie_order): a tree per POOL scene, built where a row names one; behind a
// sweep only where its gate word is set (that keyframe was rebuilt: its planes now hold the outliers in cloud order, FrameKDMap.cpp:480-485)
namespace amk {
// what kd_pool_exact_reserve allocates for a pool of `scenes` scenes of max_points points (host arithmetic: the tree's arrays,
// and the index-ordered planes where the pool has none yet -- the edge pool)
long long kd_pool_exact_bytes(long long scenes, int max_points, bool with_planes) {
    const long long cap = (long long)amk::round_up(max_points, 256) + 1024;   // amk_kd_create
    return ExactStore::bytes(scenes, cap) + (with_planes ? scenes * 12 * cap : 0);
}
// the trees' arrays of every pool scene (and the pool's planes), no scene has a tree yet
int kd_pool_exact_reserve(amk_kd *pool) {
    if (!pool) return AMK_ERR_INVALID_ARG;
    int st = pool->exact.alloc(pool->n_scenes, pool->cap);
    if (st == AMK_OK) st = pool_planes(pool);
    if (st != AMK_OK) return st;
    AMK_HIP(hipMemset(pool->exact.n_nodes(), 0, sizeof(int) * (size_t)pool->n_scenes));
    return AMK_OK;
}
int kd_pool_exact_build(amk_kd *obs_pool, amk_kd *edge_pool, int n_rows, const int *d_rows, const int *d_gate, hipStream_t stream) {
    if (!obs_pool || !obs_pool->exact.allocated() || (edge_pool && !edge_pool->exact.allocated()) || n_rows < 1 || !d_rows)
        return AMK_ERR_INVALID_ARG;
    return exact_build_launch<kGateRows>(obs_pool, edge_pool, n_rows, d_rows, d_gate, stream);
}
}  // namespace amk

// ---- search --------------------------------------------------------------------------------------------------------
// one WAVEFRONT per (scene, query): nanoflann's own traversal (kd_exact.h: exact_knn_wave).  Overwrites the outputs of the
// bucketed search (launched before it on the same stream) wherever the tree is available; a scene whose tree is not (node
// capacity or traversal depth exceeded on pathological data) keeps the bucketed index's answer.
// AUTO (kd_exact_search_auto_kernel): only the rows the search flagged, in the scenes whose tree is built.
template <bool AUTO>
__device__ __forceinline__ void exact_search_row(const amk::ExactPtrs &ep, const int *sizes, int n_scenes, const double *queries,
    int n_queries, int k, int *out_idx, double *out_d2, float *out_pts, int *out_cnt, const int *rowflag, const int *built) {
    __shared__ amk::ExactWaveStack stacks[4];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)  /* wave-uniform: keeps what derives from it in SGPRs */, lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + w;
    if (row >= (size_t)n_scenes * n_queries) return;
    const int s = (int)(row / n_queries);
    if constexpr (AUTO)
        if (!rowflag[row] || !built[s]) return;   // (wave-uniform)
    const amk::ExactTree T = ep.scene(s);
    const double *qp = queries + row * 3;
    const int size = sizes[s];
    double rd;
    int ri;
    const int got = amk::exact_knn_wave(T, qp[0], qp[1], qp[2], k, rd, ri, &stacks[w]);
    if (got < 0) return;
    const int cnt = amk::adaptor_count(size, k);
    amk::store_search_row(out_idx, out_d2, out_pts, out_cnt, row, k, lane, cnt, lane < got, ri, rd,
                          [&](int c) { return (c == 0 ? T.x : c == 1 ? T.y : T.z)[ri]; });
}
__global__ __launch_bounds__(256) void kd_exact_search_kernel(amk::ExactPtrs ep, const int *__restrict__ sizes, int n_scenes,
    const double *__restrict__ queries, int n_queries, int k, int *__restrict__ out_idx, double *__restrict__ out_d2,
    float *__restrict__ out_pts, int *__restrict__ out_cnt) {
    exact_search_row<false>(ep, sizes, n_scenes, queries, n_queries, k, out_idx, out_d2, out_pts, out_cnt, nullptr, nullptr);
}
__global__ __launch_bounds__(256) void kd_exact_search_auto_kernel(amk::ExactPtrs ep, const int *__restrict__ sizes, int n_scenes,
    const double *__restrict__ queries, int n_queries, int k, int *__restrict__ out_idx, double *__restrict__ out_d2,
    float *__restrict__ out_pts, int *__restrict__ out_cnt, const int *__restrict__ rowflag, const int *__restrict__ built) {
    exact_search_row<true>(ep, sizes, n_scenes, queries, n_queries, k, out_idx, out_d2, out_pts, out_cnt, rowflag, built);
}
int exact_search(amk_kd *kd, const double *d_queries, int n_queries, int k, int *d_indices, double *d_sqdist, float *d_pts,
                 int *d_counts, hipStream_t stream) {
    const dim3 grid((unsigned)(((size_t)kd->n_scenes * n_queries + 3) / 4));
    if (kd->auto_on())
        hipLaunchKernelGGL(kd_exact_search_auto_kernel, grid, dim3(256), 0, stream, amk_exact_ptrs(kd), kd->size.p, kd->n_scenes,
                           d_queries, n_queries, k, d_indices, d_sqdist, d_pts, d_counts, kd->au_rowflag.p, kd->au_built());
    else
        hipLaunchKernelGGL(kd_exact_search_kernel, grid, dim3(256), 0, stream, amk_exact_ptrs(kd), kd->size.p, kd->n_scenes,
                           d_queries, n_queries, k, d_indices, d_sqdist, d_pts, d_counts);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

// ---- status and diagnostics ----------------------------------------------------------------------------------------
// depth of every scene's tree: children are created after their parent (ids grow downwards), so one pass in id order carries the
// depths; one lane per scene, the build's list scratch (sa) holds depth[node] -- a diagnostic call.
// built (a handle in AMK_TIES_AUTO) or null: a scene without a tree for the current cloud has not needed one.
static __global__ __launch_bounds__(64) void kd_exact_status_kernel(int S, const int *__restrict__ built,
    const int *__restrict__ n_nodes, const int *__restrict__ feat, const int *__restrict__ child, unsigned *__restrict__ scratch,
    int max_nodes, int cap, int *__restrict__ status) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= S) return;
    if (built && !built[s]) { status[s] = AMK_EXACT_NOT_NEEDED; return; }
    const int nn = n_nodes[s];
    if (nn < 0) { status[s] = AMK_EXACT_GAVE_UP; return; }
    const int *f = feat + (size_t)s * max_nodes, *c = child + (size_t)s * max_nodes;
    unsigned *d = scratch + (size_t)s * cap;
    unsigned deepest = 0;
    if (nn > 0) d[0] = 0;
    for (int id = 0; id < nn; ++id) {
        const unsigned dep = d[id];
        if (f[id] >= 0) { d[c[id]] = dep + 1; d[c[id] + 1] = dep + 1; }   // an internal node: the traversal pushes one frame here
        else deepest = dep > deepest ? dep : deepest;                      // a leaf at depth dep is reached with dep frames on the stack
    }
    status[s] = deepest > (unsigned)amk::kExactMaxDepth ? AMK_EXACT_TOO_DEEP : AMK_EXACT_IN_USE;
}
static int exact_status_launch(amk_kd *kd, const int *d_built, int *d_status, hipStream_t stream) {
    const amk::ExactStore &ex = kd->exact;
    hipLaunchKernelGGL(kd_exact_status_kernel, dim3((kd->n_scenes + 63) / 64), dim3(64), 0, stream, kd->n_scenes, d_built, ex.n_nodes(),
                       ex.at<int>(ex.FEAT), ex.at<int>(ex.CHILD), ex.at<unsigned>(ex.SA), ex.max_nodes, kd->cap, d_status);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}
int amk::kd_pool_exact_status(amk_kd *pool, int *d_status, hipStream_t stream) {
    if (!pool || !d_status || !pool->exact.allocated()) return AMK_ERR_INVALID_ARG;
    return exact_status_launch(pool, nullptr, d_status, stream);
}

extern "C" {

// Which index answers a handle's searches, per scene (header).  Stream-ordered.
int amk_kd_exact_status(amk_kd *kd, int *d_status, void *stream) {
    if (!kd || !d_status) return AMK_ERR_INVALID_ARG;
    if (kd->tie_order == AMK_TIES_AUTO && kd->au_active) return exact_status_launch(kd, kd->au_built(), d_status, (hipStream_t)stream);
    if (kd->tie_order != AMK_TIES_NANOFLANN || !kd->ex_valid || !kd->exact.allocated()) {   // the bucketed index answers everything: not a fallback
        AMK_HIP(hipMemsetAsync(d_status, 0xff, sizeof(int) * kd->n_scenes, (hipStream_t)stream));   // AMK_EXACT_OFF == -1
        return AMK_OK;
    }
    return exact_status_launch(kd, nullptr, d_status, (hipStream_t)stream);
}

int amk_kd_exact_status_host(amk_kd *kd, int *h_status) {   // synchronises
    if (!kd || !h_status) return AMK_ERR_INVALID_ARG;
    return kd->stage.call({amk::to_host(h_status, sizeof(int) * kd->n_scenes)},
                          [&](const amk::HostStage::Dev *d) { return amk_kd_exact_status(kd, d[0], nullptr); }, hipDeviceSynchronize);
}

// internal (tests): number of nodes of every scene's tree (-1: not available), after synchronising
// A handle in AMK_TIES_AUTO: 0 for a scene whose tree has not been built for the current cloud (no tree, no nodes).
int amk__kd_exact_nodes(amk_kd *kd, int *h_nodes) {
    if (!kd || !h_nodes || !kd->exact.allocated()) return AMK_ERR_INVALID_ARG;
    const bool lazy = kd->tie_order == AMK_TIES_AUTO, cleared = lazy && kd->au_active;   // (au_state exists and belongs to this cloud)
    std::vector<int> built((size_t)kd->n_scenes, 0);
    if (const int st = amk::read_back({{h_nodes, kd->exact.n_nodes(), sizeof(int) * kd->n_scenes},
                                       {cleared ? built.data() : nullptr, cleared ? kd->au_built() : nullptr, sizeof(int) * kd->n_scenes}});
        st != AMK_OK)
        return st;
    if (lazy) {
        for (int s = 0; s < kd->n_scenes; ++s)
            if (!built[s]) h_nodes[s] = 0;
    }
    return AMK_OK;
}

#ifdef AMK_EXACT_TRACE
// diagnostics build only (tools/experiments/exact_phase_clocks.py): the first n words of the scene-0 list buffer, where the
// lower-level build kernel leaves its per-wavefront phase clocks
int amk__kd_exact_trace(amk_kd *kd, unsigned *h, int n) {
    if (!kd || !h || !kd->exact.allocated()) return AMK_ERR_INVALID_ARG;
    return amk::read_back({{h, kd->exact.at<unsigned>(amk::ExactStore::SA), sizeof(unsigned) * n}});
}
#endif

int amk_kd_set_tie_order(amk_kd *kd, int mode) {
    if (!kd) return AMK_ERR_INVALID_ARG;
    if (mode != AMK_TIES_LOWEST_INDEX && mode != AMK_TIES_NANOFLANN && mode != AMK_TIES_AUTO) return AMK_ERR_UNSUPPORTED;
    if (mode == AMK_TIES_AUTO) {   // the mode's memory, here and not on the search path (a failure leaves the handle as it was)
        const int st = auto_alloc(kd);
        if (st != AMK_OK) return st;
    }
    kd->tie_order = mode;
    return AMK_OK;
}

}  // extern "C"
