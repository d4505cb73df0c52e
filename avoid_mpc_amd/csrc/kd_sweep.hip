// The keyframe sweep of the KD index for gfx950 (FrameKDMap::KeyframeThreadWorker, AM/src/FrameKDMap.cpp:462-485): a keyframe's
// points that have no neighbour within th in the current frame are its outliers; with enough of them the keyframe is compacted to
// them in place and its index rebuilt.  amk_kd_keyframe_sweep does it for a pair of handles against the current frame's own
// index; kd_sweep_mapped for the rows of the keyframe map's pool (kfmap.hip) against a fine hashed grid of the current frame.
// The index itself -- build, searches, the handle's C ABI -- is kd_index.hip.
#include "kd_exact.h"

using amk::kCompactThreads;
using amk::kWave;

// ------------------------------------------------------------------------------------------------
// keyframe sweep (FrameKDMap::KeyframeThreadWorker, AM/src/FrameKDMap.cpp:462-485)
// ------------------------------------------------------------------------------------------------
// one thread per keyframe point: outlier iff its nearest neighbour in the current frame is farther than th.  The points are
// taken in the keyframe's RECORD order (bucket-contiguous: the lanes of a wavefront hold neighbours in space, so their bucket-table
// reads and point reads of the current frame fall into a few cache lines; in cloud order every lane reads its own -- 6.3-7.5 ms
// against 5.2-6.2 ms per 512-scene sweep of the 50 k-point flight frames); the flag goes to the point's cloud index (record.w).
__global__ __launch_bounds__(256) void kd_sweep_mark_kernel(amk::GridPtrs cur, const int *__restrict__ cur_sizes,
                                                            const float4 *__restrict__ KGP, int kcap,
                                                            const int *__restrict__ ksizes, double th_dist,
                                                            unsigned char *__restrict__ flags,
                                                            const int *__restrict__ kf_list = nullptr,
                                                            const int *__restrict__ cur_list = nullptr) {
    // kf_list / cur_list (the keyframe map's pool, kfmap.hip): row blockIdx.y sweeps scene kf_list[row] of the keyframe arrays
    // against scene cur_list[row] of the current-frame arrays; kf_list[row] < 0: nothing to sweep.  Null: scene = row in both.
    const int s = kf_list ? kf_list[blockIdx.y] : blockIdx.y;
    if (s < 0) return;
    const int sc = cur_list ? cur_list[blockIdx.y] : s;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = ksizes[s];
    if (i >= n) return;
    const float4 rec = KGP[(size_t)s * kcap + i];
    unsigned char f = 0;
    if (cur_sizes[sc] > 1) {  // SearchForNearest(pt, 1) yields a result only then (kd_tree_two.h:119-124)
        // (a wave-cooperative second phase for the queries that find no neighbour quickly -- lane j scanning candidate run j of one
        // undecided query at a time -- was built and measured SLOWER: 8.3 ms per 512-scene sweep against 5.2-6.2; the runs of a
        // 13-tile index hold ~5 points each, the phase was all bookkeeping)
        f = (unsigned char)amk::grid_outlier_thread(cur.scene(sc), (double)rec.x, (double)rec.y, (double)rec.z, th_dist);
    }
    flags[(size_t)s * kcap + __float_as_int(rec.w)] = f;
}

// (A persistent-lane version of this kernel -- a wavefront owns 256-1024 records, its lanes draw queries as they finish -- was built when
// the sensor-like flights showed that nearly every wavefront holds an outlier and runs at the outlier's pace: 9.3 -> 6.1 ms per
// 512-scene sweep of 50 k-point frames, but slower on 3072-point frames, and beside the point once the pool swept against a fine grid:
// tools/experiments/patches/r05_sweep_persistent_lanes.patch, profiles/r05_sweep_target.txt.)
static int g_sweep_target = [] { const char *e = getenv("AMK_SWEEP_TARGET"); return e ? atoi(e) : 1; }();   // 1: the pool sweeps against a fine hashed grid of the current frame (below); 0: against the frame's own index (A/B, tests)
extern "C" void amk__sweep_set_target(int v) { g_sweep_target = v; }
static int g_sweep_order = [] { const char *e = getenv("AMK_SWEEP_ORDER"); return e ? atoi(e) : 1; }();   // 1: keyframe points in the order of last sweep's grid where it is theirs; 0: always in record order (A/B)
extern "C" void amk__sweep_set_order(int v) { g_sweep_order = v; }

// one block per scene: count the outliers; with >= th_count of them compact the keyframe's planes in place
// (order preserved: the write cursor never passes the read cursor) and refresh size / bbox / max|coordinate|
__global__ __launch_bounds__(kCompactThreads) void kd_sweep_compact_kernel(
    float *__restrict__ X, float *__restrict__ Y, float *__restrict__ Z, int cap, int *__restrict__ sizes,
    float *__restrict__ pmax_out, float *__restrict__ bbox_out, const unsigned char *__restrict__ flags, int th_count,
    int *__restrict__ sweep_cnt, int *__restrict__ out_outliers, int *__restrict__ out_rebuilt,
    const int *__restrict__ kf_list = nullptr) {
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int s = kf_list ? kf_list[row] : row;   // (out_outliers / out_rebuilt / sweep_cnt are per ROW)
    if (s < 0) {
        if (tid == 0) {
            if (sweep_cnt) { sweep_cnt[2 * row] = 0; sweep_cnt[2 * row + 1] = 0; }
            if (out_outliers) out_outliers[row] = 0;
            if (out_rebuilt) out_rebuilt[row] = 0;
        }
        return;
    }
    float *xs = X + (size_t)s * cap, *ys = Y + (size_t)s * cap, *zs = Z + (size_t)s * cap;
    const unsigned char *fl = flags + (size_t)s * cap;
    const int n = sizes[s];
    __shared__ int wave_tot[kCompactThreads / kWave];
    __shared__ float wave_max[kCompactThreads / kWave];
    __shared__ float wave_bb[6][kCompactThreads / kWave];
    __shared__ int total_sh;
    // Four consecutive elements per thread and trip (round 6: one element per trip was 98 trips of dependent loads and two barriers each at
    // 50 k points: 183 us per 512-row launch).  The rows start at multiples of 256 elements and are NaN- / zero-padded to cap >= n + 1024,
    // so the 4-byte flag words and 16-byte coordinate vectors are aligned and may overhang n.
    int cnt = 0;
    for (int i = 4 * tid; i < n; i += 4 * kCompactThreads) {
        const uchar4 f4 = *reinterpret_cast<const uchar4 *>(fl + i);
        cnt += (f4.x != 0) + ((i + 1 < n) & (f4.y != 0)) + ((i + 2 < n) & (f4.z != 0)) + ((i + 3 < n) & (f4.w != 0));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if (lane == 0) wave_tot[w] = cnt;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int j = 0; j < kCompactThreads / kWave; ++j) t += wave_tot[j];
        total_sh = t;
    }
    __syncthreads();
    const int total = total_sh;
    const int rebuilt = total >= th_count ? 1 : 0;  // :477-479
    if (tid == 0) {
        if (sweep_cnt) { sweep_cnt[2 * row] = total; sweep_cnt[2 * row + 1] = rebuilt; }
        if (out_outliers) out_outliers[row] = total;
        if (out_rebuilt) out_rebuilt[row] = rebuilt;
    }
    if (!rebuilt) return;
    float amax = 0.f, bmn[3] = {3.0e38f, 3.0e38f, 3.0e38f}, bmx[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += 4 * kCompactThreads) {
        const int i = c0 + 4 * tid;
        float px[4] = {0.f, 0.f, 0.f, 0.f}, py[4] = {0.f, 0.f, 0.f, 0.f}, pz[4] = {0.f, 0.f, 0.f, 0.f};
        bool valid[4] = {false, false, false, false};
        if (i < n) {
            const float4 x4 = *reinterpret_cast<const float4 *>(xs + i), y4 = *reinterpret_cast<const float4 *>(ys + i),
                         z4 = *reinterpret_cast<const float4 *>(zs + i);
            const uchar4 f4 = *reinterpret_cast<const uchar4 *>(fl + i);
            px[0] = x4.x; px[1] = x4.y; px[2] = x4.z; px[3] = x4.w;
            py[0] = y4.x; py[1] = y4.y; py[2] = y4.z; py[3] = y4.w;
            pz[0] = z4.x; pz[1] = z4.y; pz[2] = z4.z; pz[3] = z4.w;
            valid[0] = f4.x != 0; valid[1] = i + 1 < n && f4.y != 0; valid[2] = i + 2 < n && f4.z != 0; valid[3] = i + 3 < n && f4.w != 0;
        }
        const int mine = (int)valid[0] + (int)valid[1] + (int)valid[2] + (int)valid[3];
        const int incl = amk::wave_incl_scan_i32(mine);
        __syncthreads();  // every read of this chunk is done before anybody writes (in-place; the write cursor never passes the chunk's start)
        if (lane == 63) wave_tot[w] = incl;
        __syncthreads();
        int woff = 0, tot = 0;
#pragma unroll
        for (int j = 0; j < kCompactThreads / kWave; ++j) {
            const int t = wave_tot[j];
            woff += (j < w) ? t : 0;
            tot += t;
        }
        int o = base + woff + incl - mine;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (valid[e]) {
                xs[o] = px[e]; ys[o] = py[e]; zs[o] = pz[e];
                ++o;
                amax = fmaxf(amax, fmaxf(fabsf(px[e]), fmaxf(fabsf(py[e]), fabsf(pz[e]))));
                if (amk::boxable3(px[e], py[e], pz[e])) {
                    bmn[0] = fminf(bmn[0], px[e]); bmx[0] = fmaxf(bmx[0], px[e]);
                    bmn[1] = fminf(bmn[1], py[e]); bmx[1] = fmaxf(bmx[1], py[e]);
                    bmn[2] = fminf(bmn[2], pz[e]); bmx[2] = fmaxf(bmx[2], pz[e]);
                }
            }
        base += tot;
        __syncthreads();
    }
    const float qnan = __builtin_nanf("");
    for (int i = base + tid; i < n + 1024 && i < cap; i += kCompactThreads) { xs[i] = qnan; ys[i] = qnan; zs[i] = qnan; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        amax = fmaxf(amax, __shfl_xor(amax, off));
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            bmn[a] = fminf(bmn[a], __shfl_xor(bmn[a], off));
            bmx[a] = fmaxf(bmx[a], __shfl_xor(bmx[a], off));
        }
    }
    if (lane == 0) {
        wave_max[w] = amax;
#pragma unroll
        for (int a = 0; a < 3; ++a) { wave_bb[a][w] = bmn[a]; wave_bb[3 + a][w] = bmx[a]; }
    }
    __syncthreads();
    if (tid == 0) {
        float m = 0.f;
        for (int j = 0; j < kCompactThreads / kWave; ++j) m = fmaxf(m, wave_max[j]);
        sizes[s] = base;
        pmax_out[s] = m;
    }
    if (tid < 6) {
        float v = wave_bb[tid][0];
        for (int j = 1; j < kCompactThreads / kWave; ++j) v = tid < 3 ? fminf(v, wave_bb[tid][j]) : fmaxf(v, wave_bb[tid][j]);
        bbox_out[6 * s + tid] = v;
    }
}

// the bucketed index of a compacted keyframe from its planes: every scene of a handle, or (the pool) the scenes the sweep rebuilt
__global__ __launch_bounds__(amk::kGridBuildThreads) void kd_grid_build_kernel(
    const float *__restrict__ X, const float *__restrict__ Y, const float *__restrict__ Z, int cap,
    const int *__restrict__ sizes, const float *__restrict__ bbox, float4 *__restrict__ GP,
    int *__restrict__ cell_start, int ntiles, double *__restrict__ gparams) {
    const int s = blockIdx.x;
    amk::grid_build_scene(s, X + (size_t)s * cap, Y + (size_t)s * cap, Z + (size_t)s * cap, cap, sizes[s], bbox, GP, cell_start, ntiles,
                          gparams);
}
__global__ __launch_bounds__(amk::kGridBuildThreads) void kd_grid_build_list_kernel(
    const float *__restrict__ X, const float *__restrict__ Y, const float *__restrict__ Z, int cap,
    const int *__restrict__ sizes, const float *__restrict__ bbox, float4 *__restrict__ GP, int *__restrict__ cell_start,
    int ntiles, double *__restrict__ gparams, const int *__restrict__ list, const int *__restrict__ rebuilt) {
    const int s = list[blockIdx.x];
    if (s < 0 || !rebuilt[blockIdx.x]) return;   // (block-uniform)
    amk::grid_build_scene(s, X + (size_t)s * cap, Y + (size_t)s * cap, Z + (size_t)s * cap, cap, sizes[s], bbox, GP, cell_start,
                          ntiles, gparams);
}

extern "C" int amk_kd_keyframe_sweep(amk_kd *keyframe, amk_kd *current, double th_dist, int th_count, int *d_outliers,
                                     int *d_rebuilt, void *stream_) {
    if (!keyframe || !current || keyframe == current || keyframe->n_scenes != current->n_scenes) return AMK_ERR_INVALID_ARG;
    // (the sweep compacts the keyframe's cloud in place: a lazily built tree would go stale -- header)
    if (keyframe->tie_order == AMK_TIES_AUTO || current->tie_order == AMK_TIES_AUTO) return AMK_ERR_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    const int S = keyframe->n_scenes;
    if (!keyframe->flags.p) {
        AMK_HIP(keyframe->flags.alloc((size_t)S * keyframe->cap));
        AMK_HIP(keyframe->sweep_cnt.alloc((size_t)S * 2));
    }
    const amk::GridPtrs cur = grid_ptrs(current);
    {   // the key frame's points are the queries and are compacted in place: they must exist in index order
        const int st = ensure_soa(keyframe, stream);
        if (st != AMK_OK) return st;
    }
    if (keyframe->max_points > 0) {
        hipLaunchKernelGGL(kd_sweep_mark_kernel, dim3((keyframe->max_points + 255) / 256, S), dim3(256), 0, stream, cur,
                           current->size.p, keyframe->gpt.p, keyframe->cap, keyframe->size.p, th_dist, keyframe->flags.p);
    }
    hipLaunchKernelGGL(kd_sweep_compact_kernel, dim3(S), dim3(kCompactThreads), 0, stream, keyframe->x.p, keyframe->y.p,
                       keyframe->z.p, keyframe->cap, keyframe->size.p, keyframe->pmax.p, keyframe->bbox.p, keyframe->flags.p,
                       th_count, keyframe->sweep_cnt.p, d_outliers, d_rebuilt);
    // the bucketed index of every scene is rebuilt (a no-op in effect for the untouched ones)
    hipLaunchKernelGGL(kd_grid_build_kernel, dim3(S), dim3(amk::kGridBuildThreads), 0, stream, keyframe->x.p,
                       keyframe->y.p, keyframe->z.p, keyframe->cap, keyframe->size.p, keyframe->bbox.p, keyframe->gpt.p,
                       keyframe->cell_start.p, keyframe->ntiles, keyframe->gparams.p);
    keyframe->async_pending = 1;
    AMK_HIP(hipGetLastError());
    keyframe->ex_valid = 0;   // a rebuilt keyframe's old tree describes another cloud
    if (keyframe->tie_order == AMK_TIES_NANOFLANN) return exact_build(keyframe, stream);  // (the planes are valid: the sweep compacted them)
    return AMK_OK;
}

// ------------------------------------------------------------------------------------------------
// the keyframe map's pool (kfmap.hip): one handle holds P physical frames x S scenes, scene index = slot * S + s
// ------------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------------
// The pool's sweep target as a FINE HASHED GRID.  The frames' own indices have cells of ~1 m at 50 k points (<= 1024 cells: what the
// K-NN searches want), the sweep asks "any point within th = 0.1 m?": a query read 70 (inlier) to 1200 (outlier) candidates of the
// few cells its cube touches -- 8.4 ms per 512-scene sweep even with every cell's points in one run, 62 % of a flight's kernel time
// once the frames are a forward-looking sensor's and every robot sweeps every period (profiles/r05_sweep_target.txt).  Here the
// current frame of every sweep row is sorted once more into cubic cells of edge 2.5 th on a world-fixed lattice, hashed into
// kSweepBuckets buckets (a bucket may hold several cells: more candidates, the same answer -- the distance test decides): the cube of
// a query touches <= 2 cells per axis, ~5 points each on a surface.  Points with a NaN, an infinite or a |coordinate| > 3.0e38
// stay out (boxable3: the rule this grid was written and tested with); their absence is what `finite == 0` reports.  The map is
// UNSPECIFIED for frames with such points (header): a keyframe point with an infinite coordinate passes the mark kernel's
// `q == q` gate and is an outlier on a row's first sweep, one with a NaN never is, and on later sweeps of the row (the keyframe
// taken from the previous generation's grid) neither is visited.  amk_kd_keyframe_sweep does not come here.
// ------------------------------------------------------------------------------------------------
constexpr int kSweepBuckets = 16384;   // at most: 64 KB of LDS histogram per build block; a pool of small frames takes fewer (sweep_buckets)
constexpr int kSweepBuildThreads = 1024;

// Cell of a coordinate: 32-bit, from fp32 arithmetic -- mul, floor, clamp, convert (the fp64 / 64-bit version of round 5 cost ~12 VALU
// instructions per coordinate and ~40 per hash, in kernels that are bound by their VALU instructions).  What the sweep needs of it is
// MONOTONICITY, which every step keeps (round-to-nearest, floor, clamp): a point p with q - rr <= p <= q + rr then has
// cell(q - rr) <= cell(p) <= cell(q + rr), whatever the rounding did to the cell boundaries.
__device__ __forceinline__ int sweep_cell(float p, float inv_hf) {
    return (int)fminf(fmaxf(floorf(p * inv_hf), -5.0e8f), 5.0e8f);
}
__device__ __forceinline__ int sweep_cell(double p, float inv_hf) { return sweep_cell((float)p, inv_hf); }
// Bucket of a cell.  Cells are hashed BLOCK-wise: a block of 4 x 4 x 4 cells (10 th = 1 m at th 0.1) owns 64 CONSECUTIVE buckets, the hash
// only picks which run of 64 (nb / 64 runs).  Neighbouring cells therefore share a run unless they straddle a block face: queries taken in
// grid order (kd_sweep_mapped's two generations) find their <= 8 cells' table entries and records near each other (mark kernel 1.56 ->
// 1.47 ms per 512 x 50 k sweep against the cell-wise hash).  Cells per bucket are what a cell-wise hash gives (cells / nb on average).
// (A workgroup per run with the run's records staged in LDS was built on top of this and is SLOWER, 1.94 ms: the kernel is bound by its
// VALU instructions and their divergence, not by its gathers -- tools/experiments/patches/r06_sweep_block_lds.patch, profiles/r06_sweep.txt.)
constexpr int kSweepBlockCells = 64;   // 4 x 4 x 4
__device__ __forceinline__ int sweep_block(int ix, int iy, int iz, int nb) {
    unsigned h = (unsigned)(ix >> 2) * 73856093u ^ (unsigned)(iy >> 2) * 19349663u ^ (unsigned)(iz >> 2) * 83492791u;
    h ^= h >> 15;
    return (int)(h & (unsigned)(nb / kSweepBlockCells - 1));
}
__device__ __forceinline__ int sweep_local(int ix, int iy, int iz) { return (ix & 3) | ((iy & 3) << 2) | ((iz & 3) << 4); }
__device__ __forceinline__ int sweep_bucket(int ix, int iy, int iz, int nb) {
    return sweep_block(ix, iy, iz, nb) * kSweepBlockCells + sweep_local(ix, iy, iz);
}
// buckets of a pool's sweep grids: a power of two, about two per point, between 1024 and kSweepBuckets
static int sweep_buckets(int max_points) {
    static const int forced = [] { const char *e = getenv("AMK_SWEEP_NB"); return e ? atoi(e) : 0; }();   // (experiments: a power of two in [1024, 16384])
    if (forced >= 1024 && forced <= kSweepBuckets && (forced & (forced - 1)) == 0) return forced;
    int nb = 1024;
    while (nb < kSweepBuckets && nb < 2 * max_points) nb *= 2;
    return nb;
}

// one block per sweep row: counting sort of the current frame's points by bucket (LDS histogram, block scan, LDS cursors).  The points are
// read from the frame's OWN bucketed records (kd_build's output: coarse-cell order, ~1 m cells), not from the index-ordered planes: the 64
// points of a wave-instruction then lie in one or two blocks of fine cells and their 16-byte records are scattered into a few KB instead of
// all over the row's 800 KB (round 6: the scatter, not the arithmetic, is what this kernel's time is).
__global__ __launch_bounds__(kSweepBuildThreads) void kd_sweep_hash_build_kernel(
    const float4 *__restrict__ GP, int cap, const int *__restrict__ sizes,
    double inv_h, int nb, float4 *__restrict__ recs, int *__restrict__ table, const int *__restrict__ kf_list,
    const int *__restrict__ cur_list, int *__restrict__ src, const int *__restrict__ src_prev, unsigned char *__restrict__ flags) {
    extern __shared__ int hist[];   // [nb] + [kSweepBuildThreads / 64] wave sums
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float inv_hf = (float)inv_h;
    const int kf = kf_list[row];
    if (kf < 0) {   // (block-uniform) no sweep in this row: whatever grid this generation held for it is not the next sweep's keyframe
        if (tid == 0) src[row] = -1;
        return;
    }
    const int sc = cur_list[row];
    if (tid == 0) src[row] = sc;
    // the keyframe is the frame this row swept against last time: the mark kernel takes its points from that grid, which leaves out the
    // points with a non-finite coordinate -- their flag is 0 (not what amk_kd_keyframe_sweep decides for them: the map is unspecified there)
    if (src_prev[row] == kf)
        for (int i = tid; i < sizes[kf]; i += kSweepBuildThreads) flags[(size_t)kf * cap + i] = 0;
    const int n = sizes[sc];
    const float4 *in = GP + (size_t)sc * cap;   // the frame's own records: coarse-cell order (see above)
    int *wsum = hist + nb;
    int *tab = table + (size_t)row * (nb + 1);
    float4 *out = recs + (size_t)row * cap;
    for (int i = tid; i < nb; i += kSweepBuildThreads) hist[i] = 0;
    __syncthreads();
    constexpr int U = 4;   // points per thread and trip: their loads fly together (a block's passes are two chains of dependent trips)
    for (int i0 = tid; i0 < n; i0 += U * kSweepBuildThreads) {
        float x[U], y[U], z[U];
        int id[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float4 r = in[min(i0 + u * kSweepBuildThreads, n - 1)];
            x[u] = r.x; y[u] = r.y; z[u] = r.z; id[u] = __float_as_int(r.w);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (i0 + u * kSweepBuildThreads < n && amk::boxable3(x[u], y[u], z[u]))
                atomicAdd(&hist[sweep_bucket(sweep_cell(x[u], inv_hf), sweep_cell(y[u], inv_hf), sweep_cell(z[u], inv_hf), nb)], 1);
    }
    __syncthreads();
    // exclusive scan of the nb counts: nb / kSweepBuildThreads consecutive buckets per thread (nb >= 1024 = the block)
    const int per = nb / kSweepBuildThreads;
    int loc = 0;
    for (int j = 0; j < per; ++j) loc += hist[tid * per + j];
    const int incl = amk::wave_incl_scan_i32(loc);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    int base = 0;
    for (int j = 0; j < w; ++j) base += wsum[j];
    int run = base + incl - loc;
    for (int j = 0; j < per; ++j) {
        const int c = hist[tid * per + j];
        hist[tid * per + j] = run;   // the bucket's cursor
        tab[tid * per + j] = run;
        run += c;
    }
    if (tid == kSweepBuildThreads - 1) tab[nb] = run;   // = the points with finite coordinates
    __syncthreads();
    for (int i0 = tid; i0 < n; i0 += U * kSweepBuildThreads) {
        float x[U], y[U], z[U];
        int id[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float4 r = in[min(i0 + u * kSweepBuildThreads, n - 1)];
            x[u] = r.x; y[u] = r.y; z[u] = r.z; id[u] = __float_as_int(r.w);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * kSweepBuildThreads;
            if (i < n && amk::boxable3(x[u], y[u], z[u])) {
                const int pos = atomicAdd(&hist[sweep_bucket(sweep_cell(x[u], inv_hf), sweep_cell(y[u], inv_hf), sweep_cell(z[u], inv_hf), nb)], 1);
#ifndef AMK_DIAG_NOSTORE   // (diagnostics: without the scatter the kernel takes 169 of its 458 us)
                out[pos] = make_float4(x[u], y[u], z[u], __int_as_float(id[u]));
#else
                if (pos == -12345) out[0] = make_float4(x[u], y[u], z[u], 0.f);
#endif   // (order inside a bucket: whatever the atomics gave -- the sweep asks "any", not "which")
            }
        }
    }
}

// kSweepStepH records against one query.  The counters of the first version said what bounds this kernel: 3 000 VALU instructions per
// wavefront -- the VALU pipes ~90 % busy, most of it the candidates' fp64 distances (11 instructions each: three conversions, the
// differences, the squares, the sum) -- not the loads (TA 66 % busy, 81 % of L2 requests hit).  So the candidates are screened in fp32 first: both
// points ARE floats, the fp32 squared distance is within 3e-7 relative of the real one, and a candidate above t2 (1 + 1e-5) cannot pass
// the exact test; only the few below it get the fp64 distance and the exact test (same bits as before: same flags).
__device__ __forceinline__ bool sweep_step_hits(const float4 &q, const float4 (&pr)[4], float t2f, double qx, double qy, double qz, double th,
                                                double t2lo, double t2hi) {
    bool hit = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float dx = q.x - pr[e].x, dy = q.y - pr[e].y, dz = q.z - pr[e].z;
        const float d32 = dx * dx + dy * dy + dz * dz;
        if (d32 <= t2f) {
            const double d = amk::sq_dist(qx, qy, qz, pr[e].x, pr[e].y, pr[e].z);
            hit = hit || d <= t2lo || (d <= t2hi && sqrt(d) <= th);
        }
    }
    return hit;
}

// one thread per keyframe record (record order): the <= 8 cells of its cube, its own cell first; their table entries fetched together,
// then kSweepStepH records of a run per step.  A query whose cube would span more than two cells along an axis (coordinates so large
// that the rounding allowance exceeds the cell) reads every point of the grid instead.
constexpr int kSweepStepH = 4;   // (= the array bound of sweep_step_hits)
#ifndef AMK_SWEEP_MARK_THREADS
#define AMK_SWEEP_MARK_THREADS 256
#endif
constexpr int kSweepMarkThreads = AMK_SWEEP_MARK_THREADS;
__global__ __launch_bounds__(kSweepMarkThreads) void kd_sweep_mark_hash_kernel(const int *__restrict__ cur_sizes,
                                                                 const float4 *__restrict__ trecs, const int *__restrict__ table,
                                                                 double inv_h, int nb, const float4 *__restrict__ KGP, int kcap,
                                                                 const int *__restrict__ ksizes, double th,
                                                                 unsigned char *__restrict__ flags, const int *__restrict__ kf_list,
                                                                 const int *__restrict__ cur_list, const float4 *__restrict__ prev_recs,
                                                                 const int *__restrict__ prev_table, const int *__restrict__ src_prev) {
    const int row = blockIdx.y;
    const int s = kf_list[row];
    if (s < 0) return;
    const int sc = cur_list[row];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    // the keyframe's points: in the order of the grid it was sorted into when it was the current frame (the sweep before this one, same
    // row) -- the lanes of a wavefront then ask for the same few buckets and runs -- else in its own records' order
    const bool ordered = src_prev[row] == s;   // (row-uniform)
    const bool live = i < (ordered ? prev_table[(size_t)row * (nb + 1) + nb] : ksizes[s]);
    // Two phases per workgroup.  A: every thread scans its query's OWN cell (half the inliers end there).  B: the queries that are still open
    // are compacted into LDS and taken by the first threads of the block, one each, for the other <= 7 cells of their cubes.  One query per
    // thread throughout made nearly every wavefront run at its slowest lane's pace (an outlier scans all 8 cells: a real pair of frames with
    // 14 % outliers cost 90 % of an all-outlier pair); after the compaction the wavefronts of phase B are full of open queries and the others
    // have retired.  Same cells, same screen, same exact test: same flags.
    __shared__ float4 open_q[kSweepMarkThreads];
    __shared__ int4 open_c[kSweepMarkThreads];   // the open query's own cell and, per axis, which other cell its cube reaches (bits 0-2: has one, 3-5: it is the next one up)
    __shared__ int n_open;
    if (threadIdx.x == 0) n_open = 0;
    __syncthreads();
    const int *tab = table + (size_t)row * (nb + 1);
    const float4 *pts = trecs + (size_t)row * kcap;
    const double h = 1.0 / inv_h;
    const float inv_hf = (float)inv_h;
    const double t2 = th * th, t2lo = t2 * (1.0 - 1e-15), t2hi = t2 * (1.0 + 1e-15);
    const float t2f = (float)(t2 * (1.0 + 1e-5)) * (1.0f + 1e-6f);   // fp32 screen: above it no candidate can pass the exact test
    const bool usable = cur_sizes[sc] > 1 && tab[nb] > 0;   // SearchForNearest(pt, 1) yields a result only for a tree of more than one point
                                                            // (kd_tree_two.h:119-124), and an outlier needs a nearest point at all
    if (live) {
        const float4 rec = ordered ? prev_recs[(size_t)row * kcap + i] : KGP[(size_t)s * kcap + i];
        unsigned char f = 0;
        bool open = false;
        int4 oc = make_int4(0, 0, 0, 0);
        const double qx = (double)rec.x, qy = (double)rec.y, qz = (double)rec.z;
        if (usable && qx == qx && qy == qy && qz == qz) {
            const double rr = th + 1e-9 * h + 1e-12 * (fabs(qx) + fabs(qy) + fabs(qz) + th);   // (rounding allowance, as grid_outlier_thread's)
            const int lx = sweep_cell(qx - rr, inv_hf), hx = sweep_cell(qx + rr, inv_hf);
            const int ly = sweep_cell(qy - rr, inv_hf), hy = sweep_cell(qy + rr, inv_hf);
            const int lz = sweep_cell(qz - rr, inv_hf), hz = sweep_cell(qz + rr, inv_hf);
            f = 1;
            if (hx - lx > 1 || hy - ly > 1 || hz - lz > 1) {
                // coordinates so large that the rounding allowance exceeds a cell: every point of the grid is a candidate (a plain loop)
                for (int j = 0; f && j < tab[nb]; ++j) {
                    const float4 p = pts[j];
                    const double d = amk::sq_dist(qx, qy, qz, p.x, p.y, p.z);
                    if (d <= t2lo || (d <= t2hi && sqrt(d) <= th)) f = 0;
                }
            } else {
                const int ox = sweep_cell(rec.x, inv_hf), oy = sweep_cell(rec.y, inv_hf), oz = sweep_cell(rec.z, inv_hf);   // own cell: within [l, h]
                const int b = sweep_bucket(ox, oy, oz, nb);
                const int s0 = tab[b], s1 = tab[b + 1];
                for (int pos = s0; f && pos < s1; pos += kSweepStepH) {
                    const int last = s1 - 1;
                    float4 pr[kSweepStepH];
#pragma unroll
                    for (int e = 0; e < kSweepStepH; ++e) pr[e] = pts[min(pos + e, last)];
                    if (sweep_step_hits(rec, pr, t2f, qx, qy, qz, th, t2lo, t2hi)) f = 0;
                }
                open = f && (hx != lx || hy != ly || hz != lz);
                oc = make_int4(ox, oy, oz, (hx != lx ? 1 : 0) | (hy != ly ? 2 : 0) | (hz != lz ? 4 : 0) | (ox == lx ? 8 : 0) | (oy == ly ? 16 : 0) | (oz == lz ? 32 : 0));
            }
        }
        if (open) { const int slot = atomicAdd(&n_open, 1); open_q[slot] = rec; open_c[slot] = oc; }
        else flags[(size_t)s * kcap + __float_as_int(rec.w)] = f;
    }
    __syncthreads();
#ifdef AMK_SWEEP_SKIPB
    if (false) {
#else
    if ((int)threadIdx.x < n_open) {
#endif
        const float4 rec = open_q[threadIdx.x];
        const int4 oc = open_c[threadIdx.x];
        const double qx = (double)rec.x, qy = (double)rec.y, qz = (double)rec.z;
        // the other cell of an axis: the next one up or down (phase A's cube [l, h] with h - l <= 1 around the own cell)
        const int ax = oc.x + ((oc.w & 8) ? 1 : -1), ay = oc.y + ((oc.w & 16) ? 1 : -1), az = oc.z + ((oc.w & 32) ? 1 : -1);
        const int mask = oc.w & 7;
        int s0[8], s1[8];
        // cells that share a FACE with the own cell first (one bit), then edges, then the corner: an inlier's neighbour is most often there
        constexpr int kOrder[8] = {0, 1, 2, 4, 3, 5, 6, 7};
#pragma unroll
        for (int j = 1; j < 8; ++j) {   // bit a of kk set = the OTHER cell of axis a; the table entries fetched together
            const int kk = kOrder[j];
            s0[j] = s1[j] = 0;
            if ((kk & ~mask) == 0) {
                const int b = sweep_bucket((kk & 1) ? ax : oc.x, (kk & 2) ? ay : oc.y, (kk & 4) ? az : oc.z, nb);
                s0[j] = tab[b];
                s1[j] = tab[b + 1];
            }
        }
        unsigned char f = 1;
#pragma unroll
        for (int k = 1; k < 8; ++k) {
            for (int pos = s0[k]; f && pos < s1[k]; pos += kSweepStepH) {
                const int last = s1[k] - 1;
                float4 pr[kSweepStepH];
#pragma unroll
                for (int e = 0; e < kSweepStepH; ++e) pr[e] = pts[min(pos + e, last)];
                if (sweep_step_hits(rec, pr, t2f, qx, qy, qz, th, t2lo, t2hi)) f = 0;
            }
        }
        flags[(size_t)s * kcap + __float_as_int(rec.w)] = f;
    }
}

namespace amk {
int pool_planes(amk_kd *kd) {   // allocates the index-ordered planes of a handle (a pool's: written by every build, compacted by the sweeps)
    const size_t tot = (size_t)kd->n_scenes * kd->cap;
    if (!kd->x.p) AMK_HIP(kd->x.alloc(tot));
    if (!kd->y.p) AMK_HIP(kd->y.alloc(tot));
    if (!kd->z.p) AMK_HIP(kd->z.alloc(tot));
    return AMK_OK;
}

// The sweep's two generations of hashed grids for n_rows sweep rows (a third row of sources stays -1: "no grid", what the A/B
// switch hands the mark kernel); no row has a grid yet.
static int sweep_reserve(amk_kd *pool, int n_rows) {
    const int nb = sweep_buckets(pool->max_points);
    AMK_HIP(pool->sw_gpt.alloc((size_t)2 * n_rows * pool->cap));
    AMK_HIP(pool->sw_cs.alloc((size_t)2 * n_rows * (nb + 1)));
    AMK_HIP(pool->sw_src.alloc((size_t)3 * n_rows));
    AMK_HIP(hipMemset(pool->sw_src.p, 0xff, sizeof(int) * 3 * (size_t)n_rows));   // -1: no grid yet
    pool->sw_rows = n_rows;
    return AMK_OK;
}

// Everything a map's obstacle pool will ever allocate, at once (amk_kfmap_create): the index-ordered planes, the sweep's outlier flags and
// its two generations of hashed grids -- so that a pool that does not fit fails when the map is CREATED (amk_kfmap_pool_bytes says what it
// needs), not at some later submit when the first sweep runs.
int kd_pool_reserve(amk_kd *pool, int n_rows) {
    if (!pool || n_rows < 1) return AMK_ERR_INVALID_ARG;
    const int st = pool_planes(pool);
    if (st != AMK_OK) return st;
    if (!pool->flags.p) AMK_HIP(pool->flags.alloc((size_t)pool->n_scenes * pool->cap));
    if (pool->max_points > 0 && pool->sw_rows < n_rows) return sweep_reserve(pool, n_rows);
    return AMK_OK;
}

// KeyframeThreadWorker's sweep (FrameKDMap.cpp:463-485) for n_rows scenes of a map: row r sweeps the points of pool scene
// d_kf_list[r] (the newest keyframe) against pool scene d_cur_list[r] (the current frame); with >= th_count outliers the
// keyframe's planes are compacted to them in place and its index is rebuilt.  d_outliers / d_rebuilt: [n_rows].
int kd_sweep_mapped(amk_kd *pool, int n_rows, const int *d_kf_list, const int *d_cur_list, double th_dist, int th_count,
                    int *d_outliers, int *d_rebuilt, hipStream_t stream) {
    if (!pool || n_rows < 1 || !d_kf_list || !d_cur_list || !d_rebuilt) return AMK_ERR_INVALID_ARG;
    int st = pool_planes(pool);
    if (st != AMK_OK) return st;
    if (!pool->flags.p) AMK_HIP(pool->flags.alloc((size_t)pool->n_scenes * pool->cap));
    const amk::GridPtrs cur = grid_ptrs(pool);
    if (pool->max_points > 0 && g_sweep_target) {   // the current frames once more, as fine hashed grids (one per sweep row)
        const int nb = sweep_buckets(pool->max_points);
        if (pool->sw_rows < n_rows) {
            if (pool->sw_rows > 0) AMK_HIP(hipDeviceSynchronize());   // (growing: earlier sweeps may still read the old arrays)
            st = sweep_reserve(pool, n_rows);
            if (st != AMK_OK) return st;
        }
        // > 64 KB of dynamic LDS needs the attribute; it is per device and the call is cheap, so it is made before every launch
        // (a process-wide flag would leave a second device, or a second thread's first launch, without it)
        AMK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kd_sweep_hash_build_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(sizeof(int) * (kSweepBuckets + kSweepBuildThreads / 64)) + 65536));
        static const double factor = [] { const char *e = getenv("AMK_SWEEP_CELL"); const double v = e ? atof(e) : 2.5; return v >= 2.1 ? v : 2.5; }();
        const double cell = fmax(factor * th_dist, 1e-3);   // edge of a cell: the cube [q - th, q + th] touches <= 2 cells per axis
        const double inv_h = 1.0 / cell;
        // generations alternate per call; a call with another row count than the one the arrays were sized for is refused (rows are the
        // map's scenes)
        if (n_rows != pool->sw_rows) return AMK_ERR_INVALID_ARG;
        if (pool->sw_inv_h != inv_h) {   // another lattice than the last call's: the previous generation's grids are not this one's cells
            if (pool->sw_inv_h != 0.0) AMK_HIP(hipMemsetAsync(pool->sw_src.p, 0xff, sizeof(int) * 2 * (size_t)n_rows, stream));
            pool->sw_inv_h = inv_h;
        }
        const int g = pool->sw_flip ^= 1;
        float4 *recs_g = pool->sw_gpt.p + (size_t)g * n_rows * pool->cap, *recs_p = pool->sw_gpt.p + (size_t)(g ^ 1) * n_rows * pool->cap;
        int *tab_g = pool->sw_cs.p + (size_t)g * n_rows * (nb + 1), *tab_p = pool->sw_cs.p + (size_t)(g ^ 1) * n_rows * (nb + 1);
        int *src_g = pool->sw_src.p + (size_t)g * n_rows, *src_p = pool->sw_src.p + (size_t)(g ^ 1) * n_rows;
        static const int extra_lds = [] { const char *e = getenv("AMK_SWEEP_BUILD_EXTRA_LDS"); return e ? atoi(e) : 0; }();   // (experiments: blocks per CU)
        hipLaunchKernelGGL(kd_sweep_hash_build_kernel, dim3(n_rows), dim3(kSweepBuildThreads), sizeof(int) * (nb + kSweepBuildThreads / 64) + extra_lds,
                           stream, pool->gpt.p, pool->cap, pool->size.p, inv_h, nb, recs_g, tab_g, d_kf_list, d_cur_list,
                           src_g, src_p, pool->flags.p);
        hipLaunchKernelGGL(kd_sweep_mark_hash_kernel, dim3((pool->max_points + kSweepMarkThreads - 1) / kSweepMarkThreads, n_rows), dim3(kSweepMarkThreads), 0, stream, pool->size.p,
                           recs_g, tab_g, inv_h, nb, pool->gpt.p, pool->cap, pool->size.p, th_dist, pool->flags.p, d_kf_list, d_cur_list,
                           recs_p, tab_p, g_sweep_order ? src_p : pool->sw_src.p + (size_t)2 * n_rows);
    }
    else if (pool->max_points > 0)
        hipLaunchKernelGGL(kd_sweep_mark_kernel, dim3((pool->max_points + 255) / 256, n_rows), dim3(256), 0, stream, cur, pool->size.p,
                           pool->gpt.p, pool->cap, pool->size.p, th_dist, pool->flags.p, d_kf_list, d_cur_list);
    hipLaunchKernelGGL(kd_sweep_compact_kernel, dim3(n_rows), dim3(kCompactThreads), 0, stream, pool->x.p, pool->y.p, pool->z.p,
                       pool->cap, pool->size.p, pool->pmax.p, pool->bbox.p, pool->flags.p, th_count, (int *)nullptr, d_outliers,
                       d_rebuilt, d_kf_list);
    hipLaunchKernelGGL(kd_grid_build_list_kernel, dim3(n_rows), dim3(amk::kGridBuildThreads), 0, stream, pool->x.p, pool->y.p,
                       pool->z.p, pool->cap, pool->size.p, pool->bbox.p, pool->gpt.p, pool->cell_start.p, pool->ntiles,
                       pool->gparams.p, d_kf_list, d_rebuilt);
    AMK_HIP(hipGetLastError());
    pool->async_pending = 1;
    return AMK_OK;
}
}  // namespace amk

extern "C" int amk_kd_keyframe_sweep_host(amk_kd *keyframe, amk_kd *current, double th_dist, int th_count,
                                          int *h_outliers, int *h_rebuilt) {
    int st = amk_kd_keyframe_sweep(keyframe, current, th_dist, th_count, nullptr, nullptr, nullptr);
    if (st != AMK_OK) return st;
    std::vector<int> tmp((size_t)keyframe->n_scenes * 2);
    st = amk::read_back({{tmp.data(), keyframe->sweep_cnt.p, sizeof(int) * tmp.size()}});
    if (st != AMK_OK) return st;
    for (int s = 0; s < keyframe->n_scenes; ++s) {
        if (h_outliers) h_outliers[s] = tmp[2 * s];
        if (h_rebuilt) h_rebuilt[s] = tmp[2 * s + 1];
    }
    return AMK_OK;
}
