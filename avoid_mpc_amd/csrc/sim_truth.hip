// Ground truth against the simulated world for gfx950: where a point stands relative to the true solids (amk_sim_clearance) and where
// a sphere moving along a path first touches one (amk_sim_segment_cast per leg, amk_sim_path_cast per scene).  The world is the one
// amk_sim_render_world renders (sim.hip): the ground z = 0, vertical cylinders (cx, cy, r) cut at z_top, yawed boxes
// (cx, cy, hx, hy, c, s, z0, z1).  The map queries (amk_kd_segment_cast, amk_kd_path_cast, the pipeline's audit) judge a plan against
// what the robot has SEEN; these judge it against what is THERE, in the same output shapes, so the two verdicts stand side by side.
// Contract: include/avoid_mpc_amd.h, "Ground truth against the simulated world"; the numpy restatements are avoid_mpc_amd/flight.py
// world_clearance_ordered / world_segment_cast_ordered / world_path_cast_ordered.
//
// SHAPE.  A fleet call is a few hundred scenes x ~20 legs x ~100 solids: too few rows for a thread per row.  The solids go across the
// lanes instead: a wavefront owns one point (or leg) at a time, lane k tests solid k of a round of kTruthChunk = 64, and a wave-wide
// minimum over the pair (value, position in the order ground - cylinders - boxes) picks the answer.  That pair order is total (no two
// candidates share a position and a NaN never becomes a candidate), so the minimum does not depend on the reduction tree and equals the
// sequential scan "least value under a strict <, in order" bit for bit.
// The lanes read their records straight from global memory -- lane k record base + k, a contiguous run of 64 x 24 or 64 x 64 bytes --
// and not through LDS: nothing about a record is shared between legs (every term depends on the leg's origin), the per-leg state
// lives in the owning wave's registers for any n_points, and the clearance and segment kernels then need no barrier at all, so their
// grid is (rows / waves, scenes) and fills the chip at fleet sizes.  A scene's ~6 KB of records stay in L2 / the vector L1 between
// the legs.  Only the path cast keeps a block per scene: its waves cast kTruthWaves legs per round, lane 0 of each leaves the leg's
// answer in LDS, and behind ONE barrier per round (two LDS generations, by parity) every thread runs the same in-order reduction over
// the round's legs, so "stop found" is block-uniform and the legs behind the stop leg's round are never walked.
// BARRIERS (path kernel only): the round loop's trip count comes from n_points and from LDS words every thread reads alike; a wave
// whose leg lies behind the path's end skips the cast, not the barrier.
// NaN.  A solid with a NaN in any entry answers nothing: every lane tests its record's entries with e == e and drops the candidate,
// in front of any select that could lose the NaN.  No atomics, no scratch, no inline assembly.
#include <climits>
#include <cmath>

#include "amk_common.h"

namespace {

constexpr int kTruthThreads = 256;
constexpr int kTruthWaves = kTruthThreads / amk::kWave;   // points / legs in flight per block (amk__sim_truth_waves)
constexpr int kTruthChunk = amk::kWave;                   // solids per round, one per lane (amk__sim_truth_chunk)
constexpr int kNone = INT_MAX;                            // position of "no candidate": behind every solid

struct TruthWorld {
    const double *cyl; const int *cyl_counts; int max_cyl;
    const double *box; const int *box_counts; int max_box;
    double z_top;
};

#pragma clang fp contract(off)

__device__ __forceinline__ int clamped_count(const int *counts, int scene, int max) {
    const int n = counts ? counts[scene] : max;
    return n < 0 ? 0 : (n > max ? max : n);
}

// the lexicographic minimum of (v, pos) over the wave, left in every lane; v is never NaN here
__device__ __forceinline__ void wave_min_pair(double &v, int &pos) {
#pragma unroll
    for (int off = amk::kWave / 2; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int op = __shfl_xor(pos, off);
        if (ov < v || (ov == v && op < pos)) { v = ov; pos = op; }
    }
}

// position in the order -> (kind, index): 0 ground, 1 cylinder, 2 box; kNone: (-1, -1)
__device__ __forceinline__ void kind_index(int pos, int nc, int &kind, int &index) {
    kind = pos == kNone ? -1 : pos == 0 ? 0 : pos <= nc ? 1 : 2;
    index = pos == kNone || pos == 0 ? -1 : pos <= nc ? pos - 1 : pos - 1 - nc;
}

// ---- clearance ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double cyl_distance(double cx, double cy, double r, double px, double py, double pz, double z_top) {
    const double ox = px - cx, oy = py - cy;
    const double qr = sqrt(ox * ox + oy * oy) - r, qz = pz - z_top;
    const double mr = qr > 0.0 ? qr : 0.0, mz = qz > 0.0 ? qz : 0.0;
    const double m = qr > qz ? qr : qz;
    return sqrt(mr * mr + mz * mz) + (m < 0.0 ? m : 0.0);
}

__device__ __forceinline__ double box_distance(const double *q, double px, double py, double pz) {
    const double ox = px - q[0], oy = py - q[1], hx = q[2], hy = q[3], c = q[4], s = q[5], z0 = q[6], z1 = q[7];
    const double olx = c * ox + s * oy, oly = c * oy - s * ox;
    const double qx = fabs(olx) - fabs(hx), qy = fabs(oly) - fabs(hy);
    const double lo = z0 - pz, hi = pz - z1;
    const double qz = lo > hi ? lo : hi;
    const double mx = qx > 0.0 ? qx : 0.0, my = qy > 0.0 ? qy : 0.0, mz = qz > 0.0 ? qz : 0.0;
    double m = qx > qy ? qx : qy;
    m = qz > m ? qz : m;
    return sqrt((mx * mx + my * my) + mz * mz) + (m < 0.0 ? m : 0.0);
}

// One wave per point, grid (points / kTruthWaves, scene).  No barrier: a wave behind the last point simply leaves.
__global__ __launch_bounds__(kTruthThreads) void sim_truth_clearance_kernel(TruthWorld w, const double *__restrict__ pts, int stride,
                                                                             int n_points, double *__restrict__ dist, int *__restrict__ kind,
                                                                             int *__restrict__ index) {
    const int lane = threadIdx.x % amk::kWave, wave = __builtin_amdgcn_readfirstlane(threadIdx.x / amk::kWave);
    const int scene = blockIdx.y, p = blockIdx.x * kTruthWaves + wave;
    if (p >= n_points) return;
    const double *q = pts + ((size_t)scene * n_points + p) * stride;
    const double px = q[0], py = q[1], pz = q[2];
    const int nc = clamped_count(w.cyl_counts, scene, w.max_cyl), nb = clamped_count(w.box_counts, scene, w.max_box);
    double best = pz;                                            // the ground, in every lane alike
    int pos = 0;
    if (!(pz == pz)) best = INFINITY;                            // (a NaN height is put back behind the reduction)
    const double *sc = w.cyl + (size_t)scene * w.max_cyl * 3;
    for (int base = 0; base < nc; base += kTruthChunk) {
        const int k = base + lane;
        if (k < nc) {
            const double cx = sc[(size_t)k * 3], cy = sc[(size_t)k * 3 + 1], r = sc[(size_t)k * 3 + 2];
            const double d = cyl_distance(cx, cy, r, px, py, pz, w.z_top);
            if (cx == cx && cy == cy && r == r && d < best) { best = d; pos = 1 + k; }
        }
    }
    const double *sb = w.box + (size_t)scene * w.max_box * 8;
    for (int base = 0; base < nb; base += kTruthChunk) {
        const int k = base + lane;
        if (k < nb) {
            double e[8];
            bool ok = true;
#pragma unroll
            for (int i = 0; i < 8; ++i) { e[i] = sb[(size_t)k * 8 + i]; ok = ok && e[i] == e[i]; }
            const double d = box_distance(e, px, py, pz);
            if (ok && d < best) { best = d; pos = 1 + nc + k; }
        }
    }
    wave_min_pair(best, pos);
    if (!(pz == pz)) { best = pz; pos = 0; }                     // the sequential scan starts at the ground's NaN and nothing is < NaN
    if (lane == 0) {
        const size_t o = (size_t)scene * n_points + p;
        int kd, ix;
        kind_index(pos, nc, kd, ix);
        if (dist) dist[o] = best;
        if (kind) kind[o] = kd;
        if (index) index[o] = ix;
    }
}

// ---- casts ----------------------------------------------------------------------------------------------------------------------
// the half-space z <= h along a_z + t d_z: one bound, near or far by the sign of d_z; d_z == 0: all or nothing by the origin
__device__ __forceinline__ void half_space(double h, double az, double dz, double inv_z, double &near, double &far) {
    const double bound = (h - az) * inv_z;
    near = dz < 0.0 ? bound : -INFINITY;
    far = dz > 0.0 ? bound : INFINITY;
    if (dz == 0.0) {
        const bool inside = az <= h;
        near = inside ? -INFINITY : INFINITY;
        far = inside ? INFINITY : -INFINITY;
    }
}

// sim.hip's box_slab, word for word (restated: that file is not edited)
__device__ __forceinline__ void box_slab(double lo_o, double hi_o, double d, double inv, bool inside, double &near, double &far) {
    const double t1 = lo_o * inv, t2 = hi_o * inv;
    const bool lt = t1 < t2;
    near = lt ? t1 : t2;
    far = lt ? t2 : t1;
    if (d == 0.0) {
        near = inside ? -INFINITY : INFINITY;
        far = inside ? INFINITY : -INFINITY;
    }
}

struct TruthLeg {
    double ax, ay, az, dx, dy, dz, inv_z, a2;
    bool judgeable;                                              // every coordinate of a, b and d finite
};

__device__ __forceinline__ TruthLeg load_leg(const double *a, int stride) {
    TruthLeg g;
    const double *b = a + stride;
    g.ax = a[0]; g.ay = a[1]; g.az = a[2];
    g.dx = b[0] - g.ax; g.dy = b[1] - g.ay; g.dz = b[2] - g.az;
    g.judgeable = isfinite(g.ax) && isfinite(g.ay) && isfinite(g.az) && isfinite(b[0]) && isfinite(b[1]) && isfinite(b[2]) &&
                  isfinite(g.dx) && isfinite(g.dy) && isfinite(g.dz);
    g.inv_z = 1.0 / g.dz;
    g.a2 = g.dx * g.dx + g.dy * g.dy;
    return g;
}

__device__ __forceinline__ double leg_length(const TruthLeg &g) { return sqrt((g.dx * g.dx + g.dy * g.dy) + g.dz * g.dz); }

// tn, tf of a solid whose axes all have near <= far (ok) -> touched, and the t it is touched at
__device__ __forceinline__ bool touched(bool ok, double tn, double tf, double &t) {
    t = tn > 0.0 ? tn : 0.0;
    return ok && tn <= tf && tf >= 0.0 && tn <= 1.0;
}

// The first contact of one judgeable leg with the scene's inflated solids: every lane leaves with the same (t, pos); pos == kNone: none.
__device__ __forceinline__ void cast_leg(const TruthWorld &w, int scene, int nc, int nb, const TruthLeg &g, double radius, int lane,
                                         double &best, int &pos) {
    best = INFINITY; pos = kNone;
    double n0, f0, n1, f1, n2, f2, t;
    half_space(radius, g.az, g.dz, g.inv_z, n0, f0);             // the ground, inflated: z <= radius (every lane alike)
    if (touched(n0 <= f0, n0, f0, t)) { best = t; pos = 0; }
    const double top = w.z_top + radius;
    const double *sc = w.cyl + (size_t)scene * w.max_cyl * 3;
    for (int base = 0; base < nc; base += kTruthChunk) {
        const int k = base + lane;
        if (k < nc) {
            const double cx = sc[(size_t)k * 3], cy = sc[(size_t)k * 3 + 1], r = sc[(size_t)k * 3 + 2];
            const double ox = g.ax - cx, oy = g.ay - cy, R = r + radius;
            const double b = ox * g.dx + oy * g.dy;
            const double c = (ox * ox + oy * oy) - R * R;
            const double disc = b * b - g.a2 * c;
            n0 = INFINITY; f0 = -INFINITY;                       // the mantle: nothing, unless ...
            if (g.a2 == 0.0) {
                if (c <= 0.0) { n0 = -INFINITY; f0 = INFINITY; }
            } else if (disc >= 0.0) {
                const double sq = sqrt(disc);
                n0 = (-b - sq) / g.a2;
                f0 = (-b + sq) / g.a2;
            }
            half_space(top, g.az, g.dz, g.inv_z, n1, f1);        // cut at z_top + radius
            const double tn = n0 > n1 ? n0 : n1, tf = f0 < f1 ? f0 : f1;
            if (cx == cx && cy == cy && r == r && touched(n0 <= f0 && n1 <= f1, tn, tf, t) && t < best) { best = t; pos = 1 + k; }
        }
    }
    const double *sb = w.box + (size_t)scene * w.max_box * 8;
    for (int base = 0; base < nb; base += kTruthChunk) {
        const int k = base + lane;
        if (k < nb) {
            double e[8];
            bool ok = true;
#pragma unroll
            for (int i = 0; i < 8; ++i) { e[i] = sb[(size_t)k * 8 + i]; ok = ok && e[i] == e[i]; }
            const double ox = g.ax - e[0], oy = g.ay - e[1], c = e[4], s = e[5];
            const double hx = fabs(e[2]) + radius, hy = fabs(e[3]) + radius, z0 = e[6] - radius, z1 = e[7] + radius;
            const double olx = c * ox + s * oy, oly = c * oy - s * ox;
            const double dlx = c * g.dx + s * g.dy, dly = c * g.dy - s * g.dx;
            box_slab(-hx - olx, hx - olx, dlx, 1.0 / dlx, -hx <= olx && olx <= hx, n0, f0);
            box_slab(-hy - oly, hy - oly, dly, 1.0 / dly, -hy <= oly && oly <= hy, n1, f1);
            box_slab(z0 - g.az, z1 - g.az, g.dz, g.inv_z, z0 <= g.az && g.az <= z1, n2, f2);
            double tn = n0 > n1 ? n0 : n1, tf = f0 < f1 ? f0 : f1;
            tn = n2 > tn ? n2 : tn;
            tf = f2 < tf ? f2 : tf;
            if (ok && touched(n0 <= f0 && n1 <= f1 && n2 <= f2, tn, tf, t) && t < best) { best = t; pos = 1 + nc + k; }
        }
    }
    wave_min_pair(best, pos);
}

// One wave per leg, grid (legs / kTruthWaves, scene).  No barrier.
__global__ __launch_bounds__(kTruthThreads) void sim_truth_segment_kernel(TruthWorld w, const double *__restrict__ path, int stride,
                                                                           int n_points, double radius, int *__restrict__ hit,
                                                                           double *__restrict__ t_out, int *__restrict__ kind,
                                                                           int *__restrict__ index) {
    const int lane = threadIdx.x % amk::kWave, wave = __builtin_amdgcn_readfirstlane(threadIdx.x / amk::kWave);
    const int scene = blockIdx.y, legs = n_points - 1, j = blockIdx.x * kTruthWaves + wave;
    if (j >= legs) return;
    const TruthLeg g = load_leg(path + ((size_t)scene * n_points + j) * stride, stride);
    const int nc = clamped_count(w.cyl_counts, scene, w.max_cyl), nb = clamped_count(w.box_counts, scene, w.max_box);
    double best = INFINITY;
    int pos = kNone;
    if (g.judgeable) cast_leg(w, scene, nc, nb, g, radius, lane, best, pos);   // (wave-uniform: the leg is the wave's)
    if (lane == 0) {
        const size_t o = (size_t)scene * legs + j;
        int kd, ix;
        kind_index(pos, nc, kd, ix);
        if (hit) hit[o] = pos != kNone;
        if (t_out) t_out[o] = pos != kNone ? best : 1.0;
        if (kind) kind[o] = kd;
        if (index) index[o] = ix;
    }
}

struct TruthPathOut {
    int *stop, *leg;
    double *t, *free, *pts;
    int *kind, *index;
    bool any() const { return stop || leg || t || free || pts || kind || index; }
};

// One block per scene.  Per round the block's waves cast kTruthWaves consecutive legs with cast_leg -- the segment kernel's own
// function, hence its bits -- and every thread then reduces the round in leg order from LDS.
__global__ __launch_bounds__(kTruthThreads) void sim_truth_path_kernel(TruthWorld w, const double *__restrict__ path, int stride,
                                                                        int n_points, double radius, TruthPathOut out) {
    __shared__ double s_t[2][kTruthWaves], s_len[2][kTruthWaves];
    __shared__ int s_state[2][kTruthWaves], s_pos[2][kTruthWaves];   // state: 0 no contact, 1 contact, 2 unjudgeable
    const int lane = threadIdx.x % amk::kWave, wave = __builtin_amdgcn_readfirstlane(threadIdx.x / amk::kWave);
    const int scene = blockIdx.x, legs = n_points - 1;
    const double *sp = path + (size_t)scene * n_points * stride;
    const int nc = clamped_count(w.cyl_counts, scene, w.max_cyl), nb = clamped_count(w.box_counts, scene, w.max_box);
    double acc = 0.0, t_stop = 1.0;                              // 0.0 + len_0 is len_0: the sum is (len_0 + len_1) + ...
    int stop = 0, leg = -1, pos = kNone;
    for (int base = 0, gen = 0; base < legs && !stop; base += kTruthWaves, gen ^= 1) {
        const int j = base + wave;
        if (j < legs) {
            const TruthLeg g = load_leg(sp + (size_t)j * stride, stride);
            double best = INFINITY;
            int p = kNone;
            if (g.judgeable) cast_leg(w, scene, nc, nb, g, radius, lane, best, p);
            if (lane == 0) {
                s_state[gen][wave] = !g.judgeable ? 2 : p != kNone ? 1 : 0;
                s_t[gen][wave] = best; s_pos[gen][wave] = p;
                s_len[gen][wave] = leg_length(g);
            }
        }
        __syncthreads();
        const int m = legs - base < kTruthWaves ? legs - base : kTruthWaves;
        for (int k = 0; k < m && !stop; ++k) {
            const int state = s_state[gen][k];
            if (state == 2) { stop = 2; leg = base + k; t_stop = 0.0; }
            else if (state == 1) {
                stop = 1; leg = base + k; t_stop = s_t[gen][k]; pos = s_pos[gen][k];
                acc = acc + t_stop * s_len[gen][k];
            } else acc = acc + s_len[gen][k];
        }
    }
    if (threadIdx.x != 0) return;                                // (behind the last barrier)
    int kd, ix;
    kind_index(pos, nc, kd, ix);
    if (out.stop) out.stop[scene] = stop;
    if (out.leg) out.leg[scene] = leg;
    if (out.t) out.t[scene] = t_stop;
    if (out.free) out.free[scene] = acc;
    if (out.kind) out.kind[scene] = kd;
    if (out.index) out.index[scene] = ix;
    if (out.pts) {
        double c0 = 0.0, c1 = 0.0, c2 = 0.0;
        if (stop == 1) {
            const TruthLeg g = load_leg(sp + (size_t)leg * stride, stride);
            c0 = g.ax + t_stop * g.dx; c1 = g.ay + t_stop * g.dy; c2 = g.az + t_stop * g.dz;
        }
        out.pts[(size_t)scene * 3] = c0; out.pts[(size_t)scene * 3 + 1] = c1; out.pts[(size_t)scene * 3 + 2] = c2;
    }
}

// ---- what the entries refuse, before anything is staged or launched ----------------------------------------------------------------
// A grid dimension times the block's 256 threads has to stay below 2^32: at most 2^24 - 1 blocks along x.  `rows` are the points or legs
// of a scene (kTruthWaves of them per block, scenes along y, at most 65 535) or, for the path cast, the scenes themselves (rows_per_block 1).
constexpr long long kTruthMaxBlocks = (1ll << 24) - 1;

int world_args_status(const double *cyl, int max_cyl, const double *box, int max_box, int n_scenes, double z_top, long long rows,
                      int rows_per_block, bool grid_y) {
    if (max_cyl < 0 || max_box < 0 || (!cyl && max_cyl > 0) || (!box && max_box > 0) || n_scenes < 1 || !(z_top >= 0.0))
        return AMK_ERR_INVALID_ARG;
    if ((long long)max_cyl + max_box > INT_MAX - 1) return AMK_ERR_UNSUPPORTED;   // (a solid's position in the order is an int)
    if (grid_y && n_scenes > 65535) return AMK_ERR_UNSUPPORTED;                   // (scenes are the grid's second dimension)
    if ((rows + rows_per_block - 1) / rows_per_block > kTruthMaxBlocks) return AMK_ERR_UNSUPPORTED;
    return AMK_OK;
}

int clearance_args_status(const double *cyl, int max_cyl, const double *box, int max_box, int n_scenes, double z_top, const double *pts,
                          int point_stride, int n_points, bool any_out) {
    if (!pts || point_stride < 3 || n_points < 1 || !any_out) return AMK_ERR_INVALID_ARG;
    return world_args_status(cyl, max_cyl, box, max_box, n_scenes, z_top, n_points, kTruthWaves, true);
}

// per_scene: the path cast, a block per scene along x; otherwise a wave per leg along x and the scenes along y
int cast_args_status(const double *cyl, int max_cyl, const double *box, int max_box, int n_scenes, double z_top, const double *path,
                     int point_stride, int n_points, double radius, bool any_out, bool per_scene) {
    if (!path || point_stride < 3 || n_points < 2 || !(radius >= 0.0) || !any_out) return AMK_ERR_INVALID_ARG;
    return per_scene ? world_args_status(cyl, max_cyl, box, max_box, n_scenes, z_top, n_scenes, 1, false)
                     : world_args_status(cyl, max_cyl, box, max_box, n_scenes, z_top, (long long)n_points - 1, kTruthWaves, true);
}

// the world's four host arrays as staging slots, in the order of the entries' leading arguments
enum { W_CYL, W_CYL_COUNTS, W_BOX, W_BOX_COUNTS, W_POINTS, W_OUT };
#define AMK_TRUTH_WORLD_SLOTS                                                                                                          \
    amk::to_device(h_cyl, sizeof(double) * 3 * (size_t)max_cyl * n_scenes), amk::if_given(amk::to_device(h_cyl_counts, sizeof(int) * n_scenes)), \
        amk::to_device(h_box, sizeof(double) * 8 * (size_t)max_box * n_scenes), amk::if_given(amk::to_device(h_box_counts, sizeof(int) * n_scenes))

}  // namespace

extern "C" {

int amk__sim_truth_chunk(void) { return kTruthChunk; }   // tests only: solids per round (one per lane)
int amk__sim_truth_waves(void) { return kTruthWaves; }   // tests only: points / legs in flight per block

int amk_sim_clearance(const double *d_cyl, const int *d_cyl_counts, int max_cyl, const double *d_box, const int *d_box_counts, int max_box,
                      int n_scenes, double z_top, const double *d_pts, int point_stride, int n_points, double *d_dist, int *d_kind,
                      int *d_index, void *stream) {
    if (const int st = clearance_args_status(d_cyl, max_cyl, d_box, max_box, n_scenes, z_top, d_pts, point_stride, n_points,
                                             d_dist || d_kind || d_index); st != AMK_OK)
        return st;
    if (amk_device_count() <= 0) return AMK_ERR_NO_DEVICE;
    const TruthWorld w{d_cyl, d_cyl_counts, max_cyl, d_box, d_box_counts, max_box, z_top};
    const dim3 grid((unsigned)(((long long)n_points + kTruthWaves - 1) / kTruthWaves), (unsigned)n_scenes);
    hipLaunchKernelGGL(sim_truth_clearance_kernel, grid, dim3(kTruthThreads), 0, (hipStream_t)stream, w, d_pts, point_stride, n_points,
                       d_dist, d_kind, d_index);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

int amk_sim_clearance_host(const double *h_cyl, const int *h_cyl_counts, int max_cyl, const double *h_box, const int *h_box_counts,
                           int max_box, int n_scenes, double z_top, const double *h_pts, int point_stride, int n_points, double *h_dist,
                           int *h_kind, int *h_index) {
    if (const int st = clearance_args_status(h_cyl, max_cyl, h_box, max_box, n_scenes, z_top, h_pts, point_stride, n_points,
                                             h_dist || h_kind || h_index); st != AMK_OK)
        return st;
    if (amk_device_count() <= 0) return AMK_ERR_NO_DEVICE;
    const size_t rows = (size_t)n_scenes * n_points;
    amk::HostStage stage;
    return stage.call({AMK_TRUTH_WORLD_SLOTS, amk::to_device(h_pts, sizeof(double) * amk::points_extent(n_scenes, n_points, point_stride)),
                       amk::if_given(amk::to_host(h_dist, sizeof(double) * rows)), amk::if_given(amk::to_host(h_kind, sizeof(int) * rows)),
                       amk::if_given(amk::to_host(h_index, sizeof(int) * rows))},
                      [&](const amk::HostStage::Dev *d) {
                          return amk_sim_clearance(d[W_CYL], d[W_CYL_COUNTS], max_cyl, d[W_BOX], d[W_BOX_COUNTS], max_box, n_scenes, z_top,
                                                   d[W_POINTS], point_stride, n_points, d[W_OUT], d[W_OUT + 1], d[W_OUT + 2], nullptr);
                      },
                      hipDeviceSynchronize);
}

int amk_sim_segment_cast(const double *d_cyl, const int *d_cyl_counts, int max_cyl, const double *d_box, const int *d_box_counts,
                         int max_box, int n_scenes, double z_top, const double *d_path, int point_stride, int n_points, double radius,
                         int *d_hit, double *d_t, int *d_kind, int *d_index, void *stream) {
    if (const int st = cast_args_status(d_cyl, max_cyl, d_box, max_box, n_scenes, z_top, d_path, point_stride, n_points, radius,
                                        d_hit || d_t || d_kind || d_index, false); st != AMK_OK)
        return st;
    if (amk_device_count() <= 0) return AMK_ERR_NO_DEVICE;
    const TruthWorld w{d_cyl, d_cyl_counts, max_cyl, d_box, d_box_counts, max_box, z_top};
    const dim3 grid((unsigned)(((long long)n_points - 1 + kTruthWaves - 1) / kTruthWaves), (unsigned)n_scenes);
    hipLaunchKernelGGL(sim_truth_segment_kernel, grid, dim3(kTruthThreads), 0, (hipStream_t)stream, w, d_path, point_stride, n_points,
                       radius, d_hit, d_t, d_kind, d_index);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

int amk_sim_segment_cast_host(const double *h_cyl, const int *h_cyl_counts, int max_cyl, const double *h_box, const int *h_box_counts,
                              int max_box, int n_scenes, double z_top, const double *h_path, int point_stride, int n_points, double radius,
                              int *h_hit, double *h_t, int *h_kind, int *h_index) {
    if (const int st = cast_args_status(h_cyl, max_cyl, h_box, max_box, n_scenes, z_top, h_path, point_stride, n_points, radius,
                                        h_hit || h_t || h_kind || h_index, false); st != AMK_OK)
        return st;
    if (amk_device_count() <= 0) return AMK_ERR_NO_DEVICE;
    const size_t rows = (size_t)n_scenes * (n_points - 1);
    amk::HostStage stage;
    return stage.call({AMK_TRUTH_WORLD_SLOTS, amk::to_device(h_path, sizeof(double) * amk::points_extent(n_scenes, n_points, point_stride)),
                       amk::if_given(amk::to_host(h_hit, sizeof(int) * rows)), amk::if_given(amk::to_host(h_t, sizeof(double) * rows)),
                       amk::if_given(amk::to_host(h_kind, sizeof(int) * rows)), amk::if_given(amk::to_host(h_index, sizeof(int) * rows))},
                      [&](const amk::HostStage::Dev *d) {
                          return amk_sim_segment_cast(d[W_CYL], d[W_CYL_COUNTS], max_cyl, d[W_BOX], d[W_BOX_COUNTS], max_box, n_scenes, z_top,
                                                      d[W_POINTS], point_stride, n_points, radius, d[W_OUT], d[W_OUT + 1], d[W_OUT + 2],
                                                      d[W_OUT + 3], nullptr);
                      },
                      hipDeviceSynchronize);
}

int amk_sim_path_cast(const double *d_cyl, const int *d_cyl_counts, int max_cyl, const double *d_box, const int *d_box_counts, int max_box,
                      int n_scenes, double z_top, const double *d_path, int point_stride, int n_points, double radius, int *d_stop,
                      int *d_leg, double *d_t, double *d_free, double *d_pts, int *d_kind, int *d_index, void *stream) {
    const TruthPathOut out{d_stop, d_leg, d_t, d_free, d_pts, d_kind, d_index};
    if (const int st = cast_args_status(d_cyl, max_cyl, d_box, max_box, n_scenes, z_top, d_path, point_stride, n_points, radius, out.any(),
                                        true); st != AMK_OK)
        return st;
    if (amk_device_count() <= 0) return AMK_ERR_NO_DEVICE;
    const TruthWorld w{d_cyl, d_cyl_counts, max_cyl, d_box, d_box_counts, max_box, z_top};
    hipLaunchKernelGGL(sim_truth_path_kernel, dim3((unsigned)n_scenes), dim3(kTruthThreads), 0, (hipStream_t)stream, w, d_path, point_stride,
                       n_points, radius, out);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

int amk_sim_path_cast_host(const double *h_cyl, const int *h_cyl_counts, int max_cyl, const double *h_box, const int *h_box_counts,
                           int max_box, int n_scenes, double z_top, const double *h_path, int point_stride, int n_points, double radius,
                           int *h_stop, int *h_leg, double *h_t, double *h_free, double *h_pts, int *h_kind, int *h_index) {
    if (const int st = cast_args_status(h_cyl, max_cyl, h_box, max_box, n_scenes, z_top, h_path, point_stride, n_points, radius,
                                        h_stop || h_leg || h_t || h_free || h_pts || h_kind || h_index, true); st != AMK_OK)
        return st;
    if (amk_device_count() <= 0) return AMK_ERR_NO_DEVICE;
    const size_t rows = (size_t)n_scenes;
    amk::HostStage stage;
    return stage.call({AMK_TRUTH_WORLD_SLOTS, amk::to_device(h_path, sizeof(double) * amk::points_extent(n_scenes, n_points, point_stride)),
                       amk::if_given(amk::to_host(h_stop, sizeof(int) * rows)), amk::if_given(amk::to_host(h_leg, sizeof(int) * rows)),
                       amk::if_given(amk::to_host(h_t, sizeof(double) * rows)), amk::if_given(amk::to_host(h_free, sizeof(double) * rows)),
                       amk::if_given(amk::to_host(h_pts, sizeof(double) * rows * 3)), amk::if_given(amk::to_host(h_kind, sizeof(int) * rows)),
                       amk::if_given(amk::to_host(h_index, sizeof(int) * rows))},
                      [&](const amk::HostStage::Dev *d) {
                          return amk_sim_path_cast(d[W_CYL], d[W_CYL_COUNTS], max_cyl, d[W_BOX], d[W_BOX_COUNTS], max_box, n_scenes, z_top,
                                                   d[W_POINTS], point_stride, n_points, radius, d[W_OUT], d[W_OUT + 1], d[W_OUT + 2],
                                                   d[W_OUT + 3], d[W_OUT + 4], d[W_OUT + 5], d[W_OUT + 6], nullptr);
                      },
                      hipDeviceSynchronize);
}

}  // extern "C"
