// Depth image -> world-frame obstacle cloud for gfx950: FrameKDMap::ProcessDepth
// (AM/src/FrameKDMap.cpp:90-130 with GetInvDepthImg :76-89 and UV2Camera :131-138; AM = roswrapper/ros/src/avoid_mpc
// in the reference tree).  SURVEY.md section 8 row f2: the per-pixel streaming step right before the tree build.
//
// amk_depth_to_cloud / amk_depth_to_edge_cloud: one block per scene (the edge cloud up to AMK_EDGE_MAX_PIXELS pixels);
// amk_depth_to_clouds: both clouds, above that size on one block per band of rows (depth_band_kernel).
// Every rule of the reference is written once, as a device helper (obstacle_depth, quantise, to_world, EdgeLayers); the three
// kernels are control flow over them and differ only in which image rows a block holds in LDS (one exception, for its measured
// cost: the keep test behind depth_to_edge_kernel's `any` flag is written out there).
// Only the 2x2 raw pixels under each down-scaled pixel are read (4 % of a 640x480 image at
// resize_scale 10): the reference inverts the whole image and then lets cv::resize pick the same four taps.
// The kept pixels are appended in row-major order (ballot + popcount prefix per wave, LDS combine per block),
// which is the order the reference's emplace_back produces and therefore the index space of the KD tree.
#include <algorithm>
#include <cstring>
#include <type_traits>

#include "amk_common.h"

namespace {

constexpr int kDepthThreads = 256;

struct DepthGeom {
    int rows, cols, W, H;
    double scale_x, scale_y;       // source pixels per destination pixel (cv::resize: 1 / (dsize / ssize))
    double pixel2meter, dmin, dmax;
    double fx, fy, cx, cy;         // already divided by resize_scale
    double Tbc[16];
};

#pragma clang fp contract(off)
template <typename T>
__device__ __forceinline__ float inv_depth(const T *img, int r, int c, int cols, const DepthGeom &g) {
    const float depth = (float)((double)(float)img[(size_t)r * cols + c] * g.pixel2meter);   // :80-81
    if ((double)depth < g.dmin || (double)depth > g.dmax) return 0.f;                        // :82-83
    return (float)(1.0 / (double)depth);                                                      // :85
}

// cv::resize INTER_LINEAR tap of destination index d along an axis of n source samples: source index and the
// weight of the second tap, in float as OpenCV computes them for CV_32F (imgproc/resize.cpp, resizeGeneric)
__device__ __forceinline__ void linear_tap(int d, double scale, int n, int &s0, int &s1, float &w1) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= n - 1) { f = 0.f; s = n - 1; }
    s0 = s;
    s1 = s + 1 < n ? s + 1 : n - 1;
    w1 = f;
}

// bilinear inverse depth of destination pixel (row, col): cv::resize's two float passes (horizontal, then vertical)
template <typename T>
__device__ __forceinline__ float small_inv(const T *img, int row, int col, const DepthGeom &g) {
    int x0, x1, y0, y1;
    float ax, ay;
    linear_tap(col, g.scale_x, g.cols, x0, x1, ax);
    linear_tap(row, g.scale_y, g.rows, y0, y1, ay);
    const float a0 = 1.f - ax, b0 = 1.f - ay;
    const float t0 = inv_depth(img, y0, x0, g.cols, g) * a0 + inv_depth(img, y0, x1, g.cols, g) * ax;
    const float t1 = inv_depth(img, y1, x0, g.cols, g) * a0 + inv_depth(img, y1, x1, g.cols, g) * ax;
    return t0 * b0 + t1 * ay;
}

// rows 0..2 of A * Tbc into M[12] (threads 0..11), ordered sums without FMA
__device__ __forceinline__ void pose_times_tbc(const double *A, const DepthGeom &g, double *M) {
    const int tid = threadIdx.x;
    if (tid < 12) {
        const int i = tid / 4, j = tid % 4;
        double acc = A[4 * i + 0] * g.Tbc[0 + j];
        acc = acc + A[4 * i + 1] * g.Tbc[4 + j];
        acc = acc + A[4 * i + 2] * g.Tbc[8 + j];
        acc = acc + A[4 * i + 3] * g.Tbc[12 + j];
        M[tid] = acc;
    }
}

// appends the kept points of one round in thread order; returns the new base (every thread)
__device__ __forceinline__ int append_round(bool keep, float px, float py, float pz, float *out, int point_stride, int base,
                                            int *wave_tot) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wave_tot[w] = __popcll(m);
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int j = 0; j < kDepthThreads / 64; ++j) {
        const int t = wave_tot[j];
        woff += j < w ? t : 0;
        tot += t;
    }
    if (keep) {
        float *o = out + (size_t)(base + woff + __popcll(m & ((1ull << lane) - 1ull))) * point_stride;
        o[0] = px; o[1] = py; o[2] = pz;
    }
    __syncthreads();
    return base + tot;
}

// ProcessDepth's test of one down-scaled pixel (:113-117): is it an obstacle point, and at which depth.  A NaN passes the first
// comparison and fails the other two, as in the reference.
__device__ __forceinline__ bool obstacle_depth(double invd, const DepthGeom &g, double &d) {
    d = 1.0 / invd;                                                // :116
    return !(invd < 1e-2) && d > g.dmin && d < g.dmax;             // :113-115, :117
}

// BuildEdgeCloud's 8-bit depth (:183-191)
__device__ __forceinline__ unsigned char quantise(float inv, double range) {
    return (double)inv > 1e-2 ? (unsigned char)((double)(1 / inv) / range * (double)200.0f) : (unsigned char)255;
}

// UV2Camera (:133-136), then M * (xc, yc, d, 1) with M = rows 0..2 of pose * Tbc; pcl::PointXYZ is float32 (:122)
__device__ __forceinline__ void to_world(const double *M, int row, int col, double d, const DepthGeom &g, float &px, float &py,
                                         float &pz) {
    const double xc = ((double)col - g.cx) * d / g.fx, yc = ((double)row - g.cy) * d / g.fy;
    px = (float)(((M[0] * xc + M[1] * yc) + M[2] * d) + M[3]);
    py = (float)(((M[4] * xc + M[5] * yc) + M[6] * d) + M[7]);
    pz = (float)(((M[8] * xc + M[9] * yc) + M[10] * d) + M[11]);
}

// FrameKDMap::BuildEdgeCloud (FrameKDMap.cpp:176-214) on three LDS layers of the down-scaled W x H image: quantised depth (u8), its
// 3x3 erosion (u8), Sobel L1 magnitude (i16).  Each layer holds a range of IMAGE rows: image row r is the layer's row r - (its first
// row q0 / e0 / m0).  cv::Canny(., 0.1, 0.3) on 8-bit data = non-maximum suppression of the non-zero magnitudes (both thresholds floor
// to 0: every survivor is a strong edge).
struct EdgeLayers {
    unsigned char *quant, *ero;
    short *mag;
    int W, H, q0, e0, m0;
    __device__ __forceinline__ int epx(int r, int c) const {   // BORDER_REPLICATE
        return (int)ero[(min(max(r, 0), H - 1) - e0) * W + min(max(c, 0), W - 1)];
    }
    __device__ __forceinline__ int sobx(int r, int c) const {
        return (epx(r - 1, c + 1) + 2 * epx(r, c + 1) + epx(r + 1, c + 1)) - (epx(r - 1, c - 1) + 2 * epx(r, c - 1) + epx(r + 1, c - 1));
    }
    __device__ __forceinline__ int soby(int r, int c) const {
        return (epx(r + 1, c - 1) + 2 * epx(r + 1, c) + epx(r + 1, c + 1)) - (epx(r - 1, c - 1) + 2 * epx(r - 1, c) + epx(r - 1, c + 1));
    }
    __device__ __forceinline__ int mg(int r, int c) const { return (r < 0 || r >= H || c < 0 || c >= W) ? 0 : (int)mag[(r - m0) * W + c]; }
    // cv::erode 3x3 of image rows [lo, hi), taps outside the IMAGE ignored (every thread of the block)
    __device__ __forceinline__ void erode(int lo, int hi) const {
        const int n = (hi - lo) * W;
        for (int p = threadIdx.x; p < n; p += kDepthThreads) {
            const int r = lo + p / W, c = p % W;
            int m = 255;
            for (int dr = -1; dr <= 1; ++dr)
                for (int dc = -1; dc <= 1; ++dc) {
                    const int rr = r + dr, cc = c + dc;
                    if (rr >= 0 && rr < H && cc >= 0 && cc < W) m = min(m, (int)quant[(rr - q0) * W + cc]);
                }
            ero[(r - e0) * W + c] = (unsigned char)m;
        }
    }
    __device__ __forceinline__ void magnitude(int lo, int hi) const {
        const int n = (hi - lo) * W;
        for (int p = threadIdx.x; p < n; p += kDepthThreads) {
            const int r = lo + p / W, c = p % W;
            mag[(r - m0) * W + c] = (short)(abs(sobx(r, c)) + abs(soby(r, c)));
        }
    }
    __device__ __forceinline__ bool is_edge(int r, int c) const {   // Canny's non-maximum suppression
        const int m = mag[(r - m0) * W + c];   // (r, c) is a pixel of the image
        if (m <= 0) return false;
        const int xs = sobx(r, c), ys = soby(r, c);
        const int x = abs(xs), y = abs(ys) << 15, tg22x = x * 13573;
        if (y < tg22x) return m > mg(r, c - 1) && m >= mg(r, c + 1);
        if (y > tg22x + (x << 16)) return m > mg(r - 1, c) && m >= mg(r + 1, c);
        const int sg = ((xs ^ ys) < 0) ? -1 : 1;
        return m > mg(r - 1, c - sg) && m > mg(r + 1, c + sg);
    }
    __device__ __forceinline__ bool edge_depth(int r, int c, double range, const DepthGeom &g, double &d) const {
        d = (double)(float)ero[(r - e0) * W + c];   // :199
        d = d * range / 200.0;                      // :200
        return !(d > g.dmax || d < g.dmin);         // :201-203
    }
};

// The edge cloud of one scene per block, the whole down-scaled frame in LDS.
template <typename T>
__global__ __launch_bounds__(kDepthThreads) void depth_to_edge_kernel(const T *__restrict__ depth, long long scene_stride,
                                                                      DepthGeom g, const double *__restrict__ Twc,
                                                                      float *__restrict__ cloud, int point_stride,
                                                                      long long cloud_scene_stride,
                                                                      int *__restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char edge_smem[];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int W = g.W, H = g.H, npix = W * H;
    const EdgeLayers L{edge_smem, edge_smem + npix, reinterpret_cast<short *>(edge_smem + 2 * ((npix + 1) & ~1)), W, H, 0, 0, 0};
    const T *img = depth + (long long)s * scene_stride;
    float *out = cloud + (long long)s * cloud_scene_stride;
    __shared__ double M[12];
    __shared__ int wave_tot[kDepthThreads / 64];
    __shared__ int any_obstacle;
    if (tid == 0) any_obstacle = 0;
    pose_times_tbc(Twc + 16 * s, g, M);   // (mCurFrame.Twc * mParamTbc), :209
    __syncthreads();
    const double range = g.dmax - g.dmin;
    bool any = false;
    for (int p = tid; p < npix; p += kDepthThreads) {
        const float inv = small_inv(img, p / W, p % W, g);
        const double invd = (double)inv;
        if (!(invd < 1e-2)) {               // obstacle_depth's test written out: through the helper this kernel measured 0.6 % slower
            const double d = 1.0 / invd;
            any = any || (d > g.dmin && d < g.dmax);
        }
        L.quant[p] = quantise(inv, range);
    }
    if (any) any_obstacle = 1;
    __syncthreads();
    if (!any_obstacle) {                    // cloud->empty(): BuildEdgeCloud is not reached (:126-128)
        if (tid == 0) counts[s] = 0;
        return;
    }
    L.erode(0, H);
    __syncthreads();
    L.magnitude(0, H);
    __syncthreads();
    int base = 0;
    for (int p0 = 0; p0 < npix; p0 += kDepthThreads) {
        const int p = p0 + tid;
        bool keep = false;
        float px = 0.f, py = 0.f, pz = 0.f;
        if (p < npix) {
            const int r = p / W, c = p % W;
            double d;
            if (L.is_edge(r, c) && L.edge_depth(r, c, range, g, d)) {
                to_world(M, r, c, d, g, px, py, pz);
                keep = true;
            }
        }
        base = append_round(keep, px, py, pz, out, point_stride, base, wave_tot);
    }
    if (tid == 0) counts[s] = base;
}

template <typename T>
__global__ __launch_bounds__(kDepthThreads) void depth_to_cloud_kernel(const T *__restrict__ depth, long long scene_stride,
                                                                       DepthGeom g, const double *__restrict__ Twb,
                                                                       float *__restrict__ cloud, int point_stride,
                                                                       long long cloud_scene_stride,
                                                                       int *__restrict__ counts) {
    const int s = blockIdx.x, tid = threadIdx.x;
    const T *img = depth + (long long)s * scene_stride;
    float *out = cloud + (long long)s * cloud_scene_stride;
    __shared__ double M[12];                      // rows 0..2 of Twb * Tbc
    __shared__ int wave_tot[kDepthThreads / 64];
    pose_times_tbc(Twb + 16 * s, g, M);           // (mat4Twb * mParamTbc), evaluated once (:119-120)
    __syncthreads();
    const int npix = g.W * g.H;
    int base = 0;
    for (int p0 = 0; p0 < npix; p0 += kDepthThreads) {
        const int p = p0 + tid;
        bool keep = false;
        float px = 0.f, py = 0.f, pz = 0.f;
        if (p < npix) {
            const int row = p / g.W, col = p % g.W;
            double d;
            if (obstacle_depth((double)small_inv(img, row, col, g), g, d)) {
                to_world(M, row, col, d, g, px, py, pz);
                keep = true;
            }
        }
        base = append_round(keep, px, py, pz, out, point_stride, base, wave_tot);
    }
    if (tid == 0) counts[s] = base;
}

// ---- Both clouds of a down-scaled image of any size (amk_depth_to_clouds): grid (bands, scenes), one block per band of R whole
// down-scaled rows of one scene.  Whole rows keep band order = row-major pixel order.  A band decides its rows [r0, r1) from a halo
// of 3 rows on each side, all in LDS: quantised depth over [r0 - 3, r1 + 3), its erosion over [r0 - 2, r1 + 2), the Sobel magnitude
// over [r0 - 1, r1 + 1) -- W * (4 R + 14) bytes.  Every range is clipped to the IMAGE: a row of a neighbouring band is a real row
// (recomputed here), a row outside the image is what EdgeLayers makes of it for the one-block kernel too (an ignored erosion tap, a
// replicated Sobel tap, a zero magnitude).
// Two launches of the same body.  EMIT = false writes {kept obstacle pixels, edge points} of the band into band_counts[scene][band].
// EMIT = true sums the counts of the bands before its own (no block waits for another: what crosses bands crosses the launch
// boundary), learns from the scene's obstacle total whether the scene is empty, redoes the band and appends its points at its offsets.
template <typename T, bool EMIT>
__global__ __launch_bounds__(kDepthThreads) void depth_band_kernel(const T *__restrict__ depth, long long scene_stride, DepthGeom g,
                                                                   int R, const double *__restrict__ Twb,
                                                                   const double *__restrict__ Twc, float *__restrict__ cloud,
                                                                   long long cloud_scene_stride, int *__restrict__ counts,
                                                                   float *__restrict__ edge_cloud, long long edge_scene_stride,
                                                                   int *__restrict__ edge_counts, int point_stride,
                                                                   int2 *__restrict__ band_counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char band_smem[];
    const int b = blockIdx.x, nb = gridDim.x, s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int W = g.W, H = g.H;
    const int r0 = b * R, r1 = min(H, r0 + R);
    const EdgeLayers L{band_smem, band_smem + (size_t)(R + 6) * W, reinterpret_cast<short *>(band_smem + (size_t)(2 * R + 10) * W),
                       W, H, r0 - 3, r0 - 2, r0 - 1};
    const T *img = depth + (long long)s * scene_stride;
    __shared__ double Mb[12], Mc[12];   // rows 0..2 of Twb * Tbc (obstacle points) and of Twc * Tbc (edge points)
    __shared__ int wave_tot[kDepthThreads / 64];
    __shared__ int red[kDepthThreads / 64][4];
    int obs_base = 0, edge_base = 0;
    bool want_edges = true;
    if (EMIT) {
        const int2 *bc = band_counts + (size_t)s * nb;
        int acc[4] = {0, 0, 0, 0};   // obstacle / edge points of the bands before this one, of the whole scene
        for (int j = tid; j < nb; j += kDepthThreads) {
            const int2 v = bc[j];
            acc[0] += j < b ? v.x : 0;
            acc[1] += j < b ? v.y : 0;
            acc[2] += v.x;
            acc[3] += v.y;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off, 64);
            if (lane == 0) red[wv][k] = acc[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
        const bool empty = acc[2] == 0;   // cloud->empty(): BuildEdgeCloud is not reached (:126-128)
        if (b == 0 && tid == 0) {
            counts[s] = acc[2];
            edge_counts[s] = empty ? 0 : acc[3];
        }
        const int2 mine = bc[b];
        if (empty || (mine.x == 0 && mine.y == 0)) return;   // (block-uniform)
        obs_base = acc[0]; edge_base = acc[1];
        want_edges = mine.y > 0;
        pose_times_tbc(Twb + 16 * s, g, Mb);   // (mat4Twb * mParamTbc), :119-120
        pose_times_tbc(Twc + 16 * s, g, Mc);   // (mCurFrame.Twc * mParamTbc), :209
        __syncthreads();
    }
    const double range = g.dmax - g.dmin;
    // inverse depth once per pixel: the quantised layer over the band and its halo, and ProcessDepth's points of the band's own rows
    const int qlo = want_edges ? max(r0 - 3, 0) : r0, qhi = want_edges ? min(r1 + 3, H) : r1, nq = (qhi - qlo) * W;
    float *out = cloud + (long long)s * cloud_scene_stride;
    int n_obs = 0;
    for (int p0 = 0; p0 < nq; p0 += kDepthThreads) {
        const int p = p0 + tid;
        bool keep = false;
        float px = 0.f, py = 0.f, pz = 0.f;
        if (p < nq) {
            const int row = qlo + p / W, col = p % W;
            const float inv = small_inv(img, row, col, g);
            L.quant[(row - L.q0) * W + col] = quantise(inv, range);   // (first: the emit kernel stays within 64 VGPRs this way)
            double d;
            if (row >= r0 && row < r1 && obstacle_depth((double)inv, g, d)) {
                if (EMIT) to_world(Mb, row, col, d, g, px, py, pz);
                keep = true;
            }
        }
        if (EMIT) obs_base = append_round(keep, px, py, pz, out, point_stride, obs_base, wave_tot);
        else n_obs += keep ? 1 : 0;
    }
    __syncthreads();
    int n_edge = 0;
    if (want_edges) {
        L.erode(max(r0 - 2, 0), min(r1 + 2, H));
        __syncthreads();
        L.magnitude(max(r0 - 1, 0), min(r1 + 1, H));
        __syncthreads();
        float *eout = edge_cloud + (long long)s * edge_scene_stride;
        const int nown = (r1 - r0) * W;
        for (int p0 = 0; p0 < nown; p0 += kDepthThreads) {
            const int p = p0 + tid;
            bool keep = false;
            float px = 0.f, py = 0.f, pz = 0.f;
            if (p < nown) {
                const int r = r0 + p / W, c = p % W;
                double d;
                if (L.is_edge(r, c) && L.edge_depth(r, c, range, g, d)) {
                    if (EMIT) to_world(Mc, r, c, d, g, px, py, pz);
                    keep = true;
                }
            }
            if (EMIT) edge_base = append_round(keep, px, py, pz, eout, point_stride, edge_base, wave_tot);
            else n_edge += keep ? 1 : 0;
        }
    }
    if (!EMIT) {
        for (int off = 32; off > 0; off >>= 1) {
            n_obs += __shfl_xor(n_obs, off, 64);
            n_edge += __shfl_xor(n_edge, off, 64);
        }
        if (lane == 0) { red[wv][0] = n_obs; red[wv][1] = n_edge; }
        __syncthreads();
        if (tid == 0)
            band_counts[(size_t)s * nb + b] = make_int2((red[0][0] + red[1][0]) + (red[2][0] + red[3][0]),
                                                        (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]));
    }
}

// Band height.  All three layers of a band take W * (4 R + 14) bytes of LDS; within 64 KiB less the kernel's few static words that is
// R <= band_rows_max(W): 16+ up to W = 812, 4 at AMK_DEPTH_MAX_WIDTH.  The call takes min(16, that): 49 920 B at W = 640, so two
// workgroups still share a CU's LDS.
constexpr int kBandLdsBudget = 64 * 1024 - 512;
constexpr int kBandRowsAuto = 16;
int band_rows_max(int W) { return (kBandLdsBudget / W - 14) / 4; }
int g_forced_band_rows = 0;   // amk__depth_set_band_rows (tests): > 0 forces the tiled path with this band height

int make_geom(int rows, int cols, const amk_depth_params *p, DepthGeom &g) {
    if (!p || amk_depth_out_size(rows, cols, p->resize_scale, &g.W, &g.H) != AMK_OK) return AMK_ERR_INVALID_ARG;
    g.rows = rows; g.cols = cols;
    g.scale_x = 1.0 / ((double)g.W / (double)cols);  // cv::resize: inv_scale = dsize / ssize; scale = 1 / inv_scale
    g.scale_y = 1.0 / ((double)g.H / (double)rows);
    g.pixel2meter = p->pixel2meter; g.dmin = p->depth_min; g.dmax = p->depth_max;
    g.fx = p->fx / p->resize_scale; g.fy = p->fy / p->resize_scale;   // FrameKDMap.cpp:21-24
    g.cx = p->cx / p->resize_scale; g.cy = p->cy / p->resize_scale;
    std::memcpy(g.Tbc, p->Tbc, sizeof g.Tbc);
    return AMK_OK;
}

// A checked batch of depth images on the device: what every launch needs besides its pose and its cloud
struct Frames {
    const void *depth;
    int type, n_scenes, point_stride;
    long long scene_stride;
    DepthGeom g;
};

// The refusals the three device entry points share, in the order that decides which of two faults answers.  `pointers`: none of the
// call's pointers is null; `cloud_scene_stride`: the smallest of the call's cloud strides.
int check_frames(bool pointers, const void *d_depth, int depth_type, int rows, int cols, long long scene_stride, int n_scenes,
                 const amk_depth_params *params, int point_stride, long long cloud_scene_stride, Frames &f) {
    if (!pointers || !d_depth || n_scenes <= 0 || point_stride < 3) return AMK_ERR_INVALID_ARG;
    if (depth_type != AMK_DEPTH_U16 && depth_type != AMK_DEPTH_F32) return AMK_ERR_UNSUPPORTED;
    if (const int st = make_geom(rows, cols, params, f.g); st != AMK_OK) return st;
    if (scene_stride < (long long)rows * cols || cloud_scene_stride < (long long)f.g.W * f.g.H * point_stride)
        return AMK_ERR_INVALID_ARG;
    f.depth = d_depth; f.type = depth_type; f.n_scenes = n_scenes; f.point_stride = point_stride; f.scene_stride = scene_stride;
    return AMK_OK;
}

// The pixel-type dispatch: launch(img) with the batch's images as a pointer to their pixel type; then the launch's status
template <typename Launch>
int with_pixels(const Frames &f, Launch &&launch) {
    if (f.type == AMK_DEPTH_U16) launch((const unsigned short *)f.depth);
    else launch((const float *)f.depth);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

// One cloud of a call: its pose [S][16] (Twb for the obstacle cloud, Twc for the edge cloud), its points [S][scene_stride], its counts [S]
struct Cloud {
    const double *T;
    float *points;
    long long scene_stride;
    int *counts;
};

int launch_cloud(const Frames &f, const Cloud &c, hipStream_t stream) {
    return with_pixels(f, [&](auto *img) {
        hipLaunchKernelGGL(depth_to_cloud_kernel, dim3(f.n_scenes), dim3(kDepthThreads), 0, stream, img, f.scene_stride, f.g, c.T,
                           c.points, f.point_stride, c.scene_stride, c.counts);
    });
}

int launch_edge(const Frames &f, const Cloud &c, hipStream_t stream) {
    const size_t npix = (size_t)f.g.W * f.g.H, lds = 2 * ((npix + 1) & ~(size_t)1) + 2 * npix;  // quant, eroded (u8), magnitude (i16)
    return with_pixels(f, [&](auto *img) {
        hipLaunchKernelGGL(depth_to_edge_kernel, dim3(f.n_scenes), dim3(kDepthThreads), lds, stream, img, f.scene_stride, f.g, c.T,
                           c.points, f.point_stride, c.scene_stride, c.counts);
    });
}

// {obstacle, edge} count of every band of every scene, for the smallest band (one row): covers any band height
long long work_bytes_for(int H, int n_scenes) { return (long long)sizeof(int2) * H * n_scenes; }

// What the three host-memory variants refuse before anything is staged (`work_status`, the caller's answer about its workspace,
// stands behind the pixel type and before the device)
int refuse_host_call(bool pointers, int depth_type, int n_scenes, int work_status) {
    if (!pointers || n_scenes <= 0) return AMK_ERR_INVALID_ARG;
    if (depth_type != AMK_DEPTH_U16 && depth_type != AMK_DEPTH_F32) return AMK_ERR_UNSUPPORTED;
    if (work_status != AMK_OK) return work_status;
    return amk_device_count() <= 0 ? AMK_ERR_NO_DEVICE : AMK_OK;
}

size_t image_bytes(int depth_type, long long scene_stride, int n_scenes) { return (size_t)scene_stride * n_scenes * (depth_type == AMK_DEPTH_U16 ? 2 : 4); }

// amk_depth_to_cloud_host / amk_depth_to_edge_cloud_host: one cloud through `fn`, their device call, on the null stream
int one_cloud_on_host(decltype(&amk_depth_to_cloud) fn, const void *h_depth, int depth_type, int rows, int cols, long long scene_stride,
                      int n_scenes, const amk_depth_params *params, const double *h_T, float *h_cloud, int point_stride,
                      long long cloud_scene_stride, int *h_counts) {
    if (const int st = refuse_host_call(h_depth && h_T && h_cloud && h_counts, depth_type, n_scenes, AMK_OK); st != AMK_OK) return st;
    enum { IMAGES, POSES, COUNTS, POINTS };
    amk::HostStage stage;
    return stage.call({amk::to_device(h_depth, image_bytes(depth_type, scene_stride, n_scenes)), amk::to_device(h_T, sizeof(double) * 16 * n_scenes),
                       amk::to_host(h_counts, sizeof(int) * n_scenes), amk::to_host(h_cloud, sizeof(float) * (size_t)cloud_scene_stride * n_scenes)},
                      [&](const amk::HostStage::Dev *d) {
                          return fn(d[IMAGES], depth_type, rows, cols, scene_stride, n_scenes, params, d[POSES], d[POINTS], point_stride,
                                    cloud_scene_stride, d[COUNTS], nullptr);
                      },
                      hipDeviceSynchronize);
}

}  // namespace

extern "C" {

int amk_depth_out_size(int rows, int cols, double resize_scale, int *out_w, int *out_h) {
    if (rows <= 0 || cols <= 0 || !(resize_scale > 0) || !out_w || !out_h) return AMK_ERR_INVALID_ARG;
    *out_w = (int)((double)cols / resize_scale);   // mParamWidth = cols / mParamDepthScale (int <- double, :106)
    *out_h = (int)((double)rows / resize_scale);
    return (*out_w > 0 && *out_h > 0) ? AMK_OK : AMK_ERR_INVALID_ARG;
}

int amk_depth_to_cloud(const void *d_depth, int depth_type, int rows, int cols, long long scene_stride, int n_scenes,
                       const amk_depth_params *params, const double *d_Twb, float *d_cloud, int point_stride,
                       long long cloud_scene_stride, int *d_counts, void *stream) {
    Frames f;
    if (const int st = check_frames(d_Twb && d_cloud && d_counts, d_depth, depth_type, rows, cols, scene_stride, n_scenes, params,
                                    point_stride, cloud_scene_stride, f); st != AMK_OK)
        return st;
    if (amk_device_count() <= 0) return AMK_ERR_NO_DEVICE;
    return launch_cloud(f, {d_Twb, d_cloud, cloud_scene_stride, d_counts}, (hipStream_t)stream);
}

int amk_depth_to_edge_cloud(const void *d_depth, int depth_type, int rows, int cols, long long scene_stride, int n_scenes,
                            const amk_depth_params *params, const double *d_Twc, float *d_cloud, int point_stride,
                            long long cloud_scene_stride, int *d_counts, void *stream) {
    Frames f;
    if (const int st = check_frames(d_Twc && d_cloud && d_counts, d_depth, depth_type, rows, cols, scene_stride, n_scenes, params,
                                    point_stride, cloud_scene_stride, f); st != AMK_OK)
        return st;
    if ((long long)f.g.W * f.g.H > AMK_EDGE_MAX_PIXELS) return AMK_ERR_UNSUPPORTED;
    if (amk_device_count() <= 0) return AMK_ERR_NO_DEVICE;
    return launch_edge(f, {d_Twc, d_cloud, cloud_scene_stride, d_counts}, (hipStream_t)stream);
}

// tests only (exported, not in the header): force amk_depth_to_clouds onto the tiled kernels with bands of this many rows (clipped to
// what the LDS holds at the image's width) at any image size; 0 = automatic
int amk__depth_set_band_rows(int band_rows) {
    if (band_rows < 0) return AMK_ERR_INVALID_ARG;
    g_forced_band_rows = band_rows;
    return AMK_OK;
}

int amk_depth_clouds_work_bytes(int rows, int cols, double resize_scale, int n_scenes, long long *bytes_out) {
    int w = 0, h = 0;
    if (!bytes_out || n_scenes <= 0) return AMK_ERR_INVALID_ARG;
    if (const int st = amk_depth_out_size(rows, cols, resize_scale, &w, &h); st != AMK_OK) return st;
    *bytes_out = work_bytes_for(h, n_scenes);
    return AMK_OK;
}

int amk_depth_to_clouds(const void *d_depth, int depth_type, int rows, int cols, long long scene_stride, int n_scenes,
                        const amk_depth_params *params, const double *d_Twb, const double *d_Twc, float *d_cloud,
                        long long cloud_scene_stride, int *d_counts, float *d_edge, long long edge_scene_stride,
                        int *d_edge_counts, int point_stride, void *d_work, long long work_bytes, void *stream) {
    Frames f;
    if (const int st = check_frames(d_Twb && d_Twc && d_cloud && d_counts && d_edge && d_edge_counts && d_work, d_depth, depth_type, rows,
                                    cols, scene_stride, n_scenes, params, point_stride, std::min(cloud_scene_stride, edge_scene_stride), f);
        st != AMK_OK)
        return st;
    const DepthGeom &g = f.g;
    if (work_bytes < work_bytes_for(g.H, n_scenes)) return AMK_ERR_INVALID_ARG;
    if (g.W > AMK_DEPTH_MAX_WIDTH) return AMK_ERR_UNSUPPORTED;
    const int forced = g_forced_band_rows;
    const bool one_block = forced <= 0 && (long long)g.W * g.H <= AMK_EDGE_MAX_PIXELS;
    if (!one_block && n_scenes > 65535) return AMK_ERR_UNSUPPORTED;   // (scenes are the grid's second dimension)
    if (amk_device_count() <= 0) return AMK_ERR_NO_DEVICE;
    const hipStream_t hs = (hipStream_t)stream;
    if (one_block) {   // the one-block kernels, as the two calls launch them
        if (const int st = launch_cloud(f, {d_Twb, d_cloud, cloud_scene_stride, d_counts}, hs); st != AMK_OK) return st;
        return launch_edge(f, {d_Twc, d_edge, edge_scene_stride, d_edge_counts}, hs);
    }
    const int R = std::min(forced > 0 ? forced : kBandRowsAuto, band_rows_max(g.W));
    const dim3 grid((g.H + R - 1) / R, n_scenes);
    const size_t lds = (size_t)g.W * (4 * R + 14);
    return with_pixels(f, [&](auto *img) {
        using T = std::decay_t<decltype(*img)>;
        for (auto *kernel : {depth_band_kernel<T, false>, depth_band_kernel<T, true>})   // count, then emit
            hipLaunchKernelGGL(kernel, grid, dim3(kDepthThreads), lds, hs, img, scene_stride, g, R, d_Twb, d_Twc, d_cloud,
                               cloud_scene_stride, d_counts, d_edge, edge_scene_stride, d_edge_counts, point_stride, (int2 *)d_work);
    });
}

int amk_depth_to_cloud_host(const void *h_depth, int depth_type, int rows, int cols, long long scene_stride, int n_scenes,
                            const amk_depth_params *params, const double *h_Twb, float *h_cloud, int point_stride,
                            long long cloud_scene_stride, int *h_counts) {
    return one_cloud_on_host(amk_depth_to_cloud, h_depth, depth_type, rows, cols, scene_stride, n_scenes, params, h_Twb, h_cloud,
                             point_stride, cloud_scene_stride, h_counts);
}

int amk_depth_to_edge_cloud_host(const void *h_depth, int depth_type, int rows, int cols, long long scene_stride,
                                 int n_scenes, const amk_depth_params *params, const double *h_Twc, float *h_cloud,
                                 int point_stride, long long cloud_scene_stride, int *h_counts) {
    return one_cloud_on_host(amk_depth_to_edge_cloud, h_depth, depth_type, rows, cols, scene_stride, n_scenes, params, h_Twc, h_cloud,
                             point_stride, cloud_scene_stride, h_counts);
}

int amk_depth_to_clouds_host(const void *h_depth, int depth_type, int rows, int cols, long long scene_stride, int n_scenes,
                             const amk_depth_params *params, const double *h_Twb, const double *h_Twc, float *h_cloud,
                             long long cloud_scene_stride, int *h_counts, float *h_edge, long long edge_scene_stride,
                             int *h_edge_counts, int point_stride) {
    if (scene_stride <= 0 || cloud_scene_stride <= 0 || edge_scene_stride <= 0) return AMK_ERR_INVALID_ARG;
    long long work_bytes = 0;
    const int work_status = amk_depth_clouds_work_bytes(rows, cols, params ? params->resize_scale : 0.0, n_scenes, &work_bytes);
    if (const int st = refuse_host_call(h_depth && h_Twb && h_Twc && h_cloud && h_counts && h_edge && h_edge_counts, depth_type, n_scenes, work_status);
        st != AMK_OK)
        return st;
    enum { IMAGES, TWB, TWC, WORK, COUNTS, POINTS, EDGE_COUNTS, EDGE_POINTS };
    amk::HostStage stage;
    return stage.call({amk::to_device(h_depth, image_bytes(depth_type, scene_stride, n_scenes)), amk::to_device(h_Twb, sizeof(double) * 16 * n_scenes),
                       amk::to_device(h_Twc, sizeof(double) * 16 * n_scenes), amk::scratch((size_t)work_bytes),
                       amk::to_host(h_counts, sizeof(int) * n_scenes), amk::to_host(h_cloud, sizeof(float) * (size_t)cloud_scene_stride * n_scenes),
                       amk::to_host(h_edge_counts, sizeof(int) * n_scenes), amk::to_host(h_edge, sizeof(float) * (size_t)edge_scene_stride * n_scenes)},
                      [&](const amk::HostStage::Dev *d) {
                          return amk_depth_to_clouds(d[IMAGES], depth_type, rows, cols, scene_stride, n_scenes, params, d[TWB], d[TWC], d[POINTS],
                                                     cloud_scene_stride, d[COUNTS], d[EDGE_POINTS], edge_scene_stride, d[EDGE_COUNTS], point_stride,
                                                     d[WORK], work_bytes, nullptr);
                      },
                      hipDeviceSynchronize);
}

}  // extern "C"
