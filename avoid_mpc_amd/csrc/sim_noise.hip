// What a real depth camera does to the sensor's perfect frames, for gfx950: amk_sim_depth_noise, one stream-ordered, out-of-place pass
// over a batch of depth images between amk_sim_render_world (or any recorded frames) and amk_pipeline_submit -- flying pixels and
// missing returns at depth discontinuities, plain dropouts, range-dependent axial noise, disparity quantisation and the sensor's own
// working range.  Every random number is a pure function of (seed, fleet-wide scene number, frame, pixel, draw): a counter-based
// integer hash, so a frame repeats on any machine and numpy restates the whole pass bit for bit (avoid_mpc_amd/flight.py noise_words /
// depth_noise_ordered).  Contract: include/avoid_mpc_amd.h, "Sensor noise on the simulated depth frames".
//
// SHAPE.  One thread per pixel, blocks of kNoiseThreads, grid (pixel tiles, scene).  The algorithmic traffic is one read and one write
// of the image; the four neighbours of the discontinuity stage are plain global loads -- left and right lie in the cache lines the
// wave loads anyway, up and down in lines a neighbouring wave or block loads, so they come from L1 / L2.  No LDS tile, hence no
// barrier: a thread behind the last pixel simply leaves.  The scene's key is block-uniform (scalar registers); per pixel the chain is
// at most three 64-bit mixes (w_1 always, w_0 with axial noise on, w_2 only for a flown pixel), two or three fp64 divisions with the
// disparity stage on, and one store.  Draws a pixel cannot need are skipped; every draw is addressed by its counter, so skipping one
// changes no other.  No atomics, no scratch, no inline assembly; 64-bit multiplies are plain C++.
#include <cmath>

#include "amk_common.h"

namespace {

constexpr int kNoiseThreads = 256;
constexpr long long kNoiseMaxBlocks = (1ll << 24) - 1;   // a grid dimension times the block's 256 threads stays below 2^32
constexpr double kNoiseScale = 2.6428997921303014e-05;   // 1 / sqrt((65536^2 - 1) / 3): the sum of four 16-bit fields to variance 1

struct NoiseArgs {
    int rows, cols;
    long long scene_stride;                                      // pixels between two scenes, in both images
    double pixel2meter, sigma0, sigma2, edge_jump, focal_baseline, quantum, z_min, z_max;
    unsigned long long t_drop, t_edge_drop, t_edge_fly;          // T(p): host arithmetic
    unsigned long long seed_mix, scene_id0, frame;               // mix(seed); the rest of the key is per scene
};

#pragma clang fp contract(off)

__host__ __device__ __forceinline__ unsigned long long noise_mix(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ unsigned long long scene_key(const NoiseArgs &g, unsigned scene) {
    return noise_mix(noise_mix(g.seed_mix ^ (g.scene_id0 + scene)) ^ g.frame);
}

// Pixels travel as their bits, so that a copied pixel is copied bit for bit whatever it holds (a NaN's payload included)
__device__ __forceinline__ float pixel_value(unsigned short b) { return (float)b; }
__device__ __forceinline__ float pixel_value(unsigned int b) { return __uint_as_float(b); }

// depth.hip's inv_depth read, widened: (float)((double)(float)pixel * pixel2meter)
template <typename Bits>
__device__ __forceinline__ double read_z(Bits b, double pixel2meter) {
    return (double)(float)((double)pixel_value(b) * pixel2meter);
}

// sim.hip's store_pixel rule (restated: that file is not edited)
__device__ __forceinline__ float pixel_f32(double t, double pixel2meter) { return (float)((double)(float)t / (double)(float)pixel2meter); }
__device__ __forceinline__ unsigned int stored_bits(unsigned int, double t, double p2m) { return __float_as_uint(pixel_f32(t, p2m)); }
__device__ __forceinline__ unsigned short stored_bits(unsigned short, double t, double p2m) {
    const float q = rintf(pixel_f32(t, p2m));
    return (unsigned short)(q < 65535.f ? (q > 0.f ? q : 0.f) : 65535.f);
}

// One neighbour of the discontinuity stage, in the contract's order: it makes the pixel a discontinuity pixel when it has no return or
// is a finite return further than edge_jump from z, and the first of the latter kind is the flying pixel's partner.
template <typename Bits>
__device__ __forceinline__ void tap(const Bits *__restrict__ src, long long j, bool inside, double z, const NoiseArgs &g, bool &disc,
                                    bool &have, double &zp) {
    if (!inside) return;
    const double zn = read_z(src[j], g.pixel2meter);
    const bool step = zn > 0.0 && zn < INFINITY && fabs(zn - z) > g.edge_jump;
    disc = disc || !(zn > 0.0) || step;
    if (step && !have) { have = true; zp = zn; }
}

template <typename Bits>
__global__ __launch_bounds__(kNoiseThreads) void sim_noise_kernel(const Bits *__restrict__ in, Bits *__restrict__ out, NoiseArgs g) {
    const long long npix = (long long)g.rows * g.cols, i = (long long)blockIdx.x * kNoiseThreads + threadIdx.x;
    if (i >= npix) return;                                       // (no barrier below)
    const Bits *src = in + (size_t)blockIdx.y * (size_t)g.scene_stride;
    Bits *dst = out + (size_t)blockIdx.y * (size_t)g.scene_stride;
    const Bits raw = src[i];
    double z = read_z(raw, g.pixel2meter);
    if (!(z > 0.0 && z < INFINITY)) { dst[i] = raw; return; }    // 1. not a finite return: no stage sees it
    const unsigned long long k = scene_key(g, blockIdx.y), ctr = 4ull * (unsigned long long)i;
    const unsigned long long w1 = noise_mix(k ^ (ctr + 1));
    bool zero = false, flown = false;
    if (g.edge_jump > 0.0) {                                     // 2. discontinuity (npix < 2^32: the launch limit)
        const unsigned v = (unsigned)i / (unsigned)g.cols, u = (unsigned)i - v * (unsigned)g.cols;
        bool disc = false, have = false;
        double zp = 0.0;
        tap(src, i - 1, u > 0, z, g, disc, have, zp);
        tap(src, i + 1, u + 1 < (unsigned)g.cols, z, g, disc, have, zp);
        tap(src, i - g.cols, v > 0, z, g, disc, have, zp);
        tap(src, i + g.cols, v + 1 < (unsigned)g.rows, z, g, disc, have, zp);
        if (disc) {
            const unsigned long long r = w1 & 0xffffffffull;
            if (r < g.t_edge_drop) zero = true;
            else if (r < g.t_edge_drop + g.t_edge_fly) {
                if (!have) zero = true;
                else {
                    const double f = (double)(noise_mix(k ^ (ctr + 2)) >> 11) * 0x1p-53;
                    z = z + f * (zp - z);
                    flown = true;
                }
            }
        }
    }
    if ((w1 >> 32) < g.t_drop) zero = true;                      // 3. dropout
    const bool axial = g.sigma0 > 0.0 || g.sigma2 > 0.0, disparity = g.quantum > 0.0;
    if (axial && !zero) {                                        // 4. axial noise
        const unsigned long long w0 = noise_mix(k ^ ctr);
        const long long sum = (long long)((w0 & 0xffff) + ((w0 >> 16) & 0xffff) + ((w0 >> 32) & 0xffff) + (w0 >> 48));
        const double gv = (double)(sum - 131070) * kNoiseScale;
        z = z + (g.sigma0 + (g.sigma2 * z) * z) * gv;
    }
    if (disparity && !zero) {                                    // 5. disparity
        const double d = g.focal_baseline / z, dq = rint(d / g.quantum) * g.quantum;
        if (!(dq > 0.0)) zero = true;
        else z = g.focal_baseline / dq;
    }
    if (!(z > 0.0) || z < g.z_min || (g.z_max > 0.0 && z > g.z_max)) zero = true;   // 6. range
    // 7. store: 0, the input's own bits where no enabled stage touched the pixel, else the store rule
    dst[i] = zero ? (Bits)0 : (flown || axial || disparity) ? stored_bits(raw, z, g.pixel2meter) : raw;
}

// amk__sim_noise_words: w_0, w_1, w_2 of every pixel, [S][rows cols][3]
__global__ __launch_bounds__(kNoiseThreads) void sim_noise_words_kernel(unsigned long long *__restrict__ words, NoiseArgs g) {
    const long long npix = (long long)g.rows * g.cols, i = (long long)blockIdx.x * kNoiseThreads + threadIdx.x;
    if (i >= npix) return;
    const unsigned long long k = scene_key(g, blockIdx.y), ctr = 4ull * (unsigned long long)i;
    unsigned long long *w = words + ((size_t)blockIdx.y * (size_t)npix + (size_t)i) * 3;
    w[0] = noise_mix(k ^ ctr); w[1] = noise_mix(k ^ (ctr + 1)); w[2] = noise_mix(k ^ (ctr + 2));
}

bool probability(double p) { return p >= 0.0 && p <= 1.0; }       // (a NaN fails both)
unsigned long long threshold(double p) { return p >= 1.0 ? 1ull << 32 : (unsigned long long)(p * 4294967296.0); }

int grid_status(int rows, int cols, int n_scenes) {
    const long long tiles = ((long long)rows * cols + kNoiseThreads - 1) / kNoiseThreads;
    return tiles > kNoiseMaxBlocks || n_scenes > 65535 ? AMK_ERR_UNSUPPORTED : AMK_OK;   // (scenes are the grid's second dimension)
}

// What both entries refuse, before anything is staged or launched; `bytes`: what either image spans in memory
int noise_args_status(const void *in, void *out, int depth_type, int rows, int cols, long long scene_stride, int n_scenes,
                      double pixel2meter, const amk_sim_noise_params *p, NoiseArgs &g, size_t &bytes) {
    if (!in || !out || !p || rows < 1 || cols < 1 || n_scenes < 1 || scene_stride < (long long)rows * cols || !(pixel2meter > 0.0))
        return AMK_ERR_INVALID_ARG;
    if (depth_type != AMK_DEPTH_U16 && depth_type != AMK_DEPTH_F32) return AMK_ERR_INVALID_ARG;
    if (!probability(p->p_drop) || !probability(p->p_edge_drop) || !probability(p->p_edge_fly) || p->p_edge_drop + p->p_edge_fly > 1.0)
        return AMK_ERR_INVALID_ARG;
    if (!(p->sigma0 >= 0.0) || !(p->sigma2 >= 0.0) || !(p->edge_jump >= 0.0) || !(p->disparity_quantum >= 0.0) || !(p->z_min >= 0.0) ||
        !(p->z_max >= 0.0) || (p->disparity_quantum > 0.0 && !(p->focal_baseline > 0.0)))
        return AMK_ERR_INVALID_ARG;
    const unsigned __int128 pixel = depth_type == AMK_DEPTH_U16 ? 2 : 4;
    const unsigned __int128 span = ((unsigned __int128)(n_scenes - 1) * (unsigned __int128)scene_stride + (unsigned __int128)rows * cols) * pixel;
    const unsigned __int128 a = (uintptr_t)in, b = (uintptr_t)out;
    if (a < b + span && b < a + span) return AMK_ERR_INVALID_ARG;   // the same image or overlapping ranges
    if (const int st = grid_status(rows, cols, n_scenes); st != AMK_OK) return st;
    if (span > ((unsigned __int128)1 << 62)) return AMK_ERR_UNSUPPORTED;
    bytes = (size_t)span;
    g.rows = rows; g.cols = cols; g.scene_stride = scene_stride;
    g.pixel2meter = pixel2meter; g.sigma0 = p->sigma0; g.sigma2 = p->sigma2; g.edge_jump = p->edge_jump;
    g.focal_baseline = p->focal_baseline; g.quantum = p->disparity_quantum; g.z_min = p->z_min; g.z_max = p->z_max;
    g.t_drop = threshold(p->p_drop); g.t_edge_drop = threshold(p->p_edge_drop); g.t_edge_fly = threshold(p->p_edge_fly);
    g.seed_mix = noise_mix(p->seed);
    return AMK_OK;
}

}  // namespace

extern "C" {

int amk_sim_depth_noise(const void *d_in, void *d_out, int depth_type, int rows, int cols, long long scene_stride, int n_scenes,
                        double pixel2meter, const amk_sim_noise_params *prm, long long scene_id0, unsigned long long frame, void *stream) {
    NoiseArgs g;
    size_t bytes;
    if (const int st = noise_args_status(d_in, d_out, depth_type, rows, cols, scene_stride, n_scenes, pixel2meter, prm, g, bytes); st != AMK_OK)
        return st;
    if (amk_device_count() <= 0) return AMK_ERR_NO_DEVICE;
    g.scene_id0 = (unsigned long long)scene_id0; g.frame = frame;
    const dim3 grid((unsigned)(((long long)rows * cols + kNoiseThreads - 1) / kNoiseThreads), (unsigned)n_scenes);
    if (depth_type == AMK_DEPTH_U16)
        hipLaunchKernelGGL(sim_noise_kernel<unsigned short>, grid, dim3(kNoiseThreads), 0, (hipStream_t)stream, (const unsigned short *)d_in,
                           (unsigned short *)d_out, g);
    else
        hipLaunchKernelGGL(sim_noise_kernel<unsigned int>, grid, dim3(kNoiseThreads), 0, (hipStream_t)stream, (const unsigned int *)d_in,
                           (unsigned int *)d_out, g);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

int amk_sim_depth_noise_host(const void *h_in, void *h_out, int depth_type, int rows, int cols, long long scene_stride, int n_scenes,
                             double pixel2meter, const amk_sim_noise_params *prm, long long scene_id0, unsigned long long frame) {
    NoiseArgs g;
    size_t bytes;
    if (const int st = noise_args_status(h_in, h_out, depth_type, rows, cols, scene_stride, n_scenes, pixel2meter, prm, g, bytes); st != AMK_OK)
        return st;
    if (amk_device_count() <= 0) return AMK_ERR_NO_DEVICE;
    enum { IN, OUT };
    const bool padded = scene_stride > (long long)rows * cols;   // the output's padding goes in too, so that it comes back as it was
    amk::HostStage stage;
    return stage.call({amk::to_device(h_in, bytes), padded ? amk::both_ways(h_out, bytes) : amk::to_host(h_out, bytes)},
                      [&](const amk::HostStage::Dev *d) {
                          return amk_sim_depth_noise(d[IN], d[OUT], depth_type, rows, cols, scene_stride, n_scenes, pixel2meter, prm,
                                                     scene_id0, frame, nullptr);
                      },
                      hipDeviceSynchronize);
}

// tests only (exported, not in the header): the stream itself, unsigned long long [S][rows][cols][3] = w_0, w_1, w_2 of every pixel
int amk__sim_noise_words(unsigned long long *d_words, int rows, int cols, int n_scenes, unsigned long long seed, long long scene_id0,
                         unsigned long long frame, void *stream) {
    if (!d_words || rows < 1 || cols < 1 || n_scenes < 1) return AMK_ERR_INVALID_ARG;
    if (const int st = grid_status(rows, cols, n_scenes); st != AMK_OK) return st;
    if (amk_device_count() <= 0) return AMK_ERR_NO_DEVICE;
    NoiseArgs g{};
    g.rows = rows; g.cols = cols;
    g.seed_mix = noise_mix(seed); g.scene_id0 = (unsigned long long)scene_id0; g.frame = frame;
    const dim3 grid((unsigned)(((long long)rows * cols + kNoiseThreads - 1) / kNoiseThreads), (unsigned)n_scenes);
    hipLaunchKernelGGL(sim_noise_words_kernel, grid, dim3(kNoiseThreads), 0, (hipStream_t)stream, d_words, g);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

}  // extern "C"
