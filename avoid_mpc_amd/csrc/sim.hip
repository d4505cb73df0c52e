// The two ends of a closed-loop flight for gfx950: the depth sensor (amk_sim_render_depth) and the vehicle (amk_sim_vehicle_step).
// Between them lies what the library already runs on the device every period: amk_depth_to_clouds -> the map -> the step -> the
// command.  With these two a fleet flies from a world description to commands without a host round trip ("Closed loop
// on the device"; the numpy restatements are avoid_mpc_amd/flight.py render_depth_ordered / quantise_depth / vehicle_step_ordered).
//
// The world is that of flight.FlightWorld and synth.make_cloud: vertical cylinders (cx, cy, r) standing on the ground plane z = 0
// and cut at z_top.  The sensor is the pinhole camera of amk_depth_params at Twb * Tbc; a pixel's value is the PLANAR depth of its
// first hit (the hit's z in the camera frame: the ray's camera-frame z component is 1, so the ray parameter t is that depth), which
// is what UV2Camera back-projects (depth.hip to_world).
//
// Arithmetic contract (include/avoid_mpc_amd.h, "Closed-loop simulation"): fp64, no contraction, every sum left to right in index
// order.  Division and square root are IEEE-correct on both sides, so the numpy restatement matches operation for operation.
#include <cmath>
#include <cstring>

#include "amk_common.h"

namespace {

constexpr int kSimThreads = 256;
constexpr int kSimChunk = 64;     // cylinders staged in LDS per round (amk__sim_chunk: tests place their counts around it)
constexpr int kSimOutF64 = 2;     // amk__sim_render_t only: the fp64 ray parameter itself

struct SimCam {
    int rows, cols;
    double fx, fy, cx, cy;        // FULL resolution: the sensor renders what amk_depth_to_clouds then down-scales
    double pixel2meter, z_top, max_range;
    double Tbc[16];
};

struct SimPlant { double A[100], B[40], c[10]; };   // h_ABc, by value: 1200 bytes of kernel arguments

#pragma clang fp contract(off)

// The value of a pixel whose first hit lies at ray parameter t (0: no return), in the units depth.hip's inv_depth reads: it takes
// (float)((double)(float)pixel * pixel2meter) for both types, so the F32 pixel is the float32 depth divided by the float32
// pixel2meter in float32 (computed in double and rounded once: 53 >= 2 * 24 + 2 bits, the float32 quotient correctly rounded), and
// the U16 pixel is that value rounded to the nearest integer, ties to even, clamped to [0, 65535] -- tests/_flight.py
// _depth_frame's np.clip(np.round(float32 image / pixel2meter), 0, 65535).
__device__ __forceinline__ float pixel_f32(double t, double pixel2meter) {
    return (float)((double)(float)t / (double)(float)pixel2meter);
}
__device__ __forceinline__ void store_pixel(float *out, size_t i, double t, double p2m) { out[i] = pixel_f32(t, p2m); }
__device__ __forceinline__ void store_pixel(unsigned short *out, size_t i, double t, double p2m) {
    const float q = rintf(pixel_f32(t, p2m));                     // round-to-nearest-even is the mode every kernel here runs in
    out[i] = (unsigned short)(q < 65535.f ? (q > 0.f ? q : 0.f) : 65535.f);
}
__device__ __forceinline__ void store_pixel(double *out, size_t i, double t, double) { out[i] = t; }

// One thread per pixel, grid (tiles of kSimThreads pixels, scene).  The scene's cylinders pass through LDS in chunks of kSimChunk as
// (ox, oy, c) = (o_x - cx_k, o_y - cy_k, (ox * ox + oy * oy) - r * r): the three terms of the quadratic that do not depend on the
// pixel, computed once per block by the staging thread with the operations, and therefore the bits, the contract gives every pixel.
// Every lane of a wave reads the same LDS address in the cylinder loop (a broadcast, no bank conflict).
// BARRIERS: the trip count of the chunk loop comes from counts[scene] and max_cyl, which are the same for every thread of a block,
// and no thread leaves before the loop -- threads behind the image's last pixel stay, stage their share and only skip the store --
// so every wave of a block reaches every barrier.
// No block-level culling of cylinders: every pixel tests every cylinder of its scene, which is what makes the image a pure function
// of the contract.  The square root and the division run only for lanes with disc >= 0 (a wave none of whose lanes sees the
// cylinder skips both); a lane with disc < 0 can have no hit, so the branch changes no pixel.
template <typename Out>
__global__ __launch_bounds__(kSimThreads) void sim_render_kernel(const double *__restrict__ cyl, const int *__restrict__ counts,
                                                                  int max_cyl, SimCam g, const double *__restrict__ Twb,
                                                                  Out *__restrict__ depth) {
    __shared__ double M[12];                                     // rows 0..2 of Twc = Twb * Tbc
    __shared__ double s_ox[kSimChunk], s_oy[kSimChunk], s_c[kSimChunk];
    const int tid = threadIdx.x, scene = blockIdx.y;
    const long long npix = (long long)g.rows * g.cols, pix = (long long)blockIdx.x * kSimThreads + tid;
    if (tid < 12) {
        const double *A = Twb + (size_t)scene * 16;
        const int i = tid / 4, j = tid % 4;
        double acc = A[4 * i + 0] * g.Tbc[0 + j];
        acc = acc + A[4 * i + 1] * g.Tbc[4 + j];
        acc = acc + A[4 * i + 2] * g.Tbc[8 + j];
        acc = acc + A[4 * i + 3] * g.Tbc[12 + j];
        M[tid] = acc;
    }
    int n = counts ? counts[scene] : max_cyl;                    // block-uniform; clamped: a count outside [0, max_cyl] reads no
    n = n < 0 ? 0 : (n > max_cyl ? max_cyl : n);                 // memory that is not the scene's
    __syncthreads();
    const double ox0 = M[3], oy0 = M[7], oz0 = M[11];
    const long long p = pix < npix ? pix : npix - 1;             // (a thread past the image computes the last pixel and stores nothing)
    const int v = (int)(p / g.cols), u = (int)(p % g.cols);
    const double dc0 = ((double)u - g.cx) / g.fx, dc1 = ((double)v - g.cy) / g.fy;
    const double dx = (M[0] * dc0 + M[1] * dc1) + M[2] * 1.0;
    const double dy = (M[4] * dc0 + M[5] * dc1) + M[6] * 1.0;
    const double dz = (M[8] * dc0 + M[9] * dc1) + M[10] * 1.0;
    double best = INFINITY;
    if (dz < 0.0) {                                              // the ground plane
        const double t = -oz0 / dz;
        if (t > 0.0) best = t;
    }
    const double a = dx * dx + dy * dy;
    const double *sc = cyl + (size_t)scene * max_cyl * 3;
    for (int base = 0; base < n; base += kSimChunk) {
        const int m = n - base < kSimChunk ? n - base : kSimChunk;
        if (tid < m) {
            const double *q = sc + (size_t)(base + tid) * 3;
            const double ox = ox0 - q[0], oy = oy0 - q[1], r = q[2];
            s_ox[tid] = ox; s_oy[tid] = oy;
            s_c[tid] = (ox * ox + oy * oy) - r * r;
        }
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            const double b = s_ox[k] * dx + s_oy[k] * dy;
            const double disc = b * b - a * s_c[k];
            if (disc >= 0.0) {
                const double t = (-b - sqrt(disc)) / a;          // a == 0 (a vertical ray): NaN or -inf, no hit
                const double z = oz0 + t * dz;
                if (t > 0.0 && z >= 0.0 && z <= g.z_top && t < best) best = t;   // strict <: on equal t the earlier one keeps it
            }
        }
        __syncthreads();
    }
    if (pix < npix) store_pixel(depth + (size_t)scene * (size_t)npix, (size_t)pix, best <= g.max_range ? best : 0.0, g.pixel2meter);
}

// The vehicle over one control period: x+ = A x + B u + c with u = (cmd, yaw_dot = 0), one thread per scene.  The model comes by
// value and is copied from the kernel-argument segment into LDS once per block (300 scalar registers would not hold it); every lane
// then reads the same LDS address (a broadcast).  The state's indices are compile-time constants, so it stays in registers.
__global__ __launch_bounds__(kSimThreads) void sim_vehicle_kernel(SimPlant P, const double *__restrict__ cmd, double *__restrict__ x,
                                                                   double *__restrict__ Twb, double quantum, int n_scenes) {
    __shared__ double sP[150];
    if (threadIdx.x < 150) sP[threadIdx.x] = reinterpret_cast<const double *>(&P)[threadIdx.x];
    __syncthreads();                                             // (before any thread leaves)
    const int s = blockIdx.x * kSimThreads + threadIdx.x;
    if (s >= n_scenes) return;
    const double *pA = sP, *pB = sP + 100, *pc = sP + 140;
    double xs[10], xn[10];
    const double us[4] = {cmd[(size_t)s * 3 + 0], cmd[(size_t)s * 3 + 1], cmd[(size_t)s * 3 + 2], 0.0};
#pragma unroll
    for (int j = 0; j < 10; ++j) xs[j] = x[(size_t)s * 10 + j];
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        double ax = pA[10 * i] * xs[0];
#pragma unroll
        for (int j = 1; j < 10; ++j) ax = ax + pA[10 * i + j] * xs[j];
        double bu = pB[4 * i] * us[0];
#pragma unroll
        for (int j = 1; j < 4; ++j) bu = bu + pB[4 * i + j] * us[j];
        xn[i] = (ax + bu) + pc[i];
    }
#pragma unroll
    for (int j = 0; j < 10; ++j) x[(size_t)s * 10 + j] = xn[j];
    if (!Twb) return;
    double cs = 1.0, sn = 0.0;
    if (xn[3] != 0.0) { cs = cos(xn[3]); sn = sin(xn[3]); }      // yaw == 0: exactly the identity
    double pq[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) pq[j] = quantum > 0.0 ? rint(xn[j] * quantum) / quantum : xn[j];
    double *T = Twb + (size_t)s * 16;
    T[0] = cs;  T[1] = 0.0 - sn; T[2] = 0.0;  T[3] = pq[0];
    T[4] = sn;  T[5] = cs;       T[6] = 0.0;  T[7] = pq[1];
    T[8] = 0.0; T[9] = 0.0;      T[10] = 1.0; T[11] = pq[2];
    T[12] = 0.0; T[13] = 0.0;    T[14] = 0.0; T[15] = 1.0;
}

// What both render entries refuse, before anything is staged or launched
int render_args_status(bool pointers, int max_cyl, int n_scenes, double z_top, double max_range, const amk_depth_params *p, int rows,
                       int cols, int depth_type, SimCam &g) {
    if (!pointers || !p || rows < 1 || cols < 1 || max_cyl < 0 || n_scenes < 1 || !(z_top >= 0.0) || !(max_range >= 0.0) ||
        !(p->pixel2meter > 0.0))
        return AMK_ERR_INVALID_ARG;
    if (depth_type != AMK_DEPTH_U16 && depth_type != AMK_DEPTH_F32 && depth_type != kSimOutF64) return AMK_ERR_INVALID_ARG;
    const long long tiles = ((long long)rows * cols + kSimThreads - 1) / kSimThreads;
    if (tiles * n_scenes > 0x7fffffffll || n_scenes > 65535) return AMK_ERR_UNSUPPORTED;   // (scenes are the grid's second dimension)
    g.rows = rows; g.cols = cols;
    g.fx = p->fx; g.fy = p->fy; g.cx = p->cx; g.cy = p->cy;
    g.pixel2meter = p->pixel2meter; g.z_top = z_top; g.max_range = max_range;
    std::memcpy(g.Tbc, p->Tbc, sizeof g.Tbc);
    return AMK_OK;
}

size_t pixel_bytes(int depth_type) { return depth_type == AMK_DEPTH_U16 ? 2 : depth_type == AMK_DEPTH_F32 ? 4 : 8; }

int render(const double *d_cyl, const int *d_cyl_counts, int max_cyl, int n_scenes, double z_top, double max_range,
           const amk_depth_params *params, int rows, int cols, const double *d_Twb, void *d_depth, int depth_type, void *stream) {
    SimCam g;
    if (const int st = render_args_status((d_cyl || max_cyl == 0) && d_Twb && d_depth, max_cyl, n_scenes, z_top, max_range, params,
                                          rows, cols, depth_type, g); st != AMK_OK)
        return st;
    if (amk_device_count() <= 0) return AMK_ERR_NO_DEVICE;
    const dim3 grid((unsigned)(((long long)rows * cols + kSimThreads - 1) / kSimThreads), (unsigned)n_scenes);
    const hipStream_t hs = (hipStream_t)stream;
    if (depth_type == AMK_DEPTH_U16)
        hipLaunchKernelGGL(sim_render_kernel<unsigned short>, grid, dim3(kSimThreads), 0, hs, d_cyl, d_cyl_counts, max_cyl, g, d_Twb,
                           (unsigned short *)d_depth);
    else if (depth_type == AMK_DEPTH_F32)
        hipLaunchKernelGGL(sim_render_kernel<float>, grid, dim3(kSimThreads), 0, hs, d_cyl, d_cyl_counts, max_cyl, g, d_Twb, (float *)d_depth);
    else
        hipLaunchKernelGGL(sim_render_kernel<double>, grid, dim3(kSimThreads), 0, hs, d_cyl, d_cyl_counts, max_cyl, g, d_Twb, (double *)d_depth);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

int vehicle_args_status(bool pointers, int n_scenes, double pose_quantum) {
    return pointers && n_scenes >= 1 && pose_quantum >= 0.0 ? AMK_OK : AMK_ERR_INVALID_ARG;
}

}  // namespace

extern "C" {

int amk_sim_render_depth(const double *d_cyl, const int *d_cyl_counts, int max_cyl, int n_scenes, double z_top, double max_range,
                         const amk_depth_params *params, int rows, int cols, const double *d_Twb, void *d_depth, int depth_type,
                         void *stream) {
    if (depth_type != AMK_DEPTH_U16 && depth_type != AMK_DEPTH_F32) return AMK_ERR_INVALID_ARG;
    return render(d_cyl, d_cyl_counts, max_cyl, n_scenes, z_top, max_range, params, rows, cols, d_Twb, d_depth, depth_type, stream);
}

// tests only (exported, not in the header): the fp64 ray parameter t of every pixel (0: no return), double [S][rows][cols] -- what
// the two pixel types are made from, so that the contract's operation order is pinned bit for bit and not through a float32
int amk__sim_render_t(const double *d_cyl, const int *d_cyl_counts, int max_cyl, int n_scenes, double z_top, double max_range,
                      const amk_depth_params *params, int rows, int cols, const double *d_Twb, double *d_t, void *stream) {
    return render(d_cyl, d_cyl_counts, max_cyl, n_scenes, z_top, max_range, params, rows, cols, d_Twb, d_t, kSimOutF64, stream);
}

int amk__sim_chunk(void) { return kSimChunk; }   // tests only: cylinders per LDS round

int amk_sim_render_depth_host(const double *h_cyl, const int *h_cyl_counts, int max_cyl, int n_scenes, double z_top, double max_range,
                              const amk_depth_params *params, int rows, int cols, const double *h_Twb, void *h_depth, int depth_type) {
    if (depth_type != AMK_DEPTH_U16 && depth_type != AMK_DEPTH_F32) return AMK_ERR_INVALID_ARG;
    SimCam g;
    if (const int st = render_args_status((h_cyl || max_cyl == 0) && h_Twb && h_depth, max_cyl, n_scenes, z_top, max_range, params,
                                          rows, cols, depth_type, g); st != AMK_OK)
        return st;
    if (amk_device_count() <= 0) return AMK_ERR_NO_DEVICE;
    enum { CYL, COUNTS, POSES, IMAGES };
    amk::HostStage stage;
    return stage.call({amk::to_device(h_cyl, sizeof(double) * 3 * (size_t)max_cyl * n_scenes),
                       amk::if_given(amk::to_device(h_cyl_counts, sizeof(int) * n_scenes)),
                       amk::to_device(h_Twb, sizeof(double) * 16 * n_scenes),
                       amk::to_host(h_depth, pixel_bytes(depth_type) * (size_t)rows * cols * n_scenes)},
                      [&](const amk::HostStage::Dev *d) {
                          return amk_sim_render_depth(d[CYL], d[COUNTS], max_cyl, n_scenes, z_top, max_range, params, rows, cols, d[POSES],
                                                      d[IMAGES], depth_type, nullptr);
                      },
                      hipDeviceSynchronize);
}

int amk_sim_vehicle_step(const double *h_ABc, const double *d_cmd, double *d_x, double *d_Twb, int n_scenes, double pose_quantum,
                         void *stream) {
    if (const int st = vehicle_args_status(h_ABc && d_cmd && d_x, n_scenes, pose_quantum); st != AMK_OK) return st;
    if (amk_device_count() <= 0) return AMK_ERR_NO_DEVICE;
    SimPlant P;
    std::memcpy(&P, h_ABc, sizeof P);
    hipLaunchKernelGGL(sim_vehicle_kernel, dim3((n_scenes + kSimThreads - 1) / kSimThreads), dim3(kSimThreads), 0, (hipStream_t)stream, P,
                       d_cmd, d_x, d_Twb, pose_quantum, n_scenes);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

int amk_sim_vehicle_step_host(const double *h_ABc, const double *h_cmd, double *h_x, double *h_Twb, int n_scenes, double pose_quantum) {
    if (const int st = vehicle_args_status(h_ABc && h_cmd && h_x, n_scenes, pose_quantum); st != AMK_OK) return st;
    if (amk_device_count() <= 0) return AMK_ERR_NO_DEVICE;
    enum { CMD, STATE, POSES };
    amk::HostStage stage;
    return stage.call({amk::to_device(h_cmd, sizeof(double) * 3 * n_scenes), amk::both_ways(h_x, sizeof(double) * 10 * n_scenes),
                       amk::if_given(amk::to_host(h_Twb, sizeof(double) * 16 * n_scenes))},
                      [&](const amk::HostStage::Dev *d) {
                          return amk_sim_vehicle_step(h_ABc, d[CMD], d[STATE], d[POSES], n_scenes, pose_quantum, nullptr);
                      },
                      hipDeviceSynchronize);
}

}  // extern "C"
