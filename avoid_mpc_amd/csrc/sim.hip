// The two ends of a closed-loop flight for gfx950: the depth sensor (amk_sim_render_depth; amk_sim_render_world adds boxes) and the
// vehicle (amk_sim_vehicle_step; amk_sim_vehicle_step_att tilts it into its thrust).
// Between them lies what the library already runs on the device every period: amk_depth_to_clouds -> the map -> the step -> the
// command.  With these two a fleet flies from a world description to commands without a host round trip ("Closed loop
// on the device"; the numpy restatements are avoid_mpc_amd/flight.py render_depth_ordered / quantise_depth / vehicle_step_ordered and
// render_world_ordered / vehicle_attitude_ordered).
//
// The world is that of flight.FlightWorld and synth.make_cloud: vertical cylinders (cx, cy, r) standing on the ground plane z = 0
// and cut at z_top, and for amk_sim_render_world the boxes of flight.WallWorld: yawed, each with its own [z0, z1].  The sensor is
// the pinhole camera of amk_depth_params at Twb * Tbc; a pixel's value is the PLANAR depth of its first hit (the hit's z in the
// camera frame: the ray's camera-frame z component is 1, so the ray parameter t is that depth), which is what UV2Camera
// back-projects (depth.hip to_world).
//
// Arithmetic contract (include/avoid_mpc_amd.h, "Closed-loop simulation"): fp64, no contraction, every sum left to right in index
// order.  Division and square root are IEEE-correct on both sides, so the numpy restatement matches operation for operation.
#include <cmath>
#include <cstring>

#include "amk_common.h"

namespace {

constexpr int kSimThreads = 256;
constexpr int kSimChunk = 64;     // cylinders staged in LDS per round (amk__sim_chunk: tests place their counts around it)
constexpr int kSimBoxChunk = 64;  // boxes staged in LDS per round (amk__sim_world_chunk)
constexpr int kSimOutF64 = 2;     // amk__sim_render_t / amk__sim_render_world_t only: the fp64 ray parameter itself

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

// One slab of a box: the ray meets it for t in [near, far].  lo_o = lo - o and hi_o = hi - o come from the staging thread, inv = 1 / d.
// d == 0 (a ray parallel to the slab): no bound when the origin lies in it (inside: lo <= o <= hi), else (+inf, -inf), which
// fails near <= far like a NaN does.
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
//
// kBoxes (sim_world_kernel, amk_sim_render_world with max_box > 0): behind the cylinder loop a second chunk loop over the scene's boxes.
// A box passes through LDS as its yaw (c, s), the six numerators lo - o and hi - o of its slabs in the box's own frame --
// (-hx - olx, hx - olx), (-hy - oly, hy - oly), (z0 - o_z, z1 - o_z) with olx = c ox + s oy, oly = c oy - s ox -- and three bits "the
// camera lies within this slab", all computed once per block by the staging thread with the contract's own operations: the bits every
// pixel would have computed.  Every lane reads the same LDS address in the box loop too.  Per pixel and box that leaves dlx, dly, two
// IEEE reciprocals (1 / d_z is per pixel), six products and the comparisons.  No early reject in front of the reciprocals and no
// block-level culling: every pixel tests every box, unconditionally, so the box loop has no divergent branch.  Its trip count comes
// from box_counts[scene] and max_box, the same for a whole block (BARRIERS).  Without kBoxes none of this is instantiated: the two
// kernels share every line in front of it, so zero boxes and amk_sim_render_depth give the same bits by construction.
template <typename Out, bool kBoxes>
__device__ __forceinline__ void sim_render_body(const double *__restrict__ cyl, const int *__restrict__ counts, int max_cyl,
                                                const double *__restrict__ box, const int *__restrict__ box_counts, int max_box,
                                                const SimCam &g, const double *__restrict__ Twb, Out *__restrict__ depth) {
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
    if constexpr (kBoxes) {
        __shared__ double b_c[kSimBoxChunk], b_s[kSimBoxChunk], b_x0[kSimBoxChunk], b_x1[kSimBoxChunk], b_y0[kSimBoxChunk],
            b_y1[kSimBoxChunk], b_z0[kSimBoxChunk], b_z1[kSimBoxChunk];
        __shared__ int b_in[kSimBoxChunk];
        int nb = box_counts ? box_counts[scene] : max_box;       // block-uniform, clamped like n
        nb = nb < 0 ? 0 : (nb > max_box ? max_box : nb);
        const double inv_z = 1.0 / dz;
        const double *sb = box + (size_t)scene * max_box * 8;
        for (int base = 0; base < nb; base += kSimBoxChunk) {
            const int m = nb - base < kSimBoxChunk ? nb - base : kSimBoxChunk;
            if (tid < m) {
                const double *q = sb + (size_t)(base + tid) * 8;
                const double ox = ox0 - q[0], oy = oy0 - q[1], hx = q[2], hy = q[3], c = q[4], s = q[5], z0 = q[6], z1 = q[7];
                const double olx = c * ox + s * oy, oly = c * oy - s * ox;
                b_c[tid] = c; b_s[tid] = s;
                b_x0[tid] = -hx - olx; b_x1[tid] = hx - olx;
                b_y0[tid] = -hy - oly; b_y1[tid] = hy - oly;
                b_z0[tid] = z0 - oz0;  b_z1[tid] = z1 - oz0;
                b_in[tid] = (-hx <= olx && olx <= hx ? 1 : 0) | (-hy <= oly && oly <= hy ? 2 : 0) | (z0 <= oz0 && oz0 <= z1 ? 4 : 0);
            }
            __syncthreads();
            for (int k = 0; k < m; ++k) {
                const double c = b_c[k], s = b_s[k];
                const int in = b_in[k];
                const double dlx = c * dx + s * dy, dly = c * dy - s * dx;
                double n0, f0, n1, f1, n2, f2;
                box_slab(b_x0[k], b_x1[k], dlx, 1.0 / dlx, in & 1, n0, f0);
                box_slab(b_y0[k], b_y1[k], dly, 1.0 / dly, in & 2, n1, f1);
                box_slab(b_z0[k], b_z1[k], dz, inv_z, in & 4, n2, f2);
                double tn = n0 > n1 ? n0 : n1, tf = f0 < f1 ? f0 : f1;
                tn = n2 > tn ? n2 : tn;
                tf = f2 < tf ? f2 : tf;
                // every slab crossed forwards (a NaN fails here, whichever slab it is in), entered ahead of the camera, strict < as above
                if (n0 <= f0 && n1 <= f1 && n2 <= f2 && tn > 0.0 && tn <= tf && tn < best) best = tn;
            }
            __syncthreads();
        }
    }
    if (pix < npix) store_pixel(depth + (size_t)scene * (size_t)npix, (size_t)pix, best <= g.max_range ? best : 0.0, g.pixel2meter);
}

template <typename Out>
__global__ __launch_bounds__(kSimThreads) void sim_render_kernel(const double *__restrict__ cyl, const int *__restrict__ counts,
                                                                  int max_cyl, SimCam g, const double *__restrict__ Twb,
                                                                  Out *__restrict__ depth) {
    sim_render_body<Out, false>(cyl, counts, max_cyl, nullptr, nullptr, 0, g, Twb, depth);
}

template <typename Out>
__global__ __launch_bounds__(kSimThreads) void sim_world_kernel(const double *__restrict__ cyl, const int *__restrict__ counts, int max_cyl,
                                                                 const double *__restrict__ box, const int *__restrict__ box_counts,
                                                                 int max_box, SimCam g, const double *__restrict__ Twb,
                                                                 Out *__restrict__ depth) {
    sim_render_body<Out, true>(cyl, counts, max_cyl, box, box_counts, max_box, g, Twb, depth);
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

// AMK_SIM_ATT_ACCEL, behind sim_vehicle_kernel on the same stream: that kernel has advanced x and written Twb = [Rz(yaw) | p'];
// this one reads the NEW acceleration and the (cs, sn) that kernel wrote -- exactly the yaw mode's, 1 and 0 at yaw == 0 -- and
// overwrites the rotation with acc2rotmat's [xb yb zb].  Where the thrust or its projection vanishes (or is NaN) Rz(yaw) stays.
__global__ __launch_bounds__(kSimThreads) void sim_attitude_kernel(const double *__restrict__ x, double *__restrict__ Twb, double gz,
                                                                    int n_scenes) {
    const int s = blockIdx.x * kSimThreads + threadIdx.x;
    if (s >= n_scenes) return;
    double *T = Twb + (size_t)s * 16;
    const double cs = T[0], sn = T[4];
    const double t0 = x[(size_t)s * 10 + 7], t1 = x[(size_t)s * 10 + 8], t2 = x[(size_t)s * 10 + 9] + gz;
    const double n = sqrt((t0 * t0 + t1 * t1) + t2 * t2);
    const double zb0 = t0 / n, zb1 = t1 / n, zb2 = t2 / n;
    const double y0 = 0.0 - zb2 * sn, y1 = zb2 * cs, y2 = zb0 * sn - zb1 * cs;
    const double m = sqrt((y0 * y0 + y1 * y1) + y2 * y2);
    if (!(n > 0.0 && m > 0.0)) return;
    const double yb0 = y0 / m, yb1 = y1 / m, yb2 = y2 / m;
    T[0] = yb1 * zb2 - yb2 * zb1; T[1] = yb0; T[2] = zb0;
    T[4] = yb2 * zb0 - yb0 * zb2; T[5] = yb1; T[6] = zb1;
    T[8] = yb0 * zb1 - yb1 * zb0; T[9] = yb2; T[10] = zb2;
}

// What the render entries refuse, before anything is staged or launched
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

// amk_sim_render_world and its fp64 twin.  max_box == 0 is amk_sim_render_depth's own launch: the same kernel at the same cost.
int render_world(const double *d_cyl, const int *d_cyl_counts, int max_cyl, const double *d_box, const int *d_box_counts, int max_box,
                 int n_scenes, double z_top, double max_range, const amk_depth_params *params, int rows, int cols, const double *d_Twb,
                 void *d_depth, int depth_type, void *stream) {
    if (max_box < 0 || (!d_box && max_box > 0)) return AMK_ERR_INVALID_ARG;
    if (max_box == 0)
        return render(d_cyl, d_cyl_counts, max_cyl, n_scenes, z_top, max_range, params, rows, cols, d_Twb, d_depth, depth_type, stream);
    SimCam g;
    if (const int st = render_args_status((d_cyl || max_cyl == 0) && d_Twb && d_depth, max_cyl, n_scenes, z_top, max_range, params,
                                          rows, cols, depth_type, g); st != AMK_OK)
        return st;
    if (amk_device_count() <= 0) return AMK_ERR_NO_DEVICE;
    const dim3 grid((unsigned)(((long long)rows * cols + kSimThreads - 1) / kSimThreads), (unsigned)n_scenes);
    const hipStream_t hs = (hipStream_t)stream;
    if (depth_type == AMK_DEPTH_U16)
        hipLaunchKernelGGL(sim_world_kernel<unsigned short>, grid, dim3(kSimThreads), 0, hs, d_cyl, d_cyl_counts, max_cyl, d_box,
                           d_box_counts, max_box, g, d_Twb, (unsigned short *)d_depth);
    else if (depth_type == AMK_DEPTH_F32)
        hipLaunchKernelGGL(sim_world_kernel<float>, grid, dim3(kSimThreads), 0, hs, d_cyl, d_cyl_counts, max_cyl, d_box, d_box_counts,
                           max_box, g, d_Twb, (float *)d_depth);
    else
        hipLaunchKernelGGL(sim_world_kernel<double>, grid, dim3(kSimThreads), 0, hs, d_cyl, d_cyl_counts, max_cyl, d_box, d_box_counts,
                           max_box, g, d_Twb, (double *)d_depth);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

int vehicle_args_status(bool pointers, int n_scenes, double pose_quantum) {
    return pointers && n_scenes >= 1 && pose_quantum >= 0.0 ? AMK_OK : AMK_ERR_INVALID_ARG;
}

int attitude_args_status(int attitude, double gz) {
    return (attitude == AMK_SIM_ATT_YAW || attitude == AMK_SIM_ATT_ACCEL) && gz >= 0.0 ? AMK_OK : AMK_ERR_INVALID_ARG;
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

int amk_sim_render_world(const double *d_cyl, const int *d_cyl_counts, int max_cyl, const double *d_box, const int *d_box_counts,
                         int max_box, int n_scenes, double z_top, double max_range, const amk_depth_params *params, int rows, int cols,
                         const double *d_Twb, void *d_depth, int depth_type, void *stream) {
    if (depth_type != AMK_DEPTH_U16 && depth_type != AMK_DEPTH_F32) return AMK_ERR_INVALID_ARG;
    return render_world(d_cyl, d_cyl_counts, max_cyl, d_box, d_box_counts, max_box, n_scenes, z_top, max_range, params, rows, cols, d_Twb,
                        d_depth, depth_type, stream);
}

// tests only (exported, not in the header): amk__sim_render_t for the world entry
int amk__sim_render_world_t(const double *d_cyl, const int *d_cyl_counts, int max_cyl, const double *d_box, const int *d_box_counts,
                            int max_box, int n_scenes, double z_top, double max_range, const amk_depth_params *params, int rows,
                            int cols, const double *d_Twb, double *d_t, void *stream) {
    return render_world(d_cyl, d_cyl_counts, max_cyl, d_box, d_box_counts, max_box, n_scenes, z_top, max_range, params, rows, cols, d_Twb,
                        d_t, kSimOutF64, stream);
}

int amk__sim_world_chunk(void) { return kSimBoxChunk; }   // tests only: boxes per LDS round

int amk_sim_render_world_host(const double *h_cyl, const int *h_cyl_counts, int max_cyl, const double *h_box, const int *h_box_counts,
                              int max_box, int n_scenes, double z_top, double max_range, const amk_depth_params *params, int rows,
                              int cols, const double *h_Twb, void *h_depth, int depth_type) {
    if (depth_type != AMK_DEPTH_U16 && depth_type != AMK_DEPTH_F32) return AMK_ERR_INVALID_ARG;
    if (max_box < 0 || (!h_box && max_box > 0)) return AMK_ERR_INVALID_ARG;
    SimCam g;
    if (const int st = render_args_status((h_cyl || max_cyl == 0) && h_Twb && h_depth, max_cyl, n_scenes, z_top, max_range, params,
                                          rows, cols, depth_type, g); st != AMK_OK)
        return st;
    if (amk_device_count() <= 0) return AMK_ERR_NO_DEVICE;
    enum { CYL, COUNTS, BOX, BOX_COUNTS, POSES, IMAGES };
    amk::HostStage stage;
    return stage.call({amk::to_device(h_cyl, sizeof(double) * 3 * (size_t)max_cyl * n_scenes),
                       amk::if_given(amk::to_device(h_cyl_counts, sizeof(int) * n_scenes)),
                       amk::to_device(h_box, sizeof(double) * 8 * (size_t)max_box * n_scenes),
                       amk::if_given(amk::to_device(h_box_counts, sizeof(int) * n_scenes)),
                       amk::to_device(h_Twb, sizeof(double) * 16 * n_scenes),
                       amk::to_host(h_depth, pixel_bytes(depth_type) * (size_t)rows * cols * n_scenes)},
                      [&](const amk::HostStage::Dev *d) {
                          return amk_sim_render_world(d[CYL], d[COUNTS], max_cyl, d[BOX], d[BOX_COUNTS], max_box, n_scenes, z_top,
                                                      max_range, params, rows, cols, d[POSES], d[IMAGES], depth_type, nullptr);
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

int amk_sim_vehicle_step_att(const double *h_ABc, const double *d_cmd, double *d_x, double *d_Twb, int n_scenes, double pose_quantum,
                             int attitude, double gz, void *stream) {
    if (const int st = vehicle_args_status(h_ABc && d_cmd && d_x, n_scenes, pose_quantum); st != AMK_OK) return st;
    if (const int st = attitude_args_status(attitude, gz); st != AMK_OK) return st;
    if (const int st = amk_sim_vehicle_step(h_ABc, d_cmd, d_x, d_Twb, n_scenes, pose_quantum, stream); st != AMK_OK) return st;
    if (attitude == AMK_SIM_ATT_YAW || !d_Twb) return AMK_OK;
    hipLaunchKernelGGL(sim_attitude_kernel, dim3((n_scenes + kSimThreads - 1) / kSimThreads), dim3(kSimThreads), 0, (hipStream_t)stream,
                       d_x, d_Twb, gz, n_scenes);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

int amk_sim_vehicle_step_att_host(const double *h_ABc, const double *h_cmd, double *h_x, double *h_Twb, int n_scenes,
                                  double pose_quantum, int attitude, double gz) {
    if (const int st = vehicle_args_status(h_ABc && h_cmd && h_x, n_scenes, pose_quantum); st != AMK_OK) return st;
    if (const int st = attitude_args_status(attitude, gz); st != AMK_OK) return st;
    if (amk_device_count() <= 0) return AMK_ERR_NO_DEVICE;
    enum { CMD, STATE, POSES };
    amk::HostStage stage;
    return stage.call({amk::to_device(h_cmd, sizeof(double) * 3 * n_scenes), amk::both_ways(h_x, sizeof(double) * 10 * n_scenes),
                       amk::if_given(amk::to_host(h_Twb, sizeof(double) * 16 * n_scenes))},
                      [&](const amk::HostStage::Dev *d) {
                          return amk_sim_vehicle_step_att(h_ABc, d[CMD], d[STATE], d[POSES], n_scenes, pose_quantum, attitude, gz, nullptr);
                      },
                      hipDeviceSynchronize);
}

}  // extern "C"
