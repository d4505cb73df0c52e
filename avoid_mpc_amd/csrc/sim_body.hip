// The rigid-body vehicle of a closed-loop flight for gfx950: amk_sim_vehicle_step_body, beside sim.hip's affine vehicle.
// sim.hip's amk_sim_vehicle_step advances the plant with the MPC's own model, so the MPC's first predicted state IS the next odometry.
// This vehicle is a small rigid body flown by bfctrl's GeometricController in acceleration mode -- desired attitude from the commanded
// thrust vector, thrust as the command projected on the current body z, attitude error on SO(3) -- through n_sub explicit sub-steps
// per control period, and it reports its acceleration as the node does: the COGFilter's weighted mean of the body-frame
// accelerometer samples, rotated by the current attitude, minus gravity.  ("Closed loop on the device"; the numpy
// restatement is avoid_mpc_amd/flight.py body_step_ordered.)
//
// Arithmetic contract (include/avoid_mpc_amd.h, "The rigid-body vehicle"): fp64, no contraction, every sum left to right as the
// header parenthesises it, IEEE division and square root, no transcendental.  sim.hip is not edited: what this file shares with it
// (acc2rotmat, the p' rule) is restated here.
#include <cmath>

#include "amk_common.h"

namespace {

constexpr int kBodyThreads = 256;
constexpr int kBodyDoubles = AMK_SIM_BODY_DOUBLES, kCogMax = AMK_SIM_COG_MAX;
constexpr int kQ = 0, kRate = 4, kF = 7, kHeld = 8, kHead = 9, kRing = 10;   // where the hidden state lies in a scene's 64 doubles
static_assert(kRing + 3 * kCogMax <= kBodyDoubles, "the ring lies inside the scene's state");
static_assert((kCogMax & (kCogMax - 1)) == 0, "the ring's slot is taken modulo a power of two");

struct BodyArgs {                 // by value: 29 doubles and 3 ints of kernel arguments
    double h, hh, gz, k_att, rate_max, k_rate, k_thrust, f_min, f_max, d0, d1, d2, cs, sn, quantum;
    double cog_weight[kCogMax];
    int n_sub, cog_window, n_scenes;
};

#pragma clang fp contract(off)

// v < lo ? lo : (v > hi ? hi : v): a NaN fails both comparisons and passes through
__device__ __forceinline__ double clampd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One of the two integers kept as doubles: truncated towards zero; a value outside [0, hi] (or a NaN) reads as 0, so no ring access
// leaves the scene's own 64 doubles whatever the state holds.
__device__ __forceinline__ int body_index(double v, int hi) { return v >= 0.0 && v <= (double)hi ? (int)v : 0; }

struct Rot { double r00, r01, r02, r10, r11, r12, r20, r21, r22; };
__device__ __forceinline__ Rot rotation(double qw, double qx, double qy, double qz) {
    Rot R;
    R.r00 = 1.0 - 2.0 * ((qy * qy) + (qz * qz)); R.r01 = 2.0 * ((qx * qy) - (qw * qz)); R.r02 = 2.0 * ((qx * qz) + (qw * qy));
    R.r10 = 2.0 * ((qx * qy) + (qw * qz)); R.r11 = 1.0 - 2.0 * ((qx * qx) + (qz * qz)); R.r12 = 2.0 * ((qy * qz) - (qw * qx));
    R.r20 = 2.0 * ((qx * qz) - (qw * qy)); R.r21 = 2.0 * ((qy * qz) + (qw * qx)); R.r22 = 1.0 - 2.0 * ((qx * qx) + (qy * qy));
    return R;
}
__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
    return (a0 * b0 + a1 * b1) + a2 * b2;
}

// One thread per scene.  p, v, q, the rates, f and the call's constants T and R_d stay in registers across the sub-step loop, whose
// only memory traffic is the three stores of the specific-force sample into the scene's own ring in global memory (never a private
// array: a dynamically indexed one would go to scratch).  The filter's weights are indexed by a run-time idx, so they are copied
// from the kernel-argument segment into LDS once per block; every lane then reads the same LDS address (a broadcast).
// BARRIER: the one barrier stands in front of the `s >= n_scenes` return, so every thread of a block reaches it.
// REGISTERS: the state is 14 doubles, R 9, T and R_d 12: 70 VGPRs before a single temporary, so the 64 of eight waves per SIMD cannot
// hold it.  Forcing eight waves spills (124 bytes of scratch per lane; 128 with T, Y and Z parked in LDS and X re-formed per sub-step,
// which is all the LDS eight blocks per CU leave; 52 bytes at six waves, 12 at five).  The kernel therefore takes what it needs --
// 119 VGPRs, four waves, no scratch.  Occupancy buys nothing here: a fleet of 256 is four wavefronts on a device of 1024 SIMDs, and
// the cost of a call is one thread's dependent fp64 chain times n_sub, latency and not throughput.
__global__ __launch_bounds__(kBodyThreads) void sim_body_kernel(BodyArgs g, const double *__restrict__ cmd, double *__restrict__ x,
                                                                 double *__restrict__ body, double *__restrict__ Twb) {
    __shared__ double sW[kCogMax];
    if (threadIdx.x < kCogMax) sW[threadIdx.x] = g.cog_weight[threadIdx.x];
    __syncthreads();                                             // (before any thread leaves)
    const int s = blockIdx.x * kBodyThreads + threadIdx.x;
    if (s >= g.n_scenes) return;
    double *xs = x + (size_t)s * 10, *b = body + (size_t)s * kBodyDoubles, *ring = b + kRing;
    double p0 = xs[0], p1 = xs[1], p2 = xs[2], v0 = xs[4], v1 = xs[5], v2 = xs[6];
    double qw = b[kQ], qx = b[kQ + 1], qy = b[kQ + 2], qz = b[kQ + 3];
    double w0 = b[kRate], w1 = b[kRate + 1], w2 = b[kRate + 2], f = b[kF];
    int held = body_index(b[kHeld], kCogMax), head = body_index(b[kHead], kCogMax - 1);

    // once per call: R_d = [X Y Z] of acc2rotmat on the command itself, which already holds gravity
    const double T0 = cmd[(size_t)s * 3 + 0], T1 = cmd[(size_t)s * 3 + 1], T2 = cmd[(size_t)s * 3 + 2];
    const double n = sqrt((T0 * T0 + T1 * T1) + T2 * T2);
    const double z0 = T0 / n, z1 = T1 / n, z2 = T2 / n;
    const double y0 = 0.0 - z2 * g.sn, y1 = z2 * g.cs, y2 = z0 * g.sn - z1 * g.cs;
    const double m = sqrt((y0 * y0 + y1 * y1) + y2 * y2);
    const bool valid = n > 0.0 && m > 0.0;
    const double Y0 = y0 / m, Y1 = y1 / m, Y2 = y2 / m, Z0 = z0, Z1 = z1, Z2 = z2;
    const double X0 = Y1 * Z2 - Y2 * Z1, X1 = Y2 * Z0 - Y0 * Z2, X2 = Y0 * Z1 - Y1 * Z0;

    for (int it = 0; it < g.n_sub; ++it) {
        const Rot R = rotation(qw, qx, qy, qz);
        // 1. attitude error: M = R_d^T R, e = (M21 - M12, M02 - M20, M10 - M01) / 2
        const double e0 = 0.5 * (dot3(Z0, Z1, Z2, R.r01, R.r11, R.r21) - dot3(Y0, Y1, Y2, R.r02, R.r12, R.r22));
        const double e1 = 0.5 * (dot3(X0, X1, X2, R.r02, R.r12, R.r22) - dot3(Z0, Z1, Z2, R.r00, R.r10, R.r20));
        const double e2 = 0.5 * (dot3(Y0, Y1, Y2, R.r00, R.r10, R.r20) - dot3(X0, X1, X2, R.r01, R.r11, R.r21));
        // 2. rate command (the minus sign is the stable one; bfctrl's geometric_attcontroller has none)
        const double c0 = valid ? clampd(-(g.k_att * e0), -g.rate_max, g.rate_max) : 0.0;
        const double c1 = valid ? clampd(-(g.k_att * e1), -g.rate_max, g.rate_max) : 0.0;
        const double c2 = valid ? clampd(-(g.k_att * e2), -g.rate_max, g.rate_max) : 0.0;
        // 3. thrust command: the command projected on the current body z
        const double fc = clampd(dot3(T0, T1, T2, R.r02, R.r12, R.r22), g.f_min, g.f_max);
        // 4. lags
        w0 = w0 + g.k_rate * (c0 - w0); w1 = w1 + g.k_rate * (c1 - w1); w2 = w2 + g.k_rate * (c2 - w2);
        f = f + g.k_thrust * (fc - f);
        // 5. specific force in the body frame, acceleration in the world frame, the sample into the ring
        const double vb0 = dot3(R.r00, R.r10, R.r20, v0, v1, v2), vb1 = dot3(R.r01, R.r11, R.r21, v0, v1, v2),
                     vb2 = dot3(R.r02, R.r12, R.r22, v0, v1, v2);
        const double s0 = -(g.d0 * vb0), s1 = -(g.d1 * vb1), s2 = f - g.d2 * vb2;
        const double a0 = dot3(R.r00, R.r01, R.r02, s0, s1, s2), a1 = dot3(R.r10, R.r11, R.r12, s0, s1, s2),
                     a2 = dot3(R.r20, R.r21, R.r22, s0, s1, s2) - g.gz;
        ring[3 * head + 0] = s0; ring[3 * head + 1] = s1; ring[3 * head + 2] = s2;   // head in [0, kCogMax): inside the scene's ring
        head = (head + 1) & (kCogMax - 1);
        held = held < kCogMax ? held + 1 : kCogMax;
        // 6. translation, semi-implicit: the position moves with the new velocity
        v0 = v0 + g.h * a0; v1 = v1 + g.h * a1; v2 = v2 + g.h * a2;
        p0 = p0 + g.h * v0; p1 = p1 + g.h * v1; p2 = p2 + g.h * v2;
        // 7. attitude: q <- q + (h / 2) q (x) (0, w) with the new rates, then back onto the unit sphere
        const double dw = -(((qx * w0) + (qy * w1)) + (qz * w2));
        const double dx = ((qw * w0) + (qy * w2)) - (qz * w1);
        const double dy = ((qw * w1) + (qz * w0)) - (qx * w2);
        const double dz = ((qw * w2) + (qx * w1)) - (qy * w0);
        qw = qw + g.hh * dw; qx = qx + g.hh * dx; qy = qy + g.hh * dy; qz = qz + g.hh * dz;
        const double nq = sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
        qw = qw / nq; qx = qx / nq; qy = qy / nq; qz = qz / nq;
    }

    // the filtered sample: the newest one itself, or the COGFilter's weighted mean over min(held, cog_window) samples, newest first.
    // The ring's loads follow this thread's own stores to the same addresses in program order.
    const Rot R = rotation(qw, qx, qy, qz);
    const double *nw = ring + 3 * ((head - 1) & (kCogMax - 1));
    double m0 = nw[0], m1 = nw[1], m2 = nw[2];
    if (g.cog_window >= 2) {
        const int take = held < g.cog_window ? held : g.cog_window;   // held >= 1: n_sub >= 1 has pushed
        double wsum = sW[0];
        m0 = wsum * m0; m1 = wsum * m1; m2 = wsum * m2;
        for (int idx = 1; idx < take; ++idx) {
            const double *sm = ring + 3 * ((head - 1 - idx) & (kCogMax - 1));
            const double wt = sW[idx];
            m0 = m0 + wt * sm[0]; m1 = m1 + wt * sm[1]; m2 = m2 + wt * sm[2];
            wsum = wsum + wt;
        }
        m0 = m0 / wsum; m1 = m1 / wsum; m2 = m2 / wsum;
    }
    xs[0] = p0; xs[1] = p1; xs[2] = p2;                          // x[3], the yaw, is not written
    xs[4] = v0; xs[5] = v1; xs[6] = v2;
    xs[7] = dot3(R.r00, R.r01, R.r02, m0, m1, m2);
    xs[8] = dot3(R.r10, R.r11, R.r12, m0, m1, m2);
    xs[9] = dot3(R.r20, R.r21, R.r22, m0, m1, m2) - g.gz;
    b[kQ] = qw; b[kQ + 1] = qx; b[kQ + 2] = qy; b[kQ + 3] = qz;
    b[kRate] = w0; b[kRate + 1] = w1; b[kRate + 2] = w2; b[kF] = f;
    b[kHeld] = (double)held; b[kHead] = (double)head;            // (the words behind the ring are left as they are)
    if (!Twb) return;
    double *T = Twb + (size_t)s * 16;
    T[0] = R.r00; T[1] = R.r01; T[2] = R.r02;   T[3] = g.quantum > 0.0 ? rint(p0 * g.quantum) / g.quantum : p0;
    T[4] = R.r10; T[5] = R.r11; T[6] = R.r12;   T[7] = g.quantum > 0.0 ? rint(p1 * g.quantum) / g.quantum : p1;
    T[8] = R.r20; T[9] = R.r21; T[10] = R.r22;  T[11] = g.quantum > 0.0 ? rint(p2 * g.quantum) / g.quantum : p2;
    T[12] = 0.0;  T[13] = 0.0;  T[14] = 0.0;    T[15] = 1.0;
}

// amk_sim_body_reset: one thread per double, all AMK_SIM_BODY_DOUBLES of every scene
__global__ __launch_bounds__(kBodyThreads) void sim_body_reset_kernel(double *__restrict__ body, long long total, double gz) {
    const long long i = (long long)blockIdx.x * kBodyThreads + threadIdx.x;
    if (i >= total) return;
    const int k = (int)(i % kBodyDoubles);
    body[i] = k == kQ ? 1.0 : (k == kF ? gz : 0.0);
}

// What both entries refuse, before anything is staged or launched
int body_args_status(const amk_sim_body_params *p, bool pointers, int n_scenes, double pose_quantum, BodyArgs &g) {
    if (!p || !pointers || n_scenes < 1 || !(pose_quantum >= 0.0)) return AMK_ERR_INVALID_ARG;
    if (!(p->h > 0.0) || p->n_sub < 1 || p->n_sub > 4096 || !(p->gz >= 0.0) || !(p->k_att >= 0.0) || !(p->rate_max > 0.0) ||
        !(p->k_rate > 0.0 && p->k_rate <= 1.0) || !(p->k_thrust > 0.0 && p->k_thrust <= 1.0) || !(p->f_min <= p->f_max) ||
        !(p->drag[0] >= 0.0) || !(p->drag[1] >= 0.0) || !(p->drag[2] >= 0.0) || p->yaw_cs != p->yaw_cs || p->yaw_sn != p->yaw_sn ||
        p->cog_window < 0 || p->cog_window > kCogMax)
        return AMK_ERR_INVALID_ARG;
    if (p->cog_window >= 2) {                                    // (a window of 0 or 1 divides by nothing and reads no weight)
        double sum = p->cog_weight[0];
        for (int i = 1; i < p->cog_window; ++i) sum = sum + p->cog_weight[i];
        if (!(sum > 0.0)) return AMK_ERR_INVALID_ARG;
    }
    g.h = p->h; g.hh = 0.5 * p->h; g.gz = p->gz; g.k_att = p->k_att; g.rate_max = p->rate_max; g.k_rate = p->k_rate;
    g.k_thrust = p->k_thrust; g.f_min = p->f_min; g.f_max = p->f_max; g.d0 = p->drag[0]; g.d1 = p->drag[1]; g.d2 = p->drag[2];
    g.cs = p->yaw_cs; g.sn = p->yaw_sn; g.quantum = pose_quantum;
    for (int i = 0; i < kCogMax; ++i) g.cog_weight[i] = p->cog_weight[i];
    g.n_sub = p->n_sub; g.cog_window = p->cog_window; g.n_scenes = n_scenes;
    return AMK_OK;
}

}  // namespace

extern "C" {

int amk_sim_body_reset(double *d_body, int n_scenes, double gz, void *stream) {
    if (!d_body || n_scenes < 1 || !(gz >= 0.0)) return AMK_ERR_INVALID_ARG;
    if (amk_device_count() <= 0) return AMK_ERR_NO_DEVICE;
    const long long total = (long long)n_scenes * kBodyDoubles;
    hipLaunchKernelGGL(sim_body_reset_kernel, dim3((unsigned)((total + kBodyThreads - 1) / kBodyThreads)), dim3(kBodyThreads), 0,
                       (hipStream_t)stream, d_body, total, gz);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

int amk_sim_vehicle_step_body(const amk_sim_body_params *prm, const double *d_cmd, double *d_x, double *d_body, double *d_Twb,
                              int n_scenes, double pose_quantum, void *stream) {
    BodyArgs g;
    if (const int st = body_args_status(prm, d_cmd && d_x && d_body, n_scenes, pose_quantum, g); st != AMK_OK) return st;
    if (amk_device_count() <= 0) return AMK_ERR_NO_DEVICE;
    hipLaunchKernelGGL(sim_body_kernel, dim3((n_scenes + kBodyThreads - 1) / kBodyThreads), dim3(kBodyThreads), 0, (hipStream_t)stream, g,
                       d_cmd, d_x, d_body, d_Twb);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

int amk_sim_vehicle_step_body_host(const amk_sim_body_params *prm, const double *h_cmd, double *h_x, double *h_body, double *h_Twb,
                                   int n_scenes, double pose_quantum) {
    BodyArgs g;
    if (const int st = body_args_status(prm, h_cmd && h_x && h_body, n_scenes, pose_quantum, g); st != AMK_OK) return st;
    if (amk_device_count() <= 0) return AMK_ERR_NO_DEVICE;
    enum { CMD, STATE, BODY, POSES };
    amk::HostStage stage;
    return stage.call({amk::to_device(h_cmd, sizeof(double) * 3 * n_scenes), amk::both_ways(h_x, sizeof(double) * 10 * n_scenes),
                       amk::both_ways(h_body, sizeof(double) * kBodyDoubles * n_scenes),
                       amk::if_given(amk::to_host(h_Twb, sizeof(double) * 16 * n_scenes))},
                      [&](const amk::HostStage::Dev *d) {
                          return amk_sim_vehicle_step_body(prm, d[CMD], d[STATE], d[BODY], d[POSES], n_scenes, pose_quantum, nullptr);
                      },
                      hipDeviceSynchronize);
}

}  // extern "C"
