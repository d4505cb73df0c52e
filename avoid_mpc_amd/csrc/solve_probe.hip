// Tests only (internal: not part of the C ABI in include/avoid_mpc_amd.h): the small primitives every interior-point
// iteration of the solve is made of, each on plain arrays, so that tests/test_solve_math_gpu.py can hold them against a
// high-precision reference and against their numpy restatements (tests/_solve_math_cases.py).  The kernels call the
// functions of fast_math.h / mpc_device_impl.h themselves and hold no copy of them; nothing of the product path is here.
//   scalar   exp, log (sign kept), reciprocal, and the softplus chain g = log(1 + e^x), sg = e^x / (1 + e^x) as
//            collide_term writes them                                                    out [5][n]
//   slacks   (w1, w2) of slacks(s, mu)                                                   out [2][n]
//   wave     one wavefront per block, as the solve runs; every lane's result of the reduction ladders
//            in [n_waves][64] -> out [kWavePlanes][n_waves][64]
//   scan     suffix_scan2 on two channels with per-wave coefficients, k = lane & 31
//            x0, x1 [n_waves][64], al0, al1 [n_waves] -> out [2][n_waves][64]
// Every entry point takes device pointers and a stream, launches and returns (the caller synchronises); a NULL pointer or
// n < 1 is AMK_ERR_INVALID_ARG.  Every address is a function of the thread's index alone.
#include "mpc_device.h"

namespace {
constexpr int kThreads = 256;
constexpr int kWave = 64;
// planes of the wave probe: row_reduce<OpSum>, wave_sum, wave_min, wave_max, wave_reduce2<OpSum, OpMin> (2),
// wave_reduce3<OpSum, OpMin, OpMax> (3), seg_sum for seg = 1, 2, 4, 8, 16, 32, 64 (7)
constexpr int kWavePlanes = 16;

// One set of kernels per arithmetic: NS the namespace of mpc_device_impl.h, R its `real`; EXP / LOG / RCP the functions of
// the first three scalar planes (fp64: fast_math.h's own names; fp32: the wrappers).  The chain always goes through the
// wrappers, as collide_term does.
#define AMK_SOLVE_PROBE_KERNELS(SUF, NS, R, EXP, LOG, RCP)                                                              \
    __global__ __launch_bounds__(kThreads) void scalar_kernel_##SUF(const R *__restrict__ x, R *__restrict__ out, int n) { \
        const int i = blockIdx.x * kThreads + threadIdx.x;                                                               \
        if (i >= n) return;                                                                                              \
        const size_t N = (size_t)n;                                                                                      \
        const R v = x[i];                                                                                                \
        out[i] = EXP(v);                                                                                                 \
        out[N + i] = LOG(v);                                                                                             \
        out[2 * N + i] = RCP(v);                                                                                         \
        const R ex = NS::real_exp(v);                                                                                    \
        out[3 * N + i] = NS::real_log((R)1.0 + ex);                                                                      \
        out[4 * N + i] = ex * NS::fast_rcp((R)1.0 + ex);                                                                 \
    }                                                                                                                    \
    __global__ __launch_bounds__(kThreads) void slacks_kernel_##SUF(const R *__restrict__ s, const R *__restrict__ mu,   \
                                                                      R *__restrict__ out, int n) {                      \
        const int i = blockIdx.x * kThreads + threadIdx.x;                                                               \
        if (i >= n) return;                                                                                              \
        R w1, w2;                                                                                                        \
        NS::slacks(s[i], mu[i], w1, w2);                                                                                 \
        out[i] = w1;                                                                                                     \
        out[(size_t)n + i] = w2;                                                                                         \
    }                                                                                                                    \
    __global__ __launch_bounds__(kWave) void wave_kernel_##SUF(const R *__restrict__ in, R *__restrict__ out) {          \
        const size_t plane = (size_t)gridDim.x * kWave, i = (size_t)blockIdx.x * kWave + threadIdx.x;                    \
        const R v = in[i];                                                                                               \
        out[i] = NS::row_reduce<NS::OpSum>(v);                                                                           \
        out[plane + i] = NS::wave_sum(v);                                                                                \
        out[2 * plane + i] = NS::wave_min(v);                                                                            \
        out[3 * plane + i] = NS::wave_max(v);                                                                            \
        R a = v, b = v;                                                                                                  \
        NS::wave_reduce2<NS::OpSum, NS::OpMin>(a, b);                                                                    \
        out[4 * plane + i] = a;                                                                                          \
        out[5 * plane + i] = b;                                                                                          \
        R c = v;                                                                                                         \
        a = v; b = v;                                                                                                    \
        NS::wave_reduce3<NS::OpSum, NS::OpMin, NS::OpMax>(a, b, c);                                                      \
        out[6 * plane + i] = a;                                                                                          \
        out[7 * plane + i] = b;                                                                                          \
        out[8 * plane + i] = c;                                                                                          \
        _Pragma("unroll") for (int l = 0; l < 7; ++l) out[(9 + l) * plane + i] = NS::seg_sum(v, 1 << l);                 \
    }                                                                                                                    \
    __global__ __launch_bounds__(kWave) void scan_kernel_##SUF(const R *__restrict__ x0, const R *__restrict__ x1,       \
                                                                const R *__restrict__ al0, const R *__restrict__ al1,    \
                                                                R *__restrict__ out) {                                   \
        const size_t plane = (size_t)gridDim.x * kWave, i = (size_t)blockIdx.x * kWave + threadIdx.x;                    \
        R a = x0[i], b = x1[i];                                                                                          \
        NS::suffix_scan2(a, b, al0[blockIdx.x], al1[blockIdx.x], (int)threadIdx.x & 31);                                 \
        out[i] = a;                                                                                                      \
        out[plane + i] = b;                                                                                              \
    }                                                                                                                    \
    int scalar_##SUF(const R *x, R *out, int n, void *stream) {                                                          \
        if (!x || !out || n < 1) return AMK_ERR_INVALID_ARG;                                                             \
        hipLaunchKernelGGL(scalar_kernel_##SUF, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, x, out, n); \
        return hipGetLastError() == hipSuccess ? AMK_OK : AMK_ERR_HIP;                                                   \
    }                                                                                                                    \
    int slacks_##SUF(const R *s, const R *mu, R *out, int n, void *stream) {                                             \
        if (!s || !mu || !out || n < 1) return AMK_ERR_INVALID_ARG;                                                      \
        hipLaunchKernelGGL(slacks_kernel_##SUF, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, s, mu, out, n); \
        return hipGetLastError() == hipSuccess ? AMK_OK : AMK_ERR_HIP;                                                   \
    }                                                                                                                    \
    int wave_##SUF(const R *in, R *out, int n_waves, void *stream) {                                                     \
        if (!in || !out || n_waves < 1) return AMK_ERR_INVALID_ARG;                                                      \
        hipLaunchKernelGGL(wave_kernel_##SUF, dim3(n_waves), dim3(kWave), 0, (hipStream_t)stream, in, out);              \
        return hipGetLastError() == hipSuccess ? AMK_OK : AMK_ERR_HIP;                                                   \
    }                                                                                                                    \
    int scan_##SUF(const R *x0, const R *x1, const R *al0, const R *al1, R *out, int n_waves, void *stream) {            \
        if (!x0 || !x1 || !al0 || !al1 || !out || n_waves < 1) return AMK_ERR_INVALID_ARG;                               \
        hipLaunchKernelGGL(scan_kernel_##SUF, dim3(n_waves), dim3(kWave), 0, (hipStream_t)stream, x0, x1, al0, al1, out); \
        return hipGetLastError() == hipSuccess ? AMK_OK : AMK_ERR_HIP;                                                   \
    }

AMK_SOLVE_PROBE_KERNELS(f64, amk, double, amk::fast_exp, amk::fast_log, amk::rcp_f64)
AMK_SOLVE_PROBE_KERNELS(f32, amk32, float, amk32::real_exp, amk32::real_log, amk32::fast_rcp)
#undef AMK_SOLVE_PROBE_KERNELS
}  // namespace

extern "C" int amk__solve_probe_wave_planes(void) { return kWavePlanes; }
extern "C" int amk__solve_probe_scalar_f64(const double *d_x, double *d_out, int n, void *stream) { return scalar_f64(d_x, d_out, n, stream); }
extern "C" int amk__solve_probe_scalar_f32(const float *d_x, float *d_out, int n, void *stream) { return scalar_f32(d_x, d_out, n, stream); }
extern "C" int amk__solve_probe_slacks_f64(const double *d_s, const double *d_mu, double *d_out, int n, void *stream) { return slacks_f64(d_s, d_mu, d_out, n, stream); }
extern "C" int amk__solve_probe_slacks_f32(const float *d_s, const float *d_mu, float *d_out, int n, void *stream) { return slacks_f32(d_s, d_mu, d_out, n, stream); }
extern "C" int amk__solve_probe_wave_f64(const double *d_in, double *d_out, int n_waves, void *stream) { return wave_f64(d_in, d_out, n_waves, stream); }
extern "C" int amk__solve_probe_wave_f32(const float *d_in, float *d_out, int n_waves, void *stream) { return wave_f32(d_in, d_out, n_waves, stream); }
extern "C" int amk__solve_probe_scan_f64(const double *d_x0, const double *d_x1, const double *d_al0, const double *d_al1, double *d_out, int n_waves, void *stream) {
    return scan_f64(d_x0, d_x1, d_al0, d_al1, d_out, n_waves, stream);
}
extern "C" int amk__solve_probe_scan_f32(const float *d_x0, const float *d_x1, const float *d_al0, const float *d_al1, float *d_out, int n_waves, void *stream) {
    return scan_f32(d_x0, d_x1, d_al0, d_al1, d_out, n_waves, stream);
}
