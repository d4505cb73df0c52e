// Path cast on the KD index for gfx950 (MI355X): for every scene ONE answer for a whole polyline -- the first leg that cannot be
// passed, where on it the contact begins, which point is touched and how far the path is free (include/avoid_mpc_amd.h, "Path
// cast").  The answer is the reduction of amk_kd_segment_cast's per-leg answers in leg order, bit for bit; what is new is that the
// legs behind the stop leg are never walked and that one row per scene leaves the device instead of four per leg.  The walk of a
// leg is grid_cast (kd_grid.h); the rounds, their barrier rules and the reduction are path_cast_scene (kd_path_cast.h); the
// multi-frame variants (amk_kfmap_path_cast, amk_kd_path_cast_frames) live in map_query.hip beside the frame description they share.
#include "kd_exact.h"
#include "kd_path_cast.h"

// One block per scene, block b = scene b: the dispatcher puts block b on XCD b % 8, so scene = block (mod 8) as wave_slot arranges
// it for the per-leg kernels, and the W waves of a scene share its index in one CU's L1.  Wave w walks leg W r + w in round r.
// The barrier rules stand above path_cast_scene; the only return before it is this whole-block one.
template <int W>
__global__ __launch_bounds__(64 * W) void kd_path_cast_kernel(amk::GridPtrs gpt, int n_scenes, const double *__restrict__ path,
    int point_stride, long long scene_stride, int n_points, double r2, amk::PathCastOut out) {
    __shared__ amk::PathCastLds<W> lds;
    const int s = blockIdx.x;
    if (s >= n_scenes) return;   // (the whole block)
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const amk::GridScene gs = gpt.scene(s);
    amk::path_cast_scene<W>(s, path + (size_t)s * scene_stride, point_stride, n_points - 1, lds, out,
                            [&](const amk::SegLeg &leg, double &t, int &id, float &x, float &y, float &z) {
                                int bpos;
                                const bool hit = amk::grid_cast(gs, leg, r2, 1.0, t, id, bpos, &lds.wl[w]);
                                const float4 rec = gs.pt[bpos];   // bpos = 0 without a contact: a valid address
                                x = rec.x; y = rec.y; z = rec.z;
                                return hit;
                            });
}

// the header's rules for one handle, before anything is staged or launched
static int path_cast_handle_status(const amk_kd *kd, const double *path, int point_stride, int n_points, double radius_sq, bool any_out) {
    // (mode 1, the streaming scan, has no segment walk; a block per scene: no grid of per-leg wavefronts to bound)
    return amk::kd_query_handle_status(kd, 0, amk::segment_cast_args_status(path, point_stride, n_points, radius_sq, any_out));
}

namespace amk {
int kd_path_cast_scenes(amk_kd *kd, int n_scenes, const double *d_path, int point_stride, long long scene_stride, int n_points,
                        double radius_sq, const PathCastOut &out, hipStream_t stream) {
    if (const int st = path_cast_handle_status(kd, d_path, point_stride, n_points, radius_sq, out.any()); st != AMK_OK) return st;
    if (n_scenes < 1 || n_scenes > kd->n_scenes || scene_stride < 0) return AMK_ERR_INVALID_ARG;
    hipLaunchKernelGGL(kd_path_cast_kernel<kPathCastWaves>, dim3((unsigned)n_scenes), dim3(64 * kPathCastWaves), 0, stream, grid_ptrs(kd),
                       n_scenes, d_path, point_stride, scene_stride, n_points, radius_clamped(radius_sq), out);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}
}  // namespace amk

extern "C" {

int amk_kd_path_cast(amk_kd *kd, const double *d_path, int point_stride, int n_points, double radius_sq, int *d_stop, int *d_leg,
                     double *d_t, double *d_free, float *d_pts, int *d_indices, void *stream) {
    const amk::PathCastOut out{d_stop, d_leg, d_t, d_free, d_pts, d_indices};
    if (const int st = path_cast_handle_status(kd, d_path, point_stride, n_points, radius_sq, out.any()); st != AMK_OK) return st;
    return amk::kd_path_cast_scenes(kd, kd->n_scenes, d_path, point_stride, (long long)n_points * point_stride, n_points, radius_sq, out,
                                    (hipStream_t)stream);
}

int amk_kd_path_cast_host(amk_kd *kd, const double *h_path, int point_stride, int n_points, double radius_sq, int *h_stop, int *h_leg,
                          double *h_t, double *h_free, float *h_pts, int *h_indices) {
    if (const int st = path_cast_handle_status(kd, h_path, point_stride, n_points, radius_sq,
                                               h_stop || h_leg || h_t || h_free || h_pts || h_indices);
        st != AMK_OK)
        return st;
    if (const int st = amk::kd_order_behind_pending(kd); st != AMK_OK) return st;
    const size_t np = amk::points_extent(kd->n_scenes, n_points, point_stride), rows = (size_t)kd->n_scenes;
    enum { PATH, T, FREE, STOP, LEG, INDICES, PTS };
    return kd->stage.call_pinned(
        {amk::to_device(h_path, np * sizeof(double)), amk::if_given(amk::to_host(h_t, rows * sizeof(double))),
         amk::if_given(amk::to_host(h_free, rows * sizeof(double))), amk::if_given(amk::to_host(h_stop, rows * sizeof(int))),
         amk::if_given(amk::to_host(h_leg, rows * sizeof(int))), amk::if_given(amk::to_host(h_indices, rows * sizeof(int))),
         amk::if_given(amk::to_host(h_pts, rows * 3 * sizeof(float)))},
        [&](const amk::HostStage::Dev *d, hipStream_t stream) {
            return amk_kd_path_cast(kd, d[PATH], point_stride, n_points, radius_sq, d[STOP], d[LEG], d[T], d[FREE], d[PTS], d[INDICES], stream);
        });
}

}  // extern "C"
