// Segment search on the KD index for gfx950 (MI355X): for every leg of a path -- the line between two successive positions -- every
// usable point of the scene's cloud within a radius of the leg, their number, the nearest max_results of them and where along the
// leg each comes closest (include/avoid_mpc_amd.h, "Segment search").  Not on the reference's surface (PlanWapionts checks
// reference point 0 only; the MPC sees obstacles at its sampled states): the next query of the index after the radius search, for
// the clearance of a predicted path BETWEEN its samples.  The walk itself is grid_segment (kd_grid.h); the multi-frame variants
// (amk_kfmap_segment_search, amk_kd_segment_search_frames) live in map_query.hip beside the frame description they share.
#include "kd_exact.h"

// one wavefront per (scene, leg), four legs of a scene per block (amk_kd_search's launch shape)
__global__ __launch_bounds__(256) void kd_segment_search_kernel(amk::GridPtrs gpt, int n_scenes, const double *__restrict__ path,
    int point_stride, int n_points, double r2, int k, int *__restrict__ out_idx, double *__restrict__ out_d2,
    double *__restrict__ out_t, float *__restrict__ out_pts, int *__restrict__ out_cnt) {
    __shared__ amk::GridWaveLds wl[4];
    const int n_legs = n_points - 1;
    const amk::WaveSlot m = amk::wave_slot(n_legs);
    if (m.s >= n_scenes || m.unit >= n_legs) return;
    const double *pa = path + ((size_t)m.s * n_points + m.unit) * point_stride;
    const amk::SegLeg leg = amk::seg_leg(pa, pa + point_stride);
    const size_t row = (size_t)m.s * n_legs + m.unit;
    double ld, lt;
    int li, lpos;
    const amk::GridScene gs = gpt.scene(m.s);
    const int cnt = amk::grid_segment(gs, leg, r2, k, ld, li, lpos, lt, &wl[m.w]);
    if (m.lane == 0 && out_cnt) out_cnt[row] = cnt;   // the full number, whatever k
    if (m.lane < k) {
        const bool ok = li != amk::kNoIndex;
        const float4 rec = gs.pt[lpos];  // lpos = 0 for empty slots: a valid address
        const size_t o = row * k + m.lane;
        if (out_idx) out_idx[o] = ok ? li : -1;
        if (out_d2) out_d2[o] = ok ? ld : DBL_MAX;
        if (out_t) out_t[o] = ok ? lt : 0.0;
        if (out_pts) {
            out_pts[o * 3 + 0] = ok ? rec.x : 0.f;
            out_pts[o * 3 + 1] = ok ? rec.y : 0.f;
            out_pts[o * 3 + 2] = ok ? rec.z : 0.f;
        }
    }
}

// the header's rules for one handle, before anything is staged or launched
static int segment_handle_status(const amk_kd *kd, const double *path, int point_stride, int n_points, double radius_sq, int max_results,
                                 const void *indices, const void *sqdist, const void *t, const void *pts, const void *counts) {
    if (!kd) return AMK_ERR_INVALID_ARG;
    if (const int st = amk::segment_args_status(path, point_stride, n_points, radius_sq, max_results, indices || sqdist || t || pts,
                                                indices || sqdist || t || pts || counts);
        st != AMK_OK)
        return st;
    if (kd->mode != 0) return AMK_ERR_UNSUPPORTED;   // the streaming scan has no segment walk
    if (amk::search_blocks(kd->n_scenes, n_points - 1) > 0x7fffffffll) return AMK_ERR_UNSUPPORTED;
    return AMK_OK;
}

extern "C" {

int amk_kd_segment_search(amk_kd *kd, const double *d_path, int point_stride, int n_points, double radius_sq, int max_results,
                          int *d_indices, double *d_sqdist, double *d_t, float *d_pts, int *d_counts, void *stream) {
    if (const int st = segment_handle_status(kd, d_path, point_stride, n_points, radius_sq, max_results, d_indices, d_sqdist, d_t, d_pts,
                                             d_counts);
        st != AMK_OK)
        return st;
    hipLaunchKernelGGL(kd_segment_search_kernel, dim3((unsigned)amk::search_blocks(kd->n_scenes, n_points - 1)), dim3(256), 0,
                       (hipStream_t)stream, grid_ptrs(kd), kd->n_scenes, d_path, point_stride, n_points, amk::radius_clamped(radius_sq),
                       max_results, d_indices, d_sqdist, d_t, d_pts, d_counts);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

int amk_kd_segment_search_host(amk_kd *kd, const double *h_path, int point_stride, int n_points, double radius_sq, int max_results,
                               int *h_indices, double *h_sqdist, double *h_t, float *h_pts, int *h_counts) {
    if (const int st = segment_handle_status(kd, h_path, point_stride, n_points, radius_sq, max_results, h_indices, h_sqdist, h_t, h_pts,
                                             h_counts);
        st != AMK_OK)
        return st;
    if (kd->async_pending) {  // a build / sweep enqueued on some other stream: order behind it once
        AMK_HIP(hipDeviceSynchronize());
        kd->async_pending = 0;
    }
    const size_t np = ((size_t)kd->n_scenes * n_points - 1) * point_stride + 3, rows = (size_t)kd->n_scenes * (n_points - 1),
                 k = (size_t)max_results;
    enum { PATH, SQDIST, T, INDICES, COUNTS, PTS };
    return kd->stage.call_pinned(
        {amk::to_device(h_path, np * sizeof(double)), amk::if_given(amk::to_host(h_sqdist, rows * k * sizeof(double))),
         amk::if_given(amk::to_host(h_t, rows * k * sizeof(double))), amk::if_given(amk::to_host(h_indices, rows * k * sizeof(int))),
         amk::if_given(amk::to_host(h_counts, rows * sizeof(int))), amk::if_given(amk::to_host(h_pts, rows * k * 3 * sizeof(float)))},
        [&](const amk::HostStage::Dev *d, hipStream_t stream) {
            return amk_kd_segment_search(kd, d[PATH], point_stride, n_points, radius_sq, max_results, d[INDICES], d[SQDIST], d[T], d[PTS],
                                         d[COUNTS], stream);
        });
}

}  // extern "C"
