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
    const amk::RowSlot r = amk::row_slot(path, point_stride, n_points, n_points - 1);
    const amk::WaveSlot &m = r.ws;
    if (!r.in(n_scenes)) return;
    const amk::SegLeg leg = amk::seg_leg(r.p, r.p + point_stride);
    double ld, lt;
    int li, lpos;
    const amk::GridScene gs = gpt.scene(m.s);
    const int cnt = amk::grid_segment(gs, leg, r2, k, ld, li, lpos, lt, &wl[m.w]);   // the full number, whatever k
    amk::write_list_row<true>(r.row, k, m.lane, cnt, li != amk::kNoIndex, ld, lt, [&] { return gs.pt[lpos]; }, li, out_cnt, out_d2, out_t, out_idx,
                              out_pts);
}

// the header's rules for one handle, before anything is staged or launched
static int segment_handle_status(const amk_kd *kd, const double *path, int point_stride, int n_points, double radius_sq, int max_results,
                                 const void *indices, const void *sqdist, const void *t, const void *pts, const void *counts) {
    return amk::kd_query_handle_status(kd, n_points - 1,   // (mode 1, the streaming scan, has no segment walk)
                                       amk::segment_args_status(path, point_stride, n_points, radius_sq, max_results,
                                                                indices || sqdist || t || pts, indices || sqdist || t || pts || counts));
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
    if (const int st = amk::kd_order_behind_pending(kd); st != AMK_OK) return st;
    const size_t np = amk::points_extent(kd->n_scenes, n_points, point_stride), rows = (size_t)kd->n_scenes * (n_points - 1),
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
