// Segment nearest on the KD index for gfx950 (MI355X): for every leg of a path the k usable points of the scene's cloud closest to
// the leg, ascending, and where along the leg each comes closest (include/avoid_mpc_amd.h, "Segment nearest").  The query of the
// segment search that needs no radius: the minimum clearance of a predicted path BETWEEN its samples as a number.  The walk itself
// is grid_segment_knn (kd_grid.h); the multi-frame variants (amk_kfmap_segment_nearest, amk_kd_segment_nearest_frames) live in
// map_query.hip beside the frame description they share.
#include "kd_exact.h"

// one wavefront per (scene, leg), four legs of a scene per block (kd_segment_search_kernel's launch shape)
__global__ __launch_bounds__(256) void kd_segment_nearest_kernel(amk::GridPtrs gpt, int n_scenes, const double *__restrict__ path,
    int point_stride, int n_points, int k, int *__restrict__ out_idx, double *__restrict__ out_d2, double *__restrict__ out_t,
    float *__restrict__ out_pts, int *__restrict__ out_cnt) {
    __shared__ amk::GridWaveLds wl[4];
    const amk::RowSlot r = amk::row_slot(path, point_stride, n_points, n_points - 1);
    const amk::WaveSlot &m = r.ws;
    if (!r.in(n_scenes)) return;
    const amk::SegLeg leg = amk::seg_leg(r.p, r.p + point_stride);
    double ld, lt;
    int li, lpos;
    const amk::GridScene gs = gpt.scene(m.s);
    const int cnt = amk::grid_segment_knn(gs, leg, k, ld, li, lpos, lt, &wl[m.w]);   // min(k, usable points of the scene)
    amk::write_list_row<true>(r.row, k, m.lane, cnt, li != amk::kNoIndex, ld, lt, [&] { return gs.pt[lpos]; }, li, out_cnt, out_d2, out_t, out_idx,
                              out_pts);
}

// the header's rules for one handle, before anything is staged or launched
static int segment_nearest_handle_status(const amk_kd *kd, const double *path, int point_stride, int n_points, int k, const void *indices,
                                         const void *sqdist, const void *t, const void *pts, const void *counts) {
    return amk::kd_query_handle_status(kd, n_points - 1,   // (mode 1, the streaming scan, has no segment walk)
                                       amk::segment_nearest_args_status(path, point_stride, n_points, k,
                                                                        indices || sqdist || t || pts || counts));
}

extern "C" {

int amk_kd_segment_nearest(amk_kd *kd, const double *d_path, int point_stride, int n_points, int k, int *d_indices, double *d_sqdist,
                           double *d_t, float *d_pts, int *d_counts, void *stream) {
    if (const int st = segment_nearest_handle_status(kd, d_path, point_stride, n_points, k, d_indices, d_sqdist, d_t, d_pts, d_counts);
        st != AMK_OK)
        return st;
    hipLaunchKernelGGL(kd_segment_nearest_kernel, dim3((unsigned)amk::search_blocks(kd->n_scenes, n_points - 1)), dim3(256), 0,
                       (hipStream_t)stream, grid_ptrs(kd), kd->n_scenes, d_path, point_stride, n_points, k, d_indices, d_sqdist, d_t,
                       d_pts, d_counts);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

int amk_kd_segment_nearest_host(amk_kd *kd, const double *h_path, int point_stride, int n_points, int k, int *h_indices,
                                double *h_sqdist, double *h_t, float *h_pts, int *h_counts) {
    if (const int st = segment_nearest_handle_status(kd, h_path, point_stride, n_points, k, h_indices, h_sqdist, h_t, h_pts, h_counts);
        st != AMK_OK)
        return st;
    if (const int st = amk::kd_order_behind_pending(kd); st != AMK_OK) return st;
    const size_t np = amk::points_extent(kd->n_scenes, n_points, point_stride), rows = (size_t)kd->n_scenes * (n_points - 1),
                 kk = (size_t)k;
    enum { PATH, SQDIST, T, INDICES, COUNTS, PTS };
    return kd->stage.call_pinned(
        {amk::to_device(h_path, np * sizeof(double)), amk::if_given(amk::to_host(h_sqdist, rows * kk * sizeof(double))),
         amk::if_given(amk::to_host(h_t, rows * kk * sizeof(double))), amk::if_given(amk::to_host(h_indices, rows * kk * sizeof(int))),
         amk::if_given(amk::to_host(h_counts, rows * sizeof(int))), amk::if_given(amk::to_host(h_pts, rows * kk * 3 * sizeof(float)))},
        [&](const amk::HostStage::Dev *d, hipStream_t stream) {
            return amk_kd_segment_nearest(kd, d[PATH], point_stride, n_points, k, d[INDICES], d[SQDIST], d[T], d[PTS], d[COUNTS], stream);
        });
}

}  // extern "C"
