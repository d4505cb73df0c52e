// Radius search on the KD index for gfx950 (MI355X): nanoflann's radiusSearch (AM/include/nanoflann_two.hpp:1611-1639 with
// RadiusResultSet, :345-413) for every scene of an amk_kd -- every usable point with squared distance < radius_sq, their number,
// and the nearest max_results of them.  The reference never calls it (KDTreeTwo wraps findNeighbors only): this is the surface
// of the index it was modelled on, not Avoid-MPC's.  The walk itself is grid_radius (kd_grid.h); the multi-frame variants
// (amk_kfmap_radius_search, amk_kd_radius_search_frames) live in map_query.hip beside the frame description they share.
#include "kd_exact.h"

// one wavefront per (scene, query), four queries of a scene per block (amk_kd_search's launch shape)
__global__ __launch_bounds__(256) void kd_radius_search_kernel(amk::GridPtrs gpt, int n_scenes, const double *__restrict__ queries,
    int query_stride, int n_queries, double r2, int k, int *__restrict__ out_idx, double *__restrict__ out_d2,
    float *__restrict__ out_pts, int *__restrict__ out_cnt) {
    __shared__ amk::GridWaveLds wl[4];
    const amk::RowSlot r = amk::row_slot(queries, query_stride, n_queries, n_queries);
    const amk::WaveSlot &m = r.ws;
    if (!r.in(n_scenes)) return;
    double ld;
    int li, lpos;
    const amk::GridScene gs = gpt.scene(m.s);
    const int cnt = amk::grid_radius(gs, r.p[0], r.p[1], r.p[2], r2, k, ld, li, lpos, &wl[m.w]);   // the full number, whatever k
    amk::write_list_row<false>(r.row, k, m.lane, cnt, li != amk::kNoIndex, ld, 0.0, [&] { return gs.pt[lpos]; }, li, out_cnt, out_d2, nullptr, out_idx,
                               out_pts);
}

// the header's rules for one handle, before anything is staged or launched
static int radius_handle_status(const amk_kd *kd, const double *queries, int query_stride, int n_queries, double radius_sq,
                                int max_results, const void *indices, const void *sqdist, const void *pts, const void *counts) {
    return amk::kd_query_handle_status(kd, n_queries,   // (mode 1, the streaming scan, has no radius walk)
                                       amk::radius_args_status(queries, query_stride, n_queries, radius_sq, max_results,
                                                               indices || sqdist || pts, indices || sqdist || pts || counts));
}

extern "C" {

int amk_kd_radius_search(amk_kd *kd, const double *d_queries, int query_stride, int n_queries, double radius_sq, int max_results,
                         int *d_indices, double *d_sqdist, float *d_pts, int *d_counts, void *stream) {
    if (const int st = radius_handle_status(kd, d_queries, query_stride, n_queries, radius_sq, max_results, d_indices, d_sqdist, d_pts, d_counts);
        st != AMK_OK)
        return st;
    // (the tie-order modes do not apply: nanoflann sorts radius results by distance alone, so the exact tree is not consulted)
    hipLaunchKernelGGL(kd_radius_search_kernel, dim3((unsigned)amk::search_blocks(kd->n_scenes, n_queries)), dim3(256), 0,
                       (hipStream_t)stream, grid_ptrs(kd), kd->n_scenes, d_queries, query_stride, n_queries, amk::radius_clamped(radius_sq),
                       max_results, d_indices, d_sqdist, d_pts, d_counts);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

int amk_kd_radius_search_host(amk_kd *kd, const double *h_queries, int query_stride, int n_queries, double radius_sq, int max_results,
                              int *h_indices, double *h_sqdist, float *h_pts, int *h_counts) {
    if (const int st = radius_handle_status(kd, h_queries, query_stride, n_queries, radius_sq, max_results, h_indices, h_sqdist, h_pts, h_counts);
        st != AMK_OK)
        return st;
    if (const int st = amk::kd_order_behind_pending(kd); st != AMK_OK) return st;
    const size_t rows = (size_t)kd->n_scenes * n_queries, k = (size_t)max_results;
    enum { QUERIES, SQDIST, INDICES, COUNTS, PTS };
    return kd->stage.call_pinned(
        {amk::to_device(h_queries, amk::points_extent(kd->n_scenes, n_queries, query_stride) * sizeof(double)),
         amk::if_given(amk::to_host(h_sqdist, rows * k * sizeof(double))), amk::if_given(amk::to_host(h_indices, rows * k * sizeof(int))),
         amk::if_given(amk::to_host(h_counts, rows * sizeof(int))),
         amk::if_given(amk::to_host(h_pts, rows * k * 3 * sizeof(float)))},
        [&](const amk::HostStage::Dev *d, hipStream_t stream) {
            return amk_kd_radius_search(kd, d[QUERIES], query_stride, n_queries, radius_sq, max_results, d[INDICES], d[SQDIST], d[PTS],
                                        d[COUNTS], stream);
        });
}

}  // extern "C"
