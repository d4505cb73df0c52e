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
    const amk::WaveSlot m = amk::wave_slot(n_queries);
    if (m.s >= n_scenes || m.unit >= n_queries) return;
    const size_t row = (size_t)m.s * n_queries + m.unit;
    const double *qp = queries + row * query_stride;
    double ld;
    int li, lpos;
    const amk::GridScene gs = gpt.scene(m.s);
    const int cnt = amk::grid_radius(gs, qp[0], qp[1], qp[2], r2, k, ld, li, lpos, &wl[m.w]);
    if (m.lane == 0 && out_cnt) out_cnt[row] = cnt;   // the full number, whatever k
    if (m.lane < k) {
        const bool ok = li != amk::kNoIndex;
        const float4 rec = gs.pt[lpos];  // lpos = 0 for empty slots: a valid address
        const size_t o = row * k + m.lane;
        if (out_idx) out_idx[o] = ok ? li : -1;
        if (out_d2) out_d2[o] = ok ? ld : DBL_MAX;
        if (out_pts) {
            out_pts[o * 3 + 0] = ok ? rec.x : 0.f;
            out_pts[o * 3 + 1] = ok ? rec.y : 0.f;
            out_pts[o * 3 + 2] = ok ? rec.z : 0.f;
        }
    }
}

// the header's rules for one handle, before anything is staged or launched
static int radius_handle_status(const amk_kd *kd, const double *queries, int query_stride, int n_queries, double radius_sq,
                                int max_results, const void *indices, const void *sqdist, const void *pts, const void *counts) {
    if (!kd) return AMK_ERR_INVALID_ARG;
    if (const int st = amk::radius_args_status(queries, query_stride, n_queries, radius_sq, max_results, indices || sqdist || pts,
                                               indices || sqdist || pts || counts);
        st != AMK_OK)
        return st;
    if (kd->mode != 0) return AMK_ERR_UNSUPPORTED;   // the streaming scan has no radius walk
    if (amk::search_blocks(kd->n_scenes, n_queries) > 0x7fffffffll) return AMK_ERR_UNSUPPORTED;
    return AMK_OK;
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
    if (kd->async_pending) {  // a build / sweep enqueued on some other stream: order behind it once
        AMK_HIP(hipDeviceSynchronize());
        kd->async_pending = 0;
    }
    const size_t rows = (size_t)kd->n_scenes * n_queries, k = (size_t)max_results;
    enum { QUERIES, SQDIST, INDICES, COUNTS, PTS };
    return kd->stage.call_pinned(
        {amk::to_device(h_queries, ((rows - 1) * query_stride + 3) * sizeof(double)), amk::if_given(amk::to_host(h_sqdist, rows * k * sizeof(double))),
         amk::if_given(amk::to_host(h_indices, rows * k * sizeof(int))), amk::if_given(amk::to_host(h_counts, rows * sizeof(int))),
         amk::if_given(amk::to_host(h_pts, rows * k * 3 * sizeof(float)))},
        [&](const amk::HostStage::Dev *d, hipStream_t stream) {
            return amk_kd_radius_search(kd, d[QUERIES], query_stride, n_queries, radius_sq, max_results, d[INDICES], d[SQDIST], d[PTS],
                                        d[COUNTS], stream);
        });
}

}  // extern "C"
