// Segment cast on the KD index for gfx950 (MI355X): for every leg of a path the FIRST contact of a sphere whose centre moves along
// the leg -- whether there is one, where along the leg it begins, and which point of the scene's cloud is touched
// (include/avoid_mpc_amd.h, "Segment cast").  The segment search and segment nearest order by distance to the leg; this orders by
// position along it: the free distance along a velocity vector, the line of sight to a target.  The walk itself is grid_cast
// (kd_grid.h); the multi-frame variants (amk_kfmap_segment_cast, amk_kd_segment_cast_frames) live in map_query.hip beside the
// frame description they share.
#include "kd_exact.h"

// one wavefront per (scene, leg), four legs of a scene per block (kd_segment_search_kernel's launch shape)
__global__ __launch_bounds__(256) void kd_segment_cast_kernel(amk::GridPtrs gpt, int n_scenes, const double *__restrict__ path,
    int point_stride, int n_points, double r2, int *__restrict__ out_hit, double *__restrict__ out_t, float *__restrict__ out_pts,
    int *__restrict__ out_idx) {
    __shared__ amk::GridWaveLds wl[4];
    const amk::RowSlot r = amk::row_slot(path, point_stride, n_points, n_points - 1);
    const amk::WaveSlot &m = r.ws;
    if (!r.in(n_scenes)) return;
    const amk::SegLeg leg = amk::seg_leg(r.p, r.p + point_stride);
    double bt;
    int bi, bpos;
    const amk::GridScene gs = gpt.scene(m.s);
    const bool hit = amk::grid_cast(gs, leg, r2, 1.0, bt, bi, bpos, &wl[m.w]);
    const float4 rec = gs.pt[bpos];  // bpos = 0 without a contact: a valid address
    amk::write_cast_row(r.row, m.lane, hit, hit ? bt : 1.0, hit ? rec.x : 0.f, hit ? rec.y : 0.f, hit ? rec.z : 0.f, hit ? bi : -1, out_hit,
                        out_t, out_idx, out_pts);
}

// the header's rules for one handle, before anything is staged or launched
static int cast_handle_status(const amk_kd *kd, const double *path, int point_stride, int n_points, double radius_sq, const void *hit,
                              const void *t, const void *pts, const void *indices) {
    return amk::kd_query_handle_status(kd, n_points - 1,   // (mode 1, the streaming scan, has no segment walk)
                                       amk::segment_cast_args_status(path, point_stride, n_points, radius_sq, hit || t || pts || indices));
}

extern "C" {

int amk_kd_segment_cast(amk_kd *kd, const double *d_path, int point_stride, int n_points, double radius_sq, int *d_hit, double *d_t,
                        float *d_pts, int *d_indices, void *stream) {
    if (const int st = cast_handle_status(kd, d_path, point_stride, n_points, radius_sq, d_hit, d_t, d_pts, d_indices); st != AMK_OK)
        return st;
    hipLaunchKernelGGL(kd_segment_cast_kernel, dim3((unsigned)amk::search_blocks(kd->n_scenes, n_points - 1)), dim3(256), 0,
                       (hipStream_t)stream, grid_ptrs(kd), kd->n_scenes, d_path, point_stride, n_points, amk::radius_clamped(radius_sq),
                       d_hit, d_t, d_pts, d_indices);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}

int amk_kd_segment_cast_host(amk_kd *kd, const double *h_path, int point_stride, int n_points, double radius_sq, int *h_hit,
                             double *h_t, float *h_pts, int *h_indices) {
    if (const int st = cast_handle_status(kd, h_path, point_stride, n_points, radius_sq, h_hit, h_t, h_pts, h_indices); st != AMK_OK)
        return st;
    if (const int st = amk::kd_order_behind_pending(kd); st != AMK_OK) return st;
    const size_t np = amk::points_extent(kd->n_scenes, n_points, point_stride), rows = (size_t)kd->n_scenes * (n_points - 1);
    enum { PATH, T, HIT, INDICES, PTS };
    return kd->stage.call_pinned(
        {amk::to_device(h_path, np * sizeof(double)), amk::if_given(amk::to_host(h_t, rows * sizeof(double))),
         amk::if_given(amk::to_host(h_hit, rows * sizeof(int))), amk::if_given(amk::to_host(h_indices, rows * sizeof(int))),
         amk::if_given(amk::to_host(h_pts, rows * 3 * sizeof(float)))},
        [&](const amk::HostStage::Dev *d, hipStream_t stream) {
            return amk_kd_segment_cast(kd, d[PATH], point_stride, n_points, radius_sq, d[HIT], d[T], d[PTS], d[INDICES], stream);
        });
}

}  // extern "C"
