// Path cast (include/avoid_mpc_amd.h, "Path cast"): what kd_path_cast.hip (one handle) and map_query.hip (a keyframe map, a list of
// handles) share -- the block shape, the per-leg LDS record, the rounds with their barrier and the reduction that turns per-leg
// answers into one answer per scene.  The walk of a leg is grid_cast (kd_grid.h), untouched; seg_leg and seg_contact likewise.
#pragma once
#include "kd_grid.h"

namespace amk {

// Wavefronts per block = legs per round.  Measured on the siblings' cost workload (tools/experiments/kd_path_cast_cost.py,
// profiles/kd_path_cast_cost.txt), path cast / amk_kd_segment_cast on the same 19-leg paths:
//   W   (a) every path stops on leg 0    (b) 171 of 256 paths free to the end
//   4   0.94  (32.8 us against 34.8)     1.63  (25.4 us against 15.6)
//   8   1.04  (36.0 us against 34.6)     1.30  (20.2 us against 15.5)
// 4 is the only one that meets the bar of (a) (no slower than the yardstick), so it stays, with the worse (b).  A launch of 256
// scenes is latency-bound either way: the per-leg kernel's 19 walks run side by side on a chip this size, the rounds here run
// one after the other; what the path cast saves is work (the legs behind the stop leg) and the copy of four per-leg arrays.
// 16 was not built: a 1024-thread block does not overlap with the work of other streams at all (kd_grid.h, kGridBuildThreads),
// and this kernel runs beside the pipeline's solves.
#ifndef AMK_PATH_CAST_WAVES
#define AMK_PATH_CAST_WAVES 4   // (experiments: AMK_HIPCC_FLAGS=-DAMK_PATH_CAST_WAVES=8, as for the other build-time constants)
#endif
constexpr int kPathCastWaves = AMK_PATH_CAST_WAVES;

struct PathLegLds {   // one leg's answer, written by lane 0 of the leg's wave
    double t, len;    // the contact's t (0.0 for an unjudgeable leg, 1.0 for a free one); sqrt(L2)
    int stop, id;     // 0 free, 1 contact, 2 unjudgeable; cloud index or frame of the point touched
    float x, y, z;    // the point touched
    int pad;
};
template <int W>
struct PathCastLds {
    GridWaveLds wl[W];
    PathLegLds leg[2][W];   // by round parity: round r + 1 is written while a slower wave still reads round r
};

// One scene's path cast, run by all W waves of the scene's block.  pts: the scene's first path point; cast_leg(leg, t, id, x, y, z)
// answers one leg whose SegLeg is ok for the calling wave (true: a contact, with its t, index or frame, and point).
//
// THE BARRIER RULES.  A wave that misses a barrier hangs its block, and with it the device queue behind it:
//   1. every wave of the block reaches the barrier of every round, also a wave whose leg index is >= n_legs (it contributes
//      "free, length 0" and walks nothing);
//   2. the decision to leave the loop is taken from LDS words read AFTER the barrier, the same words in every wave, so it is the
//      same decision in every wave (made wave-uniform with v_readfirstlane: the loop's branch is a scalar one);
//   3. there is no return before the last barrier -- the caller returns early only for a WHOLE block whose scene is >= n_scenes,
//      before it calls this;
//   4. the trip count is bounded by ceil(n_legs / W), known before the loop.
// One barrier per round is enough: the records alternate between two sets by round parity, and a wave can only write set r & 1
// again (round r + 2) after the barrier of round r + 1, which every wave passes after it has read round r.
//
// No global atomics; the answer is a function of the LDS records in leg order, not of which wave finished first.
template <int W, class CastLeg>
__device__ __forceinline__ void path_cast_scene(int s, const double *pts, int point_stride, int n_legs, PathCastLds<W> &lds,
                                                const PathCastOut &out, CastLeg &&cast_leg) {
#pragma clang fp contract(off)
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int rounds = (n_legs + W - 1) / W;
    double free = 0.0;                       // ((len_0 + len_1) + ...) over the legs passed, + t * len of a contact leg
    PathLegLds stop{1.0, 0.0, 0, -1, 0.f, 0.f, 0.f, 0};
    int stop_leg = -1;
    for (int r = 0; r < rounds; ++r) {
        const int j = r * W + w;             // (wave-uniform)
        PathLegLds mine{1.0, 0.0, 0, -1, 0.f, 0.f, 0.f, 0};
        if (j < n_legs) {
            const double *pa = pts + (size_t)j * point_stride;
            const SegLeg leg = seg_leg(pa, pa + point_stride);
            if (!leg.ok) {                   // case (b): an audit must not read a NaN trajectory as free
                mine.stop = 2;
                mine.t = 0.0;
            } else {
                mine.len = sqrt(seg_leg_l2(leg));
                if (cast_leg(leg, mine.t, mine.id, mine.x, mine.y, mine.z)) mine.stop = 1;
            }
        }
        PathLegLds *rec = lds.leg[r & 1];
        if (lane == 0) rec[w] = mine;
        __syncthreads();                     // rule 1: the only barrier, reached by every wave in every round
        int k = 0, code = 0;
        for (; k < W; ++k) {                 // rule 2: every wave reads the same words, in leg order
            code = __builtin_amdgcn_readfirstlane(rec[k].stop);
            if (code) break;
            free = free + rec[k].len;
        }
        if (code) {
            stop = rec[k];
            stop_leg = r * W + k;
            if (code == 1) free = free + stop.t * stop.len;
            break;
        }
    }
    if (w == 0 && lane == 0) {
        const bool hit = stop.stop == 1;
        if (out.stop) out.stop[s] = stop.stop;
        if (out.leg) out.leg[s] = stop_leg;
        if (out.t) out.t[s] = stop.t;
        if (out.free) out.free[s] = free;
        if (out.id) out.id[s] = hit ? stop.id : -1;
        if (out.pts) {
            out.pts[(size_t)s * 3 + 0] = hit ? stop.x : 0.f;
            out.pts[(size_t)s * 3 + 1] = hit ? stop.y : 0.f;
            out.pts[(size_t)s * 3 + 2] = hit ? stop.z : 0.f;
        }
    }
}

}  // namespace amk
