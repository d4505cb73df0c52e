// The reference's OWN tree, node for node, and its own traversal -- the opt-in "nanoflann tie order" mode of an amk_kd
// (amk_kd_set_tie_order).
//
// Why: the bucketed index (kd_grid.h) returns the exact k nearest, equal squared distances ordered by cloud index.
// nanoflann keeps, of equal distances, the one it VISITS first (KNNResultSet::addPoint, AM/include/nanoflann_two.hpp:
// 219-246), i.e. its answer on ties depends on the shape of its tree and on its traversal.  To return the same INDEX
// lists on tie-heavy clouds (quantised depth on a pixel grid) the tree itself has to be the same.
//
// This header is what a SEARCH needs (every unit that traverses the tree includes it): the tree's layout (ExactTree, ExactPtrs) and
// exact_knn_thread / exact_knn_wave = findNeighbors -> computeInitialDistances -> searchLevel + KNNResultSet
// (nanoflann_two.hpp:1563-1586, 1296-1315, 1729-1793, 179-255).  The device build is kd_exact_build.h; its kernels, the tree's
// arrays (amk::ExactStore, amk_common.h) and the handle's tie-order calls are kd_exact.hip, the only unit that includes the build.
#pragma once
#include <cstring>
#include "kd_grid.h"

namespace amk {

constexpr int kExactMaxDepth = 48;  // traversal stack (one frame per level); deeper trees fall back to the bucketed index

struct ExactTree {  // one scene
    const float *x, *y, *z;  // index-ordered planes of the NaN-x-filtered cloud
    unsigned *vind;          // vAcc_
    int *feat;               // divfeat, -1 = leaf
    unsigned *left, *right;  // node range [left, right) in vind
    int *child;              // child1; child2 = child1 + 1
    double *low, *high;      // divlow, divhigh
    double *nbbox;           // [node][6] boxes handed down by divideTree (lo0, hi0, lo1, hi1, lo2, hi2)
    double *root_bbox;       // [6] root_bbox_
    unsigned *sa, *sb;       // scratch lists of planeSplit
    // the coordinates in vAcc_ order: pc[d * pstride + i] == coordinate d of point vind[i] (kept so by every swap of the
    // build).  ONE base pointer and a plane stride, not three pointers: `dim == 0 ? px[i] : dim == 1 ? py[i] : pz[i]` made the
    // compiler select the ADDRESS of the member and load the pointer from the struct, which then lived in scratch memory
    // (160 B per lane; scratch on a queue is what tests/test_abi.py forbids outside the opt-in thread-per-query kernels).
    float *pc;
    size_t pstride;
    int *n_nodes;            // [1] number of nodes; -1: the tree is not available (capacity / depth exceeded)
    int max_nodes;
    int lists_local;         // sa / sb are a wavefront's own short buffers, indexed from 0 (a window in LDS); else [lo + j]
    __device__ __forceinline__ float *plane(int dim) const { return pc + (size_t)dim * pstride; }
    __device__ __forceinline__ double val(unsigned i, int dim) const { return (double)pc[(size_t)dim * pstride + i]; }
};

struct ExactPtrs {  // the batch
    const float *x, *y, *z;
    int cap;
    unsigned *vind, *left, *right, *sa, *sb;
    float *pc;        // [3][S][cap]
    size_t pstride;   // S * cap
    int *feat, *child, *n_nodes;
    double *low, *high, *nbbox, *root_bbox;
    int max_nodes;
    __device__ __forceinline__ ExactTree scene(int s) const {
        ExactTree t;
        const size_t pc = (size_t)s * cap, nc = (size_t)s * max_nodes;
        t.x = x + pc; t.y = y + pc; t.z = z + pc;
        t.vind = vind + pc; t.sa = sa + pc; t.sb = sb + pc;
        t.pc = this->pc + pc; t.pstride = pstride;
        t.feat = feat + nc; t.left = left + nc; t.right = right + nc; t.child = child + nc;
        t.low = low + nc; t.high = high + nc; t.nbbox = nbbox + nc * 6;
        t.root_bbox = root_bbox + (size_t)s * 6;
        t.n_nodes = n_nodes + s;
        t.max_nodes = max_nodes;
        t.lists_local = 0;
        return t;
    }
};

// The traversal's stack: one frame per tree level -- either "the other child of this node is still to be considered"
// (kind 0: node, cut dimension, cut distance, mindist at the node) or, once that child has been entered, "restore
// dists[idx]" (kind 1, same slot).  Storage is the caller's: private arrays for the thread-per-query kernels (scratch
// memory), LDS for the single-lane re-query inside the plan kernels.
struct ExactStack {
    int *node, *ik;  // ik = idx | kind << 2
    double *a, *b;   // a: cut distance (kind 0) / saved dists[idx] (kind 1); b: mindist at the node
};
struct ExactStackStorage {  // kExactMaxDepth frames
    int node[kExactMaxDepth], ik[kExactMaxDepth];
    double a[kExactMaxDepth], b[kExactMaxDepth];
    __device__ __forceinline__ ExactStack view() { return ExactStack{node, ik, a, b}; }
};

// findNeighbors for one query by ONE thread, exactly nanoflann's traversal.  rd / ri: the KNNResultSet arrays (k
// entries).  Returns the number of results (min(k, size)), or -1 when the tree is deeper than the stack (fallback).
__device__ __forceinline__ int exact_knn_thread(const ExactTree &T, double qx, double qy, double qz, int k, double *rd,
                                                int *ri, const ExactStack st) {
    const int nn = *T.n_nodes;
    if (nn <= 0) return nn < 0 ? -1 : 0;
    const double q[3] = {qx, qy, qz};
    int count = 0;
    rd[k - 1] = DBL_MAX;  // KNNResultSet::init (:196-202)
    double dists[3] = {0.0, 0.0, 0.0};
    double mind = 0.0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {  // computeInitialDistances (:1296-1315)
        const double blo = T.root_bbox[2 * d], bhi = T.root_bbox[2 * d + 1];
        if (q[d] < blo) { dists[d] = (q[d] - blo) * (q[d] - blo); mind += dists[d]; }
        if (q[d] > bhi) { dists[d] = (q[d] - bhi) * (q[d] - bhi); mind += dists[d]; }
    }
    auto set_dist = [&](int idx, double v) {  // dists[] stays in registers: no dynamic indexing
        dists[0] = idx == 0 ? v : dists[0];
        dists[1] = idx == 1 ? v : dists[1];
        dists[2] = idx == 2 ? v : dists[2];
    };
    int sp = 0, node = 0;  // explicit stack of the recursion of searchLevel (:1729-1793)
    for (;;) {
        for (int idx = T.feat[node]; idx >= 0; idx = T.feat[node]) {  // descend along the best children
            const double val = idx == 0 ? qx : (idx == 1 ? qy : qz);
            const double diff1 = val - T.low[node], diff2 = val - T.high[node];
            int best, other;
            double cut;
            if ((diff1 + diff2) < 0) { best = T.child[node]; other = best + 1; cut = diff2 * diff2; }
            else { other = T.child[node]; best = other + 1; cut = diff1 * diff1; }
            if (sp >= kExactMaxDepth) return -1;
            st.node[sp] = other; st.ik[sp] = idx; st.a[sp] = cut; st.b[sp] = mind;
            ++sp;
            node = best;
        }
        {   // leaf (:1733-1751): worst distance cached at entry
            const double worst = rd[k - 1];
            const unsigned lf = T.left[node], rt = T.right[node];
            for (unsigned i = lf; i < rt; ++i) {
                const unsigned a = T.vind[i];
                const double dist = sq_dist(qx, qy, qz, T.x[a], T.y[a], T.z[a]);
                if (dist < worst) {  // KNNResultSet::addPoint (:219-246)
                    int j;
                    for (j = count; j > 0; --j) {
                        if (rd[j - 1] > dist) {
                            if (j < k) { rd[j] = rd[j - 1]; ri[j] = ri[j - 1]; }
                        } else {
                            break;
                        }
                    }
                    if (j < k) { rd[j] = dist; ri[j] = (int)a; }
                    if (count < k) ++count;
                }
            }
        }
        bool go = false;
        while (sp > 0) {  // unwind
            --sp;
            const int ik = st.ik[sp], idx = ik & 3;
            if (ik >> 2) { set_dist(idx, st.a[sp]); continue; }  // kind 1: dists[idx] = dst (:1791)
            const double cut = st.a[sp], dst = idx == 0 ? dists[0] : (idx == 1 ? dists[1] : dists[2]);
            const double m2 = st.b[sp] + cut - dst;
            if (m2 * 1.0f <= rd[k - 1]) {  // (epsError = 1 + eps, eps = 0: :1572,1780)
                set_dist(idx, cut);
                node = st.node[sp];
                st.ik[sp] = idx | 4; st.a[sp] = dst;  // restore once the other child returns
                ++sp;
                mind = m2;
                go = true;
                break;
            }
        }
        if (!go) break;
    }
    return count;
}

// findNeighbors for one query by ONE WAVEFRONT (every lane holds the same query): the same traversal, node data read once
// per wave (uniform addresses), the <= 10 points of a leaf scored by lanes 0..9 from the vAcc_-ordered planes (one
// contiguous run) and then offered to the result set ONE AT A TIME in leaf order, exactly as the sequential loop does
// (:1733-1751) -- the order decides which of several equidistant points is kept.  The KNNResultSet lives in lanes
// 0..k-1 (rd, ri sorted ascending); KNNResultSet::addPoint (:219-246) = count the entries <= dist (they form a prefix),
// shift the rest up by one lane.  `st`: this wave's stack in LDS.  Returns the number of results, -1 = tree unavailable.
struct ExactWaveStack {
    int node[kExactMaxDepth], ik[kExactMaxDepth];
    double a[kExactMaxDepth], b[kExactMaxDepth];
};
__device__ __forceinline__ int exact_knn_wave(const ExactTree &T, double qx, double qy, double qz, int k, double &rd, int &ri,
                                              ExactWaveStack *st) {
    const int lane = threadIdx.x & 63;
    const int nn = *T.n_nodes;
    rd = DBL_MAX;   // KNNResultSet::init (:196-202): dists[capacity - 1] = max; the other slots are never read before written
    ri = -1;
    if (nn <= 0) return nn < 0 ? -1 : 0;
    int count = 0;
    double dists[3] = {0.0, 0.0, 0.0};
    double mind = 0.0;
    const double q[3] = {qx, qy, qz};
#pragma unroll
    for (int d = 0; d < 3; ++d) {  // computeInitialDistances (:1296-1315)
        const double blo = T.root_bbox[2 * d], bhi = T.root_bbox[2 * d + 1];
        if (q[d] < blo) { dists[d] = (q[d] - blo) * (q[d] - blo); mind += dists[d]; }
        if (q[d] > bhi) { dists[d] = (q[d] - bhi) * (q[d] - bhi); mind += dists[d]; }
    }
    auto set_dist = [&](int idx, double v) {
        dists[0] = idx == 0 ? v : dists[0];
        dists[1] = idx == 1 ? v : dists[1];
        dists[2] = idx == 2 ? v : dists[2];
    };
    int sp = 0, node = 0;
    for (;;) {
        for (int idx = T.feat[node]; idx >= 0; idx = T.feat[node]) {
            const double val = idx == 0 ? qx : (idx == 1 ? qy : qz);
            const double diff1 = val - T.low[node], diff2 = val - T.high[node];
            int best, other;
            double cut;
            if ((diff1 + diff2) < 0) { best = T.child[node]; other = best + 1; cut = diff2 * diff2; }
            else { other = T.child[node]; best = other + 1; cut = diff1 * diff1; }
            if (sp >= kExactMaxDepth) return -1;
            if (lane == 0) { st->node[sp] = other; st->ik[sp] = idx; st->a[sp] = cut; st->b[sp] = mind; }
            ++sp;
            node = best;
        }
        {   // leaf: worst distance cached at entry
            const double worst = readlane_f64(rd, k - 1);
            const unsigned lf = T.left[node], rt = T.right[node], cnt = rt - lf;
            double dist = DBL_MAX;
            int pidx = -1;
            if ((unsigned)lane < cnt) {
                const unsigned i = lf + lane;
                pidx = (int)T.vind[i];
                dist = sq_dist(qx, qy, qz, T.plane(0)[i], T.plane(1)[i], T.plane(2)[i]);
            }
            for (unsigned e = 0; e < cnt; ++e) {
                const double de = readlane_f64(dist, (int)e);
                if (!(de < worst)) continue;                       // (NaN never enters, as in the reference)
                const int ae = __builtin_amdgcn_readlane(pidx, (int)e);
                const int pos = __popcll(__ballot(lane < count && rd <= de));   // after the existing equals
                const double up = __shfl_up(rd, 1);
                const int upi = __shfl_up(ri, 1);
                if (lane > pos && lane < k) { rd = up; ri = upi; }
                if (lane == pos && pos < k) { rd = de; ri = ae; }
                if (count < k) ++count;
            }
        }
        __threadfence_block();   // lane 0's stack writes are read by the whole wave
        bool go = false;
        while (sp > 0) {
            --sp;
            const int ik = st->ik[sp], idx = ik & 3;
            if (ik >> 2) { set_dist(idx, st->a[sp]); continue; }
            const double cut = st->a[sp], dst = idx == 0 ? dists[0] : (idx == 1 ? dists[1] : dists[2]);
            const double m2 = st->b[sp] + cut - dst;
            if (m2 * 1.0f <= readlane_f64(rd, k - 1)) {
                set_dist(idx, cut);
                node = st->node[sp];
                __threadfence_block();
                if (lane == 0) { st->ik[sp] = idx | 4; st->a[sp] = dst; }
                ++sp;
                mind = m2;
                go = true;
                break;
            }
        }
        if (!go) break;
    }
    return count;
}

}  // namespace amk

// host side: the batch pointers of a handle's bucketed index (amk_common.h: amk_kd)
inline amk::GridPtrs grid_ptrs(const amk_kd *kd) {
    return amk::GridPtrs{kd->gpt.p, kd->cell_start.p, kd->gparams.p, kd->cap, kd->ntiles};
}

// host side: the batch pointers of a handle's trees (amk_common.h: ExactStore)
inline amk::ExactPtrs amk::ExactStore::ptrs(const float *x, const float *y, const float *z, int cap, int scenes) const {
    ExactPtrs ep;
    std::memset(&ep, 0, sizeof ep);   // padding bytes too: step_frames.hip compares tables of these bytewise
    ep.x = x; ep.y = y; ep.z = z; ep.cap = cap;
    ep.vind = at<unsigned>(VIND); ep.left = at<unsigned>(LEFT); ep.right = at<unsigned>(RIGHT); ep.sa = at<unsigned>(SA); ep.sb = at<unsigned>(SB);
    ep.pc = at<float>(PC); ep.pstride = (size_t)scenes * cap;
    ep.feat = at<int>(FEAT); ep.child = at<int>(CHILD); ep.n_nodes = at<int>(NN);
    ep.low = at<double>(LOW); ep.high = at<double>(HIGH); ep.nbbox = at<double>(NBBOX); ep.root_bbox = at<double>(ROOT);
    ep.max_nodes = max_nodes;
    return ep;
}
inline amk::ExactPtrs amk_exact_ptrs(const amk_kd *kd) { return kd->exact.ptrs(kd->x.p, kd->y.p, kd->z.p, kd->cap, kd->n_scenes); }
