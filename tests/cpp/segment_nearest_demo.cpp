// Segment nearest through the reference-shaped C++ adapters: KDTreeTwo::SegmentNearest and FrameKDMap::QuerySegmentNearest
// (include/avoid_mpc_amd/kd_tree_two.hpp, frame_kd_map.hpp); driven by tests/test_kd_segment_nearest_abi.py, which compares the
// numbers written here with the brute force of tests/_segment_nearest.py.
//   segment_nearest_demo <in.bin> <out.bin>
// in.bin : int32 n, nl, k ; float cloud[n*3] ; double legs[nl*6]  (a then b)
// out.bin: per leg  int32 count, c ; int32 indices[c] ; double d2[c] ; double t[c] ; float pts[c*3]   (the whole cloud as one tree)
//          per leg  int32 count, c ; double d2[c] ; double t[c] ; double pts[c*3]                     (a map of two frames: second half, first half)
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "avoid_mpc_amd/frame_kd_map.hpp"

using namespace avoid_mpc_amd;

struct Cloud {  // stands where pcl::PointCloud<pcl::PointXYZ> stands in the reference
    std::vector<PointXYZ> points;
};

template <class T>
static void rd(FILE *f, T *p, size_t n) {
    if (fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
}
template <class T>
static void wr(FILE *f, const T *p, size_t n) { fwrite(p, sizeof(T), n, f); }

int main(int argc, char **argv) {
    if (argc < 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 1;
    int hdr[3];
    rd(f, hdr, 3);
    const int n = hdr[0], nl = hdr[1], k = hdr[2];
    std::vector<float> cl((size_t)n * 3);
    std::vector<double> legs((size_t)nl * 6);
    rd(f, cl.data(), cl.size());
    rd(f, legs.data(), legs.size());
    fclose(f);
    auto part = [&](int i0, int i1) {
        auto c = std::make_shared<Cloud>();
        for (int i = i0; i < i1; ++i) c->points.emplace_back(cl[3 * i], cl[3 * i + 1], cl[3 * i + 2]);
        return c;
    };
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 1;

    KDTreeTwo<double> tree;
    tree.InitializeNew(part(0, n));
    for (int i = 0; i < nl; ++i) {
        const double *l = &legs[6 * i];
        const int count = (int)tree.SegmentNearest(l[0], l[1], l[2], l[3], l[4], l[5], k);
        const int c = (int)tree.indices.size();
        wr(o, &count, 1);
        wr(o, &c, 1);
        wr(o, tree.indices.data(), c);
        wr(o, tree.squared_distances.data(), c);
        wr(o, tree.segment_t.data(), c);
        for (int j = 0; j < c; ++j) {
            const float p[3] = {tree.closest_pts[j].x, tree.closest_pts[j].y, tree.closest_pts[j].z};
            wr(o, p, 3);
        }
    }

    // mVecQueryVector = [current frame, every keyframe but the newest] (FrameKDMap.cpp:64-74): [second half, first half]
    FrameKDMap map;
    auto first = part(0, n / 2), second = part(n / 2, n), edge = part(0, 8);
    map.AddVertex(first, edge);
    map.InsertKeyFrame();
    map.AddVertex(first, edge);
    map.InsertKeyFrame();
    map.AddVertex(second, edge);
    for (int i = 0; i < nl; ++i) {
        const double *l = &legs[6 * i];
        std::vector<Vector3d> pts;
        std::vector<double> d2, t;
        const int count = (int)map.QuerySegmentNearest(Vector3d(l[0], l[1], l[2]), Vector3d(l[3], l[4], l[5]), k, pts, d2, t);
        const int c = (int)d2.size();
        wr(o, &count, 1);
        wr(o, &c, 1);
        wr(o, d2.data(), c);
        wr(o, t.data(), c);
        for (int j = 0; j < c; ++j) {
            const double p[3] = {vx(pts[j]), vy(pts[j]), vz(pts[j])};
            wr(o, p, 3);
        }
    }
    fclose(o);
    return 0;
}
