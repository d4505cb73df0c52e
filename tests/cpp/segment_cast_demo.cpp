// Segment cast through the reference-shaped C++ adapters: KDTreeTwo::SegmentCast and FrameKDMap::QuerySegmentCast
// (include/avoid_mpc_amd/kd_tree_two.hpp, frame_kd_map.hpp); driven by tests/test_kd_segment_cast_abi.py, which compares the
// numbers written here with the brute force of tests/_cast.py.
//   segment_cast_demo <in.bin> <out.bin>
// in.bin : int32 n, nl ; double radius_sq ; float cloud[n*3] ; double legs[nl*6]  (a then b)
// out.bin: per leg  int32 hit, index ; double t ; float pt[3]     (the whole cloud as one tree; index -1 and pt 0 without a contact)
//          per leg  int32 hit ; double t ; double pt[3]           (a map of two frames: second half, first half)
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
    int hdr[2];
    double r2;
    rd(f, hdr, 2);
    rd(f, &r2, 1);
    const int n = hdr[0], nl = hdr[1];
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
        double t = -1.0;
        const int hit = tree.SegmentCast(l[0], l[1], l[2], l[3], l[4], l[5], r2, t) ? 1 : 0;
        const int index = hit ? tree.indices[0] : -1;
        float p[3] = {0.f, 0.f, 0.f};
        if (hit) { p[0] = (float)tree.closest_pts[0].x; p[1] = (float)tree.closest_pts[0].y; p[2] = (float)tree.closest_pts[0].z; }
        wr(o, &hit, 1);
        wr(o, &index, 1);
        wr(o, &t, 1);
        wr(o, p, 3);
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
        Vector3d pt(0.0, 0.0, 0.0);
        double t = -1.0;
        const int hit = map.QuerySegmentCast(Vector3d(l[0], l[1], l[2]), Vector3d(l[3], l[4], l[5]), r2, pt, t) ? 1 : 0;
        const double p[3] = {vx(pt), vy(pt), vz(pt)};
        wr(o, &hit, 1);
        wr(o, &t, 1);
        wr(o, p, 3);
    }
    fclose(o);
    return 0;
}
