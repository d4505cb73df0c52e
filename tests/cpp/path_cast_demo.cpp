// Path cast through the reference-shaped C++ adapters: KDTreeTwo::PathCast and FrameKDMap::QueryPathCast
// (include/avoid_mpc_amd/kd_tree_two.hpp, frame_kd_map.hpp); driven by tests/test_kd_path_cast_abi.py, which compares the
// numbers written here with the restatement of tests/_path_cast.py.
//   path_cast_demo <in.bin> <out.bin>
// in.bin : int32 n, n_paths, n_points ; double radius_sq ; float cloud[n*3] ; double paths[n_paths*n_points*3]
// out.bin: per path  int32 stop, leg, index ; double t, free ; float pt[3]   (the whole cloud as one tree; index -1, pt 0 unless stop 1)
//          per path  int32 stop, leg ; double t, free ; double pt[3]         (a map of two frames: second half, first half)
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
    double r2;
    rd(f, hdr, 3);
    rd(f, &r2, 1);
    const int n = hdr[0], np = hdr[1], P = hdr[2];
    std::vector<float> cl((size_t)n * 3);
    std::vector<double> paths((size_t)np * P * 3);
    rd(f, cl.data(), cl.size());
    rd(f, paths.data(), paths.size());
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
    for (int i = 0; i < np; ++i) {
        int leg = -9;
        double t = -1.0, free_dist = -1.0;
        const int stop = tree.PathCast(&paths[(size_t)i * P * 3], P, r2, leg, t, free_dist);
        const int index = stop == 1 ? tree.indices[0] : -1;
        float p[3] = {0.f, 0.f, 0.f};
        if (stop == 1) { p[0] = (float)tree.closest_pts[0].x; p[1] = (float)tree.closest_pts[0].y; p[2] = (float)tree.closest_pts[0].z; }
        wr(o, &stop, 1);
        wr(o, &leg, 1);
        wr(o, &index, 1);
        wr(o, &t, 1);
        wr(o, &free_dist, 1);
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
    for (int i = 0; i < np; ++i) {
        std::vector<Vector3d> path;
        for (int j = 0; j < P; ++j) {
            const double *q = &paths[((size_t)i * P + j) * 3];
            path.emplace_back(q[0], q[1], q[2]);
        }
        Vector3d pt(0.0, 0.0, 0.0);
        int leg = -9;
        double t = -1.0, free_dist = -1.0;
        const int stop = map.QueryPathCast(path, r2, leg, t, free_dist, pt);
        const double p[3] = {vx(pt), vy(pt), vz(pt)};
        wr(o, &stop, 1);
        wr(o, &leg, 1);
        wr(o, &t, 1);
        wr(o, &free_dist, 1);
        wr(o, p, 3);
    }
    fclose(o);
    return 0;
}
