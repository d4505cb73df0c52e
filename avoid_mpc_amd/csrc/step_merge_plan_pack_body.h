// The body of step_merge_plan_pack_kernel and step_merge_plan_pack_map_kernel (step_frames.hip) -- included as TEXT into both, not
// a function: called through a __forceinline__ wrapper the same statements compiled to one more VGPR in three of the existing
// instantiations (CPL 4 and 16), and those kernels are to stay exactly the ones that were measured.  The including kernel
// provides the parameters of step_merge_plan_pack_kernel, EXACT, CPL, and
//   kMapTrees   constexpr bool: a keyframe map in AMK_TIES_NANOFLANN -- the snap's re-query goes through `trees`
//   trees       const MapTrees *: the pools' trees (kMapTrees), else unused
//   fe          const FrameExact *: the device table of a list of handles (EXACT && !kMapTrees), else unused
// and defines AMK_STEP_MERGE_PLAN_PACK_BODY around the #include: the text takes these names from the including scope, so it is no
// header for anybody else.  (tests/test_abi.py's resource-table and no-scratch checks are what hold the register figures.)
#ifndef AMK_STEP_MERGE_PLAN_PACK_BODY
#error "step_merge_plan_pack_body.h is the body of step_frames.hip's two merge kernels; include it nowhere else"
#endif
    // One workgroup per scene: nw = blockDim.x / 64 wavefronts (4; 1 when a frame is in AMK_TIES_NANOFLANN mode).  Wavefront 0
    // decides PlanWapionts; the snapped point's re-queries (one search per frame) and the per-reference-point merges are dealt
    // round-robin to the wavefronts, the rows that take QueryNearest's fast path are copied by all threads at once.
    const int s = blockIdx.x, lane = threadIdx.x & 63, tid = threadIdx.x, nthr = blockDim.x;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
    if (done[s]) return;
    // frames this scene's map holds: every loop below runs over them only (an absent frame contributes nothing to any query, and the
    // candidate ids f K + j of the others do not move).  A map with room for 101 frames holds ~6 on a flight; each pass over
    // absent frames is a chain of dependent loads (fmap, then the size) per frame.
    int F = fs.n;
    if (fs.fmap) {
        int hi = 0;
        for (int f0 = 0; f0 < fs.n; f0 += 64) {
            const int f = f0 + lane;
            const unsigned long long b = __ballot(f < fs.n && fs.fmap[(size_t)f * fs.S + s] >= 0);
            if (b) hi = f0 + 64 - __clzll((long long)b);
        }
        F = hi;
    }
    __shared__ GridWaveLds wl[4];
    __shared__ int cntq[AMK_MAX_HORIZON];
    __shared__ int sh_safety, sh_snap;
    __shared__ double sh_e[3];
    double *rp = ref_path + (size_t)s * N * SD;
    const double *Ts = Twc ? Twc + (size_t)s * 16 : nullptr;
    auto in_frame = [&](double x, double y, double z) { return Ts ? pt_in_frame(Ts, cam, x, y, z) : true; };
    const int n_obs0 = fs.n_obs(0, s);
    // ---- PlanWapionts (:259-281) for reference point 0
    if (w == 0) {
        const double p0x = rp[0], p0y = rp[1], p0z = rp[2];
        // GetNearestDistance: 1-NN per frame exists iff the frame holds more than one point (lane = frame)
        unsigned long long d2n_key = ~0ull;
        for (int f0 = 0; f0 < F; f0 += 64) {
            const int f = f0 + lane;
            if (f < F && fs.n_obs(f, s) > 1) {
                const double d = fb.knn_d2[(((size_t)f * S + s) * N) * K];
                // fmin semantics: a NaN distance is ignored; d >= 0, so the bit pattern orders like the value
                if (d == d) { const unsigned long long k64 = (unsigned long long)__double_as_longlong(d); d2n_key = k64 < d2n_key ? k64 : d2n_key; }
            }
        }
        d2n_key = wave_min_u64(d2n_key);
        const double d2n = d2n_key == ~0ull ? DBL_MAX : __longlong_as_double((long long)d2n_key);
        int is_safety = 1, snap = 0;
        if (!(sqrt(d2n) > safety_distance)) {
            // QueryNearest(p1, 1, ..., queryEdge = true): fast path iff the current edge cloud holds >= 1 point and p1 is in frame
            int bf = -1;
            if (fs.n_edge(0, s) >= 1 && in_frame(p0x, p0y, p0z)) {
                if (fs.n_edge(0, s) > 1 && fb.edge_d2[s] < DBL_MAX) bf = 0;
            } else {
                // k' = min(1, size_f): a result iff size_f > 1; ties keep the earlier frame (lane = frame; strict < in frame order)
                unsigned long long bk = ~0ull;
                int mf = 0x7fffffff;
                for (int f0 = 0; f0 < F; f0 += 64) {
                    const int f = f0 + lane;
                    if (f < F && fs.n_edge(f, s) > 1) {
                        const double d = fb.edge_d2[(size_t)f * S + s];
                        if (d < DBL_MAX) {
                            const unsigned long long k64 = (unsigned long long)__double_as_longlong(d);
                            if (k64 < bk) { bk = k64; mf = f; }
                        }
                    }
                }
                const unsigned long long wb = wave_min_u64(bk);
                if (wb != ~0ull) {
                    int win = bk == wb ? mf : 0x7fffffff;
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) win = min(win, __shfl_xor(win, off));
                    bf = win;
                }
            }
            if (bf < 0) {
                is_safety = 0;
            } else {
                snap = 1;
                const float *ep = fb.edge_pt + 3 * ((size_t)bf * S + s);
                if (lane == 0) { sh_e[0] = (double)ep[0]; sh_e[1] = (double)ep[1]; sh_e[2] = (double)ep[2]; }
            }
        }
        if (lane == 0) { sh_safety = is_safety; sh_snap = snap; flags[4 * s + 0] = is_safety; }
    }
    __syncthreads();
    const int is_safety = sh_safety;
    if (sh_snap) {
        const double ex = sh_e[0], ey = sh_e[1], ez = sh_e[2];
        for (int f = w; f < F; f += nw) {  // the snapped point is what ProcessWaypoints queries next (:210-215)
            double gld;
            int gli, glpos;
            const int mf = fs.scene_of(f, s);
            if (mf >= 0) {   // (wave-uniform)
                const GridScene gs = fs.obs_scene(f, mf);
                grid_knn(gs, ex, ey, ez, K, gld, gli, glpos, &wl[w]);
                if (lane < K) {
                    const float4 rec = gs.pt[glpos];
                    store_nbr(fb.knn_pts, fb.knn_d2, ((size_t)f * S + s) * N * K + lane, gli != kNoIndex, gld, rec.x, rec.y,
                              rec.z);
                }
            }
            if constexpr (EXACT && kMapTrees) {   // the pool scene's tree, by this wavefront (no barrier: nw = 4)
                __shared__ ExactWaveStack xst[4];
                if (mf >= 0) {
                    // (the tree's fifteen pointers in VECTOR registers: derived from a scalar mf they were live in SGPRs across the
                    // traversal, next to this kernel's own uniform state, and the spills reserved scratch memory for the kernel)
                    int mv = mf;
                    asm volatile("" : "+v"(mv));
                    const ExactTree XT = trees->obs_pool.scene(mv);
                    double xd;
                    int xi;
                    const int got = exact_knn_wave(XT, ex, ey, ez, K, xd, xi, &xst[w]);
                    if (got >= 0 && lane < K) {
                        const bool ok = lane < got;
                        store_nbr(fb.knn_pts, fb.knn_d2, ((size_t)f * S + s) * N * K + lane, ok, xd, ok ? XT.x[xi] : 0.f, ok ? XT.y[xi] : 0.f,
                                  ok ? XT.z[xi] : 0.f);
                    }
                }
            } else if constexpr (EXACT) {   // (nw == 1: the barriers below are this wavefront's own)
                __syncthreads();
                if (mf >= 0 && fe->use_obs[f]) {  // AMK_TIES_NANOFLANN frame
                    exact_requery(fe->obs[f].scene(s), ex, ey, ez, K, fb.knn_pts, fb.knn_d2, ((size_t)f * S + s) * N);
                    __syncthreads();
                }
            }
        }
        if (tid == 0) { rp[0] = ex; rp[1] = ey; rp[2] = ez; }
    }
    __threadfence_block();
    __syncthreads();
    // ---- ProcessWaypoints' queries (:204-215): fast path or merge over the frames, per reference point
    // QueryNearestWithCurFrame (:254-275, 339-345) for the reference points the current image sees (lane = reference point)
    bool inf = false;
    if (lane < N) inf = n_obs0 >= K && in_frame(rp[lane * SD], rp[lane * SD + 1], rp[lane * SD + 2]);
    const unsigned long long fast = __ballot(inf);
    {
        const int cnt_fast = n_obs0 > K ? K : 0;      // kd_tree_two.h:119-124
        const size_t base = (size_t)s * N * K;        // frame 0's rows of this scene = the output rows' layout
        for (int e = tid; e < N * K; e += nthr) {
            const int i = e / K;
            if ((fast >> i) & 1ull) {
                knn_d2[base + e] = fb.knn_d2[base + e];
                for (int c = 0; c < 3; ++c) knn_pts[(base + e) * 3 + c] = fb.knn_pts[(base + e) * 3 + c];
            }
        }
        if (w == 0 && inf) cntq[lane] = cnt_fast;
    }
    for (int i = w; i < N; i += nw) {
        if ((fast >> i) & 1ull) continue;
        const size_t orow = ((size_t)s * N + i) * K;
        // QueryNearestThreadWorker over mVecQueryVector (:276-321) + sort (:371): candidate c = f * K + j
        const int ncand = F * K;
        int cnt = 0;
        if constexpr (CPL > 0) {
        unsigned long long key[CPL];
#pragma unroll
        for (int r = 0; r < CPL; ++r) {
            const int c = lane + 64 * r;
            key[r] = ~0ull;
            if (c < ncand) {
                const int f = c / K, jj = c - f * K;
                if (fs.n_obs(f, s) > K) {  // k' = min(K, size_f) results exist iff size_f > k'
                    const double d = fb.knn_d2[(((size_t)f * S + s) * N + i) * K + jj];
                    if (d < DBL_MAX) key[r] = (unsigned long long)__double_as_longlong(d);  // d >= 0: order-preserving
                }
            }
        }
        for (int m = 0; m < K; ++m) {  // K rounds of "smallest remaining (distance, candidate id)"
            unsigned long long loc = ~0ull;
#pragma unroll
            for (int r = 0; r < CPL; ++r) loc = key[r] < loc ? key[r] : loc;
            const unsigned long long best = wave_min_u64(loc);
            if (best == ~0ull) break;
            int myc = 0x7fffffff;  // lowest candidate id holding `best`
#pragma unroll
            for (int r = CPL - 1; r >= 0; --r)
                if (key[r] == best) myc = lane + 64 * r;
            int win = myc;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) win = min(win, __shfl_xor(win, off));
            if (myc == win) {
                const int f = win / K, jj = win - f * K;
                const size_t irow = (((size_t)f * S + s) * N + i) * K + jj;
                knn_d2[orow + m] = __longlong_as_double((long long)best);
                for (int c = 0; c < 3; ++c) knn_pts[(orow + m) * 3 + c] = fb.knn_pts[irow * 3 + c];
#pragma unroll
                for (int r = 0; r < CPL; ++r)
                    if (lane + 64 * r == win) key[r] = ~0ull;
            }
            ++cnt;
        }
        } else {
        // wide map: the same K rounds, the candidates re-read from the raw rows every round (L2-resident: F K doubles per
        // reference point), a lane's taken candidates remembered as bits (candidate lane + 64 r = bit r; F K <= 64 x 128)
        unsigned long long taken0 = 0ull, taken1 = 0ull;
        for (int m = 0; m < K; ++m) {
            unsigned long long loc = ~0ull;
            int myc = 0x7fffffff;
            for (int r = 0; lane + 64 * r < ncand; ++r) {
                if ((r < 64 ? taken0 >> r : taken1 >> (r - 64)) & 1ull) continue;
                const int c = lane + 64 * r;
                const int f = c / K, jj = c - f * K;
                if (fs.n_obs(f, s) > K) {
                    const double d = fb.knn_d2[(((size_t)f * S + s) * N + i) * K + jj];
                    if (d < DBL_MAX) {
                        const unsigned long long k64 = (unsigned long long)__double_as_longlong(d);
                        if (k64 < loc) { loc = k64; myc = c; }   // (ascending r: the lowest candidate id among equal keys of this lane)
                    }
                }
            }
            const unsigned long long best = wave_min_u64(loc);
            if (best == ~0ull) break;
            int win = loc == best ? myc : 0x7fffffff;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) win = min(win, __shfl_xor(win, off));
            if (loc == best && myc == win) {
                const int f = win / K, jj = win - f * K;
                const size_t irow = (((size_t)f * S + s) * N + i) * K + jj;
                knn_d2[orow + m] = __longlong_as_double((long long)best);
                for (int c = 0; c < 3; ++c) knn_pts[(orow + m) * 3 + c] = fb.knn_pts[irow * 3 + c];
                const int r = win >> 6;
                if (r < 64) taken0 |= 1ull << r; else taken1 |= 1ull << (r - 64);
            }
            ++cnt;
        }
        }
        if (lane == 0) cntq[i] = cnt;
    }
    __threadfence_block();
    __syncthreads();
    pack_ref_states(tid, nthr, s, N, K, nref, iter, max_iter, speed, T, safety_distance, is_safety,
                    [&](int i) { return cntq[i]; }, state_quad, pos_x, rp, knn_pts, knn_d2, ref_states, done);
