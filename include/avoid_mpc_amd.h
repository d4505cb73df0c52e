/* avoid_mpc_amd.h -- C ABI of the MI355X-native Avoid-MPC hot path.
 *
 * One shared library (avoid_mpc_amd/libavoid_mpc_amd.so, HIP for gfx950).  Plain pointers and
 * sizes only; every `d_` pointer is DEVICE memory on the current HIP device, every `h_` pointer is
 * host memory; `stream` is a hipStream_t passed as void* (NULL = the default stream).  All entry
 * points return an amk_status and are re-entrant per handle (no global state; the reference's
 * KDTreeTwo keeps results in members and is not re-entrant, AM/include/kd_tree_two.h:109-111).
 *
 * A handle holds a BATCH of S independent objects ("scenes"): scene s of an amk_kd is one
 * KDTreeTwo<double>, scene s of an amk_mpc is one ObstacleAvoidanceMPC.  S = 1 reproduces the
 * reference's single-robot use; S >> 1 is how the GPU is filled.
 *
 * Reference interfaces replaced (AM = roswrapper/ros/src/avoid_mpc in the reference tree):
 *   amk_kd_*     AM/include/kd_tree_two.h:53-144   (KDTreeTwo<double>)  and, through it,
 *                AM/include/nanoflann_two.hpp:1518-1541,1563-1586 (buildIndex / findNeighbors)
 *   amk_mpc_*    AM/include/HighLvlMpc.h:4-33, AM/src/HighLvlMpc.cpp:5-137 (ObstacleAvoidanceMPC)
 *                and the plugin it loads (AM/tools/mpc_obstacle_casadi.py:51-242,338-357)
 *   amk_step_*   AM/src/AvoidanceStateMachine.cpp:204-281,322-355 (TASK branch of Step) with
 *                AM/src/FrameKDMap.cpp:254-275,322-427 (QueryNearest / GetNearestDistance)
 * C++ adapters with the reference's class names/signatures: the .hpp files under include/avoid_mpc_amd/.
 */
#ifndef AVOID_MPC_AMD_H
#define AVOID_MPC_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

typedef enum amk_status {
    AMK_OK = 0,
    AMK_ERR_INVALID_ARG = 1, /* NULL handle, k < 0, size mismatch ...                           */
    AMK_ERR_HIP = 2,         /* a HIP runtime call failed; see amk_last_hip_error()              */
    AMK_ERR_NO_DEVICE = 3,   /* no gfx950 device visible: there is NO CPU fallback               */
    AMK_ERR_UNSUPPORTED = 4, /* e.g. k > AMK_MAX_K, N > AMK_MAX_HORIZON                          */
    AMK_ERR_TIMEOUT = 5      /* amk_shard_wait: a collective did not finish in time               */
} amk_status;

#define AMK_MAX_K 64        /* neighbours per query (reference uses 1, 3, 8, <=10)               */
#define AMK_MAX_QUERIES 64  /* queries per scene per call (reference: N <= 30 per outer pass)    */
#define AMK_MAX_HORIZON 32  /* N = int(T/dt); reference default 30                               */
#define AMK_S_DIM 10        /* [px,py,pz,yaw,vx,vy,vz,ax,ay,az]  mpc_obstacle_casadi.py:41-46    */
#define AMK_U_DIM 4         /* [ax_cmd,ay_cmd,az_cmd,yaw_dot]    mpc_obstacle_casadi.py:75       */
#define AMK_MPC_DEFAULT_MAX_ITER 100 /* iteration cap of this library's interior-point method (see amk_mpc_create) */
#define AMK_MAX_BUDGET_ROUNDS 16    /* amk_mpc_set_solve_budget: budgeted rounds of a control step */

int amk_version(void);
const char *amk_status_string(int status);
int amk_last_hip_error(void); /* hipError_t of the last failing HIP call on this thread          */
int amk_device_count(void);

/* ------------------------------------------------------------------------------------------ */
/* KD index: batch of KDTreeTwo<double>                                    kd_tree_two.h:53-144 */
/* ------------------------------------------------------------------------------------------ */
typedef struct amk_kd amk_kd;

/* KDTreeTwo() x n_scenes.  max_points = capacity per scene.                                      */
int amk_kd_create(int n_scenes, int max_points, amk_kd **out);
int amk_kd_destroy(amk_kd *kd);

/* InitializeNew(cloud) for every scene (kd_tree_two.h:76-78,88-106): the handle COPIES the points
 * whose x is not NaN (order preserved, :96-101) and builds its index.  Scene s reads
 * d_xyz[s*scene_stride + i*point_stride + {0,1,2}], i < counts[s]; point_stride = 3 (packed) or
 * 4 (pcl::PointXYZ's 16-byte layout).  d_counts == NULL means every scene has max_points.       */
int amk_kd_build(amk_kd *kd, const float *d_xyz, int point_stride, long long scene_stride,
                 const int *d_counts, void *stream);

/* FrameKDMap::AddVertex's two InitializeNew calls (obstacle cloud + edge cloud of one depth frame, FrameKDMap.cpp:44-47) as
 * ONE launch: both clouds packed [S][max_points of the handle][point_stride]; results identical to two amk_kd_build calls. */
int amk_kd_build_pair(amk_kd *obstacle, const float *d_xyz, const int *d_counts, amk_kd *edge, const float *d_edge_xyz,
                      const int *d_edge_counts, int point_stride, void *stream);

/* cloud.pts.size() per scene after the NaN-x filter (synchronises the stream).                   */
int amk_kd_sizes(amk_kd *kd, int *h_sizes, void *stream);

/* SearchForNearest(x,y,z,n) (kd_tree_two.h:108-133) for n_queries query points per scene.
 *   d_queries  [S][n_queries][3] double
 *   d_indices  [S][n_queries][k] int     -> KDTreeTwo::indices            (may be NULL)
 *   d_sqdist   [S][n_queries][k] double  -> KDTreeTwo::squared_distances  (may be NULL)
 *   d_pts      [S][n_queries][k][3] float-> KDTreeTwo::closest_pts        (may be NULL)
 *   d_counts   [S][n_queries]    int     -> number of results, reproducing :119-124 exactly:
 *                                           size < k -> size ; size > k -> k ; size == k -> 0
 * Results ascend in squared distance; equal distances order by index (nanoflann orders ties by
 * tree-traversal order, nanoflann_two.hpp:224-229 -- see DESIGN.md "tie policy").  Slots beyond
 * the count hold index -1 / distance DBL_MAX / point (0,0,0).  Distances are the IEEE
 * left-to-right fp64 sums of kd_tree_two.h:24-27 with no FMA contraction.                       */
int amk_kd_search(amk_kd *kd, const double *d_queries, int n_queries, int k, int *d_indices,
                  double *d_sqdist, float *d_pts, int *d_counts, void *stream);

/* Non-finite coordinates (NaN, +-inf, values whose squared distance overflows) -- what amk_kd_build, amk_kd_build_pair,
 * amk_kd_search, amk_kd_tie_flags and their host variants do with them; tests/test_nonfinite_gpu.py asserts every sentence.
 *   * A point whose x is NaN is dropped by the build (as above).  EVERY other point is kept, keeps its index and counts in
 *     amk_kd_sizes -- a NaN y or z and an infinity in any coordinate included, as in the reference (kd_tree_two.h:99 tests x).
 *   * A kept point is USABLE for a query iff its squared distance, evaluated in fp64 as the adaptor does
 *     (((qx - x)^2 + (qy - y)^2) + (qz - z)^2), is < DBL_MAX: false for NaN, for inf and for a sum that overflows (a query
 *     coordinate of 1e200).  An unusable point is never returned, by the bucketed index and by the streaming scan alike, in
 *     any tie order.  A finite float is usable for every float query (< 1.4e78): a coordinate of FLT_MAX is returned when
 *     nothing is nearer.  A query at 1e150 is answered normally (squares near 1e300).
 *   * d_counts follows the size rule above whatever is usable; the slots beyond the usable points hold -1 / DBL_MAX / (0,0,0).
 *     So a query with a NaN or infinite coordinate gets `count` empty slots, and no tie flag.  This is the one place where
 *     the choice changes control flow against the reference as restated: amk_step_batch re-plans when the nearest squared
 *     distance of a reference point is within the safety distance, and an empty slot's DBL_MAX is not, where the restated
 *     reference's 0.0 is -- a scene whose solve failed (NaN predicted states) makes 1 solve here, 3 in oracle/step_oracle.c.
 *   * The reference differs in those slots: with zero-initialised result buffers it hands out index 0 / distance 0.0 /
 *     point 0 in every slot the traversal did not fill and DBL_MAX in the last (oracle/_ref, recorded in tests/golden/
 *     kd_ref_golden.npz; its own buffers are uninitialised, kd_tree_two.h:114-115).  And for a cloud that KEEPS a non-finite
 *     point it has no behaviour at all: nanoflann's divideTree compares coordinates with split planes, and on most such
 *     clouds the build ends in a segmentation fault (200 NaN y + 200 NaN z, 50 inf y / -inf z, 50 +inf x, all but five
 *     NaN y, each in 3000 points), on others it builds and then prunes wrongly.  There this library's answer is the rule
 *     above, whose plain restatement is tests/_oracle.py kd_brute_np.
 *   * AMK_TIES_NANOFLANN / AMK_TIES_AUTO: a scene whose cloud keeps a point with a NaN or infinite coordinate does not get
 *     the reference-shaped tree (decided on the device, per scene, at the point where the build would start):
 *     amk_kd_exact_status reports AMK_EXACT_GAVE_UP, the bucketed index answers by the rule above, equal distances in
 *     cloud-index order.  The other scenes of the batch are unaffected.                                                   */

/* Tie visibility.  For every query: d_tie_flags[s][q] = 1 when, among the k + 1 nearest points, two are at exactly the same
 * squared distance (two returned neighbours, or the k-th returned one and the best rejected one), else 0.  nanoflann keeps
 * the first VISITED of equal distances (KNNResultSet::addPoint, nanoflann_two.hpp:219-246; traversal order), this library
 * the lowest index: with flag 0 indices and neighbour set are identical to the reference's, with flag 1 only the distance
 * list is guaranteed identical (DESIGN.md "tie policy").  Queries are read at d_queries[(s*n_queries + q)*query_stride
 * + {0,1,2}] (query_stride 3 = packed; 10 = the position part of mRefPath).  k + 1 <= AMK_MAX_K.                     */
int amk_kd_tie_flags(amk_kd *kd, const double *d_queries, int query_stride, int n_queries, int k, int *d_tie_flags,
                     void *stream);

/* Tie ORDER.  AMK_TIES_LOWEST_INDEX (default): equal squared distances order by cloud index.  AMK_TIES_NANOFLANN: the
 * handle also builds the reference's own tree (divideTree / middleSplit_ / planeSplit, leaf size 10: nanoflann_two.hpp:
 * 1055-1106,1197-1294, kd_tree_two.h:68) at every amk_kd_build / keyframe rebuild and amk_kd_search answers by nanoflann's
 * own traversal (searchLevel + KNNResultSet, :1729-1793,219-246): index lists identical to the reference's on ANY cloud,
 * ties included.  Costs milliseconds per build (level-synchronous, one wavefront per tree node) where the bucketed index
 * takes a fraction of one: meant for the reference's real frame sizes (<= 3072 points, quantised edge clouds), set it
 * before amk_kd_build.  amk_step_batch and amk_step_batch_frames honour it (queries and the edge snap's
 * re-query then go through nanoflann's traversal too).  A scene whose tree would exceed the node capacity
 * (cap / 2 + 64) or a traversal depth of 48 -- pathological data -- keeps the bucketed index's answer.  The mode takes effect at the NEXT
 * build: a search between amk_kd_set_tie_order(NANOFLANN) and that build still answers from the bucketed index (the
 * handle tracks whether its exact tree belongs to the cloud it currently holds).
 * AMK_TIES_AUTO: the answers of AMK_TIES_NANOFLANN at close to the default's price when ties are rare.  The bucketed index
 * answers every query with k + 1 neighbours and tests the k + 1 for two equal squared distances (the test of amk_kd_tie_flags);
 * only a scene with such a query gets the reference's tree -- built on the device, behind the search that saw the tie, once per
 * cloud -- and only the tied queries are answered again by nanoflann's traversal.  Without a tie among the k + 1 nearest the
 * two orders give the same list, so indices, sqdist, pts and counts equal those of AMK_TIES_NANOFLANN bit for bit (a scene
 * whose tree is given up or too deep keeps the bucketed answer for its tied queries, as there).  Nothing synchronises with the
 * host: the search enqueues the lazy build and the re-answer unconditionally, they return at once where nothing tied.  k + 1 <=
 * AMK_MAX_K (else AMK_ERR_UNSUPPORTED).  The tree's memory is allocated by amk_kd_set_tie_order(AUTO), never by a search or a
 * step; the mode takes effect at the NEXT build; every index build of the handle forgets the trees of the previous cloud.
 * Searches of ONE handle in this mode share its tie flags and must not overlap on different streams.  amk_step_batch (and
 * amk_pipeline_* without keyframes) honours the mode on either handle: the N obstacle queries, the edge query and the edge
 * snap's re-query, in every pass, with the result of the same step in AMK_TIES_NANOFLANN mode (K + 1 <= AMK_MAX_K).  The
 * multi-frame paths do NOT support it: amk_step_batch_frames with a handle in this mode, amk_kd_keyframe_sweep with either
 * handle in it (the sweep compacts a cloud in place: a lazily built tree would go stale) and a pipeline slot with a keyframe
 * map or keyframe handles whose amk_pipeline_kd handles are in it return AMK_ERR_UNSUPPORTED before launching anything;
 * the keyframe map has a mode of its own, amk_kfmap_set_tie_order (AMK_TIES_LOWEST_INDEX or AMK_TIES_NANOFLANN for all of its
 * frames; no AMK_TIES_AUTO: lazily built trees under a sweep that compacts clouds in place would need per-pool-scene tie flags
 * and staleness rules of their own).  A handle in scan mode ignores the mode.                                              */
#define AMK_TIES_LOWEST_INDEX 0
#define AMK_TIES_NANOFLANN 1
#define AMK_TIES_AUTO 2
int amk_kd_set_tie_order(amk_kd *kd, int mode);
/* Whether AMK_TIES_NANOFLANN holds for a scene: d_status[s] (device, [n_scenes], stream-ordered after the build it describes)
 *   AMK_EXACT_OFF      (-1) the mode is off, or no build has run since it was switched on: the bucketed index answers (by design)
 *   AMK_EXACT_IN_USE   ( 0) the reference-shaped tree answers every search of the scene: nanoflann's index lists, ties included
 *   AMK_EXACT_GAVE_UP  ( 1) the build gave the tree up (node capacity cap / 2 + 64, its ring of open nodes, or its watchdog):
 *                           the bucketed index answers -- same distances, equal distances in cloud-index order
 *   AMK_EXACT_TOO_DEEP ( 2) the tree exists but is deeper than the traversal stack (48 levels): queries that would descend past
 *                           it are answered by the bucketed index, the others by the tree
 *   AMK_EXACT_NOT_NEEDED (3) AMK_TIES_AUTO only: no query of the scene has tied since the last build, so no tree exists and the
 *                           bucketed index has answered everything -- which is the reference's answer.  In AMK_TIES_AUTO the
 *                           values 0 / 1 / 2 describe the scenes whose tree has been built for the current cloud.
 * A caller that NEEDS the reference's index lists checks this after the build; 1 and 2 are pathological data (never seen on
 * depth-derived or synthetic clouds; tests force them with a shrunken ring and a geometric point sequence).              */
#define AMK_EXACT_OFF (-1)
#define AMK_EXACT_IN_USE 0
#define AMK_EXACT_GAVE_UP 1
#define AMK_EXACT_TOO_DEEP 2
#define AMK_EXACT_NOT_NEEDED 3
int amk_kd_exact_status(amk_kd *kd, int *d_status, void *stream);
int amk_kd_exact_status_host(amk_kd *kd, int *h_status);   /* the same into host memory; synchronises the device */

/* Keyframe sweep of FrameKDMap::KeyframeThreadWorker (AM/src/FrameKDMap.cpp:462-485), for every scene:
 * for each point of `keyframe` the nearest-neighbour distance in `current` (SearchForNearest(pt, 1));
 * points with sqrt(d2) > th_dist are outliers (a point gets no result, hence is no outlier, when `current`
 * holds <= 1 point, kd_tree_two.h:119-124).  A scene with >= th_count outliers has its `keyframe` rebuilt
 * from them (InitializeNew(newCloud), order preserved) and d_rebuilt[s] = 1; otherwise `keyframe` is left
 * untouched and d_rebuilt[s] = 0.  d_outliers[s] = number of outliers (either may be NULL).
 * Both handles must hold the same number of scenes.
 * Non-finite coordinates (see amk_kd_search): a keyframe point without a usable neighbour in `current` -- its own coordinates
 * NaN or infinite, or `current` without a point of finite coordinates -- has the nearest-neighbour distance DBL_MAX, as
 * the reference's SearchForNearest(pt, 1) reports it; it is an outlier iff `current` holds a usable point at all (no frame
 * to compare with leaves the keyframe alone).  Such outliers stay in the rebuilt keyframe like any other.
 * This holds for amk_kd_keyframe_sweep only.  The keyframe MAP (amk_kfmap_*, and pipeline slots with one) is UNSPECIFIED for
 * frames that hold a NaN, an infinite or a |coordinate| > 3.0e38: its sweep is not covered by this contract or by any test
 * (whether such a keyframe point is flagged depends on the sweep target and on the row's history); feed it finite frames. */
int amk_kd_keyframe_sweep(amk_kd *keyframe, amk_kd *current, double th_dist, int th_count,
                          int *d_outliers, int *d_rebuilt, void *stream);

/* Same, synchronising, with the per-scene results in host memory.                                 */
int amk_kd_keyframe_sweep_host(amk_kd *keyframe, amk_kd *current, double th_dist, int th_count,
                               int *h_outliers, int *h_rebuilt);

/* GetPointCloud().pts (kd_tree_two.h:134-136): the handle's copy of the cloud (points whose x is not NaN,
 * in order) as packed xyz, h_xyz[s*max_points*3 + i*3 + c], and the per-scene sizes.  Synchronises.  */
int amk_kd_points_host(amk_kd *kd, float *h_xyz, int *h_sizes);

/* Host-buffer conveniences (stage through internal device buffers, synchronise).                 */
int amk_kd_build_host(amk_kd *kd, const float *h_xyz, int point_stride, long long scene_stride,
                      const int *h_counts);
int amk_kd_search_host(amk_kd *kd, const double *h_queries, int n_queries, int k, int *h_indices,
                       double *h_sqdist, float *h_pts, int *h_counts);

/* Radius search: nanoflann's radiusSearch (nanoflann_two.hpp:1611-1639, RadiusResultSet :345-413) on every scene's index --
 * which points lie within a radius of a position, and how many.  The reference never calls it (KDTreeTwo wraps findNeighbors
 * only): this is the surface of the index it was modelled on, not Avoid-MPC's.  Queries are read at
 * d_queries[(s*n_queries + q)*query_stride + {0,1,2}] (query_stride 3 = packed, 10 = the rows of mRefPath, 14 = the rows of
 * x0array); n_queries >= 1 with no AMK_MAX_QUERIES cap; query_stride >= 3.
 *   radius_sq   a SQUARED distance, as nanoflann's L2 radius is.  It must be >= 0 and not NaN (else AMK_ERR_INVALID_ARG); +inf
 *               and anything >= DBL_MAX mean every usable point.  The test is strict: a result has squared distance < radius_sq,
 *               a point at exactly radius_sq is not a result (RadiusResultSet::addPoint) -- radius_sq = 0 finds nothing, not
 *               even a point the query coincides with.
 *   d_counts    [S][n_queries] int: the number of usable points within the radius, radiusSearch's return value.  The count is never
 *               capped: it is always the full number, whatever max_results.  A point is usable under the rule of amk_kd_search
 *               (squared distance < DBL_MAX: false for NaN, inf and overflow); a query with a NaN or infinite coordinate gets
 *               count 0 and every slot empty; an empty scene answers 0.
 *   lists       d_indices [S][n_queries][max_results] int, d_sqdist [..][max_results] double, d_pts [..][max_results][3] float:
 *               the min(count, max_results) NEAREST results, ascending by squared distance (the distances of amk_kd_search,
 *               bit for bit), equal distances by cloud index.  nanoflann sorts radius results with std::sort on the distance
 *               alone, so its order among equals is unspecified and the tie-order modes do not apply: a handle in
 *               AMK_TIES_NANOFLANN / AMK_TIES_AUTO answers identically to the default, and the exact tree is not consulted.
 *               Slots beyond the results hold -1 / DBL_MAX / (0,0,0).  Each list output may be NULL, and so may d_counts,
 *               but not all four.
 *   max_results 0 <= max_results <= AMK_MAX_K.  max_results == 0 requires every list pointer NULL (else AMK_ERR_INVALID_ARG): it
 *               is the pure count.  > AMK_MAX_K: AMK_ERR_UNSUPPORTED; < 0: AMK_ERR_INVALID_ARG.
 * The size rule does not apply: KDTreeTwo's count rule (kd_tree_two.h:119-124) belongs to SearchForNearest, and this is the
 * index's own query -- a cloud of one point, or of exactly max_results points, answers normally.
 * Every error is returned before anything is launched, the outputs untouched.  A handle in scan mode (internal, tests) returns
 * AMK_ERR_UNSUPPORTED.  The call is stream-ordered like amk_kd_search and allocates nothing.
 * Not offered (AMK_ERR_* or simply absent): per-query radii, uncapped result lists (a CSR output), radius queries inside
 * amk_step_batch, AMK_TIES_* semantics for radius results, scan-mode handles.                                              */
int amk_kd_radius_search(amk_kd *kd, const double *d_queries, int query_stride, int n_queries, double radius_sq,
                         int max_results, int *d_indices, double *d_sqdist, float *d_pts, int *d_counts, void *stream);
/* Same with host buffers: stages through the handle's own block (as amk_kd_search_host) and synchronises.  h_queries holds at
 * least (S * n_queries - 1) * query_stride + 3 doubles.                                                                    */
int amk_kd_radius_search_host(amk_kd *kd, const double *h_queries, int query_stride, int n_queries, double radius_sq,
                              int max_results, int *h_indices, double *h_sqdist, float *h_pts, int *h_counts);

/* Segment search: which points lie within a radius of the LINE between two successive positions of a path, how many, and where
 * along the leg each comes closest.  The MPC sees obstacles at its N sampled states only; at the reference's settings two samples
 * are 0.33 m apart and the scenes hold cylinders of radius 0.1 m, so a thin obstacle can stand between two samples while every
 * sampled clearance looks fine.  Not on the reference's surface either (PlanWapionts checks reference point 0 only): the
 * radius search's walk around a segment instead of a point.
 * Layout.  A path is n_points >= 2 positions per scene: point j of scene s is read at
 * d_path[(s*n_points + j)*point_stride + {0,1,2}], point_stride >= 3 (3 = packed points, 10 = the rows of mRefPath, 14 = the
 * rows of x0array).  Leg j, 0 <= j < n_points - 1, runs from point j (a) to point j + 1 (b); n_points = 2 is a lone segment.
 * Every output is [S][n_legs = n_points - 1]...
 * Per leg, in fp64 with contraction off, summing left to right as the squared distance of amk_kd_search does:
 *     ab = b - a;  L2 = (ab0*ab0 + ab1*ab1) + ab2*ab2;  inv = 1.0 / L2
 * Per stored point p (float32, widened first), by the same rules:
 *     ap  = p - a;  dot = (ap0*ab0 + ap1*ab1) + ap2*ab2
 *     t   = dot > 0 ? dot*inv : 0;  t = t < 1 ? t : 1            (comparisons, so a NaN dot gives 0)
 *     c   = t < 1 ? a + t*ab (per component: one product, one sum) : b exactly
 *     e   = c - p;  d2 = (e0*e0 + e1*e1) + e2*e2
 * There is one reciprocal per leg, not a division per candidate.  A degenerate leg (a == b) has dot == 0, so t = 0, c = a, inv
 * is never used, and the leg answers exactly what amk_kd_radius_search answers at a, bit for bit.
 *   radius_sq   a SQUARED distance under the radius search's rules: >= 0 and not NaN (else AMK_ERR_INVALID_ARG); +inf and
 *               anything >= DBL_MAX mean every usable point.  The test is strict: a result has d2 < radius_sq.  A point is
 *               usable when d2 < DBL_MAX (false for NaN, inf and overflow).
 *   d_counts    [S][n_legs] int: the full number of results of the leg, never capped by max_results.  A leg with a non-finite
 *               coordinate in either endpoint, or whose L2 is not finite, gets count 0 and empty slots; a non-finite path
 *               point spoils only the one or two legs that touch it.  An empty or never-built scene answers 0.
 *   lists       d_indices [S][n_legs][max_results] int, d_sqdist and d_t [..][max_results] double, d_pts [..][max_results][3]
 *               float: the min(count, max_results) NEAREST results, ascending by d2, equal d2 by cloud index; d_t is the t
 *               above, the position of the closest approach along the leg (0 at a, 1 at b).  The tie-order modes do not
 *               apply, as for radius results.  Empty slots hold -1 / DBL_MAX / 0.0 / (0,0,0).  Each list output may be NULL,
 *               and so may d_counts, but not all of them.
 *   max_results 0 <= max_results <= AMK_MAX_K.  max_results == 0 requires every list pointer NULL (else AMK_ERR_INVALID_ARG):
 *               the pure count, "is the tube free".  > AMK_MAX_K: AMK_ERR_UNSUPPORTED; < 0, or n_points < 2:
 *               AMK_ERR_INVALID_ARG.
 * No size rule, no fast path, no PtIsInFrame.  A handle in scan mode (internal, tests) returns AMK_ERR_UNSUPPORTED.  Every error
 * is returned before anything is launched, the outputs untouched.  The call is stream-ordered and allocates nothing.
 * Not offered: per-leg radii, uncapped result lists, an unbounded "nearest point to the segment" query, segment queries inside
 * amk_step_batch or the pipeline.                                                                                          */
int amk_kd_segment_search(amk_kd *kd, const double *d_path, int point_stride, int n_points, double radius_sq,
                          int max_results, int *d_indices, double *d_sqdist, double *d_t, float *d_pts, int *d_counts,
                          void *stream);
/* Same with host buffers: stages through the handle's own block (as amk_kd_search_host) and synchronises.  h_path holds at
 * least (S * n_points - 1) * point_stride + 3 doubles.                                                                      */
int amk_kd_segment_search_host(amk_kd *kd, const double *h_path, int point_stride, int n_points, double radius_sq,
                               int max_results, int *h_indices, double *h_sqdist, double *h_t, float *h_pts, int *h_counts);

/* Segment nearest: the k map points closest to each leg of a path, with no radius to choose.  The segment search answers "what
 * lies within r of the leg", so a caller that wants the clearance of a leg has to guess r: too small and every count is 0, too
 * large and the walk reads every record of a wide box to find one point.  This is the unbounded query the segment search does
 * not offer: per leg the smallest distances to the cloud, as numbers, and where along the leg they occur.
 * The path's layout, the legs (n_legs = n_points - 1), ab, L2, the one inv per leg, t clamped by comparisons, c = a + t*ab below
 * 1 and b exactly at 1, and d2 summed left to right in fp64 with contraction off are exactly those of "Segment search" above.
 * Per leg the result is the k usable points (d2 < DBL_MAX) with the smallest d2, ascending; equal d2 order by cloud index.
 *   d_indices [S][n_legs][k] int, d_sqdist and d_t [..][k] double, d_pts [..][k][3] float; d_t is the position of the closest
 *               approach along the leg (0 at a, 1 at b).
 *   d_counts    [S][n_legs] int: min(k, usable points of the scene).  Slots beyond the count hold -1 / DBL_MAX / 0.0 / (0,0,0).
 * A leg with a non-finite coordinate in either endpoint, or with a non-finite L2, gets count 0 and empty slots; a non-finite
 * path point spoils only the legs that touch it.  An empty or never-built scene answers 0.  A degenerate leg (a == b) has t = 0.
 * There is no radius, no size rule, no fast path and no PtIsInFrame.  The tie-order modes do not apply, as for radius and segment
 * results: the exact tree is never consulted, and a handle in AMK_TIES_NANOFLANN / AMK_TIES_AUTO answers like the default.
 *   k           1 <= k <= AMK_MAX_K.  k < 1, n_points < 2, point_stride < 3, a NULL handle, a NULL path, or every output NULL:
 *               AMK_ERR_INVALID_ARG.  k > AMK_MAX_K, a scan-mode handle, or a launch grid beyond 2^31 - 1 blocks:
 *               AMK_ERR_UNSUPPORTED.  Each output may be NULL, but not all of them.
 * Every error is returned before anything is staged or launched, the outputs untouched.  The call is stream-ordered and
 * allocates nothing.
 * Two identities.  (1) The lists equal, bit for bit, those of amk_kd_segment_search called with radius_sq = +inf and
 * max_results = k; the count is min(k, that search's count).  (2) A degenerate leg at a answers with the distances, indices and
 * points of amk_kd_search(k) at a, in the default tie order, for a scene holding more than k points; the size rule of
 * SearchForNearest belongs to amk_kd_search and is absent here (a scene of exactly k points answers all k).
 * Not offered: per-leg k, a radius cap on the nearest query, segment queries inside amk_step_batch or the pipeline.          */
int amk_kd_segment_nearest(amk_kd *kd, const double *d_path, int point_stride, int n_points, int k, int *d_indices,
                           double *d_sqdist, double *d_t, float *d_pts, int *d_counts, void *stream);
/* Same with host buffers: stages and synchronises exactly as amk_kd_segment_search_host does.                               */
int amk_kd_segment_nearest_host(amk_kd *kd, const double *h_path, int point_stride, int n_points, int k, int *h_indices,
                                double *h_sqdist, double *h_t, float *h_pts, int *h_counts);

/* Segment cast: the first contact of a moving sphere along each leg of a path.  The three queries above order by distance to the
 * leg; none says how far the vehicle can travel along a line before it loses its clearance, or which obstacle it meets first:
 * the point closest to the line can stand behind others that are reached earlier.  A sphere of squared radius radius_sq has its
 * centre at a + t*ab; the answer of a leg is the point it touches first, and the t at which that contact begins.
 * The path's layout, point_stride, n_points, the legs (n_legs = n_points - 1) and radius_sq (>= 0, not NaN; +inf and anything
 * >= DBL_MAX are clamped to DBL_MAX) are exactly those of "Segment search" above.  There is no max_results: one contact per leg.
 * All arithmetic is fp64 with contraction off and sums left to right, as in "Segment search".  Per leg ab, L2 and inv = 1.0 / L2
 * are exactly those of the segment search.  Per stored point p (float32, widened first), with r2 the clamped radius_sq:
 *     ap  = p - a;  q = (ap0*ap0 + ap1*ap1) + ap2*ap2           (the squared distance of amk_kd_search at a; usable iff q < DBL_MAX)
 *     q < r2:  contact at t = 0                                   (already inside at the start)
 *     else:    dot = (ap0*ab0 + ap1*ab1) + ap2*ab2;  c = q - r2;  disc = dot*dot - L2*c
 *              contact iff dot > 0 and disc > 0 and t < 1, with t = (dot - sqrt(disc)) * inv
 * Every test is a strict comparison, so NaN and inf - inf give no contact.  A grazing pass (disc == 0) and a contact that would
 * begin exactly at b (t == 1) do not count.  This matches the segment search's strict d2 < r2: in exact arithmetic, a cast hits
 * if and only if the segment search's count is above 0.
 * The answer of a leg is the usable point with the smallest t; equal t keeps the lower cloud index.
 *   d_hit       [S][n_legs] int: 1 when the leg has a contact, else 0.
 *   d_t         [S][n_legs] double: where along the leg the contact begins (0 at a).  A leg without contact holds 1.0 -- free all
 *               the way -- so t * |ab| is the free distance in both cases.
 *   d_pts       [S][n_legs][3] float: the point touched, (0,0,0) if none.
 *   d_indices   [S][n_legs] int: its cloud index (in the NaN-x-filtered cloud, as every index here), -1 if none.
 * Each output may be NULL, but not all of them.
 * A degenerate leg (a == b) has dot == 0 and never uses inv.  It hits iff some usable point has q < r2, at t = 0, and returns the
 * lowest such index, not the nearest such point.  radius_sq >= DBL_MAX (after clamping) puts every usable point inside at the
 * start.  radius_sq == 0 is allowed and answers by the formula.  A leg with a non-finite coordinate in either endpoint, or with a
 * non-finite L2, has no contact; a non-finite path point spoils only the one or two legs that touch it.  An empty or never-built
 * scene answers no contact.  The fp64 sqrt and the one division are correctly rounded on the device, as amk_kd_query_frames
 * already relies on; there is one reciprocal per leg and no division per candidate.
 * Errors: a NULL handle, a NULL path, point_stride < 3, n_points < 2, radius_sq < 0 or NaN, or every output NULL:
 * AMK_ERR_INVALID_ARG.  A scan-mode handle, or a launch grid beyond 2^31 - 1 blocks: AMK_ERR_UNSUPPORTED.  Every error is
 * returned before anything is staged or launched, the outputs untouched.  The call is stream-ordered and allocates nothing.  No
 * size rule, no fast path, no PtIsInFrame; the tie-order modes do not apply, as for the three queries above.
 * Not offered: several contacts per leg, per-leg radii, the first contact over a whole path as one number, casts inside
 * amk_step_batch or the pipeline; an independent ray is a path of n_points = 2.                                            */
int amk_kd_segment_cast(amk_kd *kd, const double *d_path, int point_stride, int n_points, double radius_sq, int *d_hit,
                        double *d_t, float *d_pts, int *d_indices, void *stream);
/* Same with host buffers: stages and synchronises exactly as amk_kd_segment_search_host does.                               */
int amk_kd_segment_cast_host(amk_kd *kd, const double *h_path, int point_stride, int n_points, double radius_sq, int *h_hit,
                             double *h_t, float *h_pts, int *h_indices);

/* Path cast: one answer per scene for a whole path -- the first leg that cannot be passed.  The segment cast answers every leg
 * on its own; a monitor that wants one verdict per robot would copy back four [S][n_legs] arrays and reduce them, and every leg
 * behind the first contact would still be walked.  Here the reduction happens on the device and the walk stops at the stop leg.
 * The path's layout, point_stride, n_points, the legs, radius_sq with its clamping and the error rules are exactly those of
 * "Segment cast" above, and so is every per-point formula.
 * The stop leg of a scene is the first leg j, in leg order, for which one of these holds:
 *   (a) the leg has a contact by the segment cast's rule.  It carries that contact's t, point and cloud index: the least
 *       (t, index).
 *   (b) the leg is unjudgeable: it has a non-finite endpoint coordinate or a non-finite L2.
 * A segment cast reads a non-finite leg as "no contact"; an audit must not read a NaN trajectory as free, hence (b).
 *   d_stop      [S] int: 0 = free to the end, 1 = contact, 2 = unjudgeable leg.
 *   d_leg       [S] int: the stop leg, -1 when free.
 *   d_t         [S] double: t of the contact on the stop leg; 0.0 when d_stop is 2, 1.0 when free.
 *   d_free      [S] double: the free distance along the path, ((len_0 + len_1) + ... + len_{leg-1}) + t * len_leg with
 *               len_j = sqrt(L2_j), L2_j exactly the segment search's.  fp64 with contraction off, summed left to right; the
 *               t * len_leg term is left out when d_stop is 2.  A free path gives its whole length.
 *   d_pts       [S][3] float: the point touched, (0,0,0) unless d_stop is 1.
 *   d_indices   [S] int: its cloud index, -1 unless d_stop is 1.
 * Each output may be NULL, but not all of them.  A degenerate leg has length 0 and stops the path iff a usable point lies inside
 * at its start, as the cast says.  An empty or never-built scene is free to the end unless a leg is unjudgeable.
 * Identity: the answer equals this reduction applied to amk_kd_segment_cast's per-leg outputs on the same path, bit for bit;
 * d_free is rebuilt from the path by the formula.  The legs behind the stop leg are never walked.
 * Errors as for the segment cast: a NULL handle, a NULL path, point_stride < 3, n_points < 2, radius_sq < 0 or NaN, or every
 * output NULL: AMK_ERR_INVALID_ARG; a scan-mode handle: AMK_ERR_UNSUPPORTED.  Every error is returned before anything is staged or
 * launched, the outputs untouched.  The call is stream-ordered and allocates nothing; the tie-order modes do not apply.
 * Not offered: several stops per path, per-scene radii, tie-order modes and scan-mode handles, the path cast inside
 * amk_step_batch, amk_step_batch_frames or amk_kfmap_step (their callers own the stream and enqueue it behind the step
 * themselves; the pipeline has amk_pipeline_set_path_audit).                                                                */
int amk_kd_path_cast(amk_kd *kd, const double *d_path, int point_stride, int n_points, double radius_sq, int *d_stop, int *d_leg,
                     double *d_t, double *d_free, float *d_pts, int *d_indices, void *stream);
/* Same with host buffers: stages and synchronises exactly as amk_kd_segment_cast_host does.                                  */
int amk_kd_path_cast_host(amk_kd *kd, const double *h_path, int point_stride, int n_points, double radius_sq, int *h_stop,
                          int *h_leg, double *h_t, double *h_free, float *h_pts, int *h_indices);

/* ------------------------------------------------------------------------------------------ */
/* MPC: batch of ObstacleAvoidanceMPC                          HighLvlMpc.h:4-33, .cpp:5-137    */
/* ------------------------------------------------------------------------------------------ */
typedef struct amk_mpc amk_mpc;

/* ObstacleAvoidanceMPC(T, dt, soPath) x n_scenes (HighLvlMpc.cpp:5-57).  The reference bakes
 * N = int(T/dt) and K = nearest_point_num into the generated plugin behind soPath
 * (mpc_obstacle_casadi.py:36-37,76-85); here they are constructor arguments.  Defaults after
 * create are the constructor's: weights/tau/gains of HighLvlMpc.cpp:53-56, control bounds
 * [-10,-10,1,-10]..[10,10,20,10] (:13-16,29-30), zero warm start (:26-27,35), tol 1e-4 (:19).
 * The iteration cap defaults to AMK_MPC_DEFAULT_MAX_ITER, not to the reference's ipopt.max_iter = 10 (:20): that
 * number counts IPOPT's iterations, which this library does not reproduce.  The default is a
 * safety net, not a budget: a solve runs until its last barrier problem is solved to tol (mean 10 / 21 / 25 iterations
 * at N = 10 / 20 / 30, the slowest of 1024 + 64 + 256 bench scenes 54; a cap of 40 cut 1.5 % of the cold starts short).
 * A solve that does hit the cap reports status 1 (amk_mpc_solve: info[0]; amk_step_batch: flags[2]).  Real-time hosts:
 * in a batched launch the slowest scene sets the launch time, and a non-converging scene runs to the cap (~25 us per
 * iteration and solve when the chip is full); set a tighter cap per handle (amk_mpc_set_solver_options; for a pipeline:
 * on amk_pipeline_mpc(p, slot) of every slot) and fall back to PubSlowDownCmd when flags[2] > 0.      */
int amk_mpc_create(double T, double dt, int nearest_point_num, int n_scenes, amk_mpc **out);
int amk_mpc_destroy(amk_mpc *mpc);
int amk_mpc_horizon(const amk_mpc *mpc);   /* N                                                  */
int amk_mpc_nx(const amk_mpc *mpc);        /* 10 + 14 N                                          */
int amk_mpc_ref_len(const amk_mpc *mpc);   /* 20 + 10 N + 3 K N  (what GetRefStates produces)    */

int amk_mpc_setup_weights(amk_mpc *mpc, const double *h_weights25); /* SetupWeights  .cpp:58-60  */
int amk_mpc_setup_tau(amk_mpc *mpc, const double *h_tau4);          /* SetupTau      .cpp:61-63  */
int amk_mpc_setup_gains(amk_mpc *mpc, const double *h_gains4);      /* SetupGains    .cpp:67-69  */
/* The generator's use_drag_coefficient switch (mpc_obstacle_casadi.py:95-105, mpc_parameters.yaml:4; off by default, hard-coded 0.033).
 * Its expression `rotmat * diag(k, k, k) * rotmat.T * (vx, vy, vz)`, read as the matrix products it describes, is k v whatever the attitude
 * (R (k I) R' = k I): v' = a - k .* v, linear in the state, so the RK4 map stays affine with the same sparsity and the solver is unchanged
 * -- only A differs.  (As written, with CasADi's element-wise `*`, a 3 x 3 times a 3 x 1 is a dimension error; the reference cannot have
 * exercised it, and it cannot be checked here: CasADi is absent.)  One coefficient per world axis, >= 0; 0, 0, 0 = the reference's default. */
int amk_mpc_set_drag_coefficient(amk_mpc *mpc, double kx, double ky, double kz);
int amk_mpc_set_drone_radius(amk_mpc *mpc, double radius);          /* SetDroneRadius .cpp:64-66 */
int amk_mpc_set_drone_accel_limits(amk_mpc *mpc, double aMinZ, double aMaxZ, double aMaxXy,
                                   double aMaxYawDot);              /* .cpp:70-92                */
/* ipopt.tol of HighLvlMpc.cpp:19 and the iteration cap of this library's method (see amk_mpc_create) */
int amk_mpc_set_solver_options(amk_mpc *mpc, double tol, int max_iter);
/* Scheduling of the solves inside amk_step_batch -- results are unchanged, bit for bit.  budget > 0: a solve launch of the
 * step's first `budget_rounds` rounds (0: mpc_max_iter - 1) ends after `budget` interior-point iterations per scene; a scene
 * whose solve has not converged by then is paused (iterate + multipliers kept on the device) and resumed inside the NEXT
 * round's launch, while the scenes that did converge make their next re-plan pass there -- a launch no longer lasts as long
 * as its slowest scene.  Every scene still runs PlanWapionts -> ProcessWaypoints -> GetRefStates -> Solve to convergence ->
 * refill per pass, in order (AvoidanceStateMachine.cpp:322-344; one Solve per pass, warm start in / out, HighLvlMpc.cpp:93-137);
 * mpc_max_iter catch-up rounds without a budget follow the budgeted ones.  budget = 0 (default): one round per pass, every
 * launch runs its scenes to convergence.  No effect on amk_mpc_solve / amk_step_batch_frames.                              */
int amk_mpc_set_solve_budget(amk_mpc *mpc, int budget, int budget_rounds);
/* Arithmetic of the NLP evaluation and the interior-point method: 64 (default; the reference's CasADi/IPOPT
 * path is fp64 throughout) or 32 (BASELINE.json configs[4], "fp32 tolerance check vs CPU trajectory").  The
 * interface stays double and the KD queries stay fp64 (neighbour indices remain bit-exact); only the solve
 * narrows.  Anything else: AMK_ERR_UNSUPPORTED.                                                              */
int amk_mpc_set_precision(amk_mpc *mpc, int bits);

/* Solve(vecRefStates, u, x0Array, faster) (HighLvlMpc.cpp:93-137) for every scene.
 *   d_ref_states [S][20+10N+3KN]  = [x_init | ref_k | obstacles | target]  (GetRefStates layout,
 *                                    AvoidanceStateMachine.cpp:236-257); gains, taus, weights and
 *                                    radius are appended internally as in .cpp:97-107
 *   d_u          [S][4]           = sol[10..13]                         (.cpp:124-128)
 *   d_x0array    [S][N][14]       = rows [X_k, U_k], k < N              (.cpp:130-136) (may be NULL)
 *   d_info       [S][4] int       = {status (0 converged, 1 iteration cap, 2 regularisation overflow), iterations,
 *                                    regularisations, line-search failures}   (may be NULL)
 * The full primal solution is kept as the next call's warm start (.cpp:110,129).  The reference
 * never inspects the solver status (.cpp:116-122); neither does this function -- it reports it.
 * A scene whose merit function is not a number (a NaN in d_ref_states) does not report status 0: NaN optimality errors pass
 * no convergence test, the solve ends with status 1 or 2 and its u may be NaN.  Tested for a NaN in x_init and, on the path
 * that existed before (infinite errors, the factorisation fails), for an infinity in an early and in the last reference
 * state that a stage cost reads; other placements are not pinned.  A NaN among the neighbour points is NOT such a case: every
 * comparison with it is false, its collision term never becomes active, and the solve converges as if the point were not
 * there (status 0, as in the oracle).  Scenes do not share anything: the other scenes of the batch are
 * bit-identical to a batch without the poisoned one (likewise in amk_step_batch).                                    */
int amk_mpc_solve(amk_mpc *mpc, const double *d_ref_states, double *d_u, double *d_x0array,
                  int *d_info, int faster, void *stream);

/* mNlpW0 access: [S][nx] in the reference's decision-vector order [X_0,U_0,...,U_{N-1},X_N].    */
int amk_mpc_get_warm_start(amk_mpc *mpc, double *d_w, void *stream);
int amk_mpc_set_warm_start(amk_mpc *mpc, const double *d_w, void *stream);
int amk_mpc_reset_warm_start(amk_mpc *mpc, void *stream); /* back to the constructor's zeros      */

int amk_mpc_solve_host(amk_mpc *mpc, const double *h_ref_states, double *h_u, double *h_x0array,
                       int *h_info, int faster);

/* The NLP functions of the generated solver plugin (mpc_obstacle_casadi.py:290-300; loaded at HighLvlMpc.cpp:50,52),
 * SURVEY.md section 8 rows a14-a18, evaluated for every scene at caller-supplied points:
 *   nlp_f      f(x, p)                  objective                     mpc_obstacle_casadi.py:153-214
 *   nlp_g      g(x, p)                  [X_0 - x_init ; F(X_k,U_k) - X_{k+1}]           :156-160,219,338-357
 *   nlp_grad_f grad_x f                 (d|s|/ds = sign(s), as CasADi differentiates fabs)
 *   nlp_jac_g  dg/dx, CCS values        constant: the dynamics are affine (drag off, mpc_parameters.yaml:4)
 *   nlp_hess_l lam_f * triu(hess_x f)   CCS values; the constraints are linear, lam_g contributes nothing
 *   d_w          [S][nx]    x = [X_0, U_0, X_1, ..., U_{N-1}, X_N]                        :158,164,217,224
 *   d_ref_states [S][nref]  P[0 : 20+10N+3KN]; gains, taus, weights, radius come from the handle (HighLvlMpc.cpp:97-107)
 *   d_lam_f      [S] or NULL (= 1)
 *   d_f [S], d_grad_f [S][nx], d_g [S][ng], d_jac_g [S][jac_nnz], d_hess_l [S][hess_nnz]: each may be NULL.
 * ng = 10 + 10 N; jac_nnz = 10 + 39 N; hess_nnz = 25 (N - 1) + 10 + 4 N.  The CCS patterns
 * (column pointers colind[nx + 1], row indices, rows ascending inside a column) come from the *_sparsity calls.      */
int amk_mpc_ng(const amk_mpc *mpc);
int amk_mpc_jac_nnz(const amk_mpc *mpc);
int amk_mpc_hess_nnz(const amk_mpc *mpc);
int amk_mpc_jac_sparsity(const amk_mpc *mpc, int *h_colind, int *h_row);
int amk_mpc_hess_sparsity(const amk_mpc *mpc, int *h_colind, int *h_row);
int amk_mpc_eval(amk_mpc *mpc, const double *d_w, const double *d_ref_states, const double *d_lam_f, double *d_f,
                 double *d_grad_f, double *d_g, double *d_jac_g, double *d_hess_l, void *stream);
int amk_mpc_eval_host(amk_mpc *mpc, const double *h_w, const double *h_ref_states, const double *h_lam_f, double *h_f,
                      double *h_grad_f, double *h_g, double *h_jac_g, double *h_hess_l);

/* nlp_grad, the sixth function CasADi's generate_dependencies emits for an nlpsol (mpc_obstacle_casadi.py:294-303): with
 * gamma(x, p) = lam_f f + lam_g' g,
 *   d_grad_x [S][nx]  grad_x gamma = lam_f grad f + (dg/dx)' lam_g
 *   d_grad_p [S][np]  grad_p gamma over the WHOLE parameter vector p = [P prefix (nref) | gain(4) | tau(4) | weights(25) |
 *                     radius], np = nref + 34 (:76-85): what nlpsol reports as lam_p.  The tail's values are taken from the
 *                     handle (setters), its derivatives are returned here; d/d gain = d/d tau_yaw = 0 (unused by the model,
 *                     :114-121), d/d tau through the RK4 map (dual-number probe of the same integrator).
 *   d_lam_f [S] or NULL (= 1);  d_lam_g [S][ng] or NULL (= 0).  Either output may be NULL.                                  */
int amk_mpc_np(const amk_mpc *mpc);
int amk_mpc_eval_gamma(amk_mpc *mpc, const double *d_w, const double *d_ref_states, const double *d_lam_f,
                       const double *d_lam_g, double *d_grad_x, double *d_grad_p, void *stream);
int amk_mpc_eval_gamma_host(amk_mpc *mpc, const double *h_w, const double *h_ref_states, const double *h_lam_f,
                            const double *h_lam_g, double *h_grad_x, double *h_grad_p);

/* ------------------------------------------------------------------------------------------ */
/* One control step: TASK branch of AvoidanceStateMachine::Step       AvoidanceStateMachine.cpp */
/* ------------------------------------------------------------------------------------------ */
typedef struct amk_step_params {
    double speed;           /* mSpeed                      mpc_parameters.yaml:46                 */
    double safety_distance; /* mParamSafteyDistance        mpc_parameters.yaml:56                 */
    int mpc_max_iter;       /* mParamMPCMaxIter (<= 8)     mpc_parameters.yaml:3                  */
    int reserved;
} amk_step_params;

#define AMK_MAX_OUTER_ITER 8

/* For every scene: for iter < mpc_max_iter { PlanWapionts (:259-281) ; ProcessWaypoints
 * (:204-235) ; early exit (:333-335) ; GetRefStates (:236-257) ; Solve ; refill the reference path
 * with the predicted states (:338-342) }, all on the device, no host round trip.
 *   obstacle, edge  the dual KD indices of the current frame (FrameKDMap's mCurFrame.pointCloud /
 *                   .edgeCloud, FrameKDMap.cpp:44-50); single-frame map (mVecQueryVector = [cur])
 *   d_state_quad    [S][mpc_max_iter][10]  mVecStateQuad as GetCurStateQuad (:183-203) would give
 *                   it at the start of each outer iteration (the host owns the clock model)
 *   d_pos_x         [S]                    mPos.x() used by GetRefStates (:251)
 *   d_ref_path      [S][N][10] in/out      mRefPath (after GetInitPath on entry)
 *   d_u             [S][4]                 control of the last solve
 *   d_x0array       [S][N][14]             predicted trajectory of the last solve (may be NULL)
 *   d_flags         [S][4] int             {isSafety, solves done, WORST solver status over the step's
 *                                           solves (0 converged, 1 iteration cap, 2 regularisation
 *                                           overflow; -1 no solve ran), total interior-point
 *                                           iterations}.  The reference ignores IPOPT's status
 *                                           (HighLvlMpc.cpp:116-122); a host that wants to fall back to
 *                                           PubSlowDownCmd on an unconverged solve tests flags[2] > 0.
 * The step needs neighbours to plan with: a handle created with nearest_point_num = 0 (which amk_mpc_solve and amk_mpc_eval
 * serve) is refused here and by the multi-frame steps with AMK_ERR_INVALID_ARG, as is mpc_max_iter outside 1 .. AMK_MAX_OUTER_ITER,
 * before anything is launched: no output and no reference path is written.                                                  */
int amk_step_batch(amk_kd *obstacle, amk_kd *edge, amk_mpc *mpc, const amk_step_params *params,
                   const double *d_state_quad, const double *d_pos_x, double *d_ref_path,
                   double *d_u, double *d_x0array, int *d_flags, void *stream);

/* The same control step over a MULTI-FRAME map: mVecQueryVector = [current frame, keyframes ...] (FrameKDMap.cpp:64-74).
 * Every query follows FrameKDMap::QueryNearest (:322-376): the current frame alone when it holds >= k points and the query
 * projects into the current image (PtIsInFrame, :215-231), otherwise the k' = min(k, size_f) nearest of every frame merged by
 * squared distance; GetNearestDistance (:400-427) is the minimum over the frames.  obstacle[f] / edge[f]: the dual KD indices of
 * frame f, f = 0 the current frame; n_frames <= AMK_MAX_FRAMES; every handle holds the same number of scenes as `mpc`.
 *   d_Twc [S][16]  mCurFrame.Twc (world <- camera, row-major) per scene; NULL: every query counts as inside the current frame
 *   cam            camera model of PtIsInFrame: intrinsics ALREADY divided by the resize scale (:21-24), depth_max, and the
 *                  size of the down-scaled image (mParamWidth / mParamHeight, :106-107)
 * Remaining arguments as amk_step_batch.  With n_frames = 1 and d_Twc = NULL the results equal amk_step_batch's.            */
#define AMK_MAX_FRAMES 16
#define AMK_MAX_MAP_FRAMES 101   /* frames of a keyframe map (amk_kfmap): current + max_frame_count <= 100 (mpc_parameters.yaml:73) */
typedef struct amk_frame_camera {
    double fx, fy, cx, cy;
    double depth_max;
    int width, height;
} amk_frame_camera;
int amk_step_batch_frames(amk_kd *const *obstacle, amk_kd *const *edge, int n_frames, const double *d_Twc,
                          const amk_frame_camera *cam, amk_mpc *mpc, const amk_step_params *params,
                          const double *d_state_quad, const double *d_pos_x, double *d_ref_path, double *d_u,
                          double *d_x0array, int *d_flags, void *stream);

/* Same with host buffers (stages through device memory, synchronises); what a single-robot host
 * (S = 1) calls once per control period.                                                         */
int amk_step_batch_host(amk_kd *obstacle, amk_kd *edge, amk_mpc *mpc, const amk_step_params *params,
                        const double *h_state_quad, const double *h_pos_x, double *h_ref_path,
                        double *h_u, double *h_x0array, int *h_flags);

/* ------------------------------------------------------------------------------------------ */
/* Several control steps in flight on one GPU (the throughput configuration)                    */
/* ------------------------------------------------------------------------------------------ */
/* One step (both index builds of a fresh frame + amk_step_batch) is a chain of dependent launches around a latency-bound
 * solve: a single stream reaches ~15 % of what the chip does with 20 independent steps in flight.
 * A pipeline owns n_slots slots = {HIP stream, obstacle + edge amk_kd, amk_mpc, reference-path buffer, outputs}; submit()
 * enqueues on the next slot (round robin) -- per frame the reference's sequence FrameKDMap::AddVertex (FrameKDMap.cpp:34-52: the two
 * InitializeNew) -> AvoidanceStateMachine::Step TASK branch (AvoidanceStateMachine.cpp:322-355) -- and returns at once;
 * it blocks only when queue_depth steps of that slot are still unfinished.  Hardware queues: ROCm multiplexes a process's
 * streams onto GPU_MAX_HW_QUEUES hardware queues (4 by default) and two streams on one queue serialise.  The host no longer has
 * to export that variable: when it names fewer than n_slots + 1 queues (absent = 4), amk_pipeline_create creates the slots'
 * streams over the device's stream priority classes (the runtime keeps a pool of queues per class), cycling normal, low, high,
 * so that no class's pool serves more slots than it holds; slots beyond classes x pool share.  That recovers part of the loss,
 * not all of it (the dispatcher honours the classes: 10 slots x gang 4 reach 0.55 M steps/s, against 0.43 M with shared queues
 * and 0.60 M with GPU_MAX_HW_QUEUES=32 -- DESIGN.md section 7), so a host that can export GPU_MAX_HW_QUEUES >= n_slots + 1 (at
 * most 32) before its first HIP call still should: it gets ordinary streams, as before.  The pipeline never adds more than
 * AMK_PIPELINE_MAX_OWN_QUEUES (24) queues to the process, and a creation call that fails leaves that slot with an ordinary
 * stream.  AMK_PIPELINE_QUEUES=pooled|priority forces one way for every pipeline of the process (A/B runs);
 * amk_pipeline_queue_mode reports what a slot got.  Every slot's stream is a non-blocking stream either way.
 * Input buffers belong to the caller and must stay valid until the slot has finished.  They must also be
 * COMPLETE: a slot runs on its own non-blocking stream, which is not ordered against the stream that produced the inputs, and
 * with a gang the inputs are only read when the gang is launched (the G-th submit, wait or drain).  Either synchronise the
 * producing stream before submit(), or record an event on it and pass it as amk_pipeline_frame.input_ready -- the slot's stream
 * then waits for it on the device (hipStreamWaitEvent), the host does not.                                                */
typedef struct amk_pipeline amk_pipeline;
/* FrameKDMap's perception parameters (used by amk_depth_to_cloud / _edge_cloud below and by pipeline frames that start at the
 * raw depth image).                                                                                                       */
typedef struct amk_depth_params {
    double pixel2meter;   /* mParamPixel2Meter   mpc_parameters.yaml:64                            */
    double depth_min;     /* mParamDepthMin      :66                                               */
    double depth_max;     /* mParamDepthMax      :65                                               */
    double resize_scale;  /* mParamDepthScale    :63  (output is cols/scale x rows/scale, truncated) */
    double fx, fy, cx, cy; /* FULL-resolution intrinsics (:59-62); divided by resize_scale inside,
                             as the FrameKDMap constructor does (FrameKDMap.cpp:21-24)             */
    double Tbc[16];       /* body <- camera, row-major 4x4 (mParamTbc)                             */
} amk_depth_params;
/* What the TASK case does around the re-plan loop (AvoidanceStateMachine.cpp:322-355), for frames submitted in TASK mode.  */
typedef struct amk_task_params {
    double decay;           /* mParamDecay: assumed compute latency, mpc_parameters.yaml:77                                 */
    double iter_time;       /* assumed duration of one re-plan pass (the reference measures it, :329,343); <= 0: decay      */
    double farest_point;    /* goal_x, mpc_parameters.yaml:55 (GetInitPath :31)                                             */
    double height;          /* mHeight, :54                                                                                 */
    double slow_down_kp, slow_down_kd;   /* :79-80  (PubSlowDownCmd :379-397)                                               */
    double a_max_xy, a_max_z;            /* clamp of the slow-down command (:383-388; z clamped to +-aMaxZ as there)        */
    int use_odom_est;       /* mParamIsUseOdomEstimate, :78                                                                 */
    int task;               /* mStrTask of GetInitPath (:29-45): AMK_TASK_FORWARD (0, the launch file's default,             */
                            /* mpc_obstacle_avoidance_sim.launch:9) or AMK_TASK_GLOBAL_GOAL (1): the path's last point walks  */
                            /* towards amk_pipeline_frame.d_global_goal by at most speed * dt per period (:34-45)            */
} amk_task_params;
#define AMK_TASK_FORWARD 0
#define AMK_TASK_GLOBAL_GOAL 1
#define AMK_PIPELINE_MAX_SLOTS 64
#define AMK_PIPELINE_DEFAULT_DEPTH 3
#define AMK_PIPELINE_MAX_DEPTH 64
#define AMK_PIPELINE_MAX_GANG 8
#define AMK_PIPELINE_MAX_OWN_QUEUES 24   /* hardware queues the pipeline's streams may add to the process */
#define AMK_QUEUES_POOLED 0              /* amk_pipeline_queue_mode: hipStreamCreateWithFlags (the runtime's pool)              */
#define AMK_QUEUES_PRIORITY 1            /* hipStreamCreateWithPriority, the slots spread over the priority classes            */
/* FrameKDMap's keyframe parameters (the batched map itself: amk_kfmap_*, below) */
typedef struct amk_kfmap amk_kfmap;
typedef struct amk_kfmap_params {
    int max_frame_count;       /* mParamMaxFrameCount, mpc_parameters.yaml:73; 1 ... AMK_MAX_MAP_FRAMES - 1; 0 (pipeline      */
                               /* config only): no keyframe map, mVecQueryVector = [current]                                  */
    int keyframe_th_count;     /* mParamKeyframeCountTh, :72 (>= 1)                                                           */
    double keyframe_th_dist;   /* mParamKeyframeDistanceTh, :71                                                               */
    double depth_min;          /* mParamDepthMin (DroneBehindPts :247)                                                        */
    double Tbc[16];            /* mParamTbc, row-major (amk_pipeline_config: all zero = take amk_depth_params.Tbc, and if that  */
                               /* is all zero too the identity: camera frame = body frame)                                    */
} amk_kfmap_params;
typedef struct amk_pipeline_config {
    int n_slots;            /* independent steps in flight                                                              */
    int n_scenes;           /* scenes per step (S of every handle)                                                      */
    int max_points;         /* capacity per scene of the obstacle cloud ...                                             */
    int max_edge_points;    /* ... and of the edge cloud                                                                */
    double T, dt;           /* ObstacleAvoidanceMPC(T, dt, .)                                     HighLvlMpc.cpp:5-12  */
    int nearest_point_num;  /* K                                                                  mpc_parameters.yaml:5 */
    int queue_depth;        /* steps that may be queued per slot before submit() blocks (0 = AMK_PIPELINE_DEFAULT_DEPTH).   */
                            /* A slot's steps run in order on its stream; with depth >= 2 the next step is already queued   */
                            /* when one ends (no host round trip between them).  Results of a step must be read -- wait(),  */
                            /* outputs() -- before a later submit() on the same slot overwrites them, or go to d_u_out.      */
    int gang;               /* frames per launch (0 / 1 = every frame has its own launches; <= AMK_PIPELINE_MAX_GANG).       */
                            /* G > 1: a slot's handles hold G x n_scenes scenes and G consecutive submit()s share one set   */
                            /* of launches (both index builds of all G frames in one launch, one amk_step_batch); a frame   */
                            /* is staged until its gang is full -- wait() / drain() launch a partly filled gang.  Results   */
                            /* are those of separate launches, bit for bit (scenes are independent).  On the bench workload */
                            /* 10 slots x 4 frames of 256 scenes beat 20 slots x 1 by 11 %.           */
    amk_step_params step;
    amk_task_params task;   /* only read for frames submitted with d_odom (TASK mode, below)                                */
    amk_depth_params depth; /* only read for frames submitted with d_depth (below)                                          */
    amk_kfmap_params keyframes;  /* max_frame_count > 0: every slot keeps a keyframe map (amk_kfmap) over its gang x n_scenes    */
                            /* scenes and every frame runs AddVertex -> KeyframeThreadWorker's body -> the step over            */
                            /* mVecQueryVector = [current, keyframes ...] (the reference's default regime: FrameKDMap.cpp:29-32, */
                            /* 64-74).  The scene at position g of slot s must be the same robot every period (as in TASK mode).*/
                            /* PtIsInFrame: for depth frames the camera is amk_pipeline_config.depth's, down-scaled (:21-24,     */
                            /* 106-107); for cloud frames amk_pipeline_frame.camera + d_Twc_cur (BOTH required then, else         */
                            /* AMK_ERR_INVALID_ARG: mCurFrame.Twc also feeds DroneBehindPts, and without a camera no keyframe    */
                            /* would ever be merged).  The frames of one gang must agree on depth-vs-cloud, the depth image      */
                            /* size and the camera (AMK_ERR_INVALID_ARG): the map step takes one camera model per launch.        */
                            /* keyframes.Tbc is ignored: depth.Tbc is used.  0: single-frame map.                                */
                            /* A TASK frame that brings d_ref_path_init (a robot that starts over) also resets its scenes' map.   */
} amk_pipeline_config;
typedef struct amk_pipeline_frame {
    const float *d_cloud;          /* [S][max_points][point_stride]      obstacle cloud of the frame (NULL with d_depth)*/
    const int *d_cloud_counts;     /* [S] or NULL (= max_points)                                                        */
    const float *d_edge;           /* [S][max_edge_points][point_stride] edge cloud                                     */
    const int *d_edge_counts;      /* [S] or NULL                                                                       */
    int point_stride;              /* 3, 4 (pcl::PointXYZ) or 0 (= 3)                                                   */
    int keep_warm_start;           /* 0: zero warm start (a fresh ObstacleAvoidanceMPC, HighLvlMpc.cpp:26-27,35);        */
                                   /* 1: the slot's last solution (mNlpW0 = sol, :129)                                  */
    const double *d_state_quad;    /* [S][mpc_max_iter][10]  as amk_step_batch                                          */
    const double *d_pos_x;         /* [S]                                                                               */
    const double *d_ref_path_init; /* [S][N][10]  mRefPath after GetInitPath; copied, the slot's copy is refilled       */
    double *d_u_out;               /* [S][4] or NULL: where the control goes instead of the slot's own buffer (e.g. a   */
                                   /* row of the sweep's result array that amk_shard_gather exchanges at the end)       */
    /* TASK mode: the slot keeps the state machine's persistent state -- mRefPath next to mNlpW0 -- and the caller supplies  */
    /* per control period what the reference's callbacks supply: the frame and the odometry.  With d_odom != NULL the slot   */
    /* runs, on the device, GetInitPath (:24-54, task "forward") on ITS OWN mRefPath (position g of slot s keeps the path of */
    /* the frame submitted there last: submit the same robots in the same order every period), GetCurStateQuad (:183-203)    */
    /* for every re-plan pass (odom_age + decay for pass 0, odom_age + (i + 1) * iter_time for pass i >= 1), the step, PubCmd /  */
    /* PubSlowDownCmd (:345-350,369-397).                                                                                   */
    /* d_state_quad / d_pos_x are then ignored (may be NULL); d_ref_path_init != NULL first (re)sets mRefPath               */
    /* (InitCircleState :14-23 or any re-initialisation) BEFORE GetInitPath, NULL keeps the slot's -- which must exist: the   */
    /* first TASK frame at a position, and the first one after a launch of the slot failed half-way (the slot's persistent   */
    /* state may have been shifted / reset by what was enqueued before the failure), must bring it (AMK_ERR_INVALID_ARG).     */
    const double *d_odom;          /* [S][10] or NULL: [mPos(3), yaw, mVel(3), mAcc(3)] as the callbacks left them       */
    double odom_age;               /* now - mTimePos at the start of the step, seconds (:183-184); 0 = fresh odometry    */
    double *d_cmd_out;             /* [S][3] or NULL: Command.acceleration -- u[0..2] when isSafety, else the slow-down  */
                                   /* command (TASK mode only)                                                           */
    /* Frames that start where FrameKDMap::AddVertex starts (FrameKDMap.cpp:34-52): the raw depth image.  With d_depth != NULL  */
    /* d_cloud / d_edge are ignored (may be NULL) and the slot runs ProcessDepth (:90-130) and BuildEdgeCloud (:176-214) on the */
    /* device with amk_pipeline_config.depth -- the edge cloud through the slot's own mCurFrame.Twc (the PREVIOUS frame's        */
    /* Twb * Tbc of the same position, identity at first, as the reference: :50,209) -- then both index builds; a scene whose  */
    /* frame yields no obstacle point keeps its previous frame and its Twc (:39-41).  The down-scaled image must fit the       */
    /* pipeline's capacities: (cols / resize_scale) * (rows / resize_scale) <= max_points and <= max_edge_points; its width     */
    /* cols / resize_scale is at most AMK_DEPTH_MAX_WIDTH, else AMK_ERR_UNSUPPORTED (one amk_depth_to_clouds per frame).       */
    const void *d_depth;           /* [S][rows][cols] uint16 / float32 (depth_type: AMK_DEPTH_U16 / AMK_DEPTH_F32) or NULL */
    int depth_type, depth_rows, depth_cols, reserved;
    const double *d_Twb;           /* [S][16] world <- body, row-major (DepthCallback, AvoidanceStateMachine.cpp:153-164) */
    /* A multi-frame map: mVecQueryVector = [this frame, keyframes ...] (FrameKDMap.cpp:64-74).  With n_keyframes > 0 the slot  */
    /* runs amk_step_batch_frames over [its own two indices of this frame, kf_obstacle[i] / kf_edge[i] ...] instead of          */
    /* amk_step_batch (PtIsInFrame fast path, per-frame merge, minimum distance over the frames: :215-231,254-427).  The         */
    /* keyframe handles are the caller's (built with amk_kd_build, maintained with amk_kd_keyframe_sweep), hold n_scenes        */
    /* scenes and must not be rebuilt while the frame is in flight; gang == 1 only (AMK_ERR_UNSUPPORTED otherwise);             */
    /* n_keyframes <= AMK_MAX_FRAMES - 1.  d_Twc_cur: mCurFrame.Twc per scene for PtIsInFrame (NULL: the slot's own Twc for a   */
    /* depth frame, else every query counts as inside the current frame); camera: host pointer, copied at submit (NULL: no     */
    /* frustum test).                                                                                                        */
    amk_kd *const *kf_obstacle;
    amk_kd *const *kf_edge;
    int n_keyframes, reserved2;
    const double *d_Twc_cur;
    const struct amk_frame_camera *camera;
    void *input_ready;             /* hipEvent_t or NULL: recorded by the caller on the stream that produces this       */
                                   /* frame's inputs; the slot's stream waits for it before it reads them.  The event   */
                                   /* must stay alive (and must not be re-recorded) until the frame has been launched   */
    const double *d_global_goal;   /* [S][3] or NULL: mStateGlobalGoal of every scene (GlobalGoalCallback, :166-172), read by   */
                                   /* GetInitPath when amk_task_params.task == AMK_TASK_GLOBAL_GOAL; NULL = the constructor's   */
                                   /* {0, 0, height} (:22)                                                                   */
} amk_pipeline_frame;
int amk_pipeline_create(const amk_pipeline_config *cfg, amk_pipeline **out);
int amk_pipeline_destroy(amk_pipeline *p);
int amk_pipeline_slots(const amk_pipeline *p);
int amk_pipeline_gang(const amk_pipeline *p);       /* frames per launch (>= 1)                                            */
int amk_pipeline_queue_mode(const amk_pipeline *p, int slot);   /* AMK_QUEUES_*: how the slot's stream was really created; -1: no such slot */
/* The slot's handles, to configure them (weights, limits, tie order, precision ...) and its stream.                       */
amk_mpc *amk_pipeline_mpc(amk_pipeline *p, int slot);
amk_kd *amk_pipeline_kd(amk_pipeline *p, int slot, int which /* 0 obstacle, 1 edge */);
amk_kfmap *amk_pipeline_kfmap(amk_pipeline *p, int slot);   /* the slot's keyframe map (NULL without one), e.g. for amk_kfmap_state_host */
/* ... and for the map's own queries (amk_kfmap_query_nearest / _nearest_distance / _points_host, below): enqueue them on
 * amk_pipeline_stream(p, slot) -- behind every launch the slot was given; frames staged in an open gang are not in the map yet --
 * or on any stream after amk_pipeline_wait / _wait_stream, and order the slot's next submit behind them (input_ready).          */
void *amk_pipeline_stream(amk_pipeline *p, int slot);
/* submit() hands back a ticket = position_in_gang * n_slots + slot (without a gang: the slot index, as before);
 * ticket % n_slots is the slot, for amk_pipeline_mpc / _kd / _stream.                                                    */
int amk_pipeline_submit(amk_pipeline *p, const amk_pipeline_frame *frame, int *ticket_out);
int amk_pipeline_wait(amk_pipeline *p, int ticket);   /* until that frame's step has finished (launches an open gang)     */
/* Device-side wait: work queued on `stream` after this call runs after the frame's step has finished; the host does not
 * block (launches an open gang).  A closed loop -- outputs -> the caller's kernels -> next submit(input_ready) -- then never
 * synchronises with the host.  The slot's NEWEST launch is the one waited for: call it before the next submit on that slot. */
int amk_pipeline_wait_stream(amk_pipeline *p, int ticket, void *stream);
int amk_pipeline_query(amk_pipeline *p, int ticket);  /* 1 finished / idle, 0 running or staged, -1 error (also: the slot's     */
                                                      /* newest launch failed half-way and dropped its frames; wait() says why) */
int amk_pipeline_drain(amk_pipeline *p);              /* wait for every slot                                              */
/* Device pointers of the frame's results (valid after wait): u [S][4], x0array [S][N][14], flags [S][4], ref_path [S][N][10] */
int amk_pipeline_outputs(amk_pipeline *p, int ticket, double **d_u, double **d_x0array, int **d_flags, double **d_ref_path);
/* The trajectory audit, off by default.  The MPC's collision terms sit at the N sampled states; a predicted trajectory can keep
 * every sampled clearance and still pass through a thin obstacle between two samples.  With the audit on, every launch runs the
 * path cast ("Path cast" below the KD index) on the step's own x0array -- row 0 is X0, the state the step planned from -- against
 * the map the step planned on, on the slot's stream, after the step and before the command is written.  By definition the stage
 * is amk_kd_path_cast(the slot's obstacle index, x0array, 14, n_legs + 1, radius * radius, ...) with a scene's path every N rows,
 * or, for a slot with a keyframe map, amk_kfmap_path_cast(the slot's map, ..., query_edge 0, ...) on the map as it stands after
 * the period's AddVertex and update; it covers the scenes of the frames a launch really holds.
 *   AMK_AUDIT_REPORT     keeps the answers (amk_pipeline_audit_outputs); nothing else changes.
 *   AMK_AUDIT_SLOW_DOWN  also, for a TASK-mode frame with d_cmd_out, publishes PubSlowDownCmd instead of u for a scene with
 *                        flags[0] == 1 whose audit stops (d_stop != 0) -- the arithmetic of the flags[0] == 0 case, bit for bit.
 *                        d_flags, d_u, x0array, mRefPath and the warm start are what they are without the audit: the verdict lives
 *                        only in the audit outputs and the command, and the next period re-plans from the same persistent state.
 * amk_pipeline_set_path_audit is valid only while no frame is staged or in flight on any slot (before the first submit or after
 * amk_pipeline_drain), else AMK_ERR_UNSUPPORTED.  radius is in metres (used as radius * radius); n_legs = 0 means all N - 1.  A
 * negative or NaN radius, an unknown mode or n_legs outside [0, N - 1]: AMK_ERR_INVALID_ARG.  It allocates the slots' result
 * buffers ([gang * n_scenes] each); submit and launch allocate nothing more.  AMK_AUDIT_OFF frees nothing and stops the stage;
 * with the audit off a launch enqueues exactly what it enqueued before.  While the audit is on, a frame that brings its own keyframe
 * list (n_keyframes > 0) is refused at submit with AMK_ERR_UNSUPPORTED.  A stage that fails ends the launch like any other stage.
 * amk_pipeline_audit_outputs: device pointers of the frame's audit answers (valid after wait, until the slot's next launch):
 * d_stop / d_leg / d_src [S] int, d_t / d_free [S] double, d_pts [S][3] float; d_src is the cloud index of the point touched, the
 * frame for a slot with a keyframe map.  AMK_ERR_UNSUPPORTED before the first amk_pipeline_set_path_audit.
 * Not offered: the audit inside amk_step_batch, amk_step_batch_frames or amk_kfmap_step; an audit that changes flags, the re-plan
 * loop or the persistent path; per-scene radii; several stops per path; the edge cloud in the audit.                         */
#define AMK_AUDIT_OFF 0
#define AMK_AUDIT_REPORT 1       /* run the path cast on every step's x0array, keep the answers                  */
#define AMK_AUDIT_SLOW_DOWN 2    /* ... and in TASK mode publish PubSlowDownCmd for a scene whose audit stops   */
int amk_pipeline_set_path_audit(amk_pipeline *p, int mode, double radius, int n_legs /* 0 = all N - 1 */);
int amk_pipeline_audit_outputs(amk_pipeline *p, int ticket, int **d_stop, int **d_leg, double **d_t, double **d_free,
                               float **d_pts, int **d_src /* cloud index; frame for a map slot */);

/* ------------------------------------------------------------------------------------------ */
/* The multi-frame map with keyframes, batched: FrameKDMap's keyframe list on the device       */
/* ------------------------------------------------------------------------------------------ */
/* The reference's keyframe thread is on by default (max_frame_count = 100, only_trust_vel = false: FrameKDMap.cpp:29-32),
 * and every QueryNearest / GetNearestDistance of a control step runs over mVecQueryVector = [current frame, every keyframe
 * but the newest] (:64-74,322-427).  amk_kfmap is that map for S scenes at once -- every scene with its own deque of
 * keyframes -- entirely on the device: per control period
 *   amk_kfmap_add_vertex   FrameKDMap::AddVertex after ProcessDepth (:39-51) for the scenes whose frame is not empty
 *   amk_kfmap_update       one pass of KeyframeThreadWorker's body (:443-486): first keyframe / pop while the list is longer
 *                          than max_frame_count or DroneBehindPts fails for the oldest (:233-252) / n x 1-NN sweep of the
 *                          newest keyframe against the current frame, rebuild from >= keyframe_th_count outliers farther than
 *                          keyframe_th_dist, InsertKeyFrame
 *   amk_kfmap_step         the TASK branch over the map (amk_step_batch_frames' semantics: PtIsInFrame fast path, per-frame
 *                          k' = min(k, size), merge, minimum distance over the frames)
 * all stream-ordered, no host round trip.  A keyframe is not a copy: every scene owns max_frame_count + 2 physical slots in
 * two pool indices, its current frame is built into a slot no keyframe holds, the deque is a list of slot numbers.
 * amk_pipeline runs the three calls inside a TASK-mode slot when amk_pipeline_config.keyframes.max_frame_count > 0
 * (any gang).  Twb = Twc * Tbc^-1 of DroneBehindPts uses the rigid inverse of Tbc.                                          */
/* Memory.  The pools are allocated at creation, at full capacity: with cap(p) = round_up(p, 256) + 1024 points per pool scene
 *   bytes ~ (max_frame_count + 2) x n_scenes x [ 16 cap(max_points) + 16 cap(max_edge_points) + 13 cap(max_points) + directories ]
 *           + n_scenes x 2 x 16 cap(max_points)   (the sweep's grids: two generations per scene)    (amk_kfmap_pool_bytes)
 * i.e. ~ 30 B per obstacle point per slot + the edge pool: the reference's max_frame_count = 100 at its own 3072-point frames is 20 MB per
 * robot, at 50 k-point frames 170 MB per robot.  A flight holds ~ 6 frames; slots a scene never uses are still reserved.
 * amk_kfmap_create compares the figure with the device's free memory first and returns AMK_ERR_UNSUPPORTED (message with both
 * numbers on stderr) instead of failing half-way through the allocations with AMK_ERR_HIP.
 * Call order.  add_vertex -> update -> step per control period is what amk_pipeline issues.  add_vertex alone already points the
 * query vector's first frame at the new trees (SetCurPtCloud -> UpdateQueryVector, FrameKDMap.cpp:53-58); the keyframe rows of the
 * query vector are the worker's (update).                                                                                    */
int amk_kfmap_pool_bytes(int n_scenes, int max_points, int max_edge_points, int max_frame_count, long long *bytes_out);
int amk_kfmap_create(int n_scenes, int max_points, int max_edge_points, const amk_kfmap_params *prm, amk_kfmap **out);
int amk_kfmap_destroy(amk_kfmap *map);
/* scenes [first_scene, first_scene + n_scenes) start over: no current frame, no keyframe, Twc = identity (stream-ordered) */
int amk_kfmap_reset(amk_kfmap *map, int first_scene, int n_scenes, void *stream);
int amk_kfmap_scenes(const amk_kfmap *map);
int amk_kfmap_frames(const amk_kfmap *map);          /* frames of the query vector: 1 + max_frame_count                      */
const double *amk_kfmap_twc(const amk_kfmap *map);   /* device [S][16]: mCurFrame.Twc (what BuildEdgeCloud multiplies with, :209) */
/* Scenes [first_scene, first_scene + n_scenes): d_xyz [n][max_points][stride] / d_counts [n] (NULL = max_points) and the edge
 * cloud likewise, d_Twc [n][16] = mat4Twb * mParamTbc of the frame.  A scene whose count is 0 keeps its map untouched (:39-41). */
int amk_kfmap_add_vertex(amk_kfmap *map, int first_scene, int n_scenes, const float *d_xyz, const int *d_counts,
                         const float *d_edge_xyz, const int *d_edge_counts, int point_stride, const double *d_Twc, void *stream);
int amk_kfmap_update(amk_kfmap *map, void *stream);
/* cam == NULL: no frustum test (every query counts as inside the current frame, as amk_step_batch_frames with d_Twc = NULL) */
int amk_kfmap_step(amk_kfmap *map, const struct amk_frame_camera *cam, amk_mpc *mpc, const amk_step_params *prm,
                   const double *d_state_quad, const double *d_pos_x, double *d_ref_path, double *d_u, double *d_x0array,
                   int *d_flags, void *stream);
/* Introspection (synchronises): per scene mKeyFrameMap.size(), mVecQueryVector.size(), the outliers of the last sweep and --
 * h_frame_sizes [S][amk_kfmap_frames()] or NULL -- the obstacle-cloud size of every query frame (-1 behind the scene's last). */
int amk_kfmap_state_host(amk_kfmap *map, int *h_n_keyframes, int *h_n_query_frames, int *h_last_outliers, int *h_frame_sizes);
/* Tie order of the map (see amk_kd_set_tie_order).  AMK_TIES_LOWEST_INDEX is the default.  AMK_TIES_NANOFLANN: every frame of
 * every scene -- obstacle and edge cloud, the current frame, the keyframes, keyframes rebuilt from their outliers -- also holds
 * the reference's own tree, built on the device behind the AddVertex or the sweep that gave the slot its cloud (the host never
 * learns which), and every search whose result SET can depend on the order of equal distances answers by nanoflann's traversal:
 *   - the step's N x K-NN and edge 1-NN per frame and the snap's re-query (amk_kfmap_step),
 *   - DroneBehindPts' SearchForNearest(min(size, 10)) (amk_kfmap_update: which ten decides the pop),
 *   - amk_kfmap_query_nearest.
 * Only the per-frame list changes; the rules above it (fast path / merge path, k' = min(k, size), the merge order by distance,
 * then frame, then position in the frame's list, padding, counts) do not.  GetNearestDistance (the step's and
 * amk_kfmap_nearest_distance) and the sweep's n x 1-NN read distances only and are unchanged.  A pool scene without a tree
 * (amk_kfmap_exact_status_host: GAVE_UP, TOO_DEEP; a cloud that kept a non-finite point) keeps the bucketed index's answer for
 * its searches, as a plain handle does; other frames and scenes are unaffected.
 * The call is allowed only on a map that has never been given a frame (amk_kfmap_add_vertex, or a pipeline submit; amk_kfmap_reset
 * does not re-open it): afterwards AMK_ERR_INVALID_ARG -- every tree always belongs to the cloud its slot holds.  Any mode but
 * the two (AMK_TIES_AUTO included): AMK_ERR_UNSUPPORTED.  A pipeline has no config field for it: set it on
 * amk_pipeline_kfmap(p, slot) of every slot before the first submit.
 * Memory: the call allocates all of the mode's device memory (never a later call), amk_kfmap_tie_order_bytes (host arithmetic):
 *   (max_frame_count + 2) x n_scenes x [ 24 cap(max_points) + 36 cap(max_edge_points) + 80 (nodes(max_points) + nodes(max_edge_points)) + 104 ]
 * with nodes(p) = cap(p) / 2 + 64 -- 64 B per obstacle point per slot, about 2.5 x amk_kfmap_pool_bytes: the reference's
 * max_frame_count = 100 at its 3072-point frames (512 edge points) is 38 MB per robot.  It compares the figure with the free memory first and
 * returns AMK_ERR_UNSUPPORTED (both numbers on stderr) when it does not fit; the map then stays in the default mode.        */
int amk_kfmap_set_tie_order(amk_kfmap *map, int mode);
int amk_kfmap_tie_order_bytes(int n_scenes, int max_points, int max_edge_points, int max_frame_count, long long *bytes_out);
/* amk_kd_exact_status's codes per query frame of every scene (synchronises): h_obs / h_edge [S][amk_kfmap_frames()], either may
 * be NULL.  AMK_EXACT_OFF: an absent frame, or the map is in the default mode.  A caller that needs the reference's lists checks
 * for AMK_EXACT_IN_USE on every present frame.                                                                            */
int amk_kfmap_exact_status_host(amk_kfmap *map, int *h_obs, int *h_edge);

/* The map's own queries: FrameKDMap::QueryNearest, GetNearestDistance and GetPtCloud (FrameKDMap.h:60-67) for any points,
 * outside a control step.  They answer from the map as it stands, change no map state, need no amk_mpc and allocate nothing
 * (the *_host variants stage through device memory they allocate per call).  A query is stream-ordered: enqueue it AFTER the
 * amk_kfmap_add_vertex / amk_kfmap_update it should see (same stream, or ordered by an event), and do not let it overlap a LATER
 * add_vertex / update / reset on another stream -- those rebuild the trees it reads.
 *   d_queries   read at d_queries[(s * n_queries + q) * query_stride + {0,1,2}], s < amk_kfmap_scenes(): query_stride 3 = packed,
 *               10 = the rows of mRefPath, 14 = the rows of x0array; n_queries >= 1 (no AMK_MAX_QUERIES cap), 1 <= k <= AMK_MAX_K
 *               (k = 0: AMK_ERR_INVALID_ARG, k > AMK_MAX_K: AMK_ERR_UNSUPPORTED)
 *   d_pts [S][n_queries][k][3], d_sqdist [S][n_queries][k], d_frame [S][n_queries][k] (the position in the query vector the
 *   neighbour came from, 0 = current frame: what PtDists::isInKeyFrame carries), d_counts [S][n_queries], d_dist [S][n_queries];
 *   each output of the k-NN query may be NULL
 *   query_edge  != 0: the frames' edge clouds (QueryNearest(..., queryEdge = true)), else their obstacle clouds
 *   cam         NULL: no frustum test, every query counts as inside the current frame (as amk_kfmap_step)
 * QueryNearest, the rules of the step (amk_step_batch_frames):
 *   fast path   taken when frame 0 exists, holds >= k points and the query passes PtIsInFrame (:215-231) against the scene's
 *               mCurFrame.Twc: the answer is frame 0's SearchForNearest(k) alone, its count by KDTreeTwo's size rule
 *               (kd_tree_two.h:119-124) -- a current frame of EXACTLY k points takes the fast path and returns nothing
 *   merge path  otherwise: every present frame contributes its k nearest iff it holds MORE than k points (k' = min(k, size),
 *               size <= k: no result); the candidates are ordered by squared distance, equal distances keep the earlier frame,
 *               then the earlier neighbour within a frame; the first k are kept and the count is their number
 *   Within a frame equal distances order by cloud index (amk_kfmap_set_tie_order(AMK_TIES_NANOFLANN): in nanoflann's order).  Slots beyond the count hold DBL_MAX, (0, 0, 0) and frame -1.  A query
 *   with a NaN or infinite coordinate gets every slot empty (its count is unspecified, as in the step); a scene with no frame
 *   yet gets count 0 everywhere.
 * GetNearestDistance: sqrt of the minimum 1-NN squared distance over the frames whose obstacle cloud holds more than one point;
 *   no fast path; sqrt(DBL_MAX) when no frame answers.                                                                          */
int amk_kfmap_query_nearest(amk_kfmap *map, const struct amk_frame_camera *cam, const double *d_queries, int query_stride,
                            int n_queries, int k, int query_edge, float *d_pts, double *d_sqdist, int *d_frame,
                            int *d_counts, void *stream);
int amk_kfmap_nearest_distance(amk_kfmap *map, const double *d_queries, int query_stride, int n_queries,
                               double *d_dist, void *stream);
/* Same with host buffers (stage through device memory, synchronise the device).  h_queries holds at least
 * (S * n_queries - 1) * query_stride + 3 doubles.                                                                            */
int amk_kfmap_query_nearest_host(amk_kfmap *map, const struct amk_frame_camera *cam, const double *h_queries, int query_stride,
                                 int n_queries, int k, int query_edge, float *h_pts, double *h_sqdist, int *h_frame,
                                 int *h_counts);
int amk_kfmap_nearest_distance_host(amk_kfmap *map, const double *h_queries, int query_stride, int n_queries, double *h_dist);
/* GetPtCloud (:490-515) for one scene (synchronises): the obstacle points of the scene's query frames in query-vector order,
 * inside a frame in cloud order, packed xyz.  h_frame_sizes [amk_kfmap_frames()] (or NULL): the points per frame, -1 behind the
 * scene's last frame; *n_points_out: their total.  capacity_points < total: nothing is written to h_xyz, the total and the
 * sizes are still reported and the call returns AMK_ERR_INVALID_ARG; h_xyz == NULL with capacity 0 is the size probe (AMK_OK).  The
 * reference's colours (white for the current frame, one random colour per keyframe tree) are the caller's to assign from the
 * frame sizes.                                                                                                               */
int amk_kfmap_points_host(amk_kfmap *map, int scene, float *h_xyz, long long capacity_points, int *h_frame_sizes,
                          long long *n_points_out);
/* The same two queries over a caller's list of frame handles (the frame model of amk_step_batch_frames): frames[f] are obstacle
 * OR edge handles, as the caller chooses, frame 0 the current one; n_frames <= AMK_MAX_FRAMES (else AMK_ERR_UNSUPPORTED); every
 * handle holds the same number of scenes S.  d_Twc [S][16] or NULL (every query counts as inside the current frame); d_Twc
 * without cam is AMK_ERR_INVALID_ARG.  Scan-mode handles and handles in AMK_TIES_NANOFLANN / AMK_TIES_AUTO return
 * AMK_ERR_UNSUPPORTED before anything is launched: the multi-frame query answers in the default tie order only.              */
int amk_kd_query_frames(amk_kd *const *frames, int n_frames, const double *d_Twc, const struct amk_frame_camera *cam,
                        const double *d_queries, int query_stride, int n_queries, int k, float *d_pts, double *d_sqdist,
                        int *d_frame, int *d_counts, void *stream);
int amk_kd_nearest_distance_frames(amk_kd *const *frames, int n_frames, const double *d_queries, int query_stride,
                                   int n_queries, double *d_dist, void *stream);
int amk_kd_query_frames_host(amk_kd *const *frames, int n_frames, const double *h_Twc, const struct amk_frame_camera *cam,
                             const double *h_queries, int query_stride, int n_queries, int k, float *h_pts, double *h_sqdist,
                             int *h_frame, int *h_counts);
/* Radius search over the frames: amk_kd_radius_search (see there: radius_sq, the strict test, the uncapped count, max_results,
 * the errors) over every frame a scene holds -- a keyframe map's query vector, or a caller's list of frame handles.  This is
 * nanoflann's query, not FrameKDMap::QueryNearest: there is no fast path and no PtIsInFrame, and no size rule -- every frame the
 * scene holds contributes, whatever its size.
 *   d_counts [S][n_queries]               the SUM over the frames of the usable points within the radius (never capped)
 *   d_pts / d_sqdist / d_frame [S][n_queries][max_results]   the min(count, max_results) nearest of all frames, ascending by
 *               squared distance; equal distances keep the earlier frame, then the lower cloud index within a frame; d_frame is
 *               the position in the query vector (0 = current frame).  Slots beyond the results hold (0,0,0) / DBL_MAX / -1.
 *               Each output may be NULL, not all; max_results == 0 (the pure count) requires the three lists NULL.
 *   query_edge  != 0: the frames' edge clouds, else their obstacle clouds
 * A scene with no frame yet answers 0.  The map's tie order (amk_kfmap_set_tie_order) does not apply, nor does that of the
 * handles of a list; scan-mode handles and n_frames > AMK_MAX_FRAMES return AMK_ERR_UNSUPPORTED before anything is launched.
 * Stream-ordered, nothing allocated, no map state changed; ordering against amk_kfmap_add_vertex / _update / _reset and index
 * builds as stated for the map's own queries above.  The *_host variants stage through device memory and synchronise the device. */
int amk_kfmap_radius_search(amk_kfmap *map, const double *d_queries, int query_stride, int n_queries, double radius_sq,
                            int max_results, int query_edge, float *d_pts, double *d_sqdist, int *d_frame, int *d_counts,
                            void *stream);
int amk_kfmap_radius_search_host(amk_kfmap *map, const double *h_queries, int query_stride, int n_queries, double radius_sq,
                                 int max_results, int query_edge, float *h_pts, double *h_sqdist, int *h_frame, int *h_counts);
int amk_kd_radius_search_frames(amk_kd *const *frames, int n_frames, const double *d_queries, int query_stride, int n_queries,
                                double radius_sq, int max_results, float *d_pts, double *d_sqdist, int *d_frame, int *d_counts,
                                void *stream);
int amk_kd_radius_search_frames_host(amk_kd *const *frames, int n_frames, const double *h_queries, int query_stride, int n_queries,
                                     double radius_sq, int max_results, float *h_pts, double *h_sqdist, int *h_frame,
                                     int *h_counts);
/* Segment search over the frames: amk_kd_segment_search (see there: the path's layout, the per-leg and per-point values, radius_sq,
 * the strict test, the uncapped count, max_results, the errors) over every frame a scene holds -- a keyframe map's query vector,
 * or a caller's list of frame handles; no fast path, no PtIsInFrame, no size rule, as for the radius search over the frames.
 *   d_counts [S][n_legs]                  the SUM over the frames of the leg's results (never capped)
 *   d_pts / d_sqdist / d_t / d_frame [S][n_legs][max_results]   the min(count, max_results) nearest of all frames, ascending by
 *               d2; equal d2: the earlier frame first, then the lower cloud index within a frame; d_frame is the position in the
 *               query vector (0 = current frame).  Empty slots hold (0,0,0) / DBL_MAX / 0.0 / -1.  Each output may be NULL,
 *               not all; max_results == 0 (the pure count) requires the four lists NULL.
 *   query_edge  != 0: the frames' edge clouds, else their obstacle clouds
 * A scene with no frame yet answers 0.  Tie orders do not apply; scan-mode handles and n_frames > AMK_MAX_FRAMES return
 * AMK_ERR_UNSUPPORTED before anything is launched.  Stream-ordered, nothing allocated, no map state changed; ordering against
 * the map's updates as stated for its own queries above.  The *_host variants stage through device memory and synchronise the
 * device.                                                                                                                    */
int amk_kfmap_segment_search(amk_kfmap *map, const double *d_path, int point_stride, int n_points, double radius_sq,
                             int max_results, int query_edge, float *d_pts, double *d_sqdist, double *d_t, int *d_frame,
                             int *d_counts, void *stream);
int amk_kfmap_segment_search_host(amk_kfmap *map, const double *h_path, int point_stride, int n_points, double radius_sq,
                                  int max_results, int query_edge, float *h_pts, double *h_sqdist, double *h_t, int *h_frame,
                                  int *h_counts);
int amk_kd_segment_search_frames(amk_kd *const *frames, int n_frames, const double *d_path, int point_stride, int n_points,
                                 double radius_sq, int max_results, float *d_pts, double *d_sqdist, double *d_t, int *d_frame,
                                 int *d_counts, void *stream);
int amk_kd_segment_search_frames_host(amk_kd *const *frames, int n_frames, const double *h_path, int point_stride, int n_points,
                                      double radius_sq, int max_results, float *h_pts, double *h_sqdist, double *h_t,
                                      int *h_frame, int *h_counts);
/* Segment nearest over the frames: amk_kd_segment_nearest (see there: the path, the per-leg result, k, the errors, the two
 * identities) over every frame a scene holds -- a keyframe map's query vector, or a caller's list of frame handles; no fast path,
 * no PtIsInFrame, no size rule.  The answer is the k nearest of all frames a scene holds.
 *   d_pts / d_sqdist / d_t / d_frame [S][n_legs][k]   ascending by d2; equal d2 keep the earlier frame, then the lower index
 *               within a frame; d_frame is the position in the query vector (0 = current frame), -1 in empty slots, which hold
 *               (0,0,0) / DBL_MAX / 0.0 otherwise.  Each output may be NULL, not all.
 *   d_counts [S][n_legs]                  min(k, sum of the frames' usable points)
 *   query_edge  != 0: the frames' edge clouds, else their obstacle clouds
 * A map scene with no frame answers 0.  A map in AMK_TIES_NANOFLANN answers like the default.  Scan-mode handles and
 * n_frames > AMK_MAX_FRAMES return AMK_ERR_UNSUPPORTED before anything is staged or launched.  Stream-ordered, nothing
 * allocated, no map state changed; ordering against the map's updates as stated for its own queries above.  The *_host variants
 * stage and synchronise exactly as their segment-search counterparts do.                                                     */
int amk_kfmap_segment_nearest(amk_kfmap *map, const double *d_path, int point_stride, int n_points, int k, int query_edge,
                              float *d_pts, double *d_sqdist, double *d_t, int *d_frame, int *d_counts, void *stream);
int amk_kfmap_segment_nearest_host(amk_kfmap *map, const double *h_path, int point_stride, int n_points, int k, int query_edge,
                                   float *h_pts, double *h_sqdist, double *h_t, int *h_frame, int *h_counts);
int amk_kd_segment_nearest_frames(amk_kd *const *frames, int n_frames, const double *d_path, int point_stride, int n_points,
                                  int k, float *d_pts, double *d_sqdist, double *d_t, int *d_frame, int *d_counts, void *stream);
int amk_kd_segment_nearest_frames_host(amk_kd *const *frames, int n_frames, const double *h_path, int point_stride,
                                       int n_points, int k, float *h_pts, double *h_sqdist, double *h_t, int *h_frame,
                                       int *h_counts);

/* Segment cast over the frames: amk_kd_segment_cast (see there: the path, radius_sq, the per-point arithmetic, the strict tests,
 * the errors) over every frame a scene holds -- a keyframe map's query vector, or a caller's list of frame handles; no fast path,
 * no PtIsInFrame, no size rule.  The answer of a leg is the usable point of all frames with the smallest t; equal t keeps the
 * earlier frame, then the lower cloud index within a frame.
 *   d_hit / d_t [S][n_legs], d_pts [S][n_legs][3]   as for one handle: 1 or 0; where the contact begins, 1.0 without one; the point
 *               touched, (0,0,0) if none
 *   d_frame [S][n_legs]                   the frame touched, its position in the query vector (0 = current frame), -1 if none
 *   query_edge  != 0: the frames' edge clouds, else their obstacle clouds
 * Each output may be NULL, not all.  A map scene with no frame answers no contact.  A map in AMK_TIES_NANOFLANN answers like the
 * default.  Scan-mode handles, tie-order handles in the frame list and n_frames > AMK_MAX_FRAMES return AMK_ERR_UNSUPPORTED
 * before anything is staged or launched.  Stream-ordered, nothing allocated, no map state changed; ordering against the map's
 * updates as stated for its own queries above.  The *_host variants stage and synchronise exactly as their segment-search
 * counterparts do.                                                                                                           */
int amk_kfmap_segment_cast(amk_kfmap *map, const double *d_path, int point_stride, int n_points, double radius_sq, int query_edge,
                           int *d_hit, double *d_t, float *d_pts, int *d_frame, void *stream);
int amk_kfmap_segment_cast_host(amk_kfmap *map, const double *h_path, int point_stride, int n_points, double radius_sq,
                                int query_edge, int *h_hit, double *h_t, float *h_pts, int *h_frame);
int amk_kd_segment_cast_frames(amk_kd *const *frames, int n_frames, const double *d_path, int point_stride, int n_points,
                               double radius_sq, int *d_hit, double *d_t, float *d_pts, int *d_frame, void *stream);
int amk_kd_segment_cast_frames_host(amk_kd *const *frames, int n_frames, const double *h_path, int point_stride, int n_points,
                                    double radius_sq, int *h_hit, double *h_t, float *h_pts, int *h_frame);

/* Path cast over the frames: amk_kd_path_cast (see there: the stop leg, d_stop / d_leg / d_t / d_free, the identity, the errors)
 * with every leg answered as "Segment cast over the frames" answers it: the contact of a leg is the least (t, frame, index) over
 * the frames its scene holds.  d_frame [S] takes the place of d_indices: the frame touched, -1 unless d_stop is 1.  The answer
 * equals the reduction applied to amk_kfmap_segment_cast's (amk_kd_segment_cast_frames') per-leg outputs, bit for bit.  A map
 * scene with no frame is free to the end unless a leg is unjudgeable.  Scan-mode handles, tie-order handles in the frame list and
 * n_frames > AMK_MAX_FRAMES return AMK_ERR_UNSUPPORTED before anything is staged or launched.  Stream-ordered, nothing allocated,
 * no map state changed.  The *_host variants stage and synchronise exactly as their segment-cast counterparts do.              */
int amk_kfmap_path_cast(amk_kfmap *map, const double *d_path, int point_stride, int n_points, double radius_sq, int query_edge,
                        int *d_stop, int *d_leg, double *d_t, double *d_free, float *d_pts, int *d_frame, void *stream);
int amk_kfmap_path_cast_host(amk_kfmap *map, const double *h_path, int point_stride, int n_points, double radius_sq, int query_edge,
                             int *h_stop, int *h_leg, double *h_t, double *h_free, float *h_pts, int *h_frame);
int amk_kd_path_cast_frames(amk_kd *const *frames, int n_frames, const double *d_path, int point_stride, int n_points,
                            double radius_sq, int *d_stop, int *d_leg, double *d_t, double *d_free, float *d_pts, int *d_frame,
                            void *stream);
int amk_kd_path_cast_frames_host(amk_kd *const *frames, int n_frames, const double *h_path, int point_stride, int n_points,
                                 double radius_sq, int *h_stop, int *h_leg, double *h_t, double *h_free, float *h_pts, int *h_frame);

/* ------------------------------------------------------------------------------------------ */
/* Scenes sharded over the GPUs of a node (one process per GPU), RCCL over xGMI                 */
/* ------------------------------------------------------------------------------------------ */
/* Scenes are independent (the reference runs a single instance, mpc_obstacle_avoidance_node.cpp:8): block partition, no
 * data-path collective; the one exchange step is an ncclAllGather of the controls.  Rank 0 makes the id, the host
 * distributes its AMK_SHARD_ID_BYTES bytes by its own means (MPI, TCP, a file), every rank calls amk_shard_create with
 * its GPU current.  RCCL is bound at run time; AMK_ERR_UNSUPPORTED when librccl cannot be loaded.                        */
typedef struct amk_shard amk_shard;
#define AMK_SHARD_ID_BYTES 128
int amk_shard_scene_range(int rank, int world, int total, int *first, int *count);
int amk_shard_unique_id(char *id_out /* [AMK_SHARD_ID_BYTES] */);
int amk_shard_create(const char *id, int rank, int world, amk_shard **out);
int amk_shard_destroy(amk_shard *s);
int amk_shard_rank(const amk_shard *s);
int amk_shard_world(const amk_shard *s);
int amk_shard_last_rccl_error(void);
/* d_all[r * n + i] = rank r's d_local[i]; stream-ordered.  ncclAllGather needs the SAME count on every rank: when
 * total % world != 0 the counts of amk_shard_scene_range differ by one, so every rank passes the PADDED shard size
 * amk_shard_padded_count(world, total) = ceil(total / world) (its buffers sized for it; rows beyond its own count are
 * padding) -- passing the natural `count` would hang or corrupt d_all.  amk_shard_gather_u: n_local_scenes is that padded
 * size too (4 doubles per scene).                                                                                      */
int amk_shard_padded_count(int world, int total);
int amk_shard_gather(amk_shard *s, const double *d_local, long long n_doubles_per_rank, double *d_all, void *stream);
int amk_shard_gather_u(amk_shard *s, const double *d_u_local, int n_local_scenes, double *d_u_all, void *stream);
int amk_shard_max(amk_shard *s, double *d_values, int n, void *stream);   /* in-place max over ranks (timing)              */
/* Which RCCL was bound (the copy already in the process -- e.g. PyTorch's -- if there is one, else librccl.so.1 from the loader
 * path): file of ncclAllGather, ncclGetVersion's code, 1 if it had been loaded before this library asked.  A host prints
 * this next to its results so that the first multi-GPU run can be diagnosed (bench.py: config.rccl).                       */
int amk_shard_rccl_info(char *path, int path_len, int *version, int *was_loaded);
/* Watchdog: host-side wait (polling, <= timeout_s) for everything queued on `stream`, the gathers included.
 * AMK_ERR_TIMEOUT: a collective hangs (a rank that never entered it, a link, two RCCLs in one process): exit and re-run with
 * NCCL_DEBUG=INFO NCCL_DEBUG_SUBSYS=INIT,COLL.                                                                             */
int amk_shard_wait(amk_shard *s, void *stream, double timeout_s);

/* ------------------------------------------------------------------------------------------ */
/* Depth image -> obstacle cloud: FrameKDMap::ProcessDepth            FrameKDMap.cpp:75-138   */
/* (the step immediately before the tree build)                   */
/* ------------------------------------------------------------------------------------------ */
/* amk_depth_params: defined with the pipeline, above */

#define AMK_DEPTH_U16 0   /* CV_16UC1 */
#define AMK_DEPTH_F32 1   /* CV_32FC1 */

/* Width / height of the down-scaled image = capacity of the output cloud per scene (FrameKDMap.cpp:106-107). */
int amk_depth_out_size(int rows, int cols, double resize_scale, int *out_w, int *out_h);

/* For every scene: inverse depth of the raw pixels with the range gate (GetInvDepthImg, :76-89), bilinear
 * down-scale (cv::resize with dsize given: its 4th positional argument cv::INTER_MAX lands in `fx`, so the
 * interpolation is the default INTER_LINEAR, :109), back-projection of every pixel with inverse depth >= 1e-2
 * and min < depth < max through the scaled intrinsics (:110-118,131-138), transform by Twb * Tbc (:119-120),
 * points appended in row-major pixel order as float32 (:122).
 *   d_depth   [S][rows][cols] uint16 or float32, scene_stride in ELEMENTS
 *   d_Twb     [S][16] world <- body, row-major
 *   d_cloud   [S][W*H][point_stride] float32 out (point_stride 3 or 4: feeds amk_kd_build directly),
 *             cloud_scene_stride in floats;  d_counts [S] out: points written per scene.
 * Invalid pixels: a float32 NaN (what 32FC1 frames mark invalid pixels with) passes the first range gate as in the
 * reference (both comparisons are false), becomes a NaN inverse depth, spreads to every down-scaled pixel one of whose
 * four taps reads it (also through a border tap of weight 0) and falls out at the second gate; +-inf, negative and
 * denormal pixels fail the first gate like 0 (inverse depth 0).  No emitted coordinate is non-finite while the pose is
 * finite; a NaN in d_Twb gives NaN coordinates (a NaN x is what amk_kd_build drops).
 * Arithmetic contract: DESIGN.md section 10 (float bilinear taps in OpenCV's order without FMA, double
 * back-projection and transform without FMA); bit-exact against oracle/depth_oracle.c.  Parity with OpenCV's
 * own resize and Eigen's -march=native products is unpinned (neither is in the image).                       */
int amk_depth_to_cloud(const void *d_depth, int depth_type, int rows, int cols, long long scene_stride,
                       int n_scenes, const amk_depth_params *params, const double *d_Twb, float *d_cloud,
                       int point_stride, long long cloud_scene_stride, int *d_counts, void *stream);
int amk_depth_to_cloud_host(const void *h_depth, int depth_type, int rows, int cols, long long scene_stride,
                            int n_scenes, const amk_depth_params *params, const double *h_Twb, float *h_cloud,
                            int point_stride, long long cloud_scene_stride, int *h_counts);

/* Depth image -> edge cloud: FrameKDMap::BuildEdgeCloud (FrameKDMap.cpp:176-214), the
 * input of the Edge-KD-tree.  On the down-scaled inverse-depth image of amk_depth_to_cloud: 8-bit quantisation
 * uchar(depth / (max - min) * 200), 255 where invalid (:180-193); cv::erode with a 3x3 kernel (:194);
 * cv::Canny(img, 0.1, 0.3) (:196: aperture 3, L1 norm, thresholds floor to 0, so every pixel that survives the
 * non-maximum suppression with a non-zero Sobel magnitude is an edge); the edge pixels are back-projected at their
 * QUANTISED, ERODED depth (:199-200) and transformed by d_Twc * Tbc, appended in row-major order.
 *   d_Twc [S][16]  the matrix the reference multiplies with Tbc at :209: mCurFrame.Twc, i.e. the PREVIOUS frame's
 *                  Twb * Tbc (it is updated only after ProcessDepth, :50).  Pass Twb of the current frame instead to
 *                  get what the authors presumably meant.
 * The edge cloud of a scene is empty when its obstacle cloud is (:126-128).  Down-scaled images of more than
 * AMK_EDGE_MAX_PIXELS pixels: AMK_ERR_UNSUPPORTED (amk_depth_to_clouds below takes any size).  Bit-exact against
 * oracle/depth_oracle.c; parity with OpenCV's own erode / Canny is unpinned.             */
#define AMK_EDGE_MAX_PIXELS 16000
int amk_depth_to_edge_cloud(const void *d_depth, int depth_type, int rows, int cols, long long scene_stride,
                            int n_scenes, const amk_depth_params *params, const double *d_Twc, float *d_cloud,
                            int point_stride, long long cloud_scene_stride, int *d_counts, void *stream);
int amk_depth_to_edge_cloud_host(const void *h_depth, int depth_type, int rows, int cols, long long scene_stride,
                                 int n_scenes, const amk_depth_params *params, const double *h_Twc, float *h_cloud,
                                 int point_stride, long long cloud_scene_stride, int *h_counts);

/* Depth image -> both clouds in one call: AddVertex's image half, ProcessDepth followed by BuildEdgeCloud
 * (FrameKDMap.cpp:90-130,176-214), for down-scaled images of ANY size.  For every scene d_cloud / d_counts hold, bit
 * for bit and in the same order, what amk_depth_to_cloud(..., d_Twb, ...) writes, and d_edge / d_edge_counts what
 * amk_depth_to_edge_cloud(..., d_Twc, ...) writes (d_Twc = mCurFrame.Twc, the PREVIOUS frame's Twb * Tbc: the stale pose
 * is kept; the edge cloud of a scene is empty when its obstacle cloud is).  Only the first counts[s] points of a
 * scene are written.
 * Down-scaled images of at most AMK_EDGE_MAX_PIXELS pixels run the two kernels of those calls.  Larger ones are cut
 * into bands of whole down-scaled rows, one workgroup per band and scene, in two launches: the first counts the
 * kept pixels and the edge points of every band into the workspace, the second sums the counts of the bands before
 * its own and writes its points there, so the order is the row-major pixel order at any size and no atomic decides
 * it.  A band holds its rows and a halo of 3 on each side in LDS (quantised depth, erosion, Sobel magnitude), which
 * bounds the down-scaled WIDTH: more than AMK_DEPTH_MAX_WIDTH columns: AMK_ERR_UNSUPPORTED (and so are more than 65 535 scenes
 * in one call above AMK_EDGE_MAX_PIXELS pixels: the scenes are the grid's second dimension).
 *   d_work / work_bytes   the caller's workspace, at least amk_depth_clouds_work_bytes(rows, cols, resize_scale,
 *                         n_scenes) bytes (host arithmetic, needs no GPU; covers any band height), 8-byte aligned.
 * Stream-ordered and re-entrant: no allocation, no hidden state.  amk_depth_to_clouds_host takes host pointers,
 * allocates its own workspace and synchronises (one upload of the image for both clouds).                       */
#define AMK_DEPTH_MAX_WIDTH 2048
int amk_depth_clouds_work_bytes(int rows, int cols, double resize_scale, int n_scenes, long long *bytes_out);
int amk_depth_to_clouds(const void *d_depth, int depth_type, int rows, int cols, long long scene_stride, int n_scenes,
                        const amk_depth_params *params, const double *d_Twb, const double *d_Twc, float *d_cloud,
                        long long cloud_scene_stride, int *d_counts, float *d_edge, long long edge_scene_stride,
                        int *d_edge_counts, int point_stride, void *d_work, long long work_bytes, void *stream);
int amk_depth_to_clouds_host(const void *h_depth, int depth_type, int rows, int cols, long long scene_stride,
                             int n_scenes, const amk_depth_params *params, const double *h_Twb, const double *h_Twc,
                             float *h_cloud, long long cloud_scene_stride, int *h_counts, float *h_edge,
                             long long edge_scene_stride, int *h_edge_counts, int point_stride);

/* ------------------------------------------------------------------------------------------ */
/* Closed-loop simulation: the depth sensor and the vehicle on the device                      */
/* (the two ends of a flight around amk_pipeline_submit; DESIGN.md "Closed loop on the device") */
/* ------------------------------------------------------------------------------------------ */
/* The reference flies AirSim (DepthPlanar frames, AM/src/AvoidanceStateMachine.cpp:153-164) and bfctrl; neither is here.  These two
 * calls stand in for them so that a fleet flies from a world description to commands with no host round trip:
 *   amk_pipeline_submit(d_depth, d_Twb, d_odom = x, d_cmd_out = cmd) -> amk_pipeline_wait_stream -> amk_sim_vehicle_step(cmd, x, Twb)
 *   -> amk_sim_render_depth(Twb, depth) -> the next submit, ordered by amk_pipeline_frame.input_ready.
 *
 * amk_sim_render_depth: the depth image a pinhole camera sees in a world of vertical cylinders on a ground plane.
 *   d_cyl         [S][max_cyl][3] double = (cx, cy, r): scene s holds counts[s] vertical cylinders, each standing on the ground
 *                 plane z = 0 and cut at z_top (the world of the bench's synthetic clouds).  May be NULL when max_cyl == 0.
 *   d_cyl_counts  [S] or NULL = max_cyl in every scene; a count outside [0, max_cyl] is clamped into it.
 *   params        the sensor: FULL-resolution fx, fy, cx, cy, Tbc and pixel2meter (> 0); depth_min / depth_max / resize_scale are
 *                 not read (they belong to the consumer, amk_depth_to_clouds).
 *   d_Twb         [S][16] world <- body, row-major; the camera sits at Twc = Twb * Tbc.
 *   d_depth       [S][rows][cols] out, AMK_DEPTH_U16 or AMK_DEPTH_F32.  0 means no return within max_range; a return holds the
 *                 PLANAR depth t (the hit's z in the camera frame), which is what UV2Camera back-projects, in the units
 *                 amk_depth_to_cloud reads: F32 = float32(t) / float32(pixel2meter), the correctly rounded float32 quotient;
 *                 U16 = that value rounded to the nearest integer, ties to even, clamped to [0, 65535]
 *                 (rint(t / pixel2meter) on the float32 image, as numpy's round does it).
 * Arithmetic: fp64, no contraction, every sum left to right in index order, so that a restatement in any IEEE language matches it
 * operation for operation (avoid_mpc_amd/flight.py render_depth_ordered is one):
 *   Twc_ij = ((Twb_i0 Tbc_0j + Twb_i1 Tbc_1j) + Twb_i2 Tbc_2j) + Twb_i3 Tbc_3j;  R, o = its rotation and translation
 *   pixel (u, v) = (column, row):  dc = ((u - cx) / fx, (v - cy) / fy, 1),  d_i = (R_i0 dc_0 + R_i1 dc_1) + R_i2 dc_2
 *   ground:      t = -o_z / d_z                                  a hit when d_z < 0 and t > 0
 *   cylinder k:  ox = o_x - cx_k, oy = o_y - cy_k, a = d_x d_x + d_y d_y, b = ox d_x + oy d_y, c = (ox ox + oy oy) - r r,
 *                disc = b b - a c;  for disc >= 0: t = (-b - sqrt(disc)) / a, z = o_z + t d_z
 *                                                                a hit when t > 0 && 0 <= z <= z_top
 *   The pixel takes the least t.  The comparison is a strict <, so on equal t the ground and then the lower cylinder index keep it.
 *   The pixel's t is kept when t <= max_range, else it is 0.
 * A vertical ray (a == 0) and a camera inside a cylinder behave as the formulas say: a NaN or negative t is no hit.
 * AMK_ERR_INVALID_ARG: a NULL pointer (d_cyl_counts excepted), rows or cols < 1, max_cyl < 0, n_scenes < 1, a negative or NaN z_top
 * or max_range, pixel2meter not > 0, an unknown depth_type.  AMK_ERR_UNSUPPORTED: a launch grid beyond 2^31 - 1 blocks (256 pixels
 * per block) or more than 65 535 scenes (the scenes are the grid's second dimension).  Every error is returned before anything is
 * launched.  The call is stream-ordered and allocates nothing.  amk_sim_render_depth_host takes host pointers, stages them and
 * synchronises.                                                                                                             */
int amk_sim_render_depth(const double *d_cyl, const int *d_cyl_counts, int max_cyl, int n_scenes, double z_top, double max_range,
                         const amk_depth_params *params, int rows, int cols, const double *d_Twb, void *d_depth, int depth_type,
                         void *stream);
int amk_sim_render_depth_host(const double *h_cyl, const int *h_cyl_counts, int max_cyl, int n_scenes, double z_top,
                              double max_range, const amk_depth_params *params, int rows, int cols, const double *h_Twb,
                              void *h_depth, int depth_type);

/* amk_sim_vehicle_step: the vehicle over one control period.  Its model is the MPC's own (mpc_obstacle_casadi.py:106-122 integrated by
 * :338-357), which is exactly affine for fixed time constants: x+ = A x + B u + c.
 *   h_ABc   HOST pointer to 150 doubles, A [10][10], B [10][4], c [10], handed to the kernel by value: the model at the CALLER's
 *           control period (the node's con_dt, which need not be the MPC's dt), from wherever the caller has it.
 *   d_cmd   [S][3] the published acceleration command (amk_pipeline_frame.d_cmd_out); u = (cmd, yaw_dot = 0): Command.yaw = 0 holds
 *           the heading (AvoidanceStateMachine.cpp:376).
 *   d_x     [S][10] in/out, the layout of amk_pipeline_frame.d_odom: [p(3), yaw, v(3), a(3)].  One buffer is the plant, the
 *           odometry of the next submit and the clock model's input.
 *   d_Twb   [S][16] out or NULL: [Rz(yaw) | p'] of the NEW state, row-major, p' = rint(p q) / q for pose_quantum q > 0 (q = 1e6: the
 *           pose rounded to a micrometre, numpy's round(p, 6)); q = 0: p' = p.  At yaw == 0 the rotation is exactly the identity;
 *           otherwise its entries are the device's cos / sin of the yaw.
 * Arithmetic: x+_i = ((sum_j A_ij x_j) + (sum_j B_ij u_j)) + c_i, fp64, no contraction, each sum left to right from j = 0 (the
 * u_3 = 0 term included).  AMK_ERR_INVALID_ARG: a NULL pointer (d_Twb excepted), n_scenes < 1, a negative or NaN pose_quantum --
 * returned before anything is launched.  Stream-ordered; allocates nothing.  amk_sim_vehicle_step_host takes host pointers.    */
int amk_sim_vehicle_step(const double *h_ABc, const double *d_cmd, double *d_x, double *d_Twb, int n_scenes, double pose_quantum,
                         void *stream);
int amk_sim_vehicle_step_host(const double *h_ABc, const double *h_cmd, double *h_x, double *h_Twb, int n_scenes,
                              double pose_quantum);

/* amk_sim_render_world: amk_sim_render_depth in a world that also holds boxes -- walls, gates, lintels, beams.  Every argument it
 * shares with amk_sim_render_depth means what it means there, and so do Twc, the ray d, the ground, the cylinders, max_range and
 * both pixel types, word for word.
 *   d_box         [S][max_box][8] double = (cx, cy, hx, hy, c, s, z0, z1): a box centred at (cx, cy) in the ground plane, with half
 *                 extents hx, hy along its own axes, turned about the vertical by the yaw whose cosine and sine the CALLER computed
 *                 (c, s): the device evaluates no transcendental and does not renormalise them.  [z0, z1] is the box's own vertical
 *                 extent; it is not cut at z_top, and z0 > 0 is a floating box.  May be NULL when max_box == 0.
 *   d_box_counts  [S] or NULL = max_box in every scene; a count outside [0, max_box] is clamped into it.
 * Arithmetic, continuing the contract above (fp64, no contraction, left to right, IEEE division; avoid_mpc_amd/flight.py
 * render_world_ordered restates it).  With o the camera position and d the ray, per box:
 *   ox = o_x - cx, oy = o_y - cy;  olx = c ox + s oy, oly = c oy - s ox;  dlx = c d_x + s d_y, dly = c d_y - s d_x
 *   three slabs (o, d, lo, hi), in this order: x (olx, dlx, -hx, hx), y (oly, dly, -hy, hy), z (o_z, d_z, z0, z1)
 *   a slab with d != 0:  inv = 1.0 / d, t1 = (lo - o) inv, t2 = (hi - o) inv, near = t1 < t2 ? t1 : t2, far = t1 < t2 ? t2 : t1
 *                        (one reciprocal per slab, no division per bound)
 *   a slab with d == 0:  the ray is parallel to it.  near = -inf, far = +inf when lo <= o && o <= hi: the slab imposes no bound.
 *                        Otherwise near = +inf, far = -inf: the box is missed.
 *   tn = n_x > n_y ? n_x : n_y, then n_z > tn ? n_z : tn;  tf = f_x < f_y ? f_x : f_y, then f_z < tf ? f_z : tf
 *   a hit at t = tn when  n_x <= f_x && n_y <= f_y && n_z <= f_z && tn > 0 && tn <= tf.
 * A grazing ray counts (tn == tf is a hit, as disc == 0 is for a cylinder).  A camera inside a box gets no return from that box
 * (tn <= 0), as a camera inside a cylinder gets none from it.  A NaN anywhere -- in a box entry, in the pose -- makes some slab's
 * near or far a NaN, which fails that slab's near <= far: no hit from that box, and the other boxes are not affected.  A negative half
 * extent gives the box of its absolute value to every ray that is not parallel to that slab (near and far are ordered by the
 * comparison) and misses every ray that is (lo <= o <= hi cannot hold); z1 < z0 does the same for the z slab.
 * Order: the ground, then the cylinders in index order, then the boxes in index order.  The pixel takes the least t under the same
 * strict <, so on equal t the earlier one keeps it.
 * AMK_ERR_INVALID_ARG: what amk_sim_render_depth refuses, max_box < 0, a NULL d_box with max_box > 0.  AMK_ERR_UNSUPPORTED: as there.
 * Every error is returned before anything is launched.  The call is stream-ordered and allocates nothing.  With max_box == 0 it is
 * amk_sim_render_depth's own launch.  amk_sim_render_world_host takes host pointers, stages them and synchronises.            */
int amk_sim_render_world(const double *d_cyl, const int *d_cyl_counts, int max_cyl, const double *d_box, const int *d_box_counts,
                         int max_box, int n_scenes, double z_top, double max_range, const amk_depth_params *params, int rows,
                         int cols, const double *d_Twb, void *d_depth, int depth_type, void *stream);
int amk_sim_render_world_host(const double *h_cyl, const int *h_cyl_counts, int max_cyl, const double *h_box,
                              const int *h_box_counts, int max_box, int n_scenes, double z_top, double max_range,
                              const amk_depth_params *params, int rows, int cols, const double *h_Twb, void *h_depth,
                              int depth_type);

/* amk_sim_vehicle_step_att: amk_sim_vehicle_step with a choice of the rotation written into d_Twb.  The state update, p' and every
 * argument it shares with amk_sim_vehicle_step are that call's; only the rotation differs.
 *   attitude  AMK_SIM_ATT_YAW: [Rz(yaw) | p'], amk_sim_vehicle_step bit for bit in x and Twb.
 *             AMK_SIM_ATT_ACCEL: the vehicle tilts into its thrust, [acc2rotmat(a + (0, 0, gz), yaw) | p'] of the NEW state
 *             (mpc_obstacle_casadi.py:253-264), so a forward camera looks at the ground while the vehicle accelerates.
 *   gz        the caller's gravity (the generator's: 9.81), >= 0.
 * Arithmetic of AMK_SIM_ATT_ACCEL: fp64, no contraction, left to right, IEEE division and square root.  cs, sn are exactly the yaw
 * mode's, so 1 and 0 at yaw == 0 and the device's cos / sin otherwise:
 *   T  = (a_0, a_1, a_2 + gz);  n = sqrt((T_0 T_0 + T_1 T_1) + T_2 T_2);  zb = T / n
 *   y' = (0.0 - zb_2 sn, zb_2 cs, zb_0 sn - zb_1 cs);  m = sqrt((y'_0 y'_0 + y'_1 y'_1) + y'_2 y'_2);  yb = y' / m
 *   xb = (yb_1 zb_2 - yb_2 zb_1, yb_2 zb_0 - yb_0 zb_2, yb_0 zb_1 - yb_1 zb_0);  R = [xb yb zb] (columns)
 * Unless n > 0 && m > 0 the rotation falls back to Rz(yaw): free fall, a NaN, thrust along the heading.  At a == 0 and yaw == 0 the
 * rotation is exactly the identity, and at yaw == 0 there is no transcendental in it.
 * AMK_ERR_INVALID_ARG: what amk_sim_vehicle_step refuses, an unknown attitude, a NaN or negative gz -- returned before anything is
 * launched.  Stream-ordered; allocates nothing.  amk_sim_vehicle_step_att_host takes host pointers.                           */
#define AMK_SIM_ATT_YAW   0   /* [Rz(yaw) | p']: amk_sim_vehicle_step, bit for bit            */
#define AMK_SIM_ATT_ACCEL 1   /* [acc2rotmat(a + (0,0,gz), yaw) | p'] of the NEW state       */
int amk_sim_vehicle_step_att(const double *h_ABc, const double *d_cmd, double *d_x, double *d_Twb, int n_scenes, double pose_quantum,
                             int attitude, double gz, void *stream);
int amk_sim_vehicle_step_att_host(const double *h_ABc, const double *h_cmd, double *h_x, double *h_Twb, int n_scenes,
                                  double pose_quantum, int attitude, double gz);

/* Ground truth against the simulated world: clearance, segment cast and path cast against the TRUE solids.
 * The map queries (amk_kd_segment_cast, amk_kd_path_cast, amk_pipeline_set_path_audit) judge a position or a plan against what the
 * robot has seen.  These three judge it against the world amk_sim_render_world renders, on the device and in the same output shapes,
 * so that a monitor holds both verdicts per robot and period without a host round trip.
 * Every entry begins with the world arguments of amk_sim_render_world, in that order and with those meanings:
 *   (d_cyl [S][max_cyl][3], d_cyl_counts | NULL, max_cyl, d_box [S][max_box][8], d_box_counts | NULL, max_box, n_scenes, z_top, ...)
 * Counts are clamped into [0, max].  max_cyl == 0 and max_box == 0 are allowed with NULL lists; with both zero the world is the
 * ground alone.  Points and paths are double [S][n_points][point_stride], point_stride >= 3, x y z leading each row, as the KD
 * queries take them: d_odom (stride 10, one point) and x0array (stride 14, N rows) go in as they are.
 * Arithmetic: fp64, no contraction, every sum left to right as written; division, reciprocal and square root are IEEE-correct, so a
 * restatement in any IEEE language matches operation for operation (avoid_mpc_amd/flight.py world_clearance_ordered,
 * world_segment_cast_ordered, world_path_cast_ordered are three).  "x > y ? x : y" below is that comparison and that select.
 * NaN: a two-operand select drops a NaN, so no formula below is trusted to carry one.  A solid with a NaN in any of its entries (three
 * for a cylinder, eight for a box) answers nothing, in the clearance and in the casts: every entry e is tested with e == e in front of
 * the formulas and the solid is passed over.  Infinite entries and non-finite points are not special: they give what the formulas give.
 * Order everywhere: the ground, then the cylinders in index order, then the boxes in index order; the least value wins under a
 * strict <, so on equal values the earlier solid keeps it.
 *
 * amk_sim_clearance: for every point p the signed Euclidean distance to the nearest solid's surface (negative inside) and which
 * solid that is.
 *   d_dist   [S][P] double.   d_kind  [S][P] int: 0 ground, 1 cylinder, 2 box.   d_index  [S][P] int: -1 for the ground.
 *   ground:    dist = p_z
 *   cylinder:  the solid {rho <= r, z <= z_top}.  ox = p_x - cx, oy = p_y - cy;  qr = sqrt(ox ox + oy oy) - r;  qz = p_z - z_top;
 *              mr = qr > 0 ? qr : 0, mz = qz > 0 ? qz : 0;  m = qr > qz ? qr : qz;  dist = sqrt(mr mr + mz mz) + (m < 0 ? m : 0)
 *   box:       ox = p_x - cx, oy = p_y - cy;  olx = c ox + s oy, oly = c oy - s ox (exactly the render's);  qx = |olx| - |hx|,
 *              qy = |oly| - |hy|;  lo = z0 - p_z, hi = p_z - z1, qz = lo > hi ? lo : hi;  mx, my, mz = q > 0 ? q : 0 of each;
 *              m = qx > qy ? qx : qy, then qz > m ? qz : m;  dist = sqrt((mx mx + my my) + mz mz) + (m < 0 ? m : 0)
 *              (flight.box_clearance in three dimensions: outside, the norm of the excess; inside, the largest face term)
 *   The scan starts at the ground's p_z: a NaN height stays NaN with kind 0, since nothing is < NaN.  A distance that comes out NaN
 *   never wins.  Each output may be NULL, but not all of them.
 *
 * amk_sim_segment_cast: per leg of a path, the first contact of a sphere of `radius` >= 0 whose centre moves from point j (a) to point
 * j + 1 (b): d = b - a, t in [0, 1].  Outputs are [S][n_points - 1].  The sphere is judged as its CENTRE against the inflated solids:
 *   ground:    z <= radius
 *   cylinder:  radius R = r + radius, cut at z_top + radius
 *   box:       half extents |hx| + radius, |hy| + radius, vertical extent [z0 - radius, z1 + radius]
 * This is a superset of the true swept sphere (the rounded Minkowski sum): exact on faces and mantles, and over at edges and rims by
 * at most (sqrt(3) - 1) radius.  radius == 0 is the centre line.
 * Every solid is an intersection of per-axis intervals [near, far] of the leg's parameter; inv_z = 1.0 / d_z once per leg:
 *   a half-space z <= h:  bound = (h - a_z) inv_z;  d_z < 0: [bound, +inf];  d_z > 0: [-inf, bound];  d_z == 0: [-inf, +inf] when
 *                         a_z <= h, else [+inf, -inf]
 *   a cylinder's mantle:  ox = a_x - cx, oy = a_y - cy;  a = d_x d_x + d_y d_y, b = ox d_x + oy d_y, c = (ox ox + oy oy) - R R (the
 *                         render's, at the inflated radius);  disc = b b - a c.  a == 0: [-inf, +inf] when c <= 0, else [+inf, -inf].
 *                         Otherwise, for disc >= 0: [(-b - sqrt(disc)) / a, (-b + sqrt(disc)) / a]; else [+inf, -inf]
 *   a box's three slabs:  amk_sim_render_world's slab rule word for word -- x (olx, dlx, -HX, HX), y (oly, dly, -HY, HY),
 *                         z (a_z, d_z, Z0, Z1) with the inflated HX, HY, Z0, Z1, one reciprocal per slab, d == 0 by "lo <= o && o <= hi"
 *   the ground has one axis, a cylinder two (mantle, then z <= z_top + radius), a box three (x, y, z)
 *   tn = the largest near and tf = the smallest far, by comparisons in axis order: tn = n_0 > n_1 ? n_0 : n_1, then n_2 > tn ? n_2 : tn;
 *   tf = f_0 < f_1 ? f_0 : f_1, then f_2 < tf ? f_2 : tf
 *   the solid is touched iff every axis has near <= far, and tn <= tf && tf >= 0 && tn <= 1;  its t is tn > 0 ? tn : 0.0
 * A leg that starts inside a solid touches it at t = 0.  This is the one place the cast differs from the sensor, which returns nothing
 * from inside.  A grazing leg counts (tn == tf), and so does a contact that begins exactly at b (t == 1).
 * The leg's contact is the least t under the strict <, in the order above.  A degenerate leg (a == b) touches iff its start is inside.
 * A leg with a non-finite endpoint coordinate, or a non-finite component of d, has no contact here.
 *   d_hit    [S][L] int: 1 when the leg has a contact, else 0.
 *   d_t      [S][L] double: the t of the contact; 1.0 without one -- free all the way -- so t |d| is the free distance in both cases.
 *   d_kind   [S][L] int: 0 ground, 1 cylinder, 2 box; -1 without a contact.     d_index  [S][L] int: -1 for the ground and for none.
 * Each output may be NULL, but not all of them.
 *
 * amk_sim_path_cast: one verdict per scene, laid out like amk_kd_path_cast's.  The stop leg is the first leg, in leg order, that has
 * a contact by the segment cast's rule or is unjudgeable (the non-finite leg above: an audit must not read a NaN plan as free).
 *   d_stop   [S] int: 0 free to the end, 1 contact, 2 unjudgeable leg.      d_leg  [S] int: the stop leg, -1 when free.
 *   d_t      [S] double: t on the stop leg; 0.0 when d_stop is 2, 1.0 when free.
 *   d_free   [S] double: ((len_0 + len_1) + ...) + t len_leg with len_j = sqrt((d_x d_x + d_y d_y) + d_z d_z), left to right; the last
 *            term is left out when d_stop is 2; a free path gives its whole length.
 *   d_pts    [S][3] double: the sphere's centre at the contact, a_i + t d_i; (0, 0, 0) unless d_stop is 1.
 *   d_kind, d_index  [S] int: the solid touched, as the segment cast names it; -1, -1 unless d_stop is 1.
 * Each output may be NULL, but not all of them.
 * Identity: the answer equals this reduction applied to amk_sim_segment_cast's per-leg outputs on the same path, bit for bit; d_free
 * and d_pts are rebuilt from the path by the formulas.  Legs behind the stop leg's round of legs are not walked.
 *
 * AMK_ERR_INVALID_ARG: NULL points or path, point_stride < 3, n_points < 1 (clearance) or < 2 (casts), radius < 0 or NaN, z_top not
 * >= 0, a negative max, a NULL list with a positive max, every output NULL, n_scenes < 1.  AMK_ERR_UNSUPPORTED: a grid beyond the
 * launch limits -- for the clearance and the segment cast more than 65 535 scenes (the scenes are the grid's second dimension) or
 * more than 4 (2^24 - 1) points or legs per scene (four per block of 256 threads, and a grid dimension times the block size stays
 * below 2^32); for the path cast more than 2^24 - 1 scenes (a block per scene) -- or max_cyl + max_box beyond 2^31 - 2.
 * AMK_ERR_NO_DEVICE: no device.  Every error is returned before anything is staged or launched,
 * the outputs untouched.  The three calls are stream-ordered and allocate nothing.  The _host forms take host pointers, stage them
 * and synchronise.
 * Not offered: the exact rounded Minkowski sum, per-scene radii, several contacts per leg, moving solids, the casts inside the
 * pipeline (a caller enqueues them behind amk_pipeline_wait_stream on its own stream).                                       */
int amk_sim_clearance(const double *d_cyl, const int *d_cyl_counts, int max_cyl, const double *d_box, const int *d_box_counts,
                      int max_box, int n_scenes, double z_top, const double *d_pts, int point_stride, int n_points, double *d_dist,
                      int *d_kind, int *d_index, void *stream);
int amk_sim_clearance_host(const double *h_cyl, const int *h_cyl_counts, int max_cyl, const double *h_box, const int *h_box_counts,
                           int max_box, int n_scenes, double z_top, const double *h_pts, int point_stride, int n_points,
                           double *h_dist, int *h_kind, int *h_index);
int amk_sim_segment_cast(const double *d_cyl, const int *d_cyl_counts, int max_cyl, const double *d_box, const int *d_box_counts,
                         int max_box, int n_scenes, double z_top, const double *d_path, int point_stride, int n_points,
                         double radius, int *d_hit, double *d_t, int *d_kind, int *d_index, void *stream);
int amk_sim_segment_cast_host(const double *h_cyl, const int *h_cyl_counts, int max_cyl, const double *h_box,
                              const int *h_box_counts, int max_box, int n_scenes, double z_top, const double *h_path,
                              int point_stride, int n_points, double radius, int *h_hit, double *h_t, int *h_kind, int *h_index);
int amk_sim_path_cast(const double *d_cyl, const int *d_cyl_counts, int max_cyl, const double *d_box, const int *d_box_counts,
                      int max_box, int n_scenes, double z_top, const double *d_path, int point_stride, int n_points, double radius,
                      int *d_stop, int *d_leg, double *d_t, double *d_free, double *d_pts, int *d_kind, int *d_index, void *stream);
int amk_sim_path_cast_host(const double *h_cyl, const int *h_cyl_counts, int max_cyl, const double *h_box, const int *h_box_counts,
                           int max_box, int n_scenes, double z_top, const double *h_path, int point_stride, int n_points,
                           double radius, int *h_stop, int *h_leg, double *h_t, double *h_free, double *h_pts, int *h_kind,
                           int *h_index);

/* Sensor noise on the simulated depth frames: dropouts, flying pixels, axial noise, disparity steps, the sensor's own range.
 * amk_sim_render_depth / amk_sim_render_world give a perfect sensor: the exact planar depth of every first hit, silhouettes one
 * pixel sharp.  amk_sim_depth_noise is one out-of-place pass over a batch of such frames (or any recorded ones), placed between
 * the render and amk_pipeline_submit, that makes them the frames a depth camera gives.  It is DETERMINISTIC: every random number is
 * a pure function of (seed, fleet-wide scene number, frame, pixel, draw) through a counter-based integer hash, so a noisy flight
 * repeats on any machine and a host restatement matches bit for bit (avoid_mpc_amd/flight.py noise_words, depth_noise_ordered).
 *   d_in, d_out  [n_scenes] images of rows x cols pixels of depth_type (AMK_DEPTH_U16 / AMK_DEPTH_F32), scene s at s * scene_stride
 *                pixels in both; scene_stride >= rows cols, and the pixels between two images are neither read nor written.
 *   scene_id0    the fleet-wide number of scene 0 of the call: a sharded or split fleet draws the same stream per robot.
 *   frame        the period counter, by value.
 * Arithmetic: fp64, no contraction, every sum left to right as written; division and rint (ties to even) are IEEE-correct.  Integer
 * arithmetic is modulo 2^64.
 *
 * Stream.
 *   mix(z):  z += 0x9E3779B97F4A7C15;  z = (z ^ z >> 30) 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) 0x94D049BB133111EB;  return z ^ z >> 31
 *   per scene s and frame:  k = mix(mix(mix(seed) ^ (scene_id0 + s)) ^ frame)
 *   per pixel i = v cols + u (the position in the image, not in memory, in 64 bits) and draw j in {0, 1, 2}:  w_j = mix(k ^ (4 i + j))
 *   w_0 gives the variate g = (f0 + f1 + f2 + f3 - 131070) c, the f being the four 16-bit fields of w_0 and
 *       c = 2.6428997921303014e-05 = 1 / sqrt((65536^2 - 1) / 3): mean 0, variance 1, |g| <= 3.4642 -- the noise is bounded
 *   w_1: its high 32 bits decide the plain dropout, its low 32 bits what happens at a discontinuity
 *   w_2 >> 11 times 2^-53 is the flying pixel's fraction f in [0, 1)
 *   a probability p becomes the threshold T(p) = p >= 1 ? 2^32 : (u64)(p 4294967296.0), host arithmetic; a draw r succeeds when r < T
 *
 * Pixel.  z is read as amk_depth_to_clouds reads a pixel, (float)((double)(float)pixel pixel2meter), widened; it is written by
 * amk_sim_render_depth's rule: AMK_DEPTH_F32 holds (float)z / (float)pixel2meter correctly rounded to float32, AMK_DEPTH_U16 that
 * value under rintf, clamped to [0, 65535].  "The output is 0" ends the pixel.  The stages, in this order:
 *   1. Invalid input.  A pixel that is not a finite z > 0 (0, NaN, +-inf, negative) is copied bit for bit; no stage sees it.
 *   2. Discontinuity, only with edge_jump > 0.  The 4-neighbours inside the image, in the order left, right, up, down, are read from
 *      the INPUT image.  The pixel is a discontinuity pixel when some neighbour has no return (z_n not > 0) or is a finite return
 *      with |z_n - z| > edge_jump.  Then r = the low 32 bits of w_1:  r < T(p_edge_drop): the output is 0.  Otherwise
 *      r < T(p_edge_drop) + T(p_edge_fly): the partner is the first neighbour in that order that is a finite return with
 *      |z_n - z| > edge_jump; without one the output is 0, else z <- z + f (z_partner - z).
 *   3. Dropout.  The high 32 bits of w_1 < T(p_drop): the output is 0.
 *   4. Axial noise, only when sigma0 > 0 || sigma2 > 0:  z <- z + (sigma0 + (sigma2 z) z) g.
 *   5. Disparity, only with disparity_quantum q > 0:  d = focal_baseline / z, dq = rint(d / q) q; dq not > 0: the output is 0;
 *      else z <- focal_baseline / dq.
 *   6. Range.  z not > 0, z < z_min, or (z_max > 0 and z > z_max): the output is 0.
 *   7. Store.  A pixel that no enabled stage touched -- touched: flown, axial noise on, disparity on -- is copied bit for bit; every
 *      other pixel goes through the store rule.  A call with everything off is a copy, for both pixel types.
 * The result does not depend on the order in which pixels are processed, and a draw a pixel does not need is not part of any other.
 *
 * AMK_ERR_INVALID_ARG: a NULL pointer, d_in == d_out or overlapping ranges, rows, cols or n_scenes < 1, scene_stride < rows cols,
 * pixel2meter not > 0, a probability outside [0, 1] or NaN, p_edge_drop + p_edge_fly > 1, a negative or NaN sigma, jump, quantum or
 * range, disparity_quantum > 0 with focal_baseline not > 0, an unknown depth_type.  AMK_ERR_UNSUPPORTED: a grid beyond the launch
 * limits -- more than 65 535 scenes (the scenes are the grid's second dimension) or more than 256 (2^24 - 1) pixels per image.
 * AMK_ERR_NO_DEVICE: no device.  Every error is returned before anything is staged or launched, the output untouched.  The call is
 * stream-ordered, allocates nothing and keeps no hidden state.  amk_sim_depth_noise_host takes host pointers, stages them and
 * synchronises.
 * Not offered: a calibrated model of any camera, spatially or temporally correlated noise, lateral (pixel-position) noise,
 * multi-path and reflectance effects.                                                                                          */
typedef struct amk_sim_noise_params {
    unsigned long long seed;
    double sigma0, sigma2;                    /* axial noise [m]: sigma(z) = sigma0 + sigma2 z z                  */
    double p_drop;                            /* every valid pixel: probability of no return                       */
    double edge_jump;                         /* [m] a depth step larger than this is a discontinuity; 0 = off     */
    double p_edge_drop, p_edge_fly;           /* at a discontinuity pixel: no return / a flying pixel              */
    double focal_baseline, disparity_quantum; /* z -> fb / (rint((fb / z) / q) q); q = 0 = off                     */
    double z_min, z_max;                      /* the sensor's own working range; z_max = 0 = no upper gate         */
} amk_sim_noise_params;
int amk_sim_depth_noise(const void *d_in, void *d_out, int depth_type, int rows, int cols, long long scene_stride, int n_scenes,
                        double pixel2meter, const amk_sim_noise_params *prm, long long scene_id0, unsigned long long frame,
                        void *stream);
int amk_sim_depth_noise_host(const void *h_in, void *h_out, int depth_type, int rows, int cols, long long scene_stride,
                             int n_scenes, double pixel2meter, const amk_sim_noise_params *prm, long long scene_id0,
                             unsigned long long frame);

/* The rigid-body vehicle: a body with an attitude loop, flown in sub-steps inside one control period.
 * amk_sim_vehicle_step advances the plant with the MPC's own affine model, so the MPC's first predicted state is the next odometry
 * exactly, and amk_sim_vehicle_step_att only paints a rotation onto that pose.  amk_sim_vehicle_step_body is a SECOND vehicle beside
 * them (neither is changed): a small rigid body flown by bfctrl's GeometricController in acceleration mode -- the desired attitude from
 * the commanded thrust vector, the thrust as the command projected on the current body z, the attitude error on SO(3) -- integrated in
 * n_sub explicit sub-steps of h seconds, which reports its acceleration as the node does: the COGFilter's weighted mean of the
 * body-frame accelerometer samples, rotated by the current attitude, minus gravity (AvoidanceStateMachine.cpp, the IMU callback).
 * The plant no longer obeys the planner's model, and the camera's tilt lags its command.
 *   d_cmd   [S][3], d_x [S][10], d_Twb [S][16] or NULL: amk_sim_vehicle_step's buffers.  x[0..2] = p and x[4..6] = v are read and
 *           written; x[3], the yaw, is NOT written (what the affine plant does with it at u_3 = 0) and not read: the commanded yaw
 *           comes as (yaw_cs, yaw_sn); x[7..9] is an OUTPUT only and never read.  Twb = [R_f | p'] of the new state, row-major, with
 *           amk_sim_vehicle_step's own p': p' = rint(p q) / q for pose_quantum q > 0 (q = 1e6: the pose rounded to a micrometre,
 *           numpy's round(p, 6)); q = 0: p' = p.
 *   d_body  [S][AMK_SIM_BODY_DOUBLES] in/out, the hidden state of every scene as ONE array of doubles:
 *           [0..3] the quaternion (w, x, y, z), [4..6] the body rates w, [7] the collective thrust acceleration f,
 *           [8] held, the count of IMU samples in the ring, [9] head, the ring slot the NEXT sample goes to,
 *           [10 + 3 k .. 12 + 3 k] slot k of the ring of the last AMK_SIM_COG_MAX body-frame specific-force samples, k = 0 .. 15;
 *           [58..63] unused: the step leaves these words untouched (amk_sim_body_reset writes them as 0).
 *           The two integers are stored as doubles.  Either is read truncated towards zero, and a value outside its range -- held
 *           outside [0, AMK_SIM_COG_MAX], head outside [0, AMK_SIM_COG_MAX - 1], a NaN -- is read as 0, so that no state makes the
 *           call touch memory that is not the scene's.  The quaternion is not renormalised on the way in.
 * amk_sim_body_reset writes every scene's state: level (q = 1, 0, 0, 0), at rest, hovering (f = gz), an empty IMU window, all else 0.
 *
 * Arithmetic: fp64, no contraction, every sum left to right exactly as parenthesised below; division and square root are
 * IEEE-correct; there is no transcendental on the device; -(a) is the negation (it flips the sign of a zero).  A NaN's sign and
 * payload are not part of the contract.  avoid_mpc_amd/flight.py body_step_ordered restates it operation for operation.
 *   clamp(v, lo, hi) = v < lo ? lo : (v > hi ? hi : v), so a NaN passes through.
 *   R(q), "the usual nine polynomial entries" of q = (w, x, y, z):
 *     R00 = 1.0 - 2.0 ((y y) + (z z))   R01 = 2.0 ((x y) - (w z))         R02 = 2.0 ((x z) + (w y))
 *     R10 = 2.0 ((x y) + (w z))         R11 = 1.0 - 2.0 ((x x) + (z z))   R12 = 2.0 ((y z) - (w x))
 *     R20 = 2.0 ((x z) - (w y))         R21 = 2.0 ((y z) + (w x))         R22 = 1.0 - 2.0 ((x x) + (y y))
 * Once per call, from T = cmd.  T is already a thrust acceleration with gravity inside it (PubCmd; PubSlowDownCmd adds 9.8), so NO
 * gz is added here, unlike AMK_SIM_ATT_ACCEL.  R_d = [X Y Z] (columns) is amk_sim_vehicle_step_att's acc2rotmat with
 * cs, sn = yaw_cs, yaw_sn, the cosine and sine of the COMMANDED yaw as the caller computed them:
 *   n = sqrt((T_0 T_0 + T_1 T_1) + T_2 T_2);  Z = T / n
 *   y' = (0.0 - Z_2 sn, Z_2 cs, Z_0 sn - Z_1 cs);  m = sqrt((y'_0 y'_0 + y'_1 y'_1) + y'_2 y'_2);  Y = y' / m
 *   X = (Y_1 Z_2 - Y_2 Z_1, Y_2 Z_0 - Y_0 Z_2, Y_0 Z_1 - Y_1 Z_0);  valid = n > 0 && m > 0
 * Per sub-step, in this order, with R = R(q) built at the top of the sub-step and D . R_j = (D_0 R0j + D_1 R1j) + D_2 R2j:
 *   1. Attitude error, M = R_d^T R:  e = (0.5 ((Z . R_1) - (Y . R_2)), 0.5 ((X . R_2) - (Z . R_0)), 0.5 ((Y . R_0) - (X . R_1)))
 *      which is 0.5 (M21 - M12, M02 - M20, M10 - M01).
 *   2. Rate command:  wc_i = valid ? clamp(-(k_att e_i), -rate_max, rate_max) : 0.0
 *   3. Thrust command:  fc = clamp((T_0 R02 + T_1 R12) + T_2 R22, f_min, f_max) -- GetThrust(desired_acc.dot(zbody)) with a perfect
 *      thrust map.
 *   4. Lags:  w_i <- w_i + k_rate (wc_i - w_i);  f <- f + k_thrust (fc - f)
 *   5. Specific force and acceleration:  vb_i = (R0i v_0 + R1i v_1) + R2i v_2  (v_b = R^T v);
 *      sb = (-(drag_0 vb_0), -(drag_1 vb_1), f - drag_2 vb_2);  aw_i = (Ri0 sb_0 + Ri1 sb_1) + Ri2 sb_2, and aw_2 <- aw_2 - gz.
 *      Push sb: ring[head] = sb, head <- (head + 1) mod AMK_SIM_COG_MAX, held <- min(held + 1, AMK_SIM_COG_MAX).
 *   6. Translation:  v_i <- v_i + h aw_i, then p_i <- p_i + h v_i with the NEW v.
 *   7. Attitude, with the NEW w and hh = 0.5 h:
 *        dw = -(((x w_0) + (y w_1)) + (z w_2))      dx = ((w w_0) + (y w_2)) - (z w_1)      (on the right, w x y z are q's entries and
 *        dy = ((w w_1) + (z w_0)) - (x w_2)         dz = ((w w_2) + (x w_1)) - (y w_0)       w_0 w_1 w_2 the body rates)
 *      q_i <- q_i + hh d_i;  nq = sqrt(((w w + x x) + y y) + z z);  q_i <- q_i / nq.
 * After the last sub-step, with R_f = R(q) of the final q and s_idx the idx-th newest sample, ring[(head - 1 - idx) mod 16]:
 *   cog_window <= 1:  sbar = s_0, the newest sample itself, with no division.
 *   otherwise:  over idx = 0 .. min(held, cog_window) - 1, newest first:  acc = cog_weight[0] s_0, W = cog_weight[0], then
 *               acc <- acc + cog_weight[idx] s_idx, W <- W + cog_weight[idx];  sbar = acc / W.  This is the reference's filter over a
 *               window that is still filling; cog_weight[idx] is the weight of the idx-th newest sample (the caller's decay^idx).
 *   x[7 + i] = (Rf_i0 sbar_0 + Rf_i1 sbar_1) + Rf_i2 sbar_2, and x[9] <- x[9] - gz: the node's mAcc = R filtered - g.
 *   x[0..2] = p, x[4..6] = v, Twb = [R_f | p'], its last row (0, 0, 0, 1).
 * At hover -- level, at rest, cmd = (0, 0, gz) -- p, v, q, w and f are a fixed point bit for bit: R_d = I, e = 0 and aw = 0 without
 * rounding.
 * THE SIGN in step 2 is deliberate.  The reference's geometric_attcontroller has no minus in front of (2 / attctrl_tau_) error_att;
 * it sits behind use_bodyrate_ctrl, which the reference ships false.  With e as defined here -- the reference's -- the attitude obeys
 * theta' = +k_att sin(theta) under that sign and runs to pi; with the minus it decays.  k_att is the reference's 2 / attctrl_tau_.
 * A non-finite command or state in one scene stays in that scene.
 *
 * AMK_ERR_INVALID_ARG: a NULL pointer (d_Twb excepted), n_scenes < 1, a negative or NaN pose_quantum, any parameter outside the range
 * stated at its field or NaN (yaw_cs, yaw_sn: NaN), cog_window outside [0, AMK_SIM_COG_MAX], and for cog_window >= 2 a sum
 * ((cog_weight[0] + cog_weight[1]) + ...) of the first cog_window weights that is not > 0; amk_sim_body_reset: a NULL pointer,
 * n_scenes < 1, a negative or NaN gz.  AMK_ERR_NO_DEVICE: no device.  Every error is returned before anything is staged or launched,
 * the outputs unwritten.  The calls are stream-ordered and allocate nothing.  amk_sim_vehicle_step_body_host takes host pointers,
 * stages them and synchronises.
 * Not offered: motor and rotor dynamics, moments and inertia (the body rates follow their command through a first-order lag), wind, a
 * thrust-map estimator, odometry noise, the controller's position mode, calibrated parameters of any vehicle.                   */
#define AMK_SIM_BODY_DOUBLES 64   /* doubles of hidden state per scene */
#define AMK_SIM_COG_MAX      16
typedef struct amk_sim_body_params {
    double h;            /* sub-step, seconds, > 0 (the caller's con_dt / n_sub) */
    int    n_sub;        /* sub-steps per call, 1 .. 4096 */
    double gz;           /* gravity, >= 0 */
    double k_att;        /* attitude gain, 1/s, >= 0 (bfctrl: 2 / attctrl_tau_) */
    double rate_max;     /* |body rate command| clamp per axis, rad/s, > 0 (inf allowed) */
    double k_rate;       /* rate lag per sub-step, in (0, 1]; 1 = the rates follow at once (caller: min(1, h / tau_rate)) */
    double k_thrust;     /* thrust lag per sub-step, in (0, 1] */
    double f_min, f_max; /* collective thrust acceleration clamp, f_min <= f_max */
    double drag[3];      /* body-frame linear rotor drag, 1/s, >= 0 */
    double yaw_cs, yaw_sn; /* cosine and sine of the COMMANDED yaw, as the caller computed them (flights: 1, 0) */
    int    cog_window;   /* 0 or 1: no filter; 2 .. AMK_SIM_COG_MAX: the node's COGFilter */
    double cog_weight[AMK_SIM_COG_MAX]; /* weight of the idx-th newest sample (caller: decay^idx) */
} amk_sim_body_params;
int amk_sim_body_reset(double *d_body, int n_scenes, double gz, void *stream);
int amk_sim_vehicle_step_body(const amk_sim_body_params *prm, const double *d_cmd, double *d_x, double *d_body, double *d_Twb,
                              int n_scenes, double pose_quantum, void *stream);
int amk_sim_vehicle_step_body_host(const amk_sim_body_params *prm, const double *h_cmd, double *h_x, double *h_body, double *h_Twb,
                                   int n_scenes, double pose_quantum);

#ifdef __cplusplus
}
#endif
#endif /* AVOID_MPC_AMD_H */
