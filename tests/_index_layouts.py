"""Index layouts the builders can leave behind (TEST INFRASTRUCTURE, CPU only): one table of named layouts for the radius search and
the four leg walks (grid_radius, grid_segment, grid_segment_knn, grid_cast and the path cast over it; csrc/kd_grid.h).

A layout names the clouds its handle must answer for (one per scene, ragged, raw: NaN-x points are dropped by the build), how the
handle gets its index, and one path per scene made from the cloud's bounding box.  The references are the existing brute forces
(tests/_radius.py, _segment.py, _segment_nearest.py, _cast.py, _path_cast.py) over `clouds`; nothing here restates a query.

  degenerate   line, thick_line, plane0, plane, diag, same, two: one scene, built once -- grids of 1024 x 1 x 1, n x n x 1 and
               2 x 2 x 2 cells, most of a line clamped into the last cell, a cell edge of 6.8e-31 m
  tiles_s3/4   one ragged handle whose scenes hold 0 to 4 tiles: sizes on, before and behind the 4096-point tile boundary, a NaN-x
               run across it, a tile that is all NaN-x; point strides 3 and 4
  swept        the keyframe handle after amk_kd_keyframe_sweep: every record in tile 0 (grid_build_scene), more than a tile's worth
  rebuilt      a handle built twice, the second time with fewer points: stale tiles, tables and geometry must be invisible
  ties_*       quantised clouds in the default order, AMK_TIES_NANOFLANN and AMK_TIES_AUTO: the five queries answer alike

tests/test_index_layouts.py proves on the CPU that every layout reaches what it names; tests/test_kd_index_layouts_gpu.py runs
them."""
import functools
from types import SimpleNamespace

import numpy as np

from tests import _cast as K
from tests import _path_cast as PC
from tests import _radius as R
from tests import _segment as G
from tests import _segment_nearest as N

INF = float("inf")
TILE = 4096                                      # kTilePoints
RADII = (0.0, 0.0625, 4.0, INF)                  # squared
RADIUS_K = (0, 8, 64)
NEAREST_K = (1, 8, 64)
N_POINTS = 13                                    # 12 legs: three rounds of the path cast's four waves
WINDOWS = ((0, 13), (3, 9), (7, 6), (6, 3))      # (first point, points) of the path casts: 12, 8, 5 and 2 legs (away and far: free)
LEG = dict(along=0, back=1, to_inner=2, inner=3, into_grid=4, across=5, away=6, far=7, long=8, home=9, on_point=10, short=11)

TILE_SIZES = (4095, 4096, 4097, 8192, 8193, 512, 513, 1, 12289, 0, 3)
SWEEP_TH, SWEEP_COUNT, SWEEP_CAP = 0.5, 1, 8193
REBUILT_CAP = 8193
REBUILT_FIRST = (8193, 4097, 600, 5000)
REBUILT_SECOND = (513, 0, 1, 4097)
QUANTUM = 0.25

f32 = np.float32


# ------------------------------------------------------------------------------------------------------------------ the grid
def grid_of(cloud):
    """(cells per axis, bbmin, h) of the index over a cloud of finite points below 16384 (tests/_radius.grid_dims' geometry)"""
    c = R.kept(cloud).astype(np.float64)
    g, _ = R.grid_dims(cloud)
    lo, ext = c.min(axis=0), c.max(axis=0) - c.min(axis=0)
    e = np.maximum(ext, max(ext.max() * 1e-6, 1e-30))
    h = np.cbrt(e.prod() / min(max(len(c) / 64.0, 1.0), 1024.0))
    for _ in range(64):
        if (np.clip(np.ceil(e / h), 1, 1024).astype(int) == g).all():
            break
        h *= 1.26
    return g, lo, h


def true_cells(cloud):
    """the cell coordinates of every point BEFORE the clamp into [0, g - 1], as floats (they may be astronomically large)"""
    g, lo, h = grid_of(cloud)
    return np.floor((R.kept(cloud).astype(np.float64) - lo) / h), g


def cast_slabs(cloud, a, b):
    """the number of slabs grid_cast cuts the leg a -> b into (the comment above grid_cast, csrc/kd_grid.h):
    n = max(1, min(min(ceil(max |ab_i| / h), 1024), 1 + sum over the axes |cell(b) - cell(a)|))"""
    g, lo, h = grid_of(cloud)
    a, b = np.asarray(a, np.float64)[:3], np.asarray(b, np.float64)[:3]
    cell = lambda p: np.clip(np.floor((p - lo) * (1.0 / h)), 0, g - 1).astype(int)
    span = int(np.abs(cell(b) - cell(a)).sum())
    return max(1, min(int(min(np.ceil(np.abs(b - a).max() * (1.0 / h)), 1024.0)), span + 1))


# ------------------------------------------------------------------------------------------------------------------ the paths
def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def lonely_midpoint(cloud):
    """the midpoint of two stored points that no third point is nearer to: a leg through it, perpendicular to the cloud's plane, has
    its two nearest points at exactly equal distances (the midpoint of two floats is exact in fp64)"""
    c = R.kept(cloud).astype(np.float64)
    for i in range(len(c)):
        d = R.sq_dists(c.astype(f32), c[i])
        d[i] = np.inf
        j = int(np.argmin(d))
        m = (c[i] + c[j]) / 2
        dm = R.sq_dists(c.astype(f32), m)
        if np.sort(dm)[2] > dm[i] == dm[j]:
            return m
    raise AssertionError("no lonely pair")


def make_path(cloud, axis=(1, 0, 0), normal=(0, 0, 1), inner=None, grid=None, cross=None, reach=1.0):
    """The 13 points (12 legs, LEG names them) of one scene, float64, from the bounding box of the cloud's finite points.
    u = the long axis, v = across it; E = the low end of the box's centre line along u.
      along / back   from `reach` beyond one end of the cloud to beyond the other along u through the box's centre, and back
      inner          a leg on that centre line (IN an exact line or plane), between `inner` = (d1, d0) metres from E
      into_grid      from there to a point `grid` metres from E, half a metre beside the cloud
      across         through the cloud along v (through `cross` when given)
      far            5 m long, 100 m away;  long: 1e6 m from there through a stored point;  on_point: a == b == that point;
      short          1 cm from it;  to_inner, away, home: what joins them"""
    c = R.kept(cloud).astype(np.float64)
    c = c[np.isfinite(c).all(axis=1)]
    u, v = _unit(axis), _unit(normal)
    if len(c):
        centre = (c.min(axis=0) + c.max(axis=0)) / 2
        half, wid = np.abs((c - centre) @ u).max(), np.abs((c - centre) @ v).max()
        stored = c[len(c) // 2]
    else:
        centre, half, wid, stored = np.zeros(3), 0.0, 0.0, np.zeros(3)
    span = max(half, 1.0)
    E = centre - half * u
    d1, d0 = inner if inner is not None else (half + 0.3 * span, half + 0.1 * span)
    dg = grid if grid is not None else half - 0.2 * span
    w = wid + 0.5
    lo_end, hi_end = E - reach * u, E + (2 * half + reach) * u
    beside = (E + dg * u if cross is None else np.asarray(cross, np.float64)) - w * v
    far0 = centre + 100.0 * v + 3.0 * u
    far1 = far0 + 5.0 * u
    pts = [lo_end, hi_end, lo_end, E + d1 * u, E + d0 * u, beside, beside + 2 * w * v, far0, far1, far1 + 1e6 * _unit(stored - far1),
           stored, stored, stored + 0.01 * _unit(u + v)]
    assert len(pts) == N_POINTS
    return np.stack(pts)


# ------------------------------------------------------------------------------------------------------------------ the clouds
def _line():
    return np.stack([np.arange(1024) * 0.125, np.zeros(1024), np.zeros(1024)], axis=1).astype(f32)


def _thick_line():
    rng = np.random.default_rng(101)
    return np.stack([1000.0 * rng.random(6000), 1e-3 * rng.normal(size=6000), 1e-3 * rng.normal(size=6000)], axis=1).astype(f32)


def _plane(exact, seed=102):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-50.0, 50.0, (6000, 2))
    z = np.zeros(6000) if exact else 1e-3 * rng.normal(size=6000)
    return np.concatenate([xy, z[:, None]], axis=1).astype(f32)


def _diag():
    rng = np.random.default_rng(103)
    t = 300.0 * rng.random(6000)
    return np.stack([t, t + 0.01 * rng.normal(size=6000), 0.5 * rng.normal(size=6000)], axis=1).astype(f32)


POINT = np.array([1.5, -2.0, 0.25], f32)


def _same():
    return np.tile(POINT[None], (200, 1))


def _two():
    return np.concatenate([np.tile(POINT[None], (100, 1)), np.tile((POINT + f32(1.0))[None], (100, 1))])


def tile_clouds():
    """the ragged batch of test_tile_boundaries_of_the_one_pass_build (tests/test_kd_gpu.py), within 12289 points"""
    rng = np.random.default_rng(77)
    clouds = []
    for n in TILE_SIZES:
        c = rng.uniform([-4, -4, 0], [4, 4, 3], (n, 3)).astype(f32)
        if n > 4200:
            c[4090:4110, 0] = np.nan                      # a run across the first tile boundary
        if n >= 12289:
            c[8192:12288, 0] = np.nan                     # the third tile holds no point at all
        if n > 600:
            c[rng.choice(n, 37, replace=False), 0] = np.nan
        clouds.append(c)
    return clouds


def tiles_kept(cloud):
    """kept points per 4096-point tile of the caller's cloud (grid_build_tiles_scene cuts the RAW cloud)"""
    keep = ~np.isnan(np.asarray(cloud)[:, 0])
    return [int(keep[i:i + TILE].sum()) for i in range(0, len(keep), TILE)]


def sweep_np(kf, cur, th, th_count):
    """amk_kd_keyframe_sweep (include/avoid_mpc_amd.h) on finite clouds: a keyframe point is an outlier iff sqrt(min d2) > th over the
    current frame's points, fp64 sums left to right (tests/_radius.sq_dists); no result, hence no outlier, when the current frame
    holds <= 1 point; >= th_count outliers rebuild the keyframe from them, order preserved.  -> (outliers, rebuilt, keyframe after)"""
    k, c = R.kept(kf), R.kept(cur)
    assert np.isfinite(k).all() and np.isfinite(c).all()
    out = np.zeros(len(k), bool)
    if len(c) > 1:
        out = np.array([np.sqrt(R.sq_dists(c, q).min()) > th for q in k.astype(np.float64)], bool)
    n_out = int(out.sum())
    rebuilt = int(n_out >= th_count)
    return n_out, rebuilt, (k[out] if rebuilt else k)


@functools.lru_cache(maxsize=None)
def swept():
    """-> dict(keyframe, current: the clouds the two handles are built from; outliers, rebuilt, after: what the sweep must leave)"""
    rng = np.random.default_rng(104)
    box = [30.0, 16.0, 4.0]
    keyframe = [(rng.random((n, 3)) * box).astype(f32) for n in (8193, 4200, 300)]
    current = [(rng.random((600, 3)) * [3.0, 16.0, 4.0]).astype(f32), (rng.random((600, 3)) * box).astype(f32),
               (rng.random((1, 3)) * box).astype(f32)]
    res = [sweep_np(k, c, SWEEP_TH, SWEEP_COUNT) for k, c in zip(keyframe, current)]
    return dict(keyframe=keyframe, current=current, outliers=[r[0] for r in res], rebuilt=[r[1] for r in res], after=[r[2] for r in res])


@functools.lru_cache(maxsize=None)
def rebuilt():
    """-> (the clouds of the first build, the clouds of the second): other points in another box"""
    rng = np.random.default_rng(105)
    first = [(rng.random((n, 3)) * [30.0, 16.0, 4.0]).astype(f32) for n in REBUILT_FIRST]
    second = [rng.uniform([-4, -4, 0], [4, 4, 3], (n, 3)).astype(f32) for n in REBUILT_SECOND]
    return first, second


def tie_clouds():
    """`plane` and the 4097-point tile cloud on a 0.25 m lattice: equal distances everywhere"""
    q = lambda c: (np.round(c.astype(np.float64) / QUANTUM) * QUANTUM).astype(f32)
    return [q(_plane(False)), q(tile_clouds()[TILE_SIZES.index(4097)])]


# ------------------------------------------------------------------------------------------------------------------ the table
def _layout(name, clouds, paths, ref=None, how="build", cap=None, stride=3, ties=0, shape=None, **more):
    return SimpleNamespace(name=name, clouds=clouds, path=np.stack(paths), ref=ref or name, how=how,
                           cap=cap or max(1, max(len(c) for c in clouds)), stride=stride, ties=ties, shape=shape, **more)


@functools.lru_cache(maxsize=None)
def layouts():
    """{name: layout}.  clouds: what the handle must answer for, one raw cloud per scene; path float64 [S, 13, 3]; how: "build" (one
    amk_kd_build of `clouds`, point stride `stride`, tie order `ties`), "sweep" (swept()), "rebuild" (rebuilt()); ref: layouts with
    the same ref hold the same clouds and paths and share their references; shape: the grid a degenerate layout is meant to get"""
    out = {}

    def add(lay):
        out[lay.name] = lay

    c = _line();       add(_layout("line", [c], [make_path(c, normal=(0, 1, 0), inner=(60.0, 50.0), grid=2.0)], shape=(1024, 1, 1)))
    c = _thick_line(); add(_layout("thick_line", [c], [make_path(c, normal=(0, 1, 0), inner=(600.0, 500.0), grid=20.0)], shape=(1024, 1, 1)))
    c = _plane(True);  add(_layout("plane0", [c], [make_path(c, cross=lonely_midpoint(c))], shape=(29, 29, 1)))
    c = _plane(False); add(_layout("plane", [c], [make_path(c, cross=lonely_midpoint(c))], shape=(28, 28, 1)))
    c = _diag();       add(_layout("diag", [c], [make_path(c, axis=(1, 1, 0), normal=(1, -1, 0))], shape=(20, 20, 1)))
    c = _same();       add(_layout("same", [c], [make_path(c)], shape=(2, 2, 2)))
    c = _two();        add(_layout("two", [c], [make_path(c, axis=(1, 1, 1), normal=(1, -1, 0))], shape=(2, 2, 2)))
    tc = tile_clouds()
    tp = [make_path(c) for c in tc]
    for stride in (3, 4):
        add(_layout(f"tiles_s{stride}", tc, tp, ref="tiles", stride=stride))
    sw = swept()
    add(_layout("swept", sw["after"], [make_path(c) for c in sw["after"]], how="sweep", cap=SWEEP_CAP))
    first, second = rebuilt()
    add(_layout("rebuilt", second, [make_path(c) for c in second], how="rebuild", cap=REBUILT_CAP))
    add(_layout("rebuilt_fresh", second, [make_path(c) for c in second], ref="rebuilt", cap=REBUILT_CAP))
    qc = tie_clouds()
    qp = [make_path(qc[0], cross=qc[0][7]), make_path(qc[1])]                        # across: through a lattice site
    for name, mode in (("ties_default", 0), ("ties_nanoflann", 1), ("ties_auto", 2)):
        add(_layout(name, qc, qp, ref="ties", ties=mode))
    return out


DEGENERATE = ("line", "thick_line", "plane0", "plane", "diag", "same", "two")
NAMES = DEGENERATE + ("tiles_s3", "tiles_s4", "swept", "rebuilt", "rebuilt_fresh", "ties_default", "ties_nanoflann", "ties_auto")


def frames(lay):
    return [[c] for c in lay.clouds]


# ------------------------------------------------------------------------------------------------------------------ the references
def _by_ref(ref):
    return next(l for l in layouts().values() if l.ref == ref)


@functools.lru_cache(maxsize=None)
def want_radius(ref, r2, k):
    lay = _by_ref(ref)
    return R.expected_batch(frames(lay), lay.path, r2, k)


@functools.lru_cache(maxsize=None)
def want_segment(ref, r2, k):
    lay = _by_ref(ref)
    return G.expected_batch(frames(lay), lay.path, r2, k)


@functools.lru_cache(maxsize=None)
def want_nearest(ref, k):
    lay = _by_ref(ref)
    return N.expected_batch(frames(lay), lay.path, k)


@functools.lru_cache(maxsize=None)
def want_cast(ref, r2):
    lay = _by_ref(ref)
    return K.expected_batch(frames(lay), lay.path, r2)


@functools.lru_cache(maxsize=None)
def want_path_cast(ref, r2, window):
    lay = _by_ref(ref)
    i, n = window
    return PC.expected_batch(frames(lay), np.ascontiguousarray(lay.path[:, i:i + n]), r2)


def nearest_leg_dist(lay):
    """the least squared distance of a usable point to every leg, [S, 12]; +inf for a scene without one"""
    S, L = lay.path.shape[0], lay.path.shape[1] - 1
    out = np.full((S, L), np.inf)
    for s in range(S):
        c = R.kept(lay.clouds[s])
        for j in range(L if len(c) else 0):
            d = G.seg_dists(c, lay.path[s, j], lay.path[s, j + 1])[0]
            d = d[d < R.DBL_MAX]
            out[s, j] = d.min() if len(d) else np.inf
    return out


def clear_legs(lay, r2):
    """where hit == (count > 0) must hold in fp64: the nearest point is not within 1e-9 r2 of the radius
    (tests/test_kd_segment_cast_gpu.py: test_a_cast_hits_where_the_segment_search_counts)"""
    return np.abs(nearest_leg_dist(lay) - r2) > 1e-9 * r2


# ------------------------------------------------------------------------------------------------------------------ the frame lists
FRAME_SCENES = 3
FRAME_REBUILT = (0, 1, 3)     # the scenes of rebuilt() that the list's third frame holds: 513, 0 and 4097 points after 8193, 4097, 5000


@functools.lru_cache(maxsize=None)
def frame_list():
    """Three frames per scene, three scenes: frame 0 a plane cloud built once, frame 1 the swept keyframe (every record in tile 0),
    frame 2 a handle built twice.  -> dict(plane: the clouds of frame 0, first / second: the two builds of frame 2, held[s]: the
    three clouds scene s must answer for, path [3, 13, 3] through the region the frames share)"""
    sw = swept()
    first, second = rebuilt()
    plane = [_plane(False), _plane(True), _plane(False, seed=106)]
    held = [[plane[s], sw["after"][s], second[FRAME_REBUILT[s]]] for s in range(FRAME_SCENES)]
    path = []
    for s in range(FRAME_SCENES):
        # along the swept keyframe's box, inside the plane cloud and through the rebuilt cloud's box; `stored` is a keyframe point
        p = make_path(sw["after"][s], reach=6.0)
        p[:7, 1], p[:7, 2] = 2.0, [0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 5.0]
        path.append(p)
    return dict(plane=plane, first=[first[i] for i in FRAME_REBUILT], second=[second[i] for i in FRAME_REBUILT], held=held,
                path=np.stack(path))


FRAME_RADII = RADII
FRAME_K = (0, 8, 64)


@functools.lru_cache(maxsize=None)
def want_frames(kind, *args):
    """the brute forces over the three frames each scene holds: kind "radius" (r2, k), "segment" (r2, k), "nearest" (k), "cast" (r2),
    "path_cast" (r2, window)"""
    fl = frame_list()
    held, path = fl["held"], fl["path"]
    if kind == "radius":
        return R.expected_batch(held, path, *args)
    if kind == "segment":
        return G.expected_batch(held, path, *args)
    if kind == "nearest":
        return N.expected_batch(held, path, *args)
    if kind == "cast":
        return K.expected_batch(held, path, *args)
    r2, (i, n) = args
    return PC.expected_batch(held, np.ascontiguousarray(path[:, i:i + n]), r2)
