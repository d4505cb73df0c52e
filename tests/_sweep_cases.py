"""Inputs that aim at the keyframe map's HASHED sweep (TEST INFRASTRUCTURE): kd_sweep_hash_build_kernel / kd_sweep_mark_hash_kernel
(csrc/kd_sweep.hip) at cell faces, negative coordinates, hash-block boundaries, the threshold itself, every bucket count, the
large-coordinate fallback -- and the contract they are held to, in plain numpy.

  _sweep_np    the contract (include/avoid_mpc_amd.h at amk_kd_keyframe_sweep): fp64 squared distance ((dx^2 + dy^2) + dz^2), outlier
               iff sqrt(min) > th, a keyframe point without a usable neighbour an outlier iff the current frame holds a usable point,
               nothing unless the current frame holds more than one point
  SweepMap     tests/_kfmap_cases.NumpyMap's deque and gate around _sweep_np; records which sweeps ran and in which query order the
               default kernel takes the keyframe (record order, or the order of the grid the keyframe was sorted into last sweep)
  cases()      one scene per case, three periods (clouds A, B, C).  Tbc = identity, the drone at (-40, 0, 0); a porch of 12 fixed
               points 2-3 m ahead of it in every cloud of more than 11 points keeps the gate quiet, every other finite point is
               more than 10 m away.  Period 0 inserts A, period 1 sweeps A against B in RECORD order (no grid of A exists), with
               th_count = 1 and an outlier A becomes A' and B is inserted, period 2 sweeps B against C in GRID order.
  groups()     the cases by (max_points, th_dist, th_count): one map each

tests/test_kfmap_sweep_cases.py proves on the CPU that every family reaches the edge it names; tests/test_kfmap_sweep_gpu.py runs
the maps."""
import functools
import itertools

import numpy as np

from tests import _kfmap_cases as kc
from tests import _oracle

DBL_MAX = _oracle.DBL_MAX
FLT_MAX = np.finfo(np.float32).max
f32 = np.float32

TBC = np.eye(4)
DRONE = np.array([-40.0, 0.0, 0.0])
TWC = np.eye(4); TWC[:3, 3] = DRONE
DEPTH_MIN = 0.25
MAX_FRAMES = 3
ECAP = 8
CAPS = (300, 3072, 4200)
NQ = 8                                            # nearest_distance queries per scene after period 2


def _kept(cloud):
    return np.ascontiguousarray(cloud[~np.isnan(cloud[:, 0]), :3], np.float32)


def _sweep_np(kf, cur, th, th_count):
    """FrameKDMap.cpp:462-485 on the contract: SearchForNearest(pt, 1) in the current frame yields a result iff that frame holds
    more than one point (size rule); the result's squared distance is that of the nearest usable point, or DBL_MAX when the
    point has none (a NaN / infinite keyframe point; a current frame of unusable points only) -- an outlier then iff the
    current frame holds a usable point at all.  -> (outliers, rebuilt, keyframe afterwards)."""
    kfk, curk = _kept(kf), _kept(cur)
    out = np.zeros(len(kfk), bool)
    if len(curk) > 1:
        c = curk.astype(np.float64)
        any_usable = bool(np.isfinite(c).all(axis=1).any())
        for i0 in range(0, len(kfk), 256):
            q = kfk[i0:i0 + 256].astype(np.float64)
            with np.errstate(all="ignore"):
                d = ((q[:, None, 0] - c[None, :, 0]) ** 2 + (q[:, None, 1] - c[None, :, 1]) ** 2) + (q[:, None, 2] - c[None, :, 2]) ** 2
                dmin = np.where(d < DBL_MAX, d, np.inf).min(axis=1)
                out[i0:i0 + 256] = np.where(np.isinf(dmin), any_usable, np.sqrt(dmin) > th)
    n_out = int(out.sum())
    rebuilt = int(n_out >= th_count)
    return n_out, rebuilt, (kfk[out] if rebuilt else kfk)


class SweepMap(kc.NumpyMap):
    """NumpyMap with _sweep_np as its sweep.  sweeps: [(period, keyframe, current, order, outliers, rebuilt)], order 'grid' when the
    keyframe was the current frame of the sweep one update earlier (the default kernel then reads it from that sweep's grid)."""

    def __init__(self, th_dist, th_count):
        super().__init__(MAX_FRAMES, th_dist, th_count, DEPTH_MIN, TBC)
        self.sweeps, self.last_outliers, self.period, self.gridded = [], 0, -1, None

    def update(self):
        self.period += 1
        gridded, self.gridded, self.last_outliers = self.gridded, None, 0
        if not self.need:
            return
        self.need = False
        if not self.kfs:
            self.kfs.append(self.cur)
            return
        while self.kfs and (len(self.kfs) > self.mfc or not self.behind(self.kfs[0])):
            self.kfs.pop(0)
        if not self.kfs or self.kfs[-1] is self.cur:
            return
        last = self.kfs[-1]
        n_out, rebuilt, after = _sweep_np(last, self.cur, self.th_dist, self.th_count)
        self.sweeps.append((self.period, last, self.cur, "grid" if last is gridded else "record", n_out, rebuilt))
        self.gridded, self.last_outliers = self.cur, n_out
        if rebuilt:
            self.kfs[-1] = after
            self.kfs.append(self.cur)

    def frames(self):
        """the query vector: the current frame, then every keyframe but the newest, oldest first"""
        return [] if self.cur is None else [self.cur] + self.kfs[:-1]


# ------------------------------------------------------------------------------------------------------------------ the kernel's cells
def cell_f32(p, th):
    """sweep_cell (csrc/kd_sweep.hip) in numpy float32: floor(p * (float)(1 / cell)), clamped to +-5e8; cell = max(2.5 th, 1e-3)"""
    inv_hf = f32(1.0 / max(2.5 * th, 1e-3))
    with np.errstate(all="ignore"):
        return np.clip(np.floor(np.asarray(p, f32) * inv_hf), f32(-5.0e8), f32(5.0e8)).astype(np.int64)


def cube_f32(q, th):
    """(lo, hi) cells of the mark kernel's cube around the float32 points q [n, 3]: the fp64 allowance rr, the corners through float"""
    h = max(2.5 * th, 1e-3)
    qd = np.asarray(q, f32).astype(np.float64)
    rr = th + 1e-9 * h + 1e-12 * (np.abs(qd).sum(axis=1) + th)
    return cell_f32((qd - rr[:, None]).astype(f32), th), cell_f32((qd + rr[:, None]).astype(f32), th)


def sweep_buckets(max_points):
    """sweep_buckets (csrc/kd_sweep.hip): a power of two, about two per point, between 1024 and 16384"""
    nb = 1024
    while nb < 16384 and nb < 2 * max_points:
        nb *= 2
    return nb


# ------------------------------------------------------------------------------------------------------------------------- the scenes
def porch():
    rng = np.random.default_rng(4)
    return np.stack([-38.0 + rng.uniform(0, 1, 12), rng.uniform(-0.5, 0.5, 12), rng.uniform(-0.3, 0.3, 12)], 1).astype(f32)


def cloud(*parts, with_porch=True):
    parts = [np.asarray(p, np.float64).reshape(-1, 3).astype(f32) for p in parts]
    return np.concatenate(([porch()] if with_porch else []) + parts) if parts or with_porch else np.zeros((0, 3), f32)


def _case(name, family, A, B, C, th, th_count=1, caps=(300,), **info):
    return dict(name=name, family=family, clouds=(A, B, C), th=float(th), th_count=int(th_count), caps=tuple(caps), info=info)


DIRS = tuple(d for d in itertools.product((-1, 0, 1), repeat=3) if any(d))     # the 26 face, edge and corner directions
LATTICE_K = (-4, -1, 0, 1, 4)
CELL = 0.25                                                                    # th 0.1


def _lattice_pairs(ks, seed, far, taken):
    """One pair per (direction, k in ks): the keyframe point in a cell whose index is k along the FIRST axis the direction crosses
    and 12 u + k along the other two (12 cells = three hash blocks: the same place in its block, the same kind of face), the partner
    across the face / edge / corner, `far` False: 0.062-0.088 m away, True: 0.103-0.128 m.  (u, v) is the first place more than
    1.5 m from every pair placed before (`taken`, extended).  -> (keyframe points, partners, [(direction, k)])"""
    rng = np.random.default_rng(seed)
    places = sorted(itertools.product(range(-7, 8), repeat=2), key=lambda uv: (max(abs(uv[0]), abs(uv[1])), uv))
    q, p, tags = [], [], []
    for d in DIRS:
        a1 = next(a for a in range(3) if d[a])
        others = [a for a in range(3) if a != a1]
        for k in ks:
            dist = rng.uniform(0.103, 0.128) if far else rng.uniform(0.062, 0.088)
            step = dist / np.sqrt(sum(abs(c) for c in d))
            for u, v in places:
                cellidx = [0, 0, 0]
                cellidx[a1] = k; cellidx[others[0]] = 12 * u + k; cellidx[others[1]] = 12 * v + k
                kf = np.zeros(3)
                for a in range(3):
                    lo = cellidx[a] * CELL
                    kf[a] = lo + CELL - step / 2 if d[a] > 0 else lo + step / 2 if d[a] < 0 else lo + rng.uniform(0.08, 0.17)
                if kf[0] < -25.0 or (taken and np.min(np.linalg.norm(np.asarray(taken) - kf, axis=1)) < 1.5):
                    continue
                break
            else:
                raise AssertionError("no place left")
            taken.append(kf)
            q.append(kf); p.append(kf + step * np.asarray(d, np.float64)); tags.append((d, k))
    return np.asarray(q), np.asarray(p), tags


def lattice_case(name, ks, seed, caps):
    taken = []
    sets = {(sw, far): _lattice_pairs(ks, seed + 10 * sw + far, far, taken) for sw in (0, 1) for far in (0, 1)}
    A = cloud(sets[0, 0][0], sets[0, 1][0])
    B = cloud(sets[0, 0][1], sets[0, 1][1], sets[1, 0][0], sets[1, 1][0])
    C = cloud(sets[1, 0][1], sets[1, 1][1])
    return _case(name, "a", A, B, C, 0.1, 1, caps, sets=sets)


def _spots(axes, sign):
    """place i at sign * 2 (i + 1) m along axes[i], 0 along the other two: offsets along those stay exact in float32"""
    out = np.zeros((len(axes), 3))
    out[np.arange(len(axes)), axes] = sign * 2.0 * (np.arange(len(axes)) + 1)
    return out


def threshold_exact_case():
    """th 0.125: partners at exactly th along each axis (d = th^2: no outlier), one float above (outlier) and below, and at
    (float32(0.075), float32(0.1), 0), whose squared distance is th^2 to within 1e-7 relative"""
    th = 0.125
    offs = []
    for a in range(3):
        for v in (f32(0.125), np.nextafter(f32(0.125), f32(1)), np.nextafter(f32(0.125), f32(0))):
            o = np.zeros(3); o[a] = v; offs.append(o)
    for x, y in ((f32(0.075), f32(0.1)), (np.nextafter(f32(0.075), f32(1)), f32(0.1)), (np.nextafter(f32(0.075), f32(0)), f32(0.1)),
                 (f32(0.1), -f32(0.075))):
        offs.append(np.array([x, y, 0.0]))
    offs = np.asarray(offs, np.float64)
    axes = [1 if o[2] else 2 for o in offs]
    q1, q2 = _spots(axes, 1), _spots(axes, -1)
    A, B, C = cloud(q1), cloud(q1 + offs, q2), cloud(q2 + offs)
    return _case("threshold_exact", "b", A, B, C, th, 1, CAPS, n=len(offs), offs=offs)


@functools.lru_cache(maxsize=None)
def band_pairs():
    """th 0.1: pairs (keyframe (x, y), partner (px, 0)) of float32 numbers whose fp64 squared distance lies in
    [th^2 (1 - 1e-15), th^2 (1 + 1e-15)], where the kernel needs the square root.  The partner's x is about 1e-9: the difference
    of two floats of such different size is exact in fp64 and moves in steps of 1e-16.  -> [(x, y, px, outlier)]"""
    th = 0.1
    t2 = th * th
    out = []
    y = f32(0.03)
    for _ in range(400):
        y = np.nextafter(y, f32(1))
        dx = np.sqrt(t2 - float(y) ** 2)
        x = np.nextafter(f32(dx), f32(1))
        x = x if float(x) - dx > 5e-10 else np.nextafter(x, f32(1))
        p0 = f32(float(x) - dx)
        for px in (np.nextafter(p0, f32(0)), p0, np.nextafter(p0, f32(1))):
            ddx = float(x) - float(px)
            d = ddx * ddx + float(y) * float(y)
            if t2 * (1 - 1e-15) <= d <= t2 * (1 + 1e-15):
                out.append((x, y, px, bool(np.sqrt(d) > th)))
                break
    return tuple(out)


def threshold_band_case():
    pairs = band_pairs()[:24]
    n = len(pairs)
    q = np.array([[x, y, 0.0] for x, y, _, _ in pairs], np.float64)
    p = np.array([[px, 0.0, 0.0] for _, _, px, _ in pairs], np.float64)
    z1, z2 = _spots([2] * n, 1), _spots([2] * n, -1)
    A, B, C = cloud(q + z1), cloud(p + z1, q + z2), cloud(p + z2)
    return _case("threshold_band", "b", A, B, C, 0.1, 1, CAPS, n=n, outlier=[o for *_, o in pairs])


def zero_threshold_case():
    """th 0: only a bit-identical point (or -0.0 for +0.0) is near enough"""
    base = np.array([[1.5, 0.75, 0.0], [-2.25, 1.0, 3.0], [0.0, 0.0, 5.0], [-0.0, 3.0, -0.0], [1e-30, 4.0, 7.0], [3.0, -3.0, 1e-3]])
    base = np.concatenate([base, base + [0.0, 10.0, 0.0]]).astype(f32)

    def partners(q):
        p = q.copy()
        p[1, 0] = np.nextafter(p[1, 0], f32(0))                       # one ulp away: an outlier
        p[2, :2] = -0.0                                                # +0.0 against -0.0: equal
        p[3, 0] = 0.0; p[3, 2] += f32(0.0)
        p[4, 0] = np.nextafter(p[4, 0], f32(1))                       # a difference whose fp32 square underflows: still an outlier
        p[5, 2] = np.nextafter(p[5, 2], f32(1))
        p[7, 2] = np.nextafter(p[7, 2], f32(9))
        return p
    q2 = base + f32([0.0, 0.0, 64.0])
    A, B, C = cloud(base), cloud(partners(base), q2), cloud(partners(q2))
    return _case("zero_threshold", "c", A, B, C, 0.0, 1, (300,), n=len(base))


def tiny_threshold_case():
    """th 1e-4, cells of 1e-3 (the floor): partners across the cell face at x = 0.5 + k / 1000, 6e-5 (within) and 1.6e-4 (outside) away"""
    q, p = [], []
    for i, half in enumerate((3e-5, 8e-5, 3e-5, 8e-5, 4.5e-5, 5.5e-5)):
        face = (0.5 + i / 1000.0) * (-1 if i % 2 else 1)
        q.append([face - half, 2.0 * i, 0.0005]); p.append([face + half, 2.0 * i, 0.0005])
    q, p = np.asarray(q), np.asarray(p)
    up = np.array([0.0, 0.0, 64.0])
    A, B, C = cloud(q), cloud(p, q + up), cloud(p + up)
    return _case("tiny_threshold", "d", A, B, C, 1e-4, 1, (300,), n=len(q))


def huge_threshold_case():
    """th 50: cells of 125 m, the whole cloud in one or two of them"""
    q = np.array([[120.0, 5.0, 5.0], [5.0, 120.0, 5.0], [110.0, 110.0, 100.0], [60.0, 60.0, 5.0], [5.0, 5.0, 110.0]])   # one cell
    p = q + np.array([[-40.0, 0.0, 0.0], [0.0, -60.0, 0.0], [-30.0, -30.0, -20.0], [0.0, 36.0, 36.0], [0.0, 0.0, -49.9]])
    q2 = q * [1, -1, 1] + [0.0, -60.0, 0.0]
    A, B, C = cloud(q), cloud(p, q2), cloud(q2 + (p - q))
    return _case("huge_threshold", "d", A, B, C, 50.0, 1, (300,), n=len(q))


LADDER = (1e3, 1e5, 1e6, 1e7, 1e8, 2e9, 1e30)


def _ladder_clusters():
    """three points per centre, one float ulp of the scale apart, or 0.0625 where the ulp is smaller"""
    out = []
    for scale in LADDER:
        for axis, sign in ((1, 1), (1, -1), (2, 1), (2, -1), (0, 1)):
            c = f32(sign * scale)
            step = max(float(np.spacing(np.abs(c))), 0.0625)
            pts = np.zeros((3, 3))
            pts[:, axis] = [float(c) - step, float(c), float(c) + step]
            out.append((scale, axis, sign, step, pts))
    return out


def ladder_case():
    """keyframe: the first two points of every cluster; current frame: the second (equal: near enough) and the third -- the first
    has its neighbour at one step: within th = 0.1 up to 1e6, not from 1e7 on"""
    cl = _ladder_clusters()
    q = np.concatenate([c[4][:2] for c in cl]); p = np.concatenate([c[4][1:] for c in cl])
    q2 = np.concatenate([c[4][1:] for c in cl]); p2 = np.concatenate([c[4][:2] for c in cl])
    # (the far clusters come in pairs at equal distance from the drone; 12 plain outliers nearer to it are what the gate examines in A')
    yard = np.stack([-28.0 + 0.3 * np.arange(12), 1.0 + np.arange(12) % 5, np.arange(12) % 3], 1)
    A, B, C = cloud(q, yard), cloud(p), cloud(p2)
    # (B's keyframe points against C ARE B's partners: the second and third of a cluster against the first and second)
    return _case("ladder", "e", A, B, C, 0.1, 1, (300,), clusters=cl, q=q, q2=q2)


def _dense_groups(counts, z0, seed):
    """per count: that many current-frame points in ONE fine cell (a 1 cm cube at its middle), none within th of the keyframe point
    that sits in the next cell along x -- but one of them, moved to the cell's face, is"""
    rng = np.random.default_rng(seed)
    q, groups = [], []
    for i, n in enumerate(counts):
        lo = np.array([4.0 * CELL * (i - 4), 8.0 * CELL, z0])               # the dense cell's corner
        pts = lo + [0.12, 0.12, 0.12] + rng.uniform(0, 0.01, (n, 3))
        j = int(rng.integers(0, n))
        pts[j] = lo + [0.24, 0.125, 0.125]
        q.append(lo + [0.29, 0.125, 0.125])                                   # 0.05 from point j, 0.16 and more from the others
        q.append(lo + [-0.06, 0.125, 0.125])                                  # on the other side: 0.18 from the nearest -- an outlier
        groups.append(pts)
    return np.asarray(q), groups


def dense_case(name, counts, caps):
    q1, g1 = _dense_groups(counts, 0.0, 31)
    q2, g2 = _dense_groups(counts, 64.0, 32)
    A, B, C = cloud(q1), cloud(*g1, q2), cloud(*g2)
    return _case(name, "f", A, B, C, 0.1, 1, caps, counts=counts, q=(q1, q2), groups=(g1, g2))


def _scatter(n, seed, x0=0.0):
    """n points on a 1 m lattice (jittered by < 0.2 m) in the slab x0 + [0, 16) x [-32, 32) x [0, ...): more than 0.6 m apart"""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    base = np.stack([x0 + i % 16, (i // 16) % 64 - 32, i // 1024], 1).astype(np.float64)
    return base + rng.uniform(-0.2, 0.2, (n, 3))


def block_cases():
    out = []
    ahead = np.array([0.0, 0.0, 40.0])
    # 256 keyframe points, every one an outlier whose cube reaches a second cell (0.02 m from a corner of its cell): phase B's queue is full
    i = np.arange(256)
    corners = np.stack([2.0 * (i % 16) - 16, 2.0 * (i // 16) - 16, np.zeros(256)], 1)
    A = cloud(corners + 0.02, with_porch=False)
    B = cloud(_scatter(40, 51) + ahead)
    out.append(_case("queue_full", "g", A, B, cloud(_scatter(40, 52) + ahead), 0.1, 1, (4200,), kf_size=256))
    # 256 keyframe points at the middle of their cells: the cube stays inside (0.125 +- 0.1), nobody is open; every other one has a partner there
    mids = corners + 0.125
    out.append(_case("queue_empty", "g", cloud(mids, with_porch=False), cloud(mids[::2] + [0.03, 0.0, 0.0], _scatter(40, 53) + ahead),
                     cloud(_scatter(40, 54) + ahead), 0.1, 1, (4200,), kf_size=256))
    for n in (1, 2, 255, 257):
        pts = _scatter(n, 60 + n)
        A = cloud(pts, with_porch=False)
        B = cloud(pts[1::3] + [0.0, 0.05, 0.0], _scatter(30, 61) + ahead)
        out.append(_case(f"kf_size_{n}", "g", A, B, cloud(_scatter(40, 62) + ahead), 0.1, 1, (4200,), kf_size=n))
    kfp = _scatter(40, 70)
    for n in (0, 1, 2, 1023, 1024, 1025, 4095, 4096, 4097):
        rest = _scatter(max(n - 32, 0), 71 + n, x0=20.0)
        B = cloud(kfp[:20] + [0.04, 0.0, 0.0], rest) if n >= 32 else cloud((kfp[:20] + [0.04, 0.0, 0.0])[:n], with_porch=False)
        assert len(B) == n
        A, C = cloud(kfp), cloud(kfp[10:] + [0.0, 0.04, 0.0], kfp[:1] + [0.04, 0.03, 0.0], rest[::2] + [0.0, 0.0, 0.05])
        out.append(_case(f"cur_size_{n}", "g", A, B, C, 0.1, 1, (4200,), cur_size=n))
    return out


def count_cases():
    """th_count 7: exactly 6 outliers leave the keyframe alone, exactly 7 rebuild it"""
    out = []
    for n_out in (6, 7):
        pts = _scatter(60, 80)
        B = cloud(pts[n_out:] + [0.05, 0.0, 0.0])
        C = cloud(pts[7 if n_out == 6 else 14:] + [0.0, 0.05, 0.0])
        out.append(_case(f"th_count_{n_out}", "h", cloud(pts), B, C, 0.1, 7, (300,), n_out=n_out))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = [lattice_case(f"lattice_k{k}", (k,), 100 + 7 * i, (300,)) for i, k in enumerate(LATTICE_K)]
    out.append(lattice_case("lattice_all", LATTICE_K, 200, (3072, 4200)))
    out += [threshold_exact_case(), threshold_band_case(), zero_threshold_case(), tiny_threshold_case(), huge_threshold_case(), ladder_case()]
    out.append(dense_case("dense_1_to_9", tuple(range(1, 10)), CAPS))
    out.append(dense_case("dense_3000", (4, 3000), (3072, 4200)))
    out += block_cases() + count_cases()
    return tuple(out)


@functools.lru_cache(maxsize=None)
def groups():
    """{(max_points, th_dist, th_count): [case]}: one map each, one scene per case"""
    g = {}
    for c in cases():
        for cap in c["caps"]:
            assert max(len(x) for x in c["clouds"]) <= cap, (c["name"], cap)
            g.setdefault((cap, c["th"], c["th_count"]), []).append(c)
    return g


@functools.lru_cache(maxsize=None)
def reference(name):
    """The numpy map over a case's three periods -> dict(rows = per period (n_keyframes, frame sizes, last_outliers, frames),
    sweeps, ties)"""
    c = next(c for c in cases() if c["name"] == name)
    m = SweepMap(c["th"], c["th_count"])
    rows = []
    for cl in c["clouds"]:
        m.add_vertex(cl, TWC)
        m.update()
        fr = m.frames()
        rows.append((len(m.kfs), [len(f) for f in fr], m.last_outliers, [f.copy() for f in fr]))
    return dict(rows=rows, sweeps=m.sweeps, ties=m.ties)


def distance_queries(name):
    """NQ queries for the map after period 2: 4 points of C (finite ones) and 4 random ones around the scene's ordinary points"""
    c = next(c for c in cases() if c["name"] == name)
    rng = np.random.default_rng(sum(map(ord, name)))
    C = c["clouds"][2].astype(np.float64)
    fin = C[np.isfinite(C).all(axis=1)]
    if not len(fin):
        fin = porch().astype(np.float64)
    mod = fin[(np.abs(fin) < 1e4).all(axis=1)]
    lo, hi = mod.min(axis=0) - 1.0, mod.max(axis=0) + 1.0
    return np.concatenate([fin[rng.integers(0, len(fin), NQ // 2)], rng.uniform(lo, hi, (NQ - NQ // 2, 3))])


def expected_distance(frames, q):
    """GetNearestDistance: sqrt of the least squared distance to a usable point of the frames that hold more than one point"""
    best = DBL_MAX
    for f in frames:
        if len(f) <= 1:
            continue
        c = f.astype(np.float64)
        with np.errstate(all="ignore"):
            d = ((q[0] - c[:, 0]) ** 2 + (q[1] - c[:, 1]) ** 2) + (q[2] - c[:, 2]) ** 2
        d = d[np.isfinite(c).all(axis=1) & (d < DBL_MAX)]
        if len(d):
            best = min(best, float(d.min()))
    return np.sqrt(best)
