"""GPU: NaN, +-inf and overflowing coordinates through the KD index, the keyframe sweep and the depth kernels -- the contract
"non-finite coordinates" of include/avoid_mpc_amd.h, every sentence of it:

  a  hostile QUERIES on finite clouds        == the oracle tree (slots the traversal filled) / -1, DBL_MAX, zeros (the others)
  b  hostile CLOUDS, default tie order       == _oracle.kd_brute_np (no tree exists for such clouds: tests/test_kd_oracle.py)
  c  hostile clouds, reference tie orders    -> AMK_EXACT_GAVE_UP, answers of b; the batch's other scenes keep their trees
  d  keyframe sweep                          == a numpy statement of FrameKDMap.cpp:462-485 on that contract
  e  depth images with NaN / inf / ... pixels == oracle/depth_oracle.c, and nothing non-finite comes out of a finite pose
  f  a poisoned scene in a step / solve batch -> the other scenes bit-identical; no status 0 on a NaN state or path

Every comparison is bit for bit; no case is filtered after the fact.

Each case was seen to fail against a library with one value-level change in the kernel it covers (no address depends on any of
them): the trash rule back at |c| <= 3.0e38 (b, c: bucketed index), `valid = true` in the scan's bootstrap (a, b: scan), the
search's store without its empty-slot test (a, b: bucketed index), the sweep's tail returning 0 (d), the obstacle kernel's
second range gate as !(d <= min || d >= max) (e), the solve without its NaN-merit test (f: status 0 after 0 iterations)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _oracle
from tests.test_depth_oracle import YAML, hostile_scene
from tests.test_kd_oracle import _hostile_queries
from tests._sweep_cases import _kept, _sweep_np   # (the sweep's contract in numpy: shared with the keyframe map's sweep tests)
from avoid_mpc_amd import synth

pytestmark = pytest.mark.gpu
DBL_MAX = _oracle.DBL_MAX
FLT_MAX = np.finfo(np.float32).max
MODES = {"grid": 0, "scan": 1}      # bucketed index (the product path) / streaming scan (cross-check): both must answer alike


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test needs a GPU"
    return torch


def _pack(clouds, stride, counts=None):
    S, nmax = len(clouds), max(max(len(c) for c in clouds), 1)
    buf = np.full((S, nmax, stride), 7.0, np.float32)
    for s, c in enumerate(clouds):
        buf[s, :len(c), :3] = c
    cnt = np.array([len(c) for c in clouds], np.int32) if counts is None else np.asarray(counts, np.int32)
    return buf, cnt


def _handle(torch, clouds, mode="grid", tie=0, stride=3, counts=None):
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import KdBatch
    buf, cnt = _pack(clouds, stride, counts)
    kd = KdBatch(len(clouds), buf.shape[1])
    capi.load().amk__kd_set_mode(kd.h, MODES[mode])
    kd.set_tie_order(tie)
    kd.build(torch.from_numpy(buf).cuda(), torch.from_numpy(cnt).cuda())
    return kd


def _search(torch, kd, qs, k):
    out = kd.search(torch.from_numpy(np.ascontiguousarray(qs, np.float64)).cuda(), k)
    torch.cuda.synchronize()
    return {n: v.cpu().numpy() for n, v in out.items()}


def _check_row(res, s, j, k, exp_idx, exp_d, kept, ctx):
    """Row (s, j) of a search: `counts` by the size rule; the first len(exp_idx) slots hold the expected neighbours (index,
    distance bits, the point's own bits); every slot behind them holds -1 / DBL_MAX / (0, 0, 0)."""
    m = len(exp_idx)
    idx, d2, pts = res["indices"][s, j], res["sqdist"][s, j], res["pts"][s, j]
    assert res["counts"][s, j] == _oracle.kd_count_rule(len(kept), k), (ctx, res["counts"][s, j])
    assert m <= k and np.array_equal(idx[:m], exp_idx), (ctx, idx, exp_idx)
    assert np.array_equal(d2[:m].view(np.int64), np.asarray(exp_d, np.float64).view(np.int64)), (ctx, d2, exp_d)
    assert np.array_equal(pts[:m].view(np.int32), kept[exp_idx].view(np.int32)), ctx
    assert (idx[m:] == -1).all() and (d2[m:] == DBL_MAX).all() and not pts[m:].view(np.int32).any(), (ctx, idx, d2)


def _prefix(exp16, size, k):
    """The answer for k from the answer for 16 (size > 16: the k nearest in (distance, index) order are a prefix)."""
    assert size > 16
    n = min(_oracle.kd_count_rule(size, k), len(exp16[0]))
    return exp16[0][:n], exp16[1][:n]


def _tie_flag_np(cloud, q, k):
    """amk_kd_tie_flags restated: two of the k + 1 nearest usable points at the same squared distance, the first of them
    among the `count` returned ones."""
    _, d, size = _oracle.kd_brute_np(cloud, q, k + 1)
    cnt = _oracle.kd_count_rule(size, k)
    return int(any(d[i] == d[i + 1] for i in range(min(cnt, len(d) - 1))))


# ---- a. hostile queries, finite clouds ---------------------------------------------------------------------------------
def _query_batch(clouds, with_huge=True):
    """[S, 30, 3]: the 15 hostile queries interleaved with ordinary ones (hostile and ordinary rows share workgroups)."""
    names, hq = _hostile_queries()
    rng = np.random.default_rng(77)
    qs = np.zeros((len(clouds), 2 * len(hq), 3))
    for s, c in enumerate(clouds):
        ordinary = rng.uniform([0, -8, 0], [30, 8, 4], (len(hq), 3))
        ordinary[:3] = c[rng.integers(0, len(c), 3)]                          # queries on data points
        qs[s, 0::2] = ordinary
        qs[s, 1::2] = hq
        if not with_huge:                                                     # (the 1e150 rows tie every point with every other)
            for i, nm in enumerate(names):
                if "huge" in nm:
                    qs[s, 2 * i + 1] = rng.uniform([0, -8, 0], [30, 8, 4])
    return qs, [None if i % 2 == 0 else names[i // 2] for i in range(2 * len(hq))]


@pytest.mark.parametrize("mode", ["grid", "scan"])
@pytest.mark.parametrize("tie", [0, 1, 2])
@pytest.mark.parametrize("n", [3000, 4097, 50000])
def test_hostile_queries_on_finite_clouds(n, tie, mode, torch_cuda, oracle):
    """Ordinary rows: the oracle.  A query at a NaN / infinite / overflowing distance from every point: `counts` by the size rule,
    every slot -1 / DBL_MAX / zeros.  1e150 (squares near 1e300, finite): answered normally -- every point ties, so the
    lowest indices in the default order and the reference tree's visiting order in AMK_TIES_NANOFLANN / AUTO.  -0.0: ordinary.
    amk_kd_tie_flags: no flag on a row without a usable neighbour; AUTO: such rows raise no scene's need for a tree."""
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import kd_tie_flags
    torch = torch_cuda
    clouds = [synth.make_cloud(n, 31 + s)[0] for s in range(2)]
    trees = [_oracle.kd_oracle(c) for c in clouds]
    qs, names = _query_batch(clouds)
    kd = _handle(torch, clouds, mode, tie)
    tree_order = mode == "grid" and tie != 0                                  # (a handle in scan mode ignores the tie order)
    if mode == "grid" and tie == capi.AMK_TIES_AUTO:                          # before anything can tie
        q0, _ = _query_batch(clouds, with_huge=False)
        r0 = _search(torch, kd, q0, 8)
        assert kd.exact_status().cpu().numpy().tolist() == [capi.AMK_EXACT_NOT_NEEDED] * 2
        for s in range(2):
            for j in range(q0.shape[1]):
                ie, de, _ = _oracle.kd_brute_np(clouds[s], q0[s, j], 8)
                _check_row(r0, s, j, 8, ie, de, clouds[s], ("auto, no huge rows", n, s, j))
    for k in (1, 8, 16):
        res = _search(torch, kd, qs, k)
        for s in range(2):
            for j, nm in enumerate(names):
                q = qs[s, j]
                ib, db, size = _oracle.kd_brute_np(clouds[s], q, k)
                it, dt, _ = trees[s].search(q, k)
                nraw = len(trees[s].search_raw(q, k)[0])                      # what the traversal filled
                assert nraw == len(ib) == (0 if nm and nm.split("_")[0] in ("nan", "inf", "ninf", "big", "nbig") else k)
                if nm is None or "huge" not in nm:                            # tie-free: both orders are one
                    assert np.array_equal(ib, it[:nraw]) and np.array_equal(db.view(np.int64), dt[:nraw].view(np.int64))
                ie, de = (it[:nraw], dt[:nraw]) if tree_order else (ib, db)
                _check_row(res, s, j, k, ie, de, clouds[s], (mode, tie, n, k, s, j, nm))
        if mode == "grid" and tie == 0:
            fl = kd_tie_flags(kd, torch.from_numpy(qs).cuda(), k).cpu().numpy()
            exp = np.array([[_tie_flag_np(clouds[s], qs[s, j], k) for j in range(qs.shape[1])] for s in range(2)])
            assert np.array_equal(fl, exp), (n, k, fl, exp)
            for j, nm in enumerate(names):
                if nm and nm.split("_")[0] in ("nan", "inf", "ninf", "big", "nbig"):
                    assert not fl[:, j].any()
    st = kd.exact_status().cpu().numpy().tolist()
    # (AUTO: the 1e150 rows tied, so both scenes built their trees -- unless the handle scans and never looks at ties)
    want = {0: capi.AMK_EXACT_OFF, 1: capi.AMK_EXACT_IN_USE, 2: capi.AMK_EXACT_IN_USE if mode == "grid" else capi.AMK_EXACT_NOT_NEEDED}
    assert st == [want[tie]] * 2, (mode, tie, st)
    kd.close()


# ---- b. hostile clouds, default tie order -------------------------------------------------------------------------------
KINDS = ["nan_y", "nan_z", "inf_x", "ninf_x", "inf_y", "ninf_z", "big32", "fltmax"]
AMOUNTS = ["one", "fifteenth", "tile", "all_but_5", "all"]
_POISON = {"nan_y": (1, np.nan), "nan_z": (2, np.nan), "inf_x": (0, np.inf), "ninf_x": (0, -np.inf), "inf_y": (1, np.inf),
           "ninf_z": (2, -np.inf), "big32": (1, np.float32(3.2e38)), "fltmax": (0, -FLT_MAX)}


def _poison(base, kind, amount, rng, nan_x=True):
    """base with `amount` of its points given one coordinate of `kind`.  NaN / +-inf: the point stays in the cloud (only a NaN x
    is filtered), keeps its index, counts in the size, and is never returned.  3.2e38 / FLT_MAX: finite, so usable (squared
    distance ~1e77) and returned when nothing is nearer.  On top, runs of NaN-x points, so that the indices behind them shift."""
    c, n = base.copy(), len(base)
    col, val = _POISON[kind]
    ki = KINDS.index(kind)
    if amount == "one":          # a position the bounding-box sample of a large cloud reads (runs of 64, one run in 16) or one it skips
        c[5 if ki % 2 == 0 else 700, col] = val
    elif amount == "fifteenth":
        c[ki % 15::15, col] = val
    elif amount == "tile":       # one whole 4096-point tile of the build
        t0 = 4096 if n > 8192 else 0
        c[t0:t0 + 4096, col] = val
    elif amount == "all_but_5":  # fewer usable points than k
        keep = 400 + rng.choice(min(n, 2500) - 400, 5, replace=False)
        mask = np.ones(n, bool); mask[keep] = False
        c[mask, col] = val
    else:
        c[:, col] = val
    if nan_x:
        c[200:330, 0] = np.nan                                                # two full 64-point groups and two ragged ones
        c[4090:4110, 0] = np.nan                                              # across the first tile boundary (n > 4096)
        c[rng.choice(np.arange(2600, n), (n - 2600) // 50, replace=False), 0] = np.nan
    return c


@functools.lru_cache(maxsize=None)
def _hostile_batch(n):
    """40 scenes (kind x amount) of n points with ragged counts, 12 queries each, and the numpy reference's answer for k = 16."""
    rng = np.random.default_rng(1000 + n)
    base = synth.make_cloud(n, 60 + n % 11)[0]
    clouds, tags = [], []
    for kind in KINDS:
        for amount in AMOUNTS:
            c = _poison(base, kind, amount, rng)
            clouds.append(c[:n - (len(clouds) * 37) % 300])                   # ragged counts (>= 2700 points)
            tags.append((kind, amount))
    S, Q = len(clouds), 12
    qs = rng.uniform([-2, -9, -1], [32, 9, 5], (S, Q, 3))
    for s, c in enumerate(clouds):
        qs[s, 0] = base[rng.integers(0, 2600)]                                # on a data point (perhaps a poisoned one)
        qs[s, 1] = [3.0e38, 0.0, 1.0]                                         # nearer to a point at FLT_MAX than to the corridor
        qs[s, 2] = [-3.3e38, 3.0e38, 1.0]
        qs[s, 3] = [200.0, -150.0, 60.0]                                      # far outside the box
    exp = {(s, j): _oracle.kd_brute_np(clouds[s], qs[s, j], 16) for s in range(S) for j in range(Q)}
    return clouds, tags, qs, exp


def _check_hostile(res, clouds, tags, qs, exp, k, ctx):
    for s, c in enumerate(clouds):
        kept = _kept(c)
        for j in range(qs.shape[1]):
            i16, d16, size = exp[(s, j)]
            assert size == len(kept)
            ie, de = _prefix((i16, d16), size, k)
            _check_row(res, s, j, k, ie, de, kept, (ctx, tags[s], k, s, j))


@pytest.mark.parametrize("mode", ["grid", "scan"])
@pytest.mark.parametrize("n", [3000, 4096, 4097, 12289, 50000])
def test_hostile_clouds_default_tie_order(n, mode, torch_cuda):
    """Indices, distance bits, points, counts and sizes == the numpy reference, in both search modes: a point with a NaN or
    infinite coordinate is never returned, everything else is -- a coordinate of 3.2e38 or FLT_MAX included."""
    torch = torch_cuda
    clouds, tags, qs, exp = _hostile_batch(n)
    kd = _handle(torch, clouds, mode, 0, stride=4 if n in (4096, 12289) else 3)
    assert np.array_equal(kd.sizes(), [len(_kept(c)) for c in clouds])
    short = 0
    for k in (1, 8, 16):
        res = _search(torch, kd, qs, k)
        _check_hostile(res, clouds, tags, qs, exp, k, (mode, n))
        short += int((res["indices"][:, :, :k] == -1).any(axis=2).sum())
    assert short > 0                                                          # the short-list path did run
    kd.close()


def test_hostile_clouds_through_build_pair_and_host_entry_points(torch_cuda):
    from avoid_mpc_amd.host import KdBatch, kd_build_pair
    torch = torch_cuda
    (co, to, qo, eo), (ce, te, qe, ee) = _hostile_batch(4097), _hostile_batch(3000)
    bo, no = _pack(co, 4); be, ne = _pack(ce, 4)
    kd_o, kd_e = KdBatch(len(co), bo.shape[1]), KdBatch(len(ce), be.shape[1])
    kd_build_pair(kd_o, torch.from_numpy(bo).cuda(), kd_e, torch.from_numpy(be).cuda(), torch.from_numpy(no).cuda(),
                  torch.from_numpy(ne).cuda())
    _check_hostile(_search(torch, kd_o, qo, 8), co, to, qo, eo, 8, "pair, obstacle")
    _check_hostile(_search(torch, kd_e, qe, 8), ce, te, qe, ee, 8, "pair, edge")
    assert np.array_equal(kd_o.sizes(), [len(_kept(c)) for c in co]) and np.array_equal(kd_e.sizes(), [len(_kept(c)) for c in ce])
    kd_o.close(); kd_e.close()
    kd = KdBatch(len(co), bo.shape[1])
    kd.build_host(bo, no)
    _check_hostile(kd.search_host(qo, 16), co, to, qo, eo, 16, "host")
    assert np.array_equal(kd.sizes(), [len(_kept(c)) for c in co])
    kd.close()


# ---- c. hostile clouds, reference tie orders ----------------------------------------------------------------------------
def _lattice(n, seed):
    return (np.round(synth.make_cloud(n, seed)[0] * 4) / 4).astype(np.float32)   # 0.25 m lattice: exact ties everywhere


@pytest.mark.parametrize("tie", [1, 2])
def test_hostile_clouds_in_reference_tie_orders(tie, torch_cuda, oracle):
    """nanoflann's build is undefined on a NaN or an infinity, so a scene that keeps such a point gets no reference-shaped tree:
    AMK_EXACT_GAVE_UP, the bucketed index's answers (lowest index among equals).  Decided per scene on the device: the
    other scenes of the batch keep IN_USE / NOT_NEEDED and the oracle tree's index lists.  A coordinate of FLT_MAX is finite:
    that scene has its tree."""
    from avoid_mpc_amd import capi
    torch = torch_cuda
    rng = np.random.default_rng(8)
    n = 6000
    lat, free = _lattice(n, 71), synth.make_cloud(n, 72)[0]
    scenes = [("lattice nan_y", _poison(lat, "nan_y", "fifteenth", rng), True),
              ("lattice", lat, False),
              ("tie-free", free, False),
              ("tie-free inf_x", _poison(free, "inf_x", "one", rng), True),
              ("lattice fltmax", _poison(lat, "fltmax", "fifteenth", rng, nan_x=False), False),
              ("lattice all nan_z", _poison(lat, "nan_z", "all", rng), True),
              ("lattice ninf_z tile", _poison(lat, "ninf_z", "tile", rng), True)]
    clouds = [c for _, c, _ in scenes]
    Q, k = 16, 8
    qs = np.zeros((len(scenes), Q, 3))
    for s, (name, c, _) in enumerate(scenes):
        qs[s] = rng.uniform([0, -8, 0], [30, 8, 4], (Q, 3))
        if "lattice" in name:
            qs[s, :10] = lat[rng.integers(0, n, 10)] + 0.125                  # cell centres: equidistant to the corners
            qs[s, 10:13] = lat[rng.integers(0, n, 3)]
    kd = _handle(torch, clouds, "grid", tie)
    res = _search(torch, kd, qs, k)
    st = kd.exact_status().cpu().numpy()
    for s, (name, c, hostile) in enumerate(scenes):
        flagged = any(_tie_flag_np(c, qs[s, j], k) for j in range(Q))
        if tie == capi.AMK_TIES_AUTO and not flagged:
            want = capi.AMK_EXACT_NOT_NEEDED
        else:
            want = capi.AMK_EXACT_GAVE_UP if hostile else capi.AMK_EXACT_IN_USE
        assert st[s] == want, (name, tie, st.tolist())
        assert flagged == ("lattice" in name and "all" not in name), name     # the inputs are what the docstring says
        kept = _kept(c)
        tree = None if hostile else _oracle.kd_oracle(c)
        for j in range(Q):
            if hostile:
                ie, de, _ = _oracle.kd_brute_np(c, qs[s, j], k)
            else:
                ie, de, _ = tree.search(qs[s, j], k)
            _check_row(res, s, j, k, ie, de, kept, (name, tie, j))
    assert sorted(set(st.tolist())) == ([0, 1] if tie == 1 else [0, 1, 3])
    kd.close()


# ---- d. keyframe sweep --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tie_order", [0, 1])
def test_keyframe_sweep_with_nonfinite_points(tie_order, torch_cuda, oracle):
    """Non-finite points in the keyframe, in the current frame, in both; a current frame without a usable point; points with a
    coordinate in (3.0e38, FLT_MAX] (finite, so they sit in boundary cells of the index and are walked) on either side.  Outlier counts,
    rebuilt flags, the compacted keyframe point for point, and what the keyframe answers afterwards.  tie_order 1 (lattice
    clouds, both handles in AMK_TIES_NANOFLANN): a keyframe that still holds a non-finite point after the sweep gets no
    reference-shaped tree (AMK_EXACT_GAVE_UP), the others do."""
    from avoid_mpc_amd import capi
    torch = torch_cuda
    rng = np.random.default_rng(15)
    th_dist, th_count, n = 0.1, 10, 5000

    def frame(seed, shake):
        cur = synth.make_cloud(n, seed)[0]
        kf = cur + rng.normal(0, shake, cur.shape).astype(np.float32)
        kf[:800, 0] -= 6.0                                                    # a region the current frame no longer sees
        if tie_order:
            kf, cur = np.round(kf * 20) / 20, np.round(cur * 20) / 20
        return kf.astype(np.float32), cur.astype(np.float32)

    def mixed(c):
        c = c.copy()
        c[3::41, 1] = np.nan; c[7::53, 0] = np.inf; c[11::67, 2] = -np.inf; c[13::97, 0] = np.nan; c[900:964, 2] = np.nan
        c[17::211, 1] = np.float32(3.2e38); c[19::223, 0] = -FLT_MAX      # finite: usable, in boundary cells of the index
        return c

    def huge(c, rows):                                                        # the same three far points, finite: (3.0e38, FLT_MAX]
        c = c.copy()
        c[rows] = np.array([[FLT_MAX, 1.0, 1.0], [2.0, 3.2e38, -FLT_MAX], [-3.3e38, -3.3e38, 3.3e38]], np.float32)
        return c
    scenes = []
    kf, cur = frame(801, 0.02); scenes.append((mixed(kf), cur))               # non-finite points in the keyframe
    kf, cur = frame(802, 0.02); scenes.append((huge(kf, [2001, 2002, 2003]), mixed(cur)))   # ... in the current frame (+ far keyframe points)
    kf, cur = frame(803, 0.2)                                                 # ... in both; three far points that ARE in both: inliers
    scenes.append((huge(mixed(kf), [3001, 3002, 3003]), huge(mixed(cur), [10, 2500, 4000])))
    kf, cur = frame(804, 0.02); cur[:, 1] = np.nan; scenes.append((mixed(kf), cur))   # no usable point to be near to
    kf, cur = frame(805, 0.02); kf = cur.copy(); kf[5:9, 1] = np.nan; scenes.append((kf, cur))   # 4 outliers < th_count: untouched
    S = len(scenes)
    kd_k = _handle(torch, [k for k, _ in scenes], "grid", tie_order)
    kd_c = _handle(torch, [c for _, c in scenes], "grid", tie_order)
    outl, reb = kd_k.keyframe_sweep(kd_c, th_dist, th_count)
    torch.cuda.synchronize()
    outl, reb, sizes = outl.cpu().numpy(), reb.cpu().numpy(), kd_k.sizes()
    pts = np.zeros((S, kd_k.max_points, 3), np.float32); psz = np.zeros(S, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert capi.load().amk_kd_points_host(kd_k.h, vp(pts), vp(psz)) == capi.AMK_OK
    qs = np.stack([rng.uniform(-6, 20, (S, 12)), rng.uniform(-6, 6, (S, 12)), rng.uniform(0, 4, (S, 12))], -1)
    if tie_order:
        qs = np.round(qs * 40) / 40
    res = _search(torch, kd_k, qs, 8)
    st = kd_k.exact_status().cpu().numpy()
    for s, (kf, cur) in enumerate(scenes):
        n_out, rebuilt, after = _sweep_np(kf, cur, th_dist, th_count)
        assert (outl[s], reb[s], sizes[s], psz[s]) == (n_out, rebuilt, len(after), len(after)), (s, outl[s], n_out, reb[s], rebuilt)
        assert np.array_equal(pts[s, :len(after)].view(np.int32), after.view(np.int32)), s
        hostile = not np.isfinite(after).all()
        if tie_order:
            assert st[s] == (capi.AMK_EXACT_GAVE_UP if hostile else capi.AMK_EXACT_IN_USE), (s, st.tolist())
        tree = _oracle.kd_oracle(after) if tie_order and not hostile else None
        for j in range(qs.shape[1]):
            ie, de = tree.search(qs[s, j], 8)[:2] if tree else _oracle.kd_brute_np(after, qs[s, j], 8)[:2]
            _check_row(res, s, j, 8, ie, de, after, ("after the sweep", tie_order, s, j))
    kf2 = _kept(scenes[2][0])                                                 # the far points that both frames of scene 2 hold: kept out of
    far2 = _kept(huge(np.zeros((3, 3), np.float32), [0, 1, 2]))               # its rebuilt keyframe; scene 1's have no partner: outliers
    in2 = lambda a: sum(int((a.view(np.int32) == f.view(np.int32)).all(axis=1).any()) for f in far2)
    assert in2(kf2) == 3 and in2(pts[2, :psz[2]]) == 0 and in2(pts[1, :psz[1]]) == 3
    assert reb.tolist() == [1, 1, 1, 0, 0] and outl[3] == 0 and outl[4] == 4 and outl[0] > 800
    kd_k.close(); kd_c.close()


# ---- e. depth -----------------------------------------------------------------------------------------------------------
def _poses(rng, S):
    out = np.zeros((S, 4, 4))
    for s in range(S):
        th = rng.uniform(-np.pi, np.pi)
        out[s] = [[np.cos(th), -np.sin(th), 0, rng.uniform(-5, 5)], [np.sin(th), np.cos(th), 0, rng.uniform(-5, 5)],
                  [0, 0, 1, rng.uniform(0.5, 3)], [0, 0, 0, 1]]
    return out


TBC = np.array([[0, 0, 1, 0.1], [-1, 0, 0, 0.0], [0, -1, 0, 0.05], [0, 0, 0, 1.0]])


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("shape,scale,stride", [((480, 640), 10.0, 3), ((97, 131), 4.0, 4), ((60, 80), 2.5, 3)])
def test_depth_with_hostile_pixels(shape, scale, stride, dtype, edge, torch_cuda):
    """float32 frames with NaN (the invalid pixel of 32FC1), +-inf, negative and denormal pixels -- isolated, in a block, in the
    last row and column --, uint16 frames with 0 and 65535; a frame of nothing but NaN (uint16: 0).  Obstacle and edge cloud
    == the C oracle (bits, order, count), and no coordinate that comes out of a finite pose is non-finite."""
    torch = torch_cuda
    from avoid_mpc_amd.host import depth_params, depth_to_cloud
    rng = np.random.default_rng(23)
    S = 4
    imgs, p2m = zip(*[hostile_scene(rng, *shape, dtype) for _ in range(S)])
    imgs = np.stack(imgs)
    imgs[S - 1] = np.nan if dtype == np.float32 else 0
    prm = dict(YAML, pixel2meter=p2m[0], resize_scale=scale, Tbc=TBC)
    T = _poses(rng, S)
    dev = torch.from_numpy(imgs.view(np.int16) if dtype == np.uint16 else imgs).cuda()
    cloud, counts = depth_to_cloud(dev, depth_params(**prm), torch.from_numpy(T).cuda(), point_stride=stride, edge=edge)
    torch.cuda.synchronize()
    cloud, counts = cloud.cpu().numpy(), counts.cpu().numpy()
    for s in range(S):
        ref = _oracle.depth_edge_oracle(imgs[s], prm, T[s])[0] if edge else _oracle.depth_oracle(imgs[s], prm, T[s])[0]
        assert counts[s] == len(ref), (s, counts[s], len(ref))
        assert np.array_equal(cloud[s, :counts[s], :3].view(np.uint32), ref.view(np.uint32)), s
        assert np.isfinite(cloud[s, :counts[s], :3]).all(), s
    assert counts[S - 1] == 0 and counts[:S - 1].min() > 10


def test_nan_pose_gives_a_cloud_the_index_drops(torch_cuda):
    """A pose that has not arrived yet (NaN in the translation's x): every point comes out with a NaN x (y, z as the oracle's),
    amk_kd_build on that cloud reports size 0, a search returns count 0 and empty slots."""
    torch = torch_cuda
    from avoid_mpc_amd.host import KdBatch, depth_params, depth_to_cloud
    rng = np.random.default_rng(24)
    S = 2
    imgs = np.stack([hostile_scene(rng, 480, 640, np.float32)[0] for _ in range(S)])
    prm = dict(YAML, Tbc=TBC)
    T = _poses(rng, S)
    T[0, 0, 3] = np.nan
    cloud, counts = depth_to_cloud(torch.from_numpy(imgs).cuda(), depth_params(**prm), torch.from_numpy(T).cuda())
    kd = KdBatch(S, cloud.shape[1])
    kd.build(cloud, counts)
    q = rng.uniform(-5, 5, (S, 4, 3))
    res = _search(torch, kd, q, 8)
    hc, hn = cloud.cpu().numpy(), counts.cpu().numpy()
    ref0, ref1 = (_oracle.depth_oracle(imgs[s], prm, T[s])[0] for s in range(S))
    assert hn[0] == len(ref0) > 100 and np.isnan(hc[0, :hn[0], 0]).all() and np.isnan(ref0[:, 0]).all()
    assert np.array_equal(hc[0, :hn[0], 1:].view(np.uint32), ref0[:, 1:].view(np.uint32))
    assert np.array_equal(hc[1, :hn[1]].view(np.uint32), ref1.view(np.uint32))
    assert kd.sizes().tolist() == [0, hn[1]]
    empty = np.zeros((0, 3), np.float32)
    tree = _oracle.kd_oracle(ref1)
    for j in range(4):
        _check_row(res, 0, j, 8, np.zeros(0, np.int32), np.zeros(0), empty, ("nan pose", j))
        ie, de, _ = tree.search(q[1, j], 8)
        _check_row(res, 1, j, 8, ie, de, ref1, ("finite pose", j))
    kd.close()


# ---- f. the control step and the solve with one poisoned scene in the batch ------------------------------------------------
STEP_POISONS = ["state_quad_nan", "cloud_all_nan_y", "ref_path_inf"]
POISONED = 5


def _step_inputs(prm, poison=None):
    scenes = [synth.make_scene(5000, 900 + i, prm) for i in range(8)]
    sq = np.stack([_oracle.scene_state_quads(sc, prm) for sc in scenes])
    ref = np.stack([sc["ref_path"] for sc in scenes])
    if poison == "state_quad_nan":
        sq[POISONED, :, 1] = np.nan
    elif poison == "cloud_all_nan_y":
        scenes[POISONED]["cloud"] = scenes[POISONED]["cloud"].copy()
        scenes[POISONED]["cloud"][:, 1] = np.nan
    elif poison == "ref_path_inf":
        ref[POISONED, 2, 0] = np.inf
    return scenes, sq, ref


def _run_step(torch, prm, scenes, sq, ref):
    from avoid_mpc_amd.host import MpcBatch, step_batch
    kd_o = _handle(torch, [sc["cloud"] for sc in scenes]); kd_e = _handle(torch, [sc["edge"] for sc in scenes])
    mpc = MpcBatch(prm.T, prm.dt, prm.K, len(scenes)); mpc.configure(prm)
    refd = torch.from_numpy(ref.copy()).cuda()
    pos_x = torch.from_numpy(np.array([sc["pos"][0] for sc in scenes])).cuda()
    out = step_batch(kd_o, kd_e, mpc, prm, torch.from_numpy(sq).cuda(), pos_x, refd)
    torch.cuda.synchronize()
    res = dict(u=out["u"].cpu().numpy(), x0array=out["x0array"].cpu().numpy(), flags=out["flags"].cpu().numpy(),
               ref_path=refd.cpu().numpy())
    kd_o.close(); kd_e.close(); mpc.close()
    return res


@pytest.mark.parametrize("poison", STEP_POISONS)
def test_step_isolates_a_poisoned_scene(poison, torch_cuda):
    """8 C1 scenes through amk_step_batch, one of them with a NaN in its state, an obstacle cloud of nothing but NaN-y points, or
    an infinity in its reference path: the seven others are BIT-identical to the same batch with a healthy eighth scene (one
    wavefront per scene: nothing is shared), the poisoned scene returns, and its last solve does not report success when
    its state or its path is not a number."""
    prm = synth.MpcParams(T=0.33, K=3)
    healthy = _run_step(torch_cuda, prm, *_step_inputs(prm))
    got = _run_step(torch_cuda, prm, *_step_inputs(prm, poison))
    others = [s for s in range(8) if s != POISONED]
    for key in ("u", "x0array", "ref_path"):
        assert np.array_equal(got[key][others].view(np.int64), healthy[key][others].view(np.int64)), (poison, key)
    assert np.array_equal(got["flags"][others], healthy["flags"][others]), poison
    print(poison, "poisoned scene: flags", got["flags"][POISONED].tolist(), "u", got["u"][POISONED].tolist(),
          "healthy flags", healthy["flags"][POISONED].tolist())
    assert healthy["flags"][:, 1].min() > 0 and (healthy["flags"][:, 2] == 0).all()      # the healthy batch does solve, and converges
    if poison != "cloud_all_nan_y":
        assert got["flags"][POISONED, 2] != 0, got["flags"][POISONED]


def _solve_inputs(prm, poison):
    """vecRefStates of the first outer iteration of the 8 scenes' own steps (from the oracle), scene POISONED's poisoned."""
    refs = []
    for sc in _step_inputs(prm)[0]:
        kd, ke = _oracle.kd_oracle(sc["cloud"]), _oracle.kd_oracle(sc["edge"])
        m = _oracle.MpcOracle(prm.T, prm.dt, prm.K); m.configure(prm)
        r = _oracle.step_oracle(kd, ke, m, prm, _oracle.scene_state_quads(sc, prm), sc["pos"][0], sc["ref_path"].copy(), want_log=True)
        assert r["flags"][1] > 0
        refs.append(r["ref_log"][0])
    ref = np.stack(refs)
    if poison == "state_quad_nan":
        ref[POISONED, 1] = np.nan                  # [0, 10): x_init
    elif poison == "ref_path_inf":
        ref[POISONED, 10 + 3 * 10] = np.inf        # [10, 10 + 10 N): the reference states
    elif poison == "ref_path_inf_late":
        ref[POISONED, 10 + (prm.N - 2) * 10 + 1] = -np.inf   # the last reference state a stage cost reads (stage N - 1 takes the target)
    elif poison == "neighbour_nan":
        ref[POISONED, 10 + 10 * prm.N + 3 * (2 * prm.K + 1) + 2] = np.nan   # [10 + 10 N, + 3 K N): the neighbour points
    return ref


@pytest.mark.parametrize("poison", ["state_quad_nan", "ref_path_inf", "ref_path_inf_late", "neighbour_nan"])
def test_solve_with_a_poisoned_scene_equals_the_oracle(poison, torch_cuda):
    """amk_mpc_solve on the same batch: the poisoned scene's status (info[0]) and the NaN mask of its control equal MpcOracle's on
    the same inputs (the C restatement runs the same comparisons); the other scenes are bit-identical to the healthy batch."""
    torch = torch_cuda
    from avoid_mpc_amd.host import MpcBatch
    prm = synth.MpcParams(T=0.33, K=3)
    res = {}
    for tag in (None, poison):
        ref = _solve_inputs(prm, tag)
        gpu = MpcBatch(prm.T, prm.dt, prm.K, 8); gpu.configure(prm)
        u, x0, info = gpu.Solve(torch.from_numpy(ref).cuda(), faster=True)
        torch.cuda.synchronize()
        res[tag] = (u.cpu().numpy(), x0.cpu().numpy(), info.cpu().numpy(), ref)
        gpu.close()
    (u0, x0, i0, _), (u1, x1, i1, ref) = res[None], res[poison]
    others = [s for s in range(8) if s != POISONED]
    assert np.array_equal(u1[others].view(np.int64), u0[others].view(np.int64)) and np.array_equal(i1[others], i0[others])
    assert np.array_equal(x1[others].view(np.int64), x0[others].view(np.int64))
    m = _oracle.MpcOracle(prm.T, prm.dt, prm.K); m.configure(prm)
    uc, _, ic = m.Solve(ref[POISONED], True)
    print(poison, "gpu info", i1[POISONED].tolist(), "u", u1[POISONED].tolist(), "| oracle info", ic.tolist(), "u", uc.tolist())
    assert i1[POISONED, 0] == ic[0], (i1[POISONED], ic)
    # a NaN among the neighbour points is a collision term that never becomes active (every comparison with it is false): the
    # solve converges as if the point were not there; a NaN / infinite state or reference state must not report success
    assert (ic[0] == 0) == (poison == "neighbour_nan"), (poison, ic)
    assert np.array_equal(np.isnan(u1[POISONED]), np.isnan(uc))
