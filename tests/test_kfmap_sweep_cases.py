"""CPU: the scripts of tests/_sweep_cases.py reach the edges of the keyframe map's hashed sweep that they name -- judged from the numpy
map (SweepMap: NumpyMap's deque and gate around _sweep_np) and from numpy float32 restatements of the kernel's cell function, cube and
bucket count.  tests/test_kfmap_sweep_gpu.py runs the same scripts on the device against the same numpy map."""
import numpy as np
import pytest

from tests import _sweep_cases as sc

CASES = {c["name"]: c for c in sc.cases()}


def _d(q, p):
    q, p = np.asarray(q, np.float32).astype(np.float64), np.asarray(p, np.float32).astype(np.float64)
    return ((q[..., 0] - p[..., 0]) ** 2 + (q[..., 1] - p[..., 1]) ** 2) + (q[..., 2] - p[..., 2]) ** 2


def _flags(kf, cur, th):
    """outlier flag per keyframe point (the reference run with th_count past every count: nothing is rebuilt)"""
    big = sc._sweep_np(kf, cur, th, 1 << 30)
    assert big[1] == 0
    n1 = np.array([sc._sweep_np(kf[i:i + 1], cur, th, 1)[0] for i in range(len(kf))])
    assert n1.sum() == big[0]
    return n1.astype(bool)


# ---------------------------------------------------------------------------------------------------------- every case: the two sweeps
@pytest.mark.parametrize("name", list(CASES))
def test_both_sweeps_run_in_the_order_they_are_meant_to(name):
    """Period 1 sweeps A against B in record order; with an outlier (th_count of them) A is rebuilt, B inserted, and period 2
    sweeps B against C in GRID order; without, A stays the newest keyframe and period 2 sweeps A against C (record order: the grid
    of period 1 was B's).  The gate pops nothing and meets no tie."""
    c, ref = CASES[name], sc.reference(name)
    A, B, C = c["clouds"]
    sw = ref["sweeps"]
    assert ref["ties"] == 0
    assert ref["rows"][0][:3] == (1, [len(A)], 0)
    if len(B) == 0:                                                   # the period is skipped: A against C, record order
        assert name == "cur_size_0" and [(s[0], s[3]) for s in sw] == [(2, "record")] and sw[0][1] is A
        assert ref["rows"][1][:3] == (1, [len(A)], 0)
        return
    assert len(sw) == 2 and (sw[0][0], sw[0][3]) == (1, "record") and sw[0][1] is A and sw[0][2] is B
    n_out, rebuilt = sw[0][4], sw[0][5]
    assert ref["rows"][1][2] == n_out
    if rebuilt:
        assert n_out >= c["th_count"] and ref["rows"][1][:2] == (2, [len(B), n_out])
        assert (sw[1][0], sw[1][3]) == (2, "grid") and sw[1][1] is B and sw[1][2] is C
        assert [len(f) for f in ref["rows"][1][3]] == [len(B), n_out]                       # the query frames are [B, A']
    else:
        assert name in ("cur_size_1", "th_count_6") and ref["rows"][1][:2] == (1, [len(B)])
        assert (sw[1][0], sw[1][3]) == (2, "record") and sw[1][1] is A and sw[1][2] is C   # A is still the newest keyframe
    for cl in c["clouds"]:                                             # a porch ahead of the drone, everything else far from it
        fin = cl[np.isfinite(cl).all(axis=1)].astype(np.float64)
        far = np.linalg.norm(fin - sc.DRONE, axis=1) >= 10.0
        has = len(cl) >= 12 and np.array_equal(cl[:12], sc.porch())
        assert (~far).sum() == (12 if has else 0)
        assert has or (cl is A and "kf_size" in c["info"]) or (cl is B and c["info"].get("cur_size", 99) < 32)
        assert (fin[:, 0][fin[:, 0] > -1e30] > sc.DRONE[0] + sc.DEPTH_MIN).all()


def test_grid_order_sweeps_have_outliers_and_inliers():
    """(a sweep that flags everything or nothing would pass a kernel that ignores its input)"""
    for name in ("lattice_all", "threshold_exact", "threshold_band", "zero_threshold", "tiny_threshold", "huge_threshold", "ladder", "dense_3000"):
        for s in sc.reference(name)["sweeps"]:
            assert 0 < s[4] < len(s[1]) - 12 or name.startswith("threshold") and 0 < s[4] < len(s[1]), (name, s[0], s[4], len(s[1]))


def test_capacities_give_the_three_bucket_counts():
    assert [sc.sweep_buckets(c) for c in sc.CAPS] == [1024, 8192, 16384]
    g = sc.groups()
    assert {k[0] for k in g} == set(sc.CAPS)
    for fam in "abf":                                                 # families a, b and f in all three capacities
        assert {k[0] for k, v in g.items() if any(c["family"] == fam for c in v)} == set(sc.CAPS), fam
    assert sum(len(v) for v in g.values()) <= 44 and max(k[0] for k in g) == 4200
    assert {c["family"] for c in sc.cases()} == set("abcdefgh")


# ------------------------------------------------------------------------------------------------------------------------ a. the lattice
def test_lattice_crosses_every_direction_at_every_position():
    seen = {sw: set() for sw in (0, 1)}
    for name, c in CASES.items():
        if c["family"] != "a":
            continue
        A, B, C = c["clouds"]
        for (sw, far), (q, p, tags) in c["info"]["sets"].items():
            q, p = q.astype(np.float32), p.astype(np.float32)
            kf, cur = ((A, B), (B, C))[sw]
            cq, cp = sc.cell_f32(q, 0.1), sc.cell_f32(p, 0.1)
            d = np.sqrt(_d(q, p))
            assert ((d > 0.101) & (d < 0.13)).all() if far else ((d > 0.06) & (d < 0.09)).all()
            for i, (dr, k) in enumerate(tags):
                assert tuple(cp[i] - cq[i]) == dr and any(cq[i][a] == k for a in range(3) if dr[a]), (name, dr, k, cq[i], cp[i])
                assert all((cq[i][a] - k) % 12 == 0 for a in range(3) if dr[a])        # the same place in its hash block on every crossed axis
                assert (kf.view(np.int32) == q[i].view(np.int32)).all(axis=1).any() and (cur.view(np.int32) == p[i].view(np.int32)).all(axis=1).any()
                others = np.sqrt(_d(q[i], cur))
                assert np.sort(others)[1] > 1.0, (name, dr, k)                          # nothing but the partner within a metre
                if not far:
                    seen[sw].add((dr, k, c["caps"]))
            assert np.array_equal(_flags(q, cur, 0.1), np.full(len(q), bool(far)))
    for sw in (0, 1):
        for caps in ((300,), (3072, 4200)):
            assert {(dr, k) for dr, k, cc in seen[sw] if cc == caps} == {(dr, k) for dr in sc.DIRS for k in sc.LATTICE_K}
    assert len(sc.DIRS) == 26
    # the positions cover the sign change, the inside of a 4-cell hash block and both block boundaries
    faces = {(k, k + 1) for k in sc.LATTICE_K} | {(k - 1, k) for k in sc.LATTICE_K}
    assert (-1, 0) in faces and (3, 4) in faces and (-5, -4) in faces and (1, 2) in faces and all((a >> 2 != b >> 2) == (b % 4 == 0) for a, b in faces)


# --------------------------------------------------------------------------------------------------------------------- b. the threshold
def test_threshold_pairs_sit_on_and_beside_the_threshold():
    c = CASES["threshold_exact"]
    A, B, C = c["clouds"]
    n, offs, th = c["info"]["n"], c["info"]["offs"], c["th"]
    q, p = A[12:12 + n], B[12:12 + n]
    assert np.array_equal((p.astype(np.float64) - q.astype(np.float64)), offs)                       # the offsets survived float32
    d = _d(q, p)
    assert (d[[0, 3, 6]] == th * th).all() and (d[[1, 4, 7]] > th * th).all() and (d[[2, 5, 8]] < th * th).all()
    assert (np.abs(d[9:] / (th * th) - 1) < 2e-7).all() and (d[9:] != th * th).all()
    fl = _flags(q, B, th)
    assert fl[:9].tolist() == [False, True, False] * 3 and np.array_equal(fl[9:], np.sqrt(d[9:]) > th)
    assert np.array_equal(_flags(B[12 + n:], C, th), fl)                                             # the same pairs, mirrored, in the second sweep
    assert 0 < fl.sum() < n


def test_band_pairs_need_the_square_root():
    pairs = sc.band_pairs()
    t2 = 0.1 * 0.1
    for x, y, px, out in pairs:
        dx = float(x) - float(px)
        d = dx * dx + float(y) * float(y)
        assert t2 * (1 - 1e-15) <= d <= t2 * (1 + 1e-15) and out == (np.sqrt(d) > 0.1)
        assert np.float32(x) == x and 1e-10 < px < 2e-8
    used = CASES["threshold_band"]["info"]["outlier"]
    assert len(used) >= 4 and 0 < sum(used) < len(used)
    c = CASES["threshold_band"]
    A, B, C = c["clouds"]
    n = len(used)
    assert _flags(A[12:], B, 0.1).tolist() == used and _flags(B[12 + n:], C, 0.1).tolist() == used
    assert np.array_equal(_d(A[12:], B[12:12 + n]), _d(B[12 + n:], C[12:]))                          # z = +-2 (i + 1): exact


# ------------------------------------------------------------------------------------------------------ c, d. th = 0, tiny and huge
def test_zero_tiny_and_huge_thresholds():
    c = CASES["zero_threshold"]
    A, B, C = c["clouds"]
    n = c["info"]["n"]
    fl = _flags(A[12:], B, 0.0)
    assert fl.tolist() == [False, True, False, False, True, True, False, True] + [False] * 4
    assert np.signbit(B[12 + 2, 0]) and not np.signbit(A[12 + 2, 0]) and A[12 + 2, 0] == B[12 + 2, 0]   # +0.0 against -0.0
    d = (A[12 + 4, 0] - B[12 + 4, 0])
    assert d != 0 and np.float32(d) * np.float32(d) == 0                                              # its fp32 square underflows
    assert _flags(B[12 + n:], C, 0.0).tolist() == fl.tolist()
    c = CASES["tiny_threshold"]
    A, B, C = c["clouds"]
    n = c["info"]["n"]
    assert max(2.5 * c["th"], 1e-3) == 1e-3                                                           # the cell floor
    cq, cp = sc.cell_f32(A[12:], c["th"]), sc.cell_f32(B[12:12 + n], c["th"])
    assert (np.abs(cq[:, 0] - cp[:, 0]) == 1).all() and (cq[:, 1:] == cp[:, 1:]).all() and (cq[1::2, 0] < 0).all()
    assert _flags(A[12:], B, c["th"]).tolist() == [False, True, False, True, False, True]
    assert _flags(B[12 + n:], C, c["th"]).tolist() == [False, True, False, True, False, True]
    c = CASES["huge_threshold"]
    A, B, C = c["clouds"]
    assert len(np.unique(sc.cell_f32(A[12:], 50.0), axis=0)) == 1                                     # one cell holds the keyframe (but its porch)
    for cl in c["clouds"]:
        assert np.ptp(sc.cell_f32(cl, 50.0), axis=0).max() <= 2 and np.abs(sc.cell_f32(cl, 50.0)).max() <= 2
    assert _flags(A[12:], B, 50.0).tolist() == [False, True, False, True, False]
    assert _flags(B[12 + 5:], C, 50.0).tolist() == [False, True, False, True, False]


# ------------------------------------------------------------------------------------------------------------------------ e. the ladder
def test_ladder_reaches_the_fallback_and_the_clamp():
    c = CASES["ladder"]
    A, B, C = c["clouds"]
    q = c["info"]["q"].astype(np.float32)
    assert np.array_equal(A[12:12 + len(q)], q) and len(A) == 12 + len(q) + 12
    lo, hi = sc.cube_f32(q, 0.1)
    scale = np.repeat([cl[0] for cl in c["info"]["clusters"]], 2)
    wide = ((hi - lo) > 1).any(axis=1)
    assert wide[scale == 1e30].all() and not wide[scale < 1e30].any()                                  # the whole-grid loop: the 1e30 rows only
    clamped = (np.abs(sc.cell_f32(q, 0.1)) == 500000000).any(axis=1)
    assert clamped[scale >= 2e9].all() and not clamped[scale <= 1e8].any()                             # past the +-5e8-cell clamp
    assert ((hi - lo) <= 1).all(axis=1)[scale <= 1e8].all()                                            # the ordinary path
    fl = _flags(q, B, 0.1)
    assert not fl[1::2].any()                                                                          # the shared middle point
    assert np.array_equal(fl[0::2], np.array([cl[3] > 0.1 for cl in c["info"]["clusters"]]))          # one step away
    assert fl[0::2][[cl[0] <= 1e6 for cl in c["info"]["clusters"]]].sum() == 0 and fl[0::2].sum() == 20
    for cl in c["info"]["clusters"]:
        pts = cl[4].astype(np.float32)
        assert len(np.unique(pts[:, cl[1]])) == 3 and (cl[3] == 0.0625) == (cl[0] <= 1e6)
    lo2, hi2 = sc.cube_f32(B[12:], 0.1)                                                                # B's points are the second sweep's queries
    assert ((hi2 - lo2) > 1).any() and 0 < _flags(B[12:], C, 0.1).sum() < len(B) - 12


# -------------------------------------------------------------------------------------------------------------------- f. the dense cell
def test_dense_cells_hold_their_counts_and_one_point_within_th():
    for name in ("dense_1_to_9", "dense_3000"):
        c = CASES[name]
        clouds = c["clouds"]
        for sw in (0, 1):
            q, groups = c["info"]["q"][sw], c["info"]["groups"][sw]
            kf, cur = clouds[sw], clouds[sw + 1]
            assert [len(g) for g in groups] == list(c["info"]["counts"])
            for i, g in enumerate(groups):
                g32 = g.astype(np.float32)
                cells = sc.cell_f32(g32, 0.1)
                assert (cells == cells[0]).all()                                                      # ONE fine cell
                in_cell = (sc.cell_f32(cur, 0.1) == cells[0]).all(axis=1).sum()
                assert in_cell == len(g)
                near, away = q[2 * i].astype(np.float32), q[2 * i + 1].astype(np.float32)
                assert not (sc.cell_f32(near, 0.1) == cells[0]).all() and not (sc.cell_f32(away, 0.1) == cells[0]).all()
                assert (np.sqrt(_d(near, cur)) <= 0.1).sum() == 1 and (np.sqrt(_d(away, cur)) <= 0.1).sum() == 0
                if len(g) > 100:
                    assert np.ptp(np.delete(g, np.argmin(_d(near, g32)), axis=0), axis=0).max() <= 0.01   # 2999 of them in a 1 cm cube
            assert _flags(q.astype(np.float32), cur, 0.1).tolist() == [False, True] * len(groups)
    assert CASES["dense_3000"]["info"]["counts"] == (4, 3000) and CASES["dense_1_to_9"]["info"]["counts"] == tuple(range(1, 10)) and [n % 4 for n in range(1, 10)].count(0) == 2   # runs that end inside a 4-record step


# -------------------------------------------------------------------------------------------------------------------- g. block shapes
def test_block_shapes():
    c = CASES["queue_full"]
    A, B, _ = c["clouds"]
    lo, hi = sc.cube_f32(A, 0.1)
    assert len(A) == 256 and (hi != lo).any(axis=1).all() and ((hi - lo) <= 1).all() and _flags(A, B, 0.1).all()   # 256 open queries
    own = sc.cell_f32(A, 0.1)
    assert not any((sc.cell_f32(B, 0.1) == o).all(axis=1).any() for o in own)
    c = CASES["queue_empty"]
    A, B, _ = c["clouds"]
    lo, hi = sc.cube_f32(A, 0.1)
    assert len(A) == 256 and (hi == lo).all() and _flags(A, B, 0.1).tolist() == [False, True] * 128
    assert sorted(CASES[n]["info"]["kf_size"] for n in CASES if "kf_size" in CASES[n]["info"]) == [1, 2, 255, 256, 256, 257]
    for n in (1, 2, 255, 257):
        A, B, _ = CASES[f"kf_size_{n}"]["clouds"]
        fl = _flags(A, B, 0.1)
        assert len(A) == n and (n == 1 or 0 < fl.sum() < n)
    sizes = (0, 1, 2, 1023, 1024, 1025, 4095, 4096, 4097)
    for n in sizes:
        c = CASES[f"cur_size_{n}"]
        A, B, C = c["clouds"]
        ref = sc.reference(c["name"])
        assert len(B) == n and c["caps"] == (4200,)
        if n <= 1:
            assert ref["rows"][1][2] == 0 and ref["rows"][1][0] == 1                                  # skipped / no result for anyone
            assert 0 < ref["rows"][2][2] < len(A)
        else:
            assert 0 < ref["rows"][1][2] < len(A) and 0 < ref["rows"][2][2] < n
    assert 4 * 1024 in sizes                                                                          # the hash build's trip of 4 x 1024 points


# --------------------------------------------------------------------------------------------------------------------------- h. th_count
def test_th_count_edge():
    for n_out in (6, 7):
        ref = sc.reference(f"th_count_{n_out}")
        assert CASES[f"th_count_{n_out}"]["th_count"] == 7
        assert ref["sweeps"][0][4] == n_out and ref["sweeps"][0][5] == int(n_out == 7)
        assert ref["rows"][1][0] == 1 + int(n_out == 7)
    assert sc.reference("th_count_6")["sweeps"][1][4] == 7 and sc.reference("th_count_6")["rows"][2][0] == 2


def test_sweep_np_is_the_contract():
    """the reference on four points whose answers can be read off"""
    kf = np.array([[0, 0, 0], [1, 0, 0], [np.inf, 0, 0], [0, np.nan, 0]], np.float32)
    cur = np.array([[0.06, 0.08, 0], [5, 5, 5]], np.float32)
    assert sc._sweep_np(kf, cur, 0.1, 1)[0] == 3 and sc._sweep_np(kf, cur, 0.11, 9)[:2] == (3, 0)
    assert sc._sweep_np(kf, cur[:1], 0.1, 1)[0] == 0                                                  # the size rule
    assert sc._sweep_np(kf, np.array([[np.nan, 0, 0], [0, np.inf, 0], [1, np.nan, 1]], np.float32), 0.1, 1)[0] == 0   # no usable point
    assert np.array_equal(sc._sweep_np(kf, cur, 0.1, 1)[2].view(np.int32), kf[1:].view(np.int32))
