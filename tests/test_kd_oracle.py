"""Pins the C restatement of the KD path (oracle/kd_oracle.c) against the reference's own
nanoflann header compiled in place (oracle/_ref): its answers on these clouds and queries are stored in
tests/golden/kd_ref_golden.npz (tests/golden/make_kd_ref_golden.py), so the tests run without the reference."""
import numpy as np
import pytest

from tests import _oracle
from avoid_mpc_amd import synth


def _clouds():
    rng = np.random.default_rng(1)
    out = {}
    out["uniform5k"] = rng.uniform(-10, 10, (5000, 3)).astype(np.float32)
    out["corridor20k"] = synth.make_cloud(20000, 3)[0]
    g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(10), indexing="ij"), -1)
    out["grid_ties"] = g.reshape(-1, 3).astype(np.float32)              # massive exact ties
    out["dupes"] = np.repeat(rng.uniform(-1, 1, (300, 3)).astype(np.float32), 4, axis=0)
    out["planar"] = np.concatenate([rng.uniform(-5, 5, (3000, 2)), np.zeros((3000, 1))], 1).astype(np.float32)
    out["tiny7"] = rng.uniform(-1, 1, (7, 3)).astype(np.float32)
    out["one"] = np.array([[1.0, 2.0, 3.0]], np.float32)
    return out


def _queries(name, cloud):
    rng = np.random.default_rng(7)
    lo, hi = cloud.min(0) - 1.0, cloud.max(0) + 1.0
    qs = rng.uniform(lo, hi, (200, 3))
    qs[:20] = cloud[rng.integers(0, len(cloud), 20)]                     # queries on data points
    if name == "grid_ties":
        qs[20:40] = rng.integers(0, 9, (20, 3)) + 0.5                    # equidistant to 8 corners
    return qs


def _nan_x_cloud():
    rng = np.random.default_rng(2)
    cloud = rng.uniform(-1, 1, (50, 3)).astype(np.float32)
    cloud[[3, 17, 40], 0] = np.nan                                       # dropped (kd_tree_two.h:99)
    return cloud


def _nan_y_cloud_and_queries():
    rng = np.random.default_rng(3)
    cloud = rng.uniform(-1, 1, (50, 3)).astype(np.float32)
    cloud[5, 1] = np.nan                                                 # kept: only x is tested (:99)
    return cloud, rng.uniform(-1, 1, (20, 3))


HOSTILE_CLOUDS = ("uniform5k", "corridor20k")   # the two finite clouds the reference's answers to hostile queries are stored for


def _hostile_queries():
    """Queries with a non-finite or overflowing coordinate -> (names, float64 [Q, 3]).  The squared distance of every point is
    NaN (nan_*), inf (inf_*, big_*: 1e200 squared overflows) -- no point enters the result set -- or about 1e300 (huge_*: finite,
    answered normally; all points tie unless the other two coordinates decide at 1e284 resolution); -0.0 is an ordinary query."""
    nan, inf = np.nan, np.inf
    cases = [("nan_x", (nan, 0.0, 1.0)), ("nan_y", (0.0, nan, 1.0)), ("nan_z", (3.0, 0.5, nan)), ("nan_all", (nan, nan, nan)),
             ("inf_x", (inf, 0.0, 1.0)), ("ninf_x", (-inf, 0.0, 1.0)), ("inf_y", (2.0, inf, 1.0)), ("ninf_z", (2.0, 0.5, -inf)),
             ("big_x", (1e200, 0.0, 0.0)), ("nbig_y", (1.0, -1e200, 0.5)), ("big_z", (1.0, 0.5, 1e200)),
             ("huge_x", (1e150, 0.0, 0.0)), ("nhuge_z", (4.0, 0.25, -1e150)),
             ("negzero", (-0.0, -0.0, -0.0)), ("negzero_x", (-0.0, 0.5, 1.0))]
    return [c[0] for c in cases], np.array([c[1] for c in cases], np.float64)


def _fma_cloud_and_queries():
    return synth.make_cloud(20000, 5)[0], np.random.default_rng(9).uniform([0, -8, 0], [30, 8, 4], (300, 3))


@pytest.mark.parametrize("name", list(_clouds().keys()))
@pytest.mark.parametrize("k", [1, 3, 8])
def test_restatement_equals_reference(name, k, oracle):
    cloud = _clouds()[name]
    a = _oracle.kd_oracle(cloud)
    b = _oracle.ref_answers(name, cloud)
    qs = _queries(name, cloud)
    for q in qs:
        ia, da, pa = a.search(q, k)
        ib, db, pb = b.search(q, k)
        assert np.array_equal(ia, ib), (name, k, q)
        assert np.array_equal(da.view(np.int64), db.view(np.int64))
        assert np.array_equal(pa, pb)
        ra, rb = a.search_raw(q, k), b.search_raw(q, k)
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1])


def test_nan_x_filter_and_count_quirk(oracle):
    cloud = _nan_x_cloud()
    a, b = _oracle.kd_oracle(cloud), _oracle.ref_answers("nan_x", cloud)
    assert a.size() == b.size() == 47
    q = np.array([0.1, 0.2, 0.3])
    for n in (1, 8, 46, 47, 48, 60):
        ia, da, _ = a.search(q, n)
        ib, db, _ = b.search(q, n)
        assert np.array_equal(ia, ib) and np.array_equal(da.view(np.int64), db.view(np.int64))
        if n == 47:
            assert len(ia) == 0                                          # size == n quirk (:119-124)
        elif n > 47:
            assert len(ia) == 47
        else:
            assert len(ia) == n


def test_nan_y_is_kept(oracle):
    cloud, qs = _nan_y_cloud_and_queries()
    # (the one cloud with a kept non-finite coordinate that the reference is recorded on: it happens to build)
    a, b = _oracle.kd_oracle(cloud, allow_nonfinite=True), _oracle.ref_answers("nan_y", cloud)
    assert a.size() == b.size() == 50
    for q in qs:
        ia, da, _ = a.search(q, 8)
        ib, db, _ = b.search(q, 8)
        assert np.array_equal(ia, ib) and np.array_equal(da.view(np.int64), db.view(np.int64))
        assert 5 not in ia                                               # NaN distance never inserted


def test_empty_cloud(oracle):
    cloud = np.zeros((0, 3), np.float32)
    a, b = _oracle.kd_oracle(cloud), _oracle.ref_answers("empty", cloud)
    assert a.size() == b.size() == 0
    assert len(a.search(np.zeros(3), 3)[0]) == 0 and len(b.search(np.zeros(3), 3)[0]) == 0


def test_bruteforce_agrees_when_no_ties(oracle):
    cloud = synth.make_cloud(5000, 11)[0]
    a = _oracle.kd_oracle(cloud)
    rng = np.random.default_rng(5)
    for q in rng.uniform([0, -8, 0], [30, 8, 4], (100, 3)):
        i1, d1 = a.search_raw(q, 8)
        i2, d2 = a.bruteforce(q, 8)
        assert np.array_equal(i1, i2) and np.array_equal(d1, d2)


def test_fma_build_of_reference_same_indices(oracle):
    """The reference's own flags (-O3 -march=native) contract the distance into FMAs: index lists
    must not change (SURVEY.md appendix C finding 3)."""
    cloud, qs = _fma_cloud_and_queries()
    a = _oracle.kd_oracle(cloud)
    b = _oracle.ref_answers("fma", cloud)
    for q in qs:
        assert np.array_equal(a.search(q, 8)[0], b.search(q, 8)[0])


@pytest.mark.parametrize("name", HOSTILE_CLOUDS)
def test_restatement_equals_reference_on_hostile_queries(name, oracle):
    """NaN / +-inf / overflowing query coordinates on finite clouds: SearchForNearest still returns `count` entries by the size
    rule; the slots the traversal did not fill hold what the reference's value-initialised result vectors hold (index 0,
    distance 0.0, DBL_MAX in the last of the n) and its point 0.  All slots, bits.  (kdo_search used to copy them out of
    uninitialised heap and index the cloud with them: segmentation fault.)"""
    cloud = _clouds()[name]
    a, b = _oracle.kd_oracle(cloud), _oracle.ref_answers("hostile." + name, cloud)
    names, qs = _hostile_queries()
    for nm, q in zip(names, qs):
        for k in (1, 3, 8):
            ia, da, pa = a.search(q, k)
            ib, db, pb = b.search(q, k)
            assert len(ia) == k and np.array_equal(ia, ib), (name, nm, k, ia, ib)
            assert np.array_equal(da.view(np.int64), db.view(np.int64)), (name, nm, k, da, db)
            assert np.array_equal(pa.view(np.int32), pb.view(np.int32)), (name, nm, k)
            ra, rb = a.search_raw(q, k), b.search_raw(q, k)
            assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1].view(np.int64), rb[1].view(np.int64)), (name, nm, k)
            if nm.startswith(("nan", "inf", "ninf", "big", "nbig")):     # no point at a distance < DBL_MAX: nothing found
                assert len(ra[0]) == 0 and da[-1] == _oracle.DBL_MAX and not da[:-1].any() and not ia.any()
            else:
                assert len(ra[0]) == k


def _poisoned(kind):
    rng = np.random.default_rng(21)
    c = rng.uniform(-10, 10, (3000, 3)).astype(np.float32)
    if kind == "nan_y_nan_z":
        c[100:300, 1] = np.nan; c[1000:1200, 2] = np.nan
    elif kind == "inf_y_ninf_z":
        c[::60, 1] = np.inf; c[7::60, 2] = -np.inf
    elif kind == "inf_x":
        c[::60, 0] = np.inf
    elif kind == "all_but_five_nan_y":
        c[5:, 1] = np.nan
    elif kind == "nan_x_only":
        c[::9, 0] = np.nan                                               # dropped, not kept: accepted
    return c


@pytest.mark.parametrize("kind", ["nan_y_nan_z", "inf_y_ninf_z", "inf_x", "all_but_five_nan_y"])
def test_tree_refuses_a_cloud_with_a_kept_nonfinite_coordinate(kind, oracle):
    """The four kinds of cloud on which the reference's build and the restatement's both ended the process with a segmentation
    fault: kdo_create returns NULL, the wrappers of both flavours raise before any build runs."""
    c = _poisoned(kind)
    lib = _oracle.load_oracle()
    assert lib.kdo_create(np.ascontiguousarray(c).reshape(-1), len(c), 3) is None
    with pytest.raises(ValueError):
        _oracle.kd_oracle(c)
    with pytest.raises(ValueError):
        _oracle.kd_ref(c) if _oracle.load_ref() is not None else _oracle.KdHandle(lib, "ref_kd", c)
    assert _oracle.kd_oracle(_poisoned("nan_x_only")).size() == 3000 - len(range(0, 3000, 9))


def _lattice_cloud():
    return (np.round(synth.make_cloud(5000, 6)[0] * 20) / 20).astype(np.float32)   # 5 cm lattice: exact ties


@pytest.mark.parametrize("name", ["corridor20k_5", "lattice5k"])
def test_numpy_reference_equals_bruteforce_on_finite_clouds(name, oracle):
    """_oracle.kd_brute_np (the expected values wherever a cloud keeps non-finite points and no tree exists) is the same
    function as kdo_bruteforce where both are defined: indices and distance bits, ties included."""
    cloud = synth.make_cloud(20000, 5)[0] if name == "corridor20k_5" else _lattice_cloud()
    a = _oracle.kd_oracle(cloud)
    rng = np.random.default_rng(13)
    qs = rng.uniform([0, -8, 0], [30, 8, 4], (250, 3))
    qs[:40] = cloud[rng.integers(0, len(cloud), 40)]
    qs[40:140] = cloud[rng.integers(0, len(cloud), 100)] + 0.025         # lattice5k: cell centres, equidistant to the corners
    tied = 0
    for q in qs:
        for k in (1, 8, 16):
            i1, d1 = a.bruteforce(q, k)
            i2, d2, size = _oracle.kd_brute_np(cloud, q, k)
            assert size == a.size() and np.array_equal(i1, i2), (name, q, k)
            assert np.array_equal(d1.view(np.int64), d2.view(np.int64)), (name, q, k)
            tied += k == 16 and len(np.unique(d1)) < len(d1)
    assert name != "lattice5k" or tied >= 30                             # the lattice does exercise the (distance, index) order


def test_numpy_reference_on_hostile_clouds():
    """Defined where the trees are not: fewer usable points than k -> that many entries; none -> none; a point at FLT_MAX is
    usable (its fp64 squared distance is ~1e77); the size counts every kept point."""
    q = np.array([0.5, 0.25, 1.0])
    c = _poisoned("all_but_five_nan_y")
    i, d, size = _oracle.kd_brute_np(c, q, 8)
    assert size == 3000 and sorted(i.tolist()) == [0, 1, 2, 3, 4] and (np.diff(d) >= 0).all()
    c[:, 2] = np.inf
    i, d, size = _oracle.kd_brute_np(c, q, 8)
    assert size == 3000 and len(i) == 0
    c = _poisoned("nan_x_only"); c[1, 1] = np.finfo(np.float32).max; c[2, :] = 1e30
    i, d, size = _oracle.kd_brute_np(c, q, 3000)
    assert len(i) == size and i[-1] == 0 and 1e76 < d[-1] < 1e78 and i[-2] == 1   # (point 0 has a NaN x: indices shift by one)
