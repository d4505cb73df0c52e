"""GPU: amk_kd_set_tie_order(AMK_TIES_AUTO) -- the index lists of AMK_TIES_NANOFLANN, with the reference-shaped tree built on
the device only for the scenes where a query ties among its k + 1 nearest, and only the tied queries answered by its traversal.
The comparisons are those of tests/test_kd_gpu.py for AMK_TIES_NANOFLANN (oracle tree, recorded reference answers), plus: mode 2
== mode 1 bit for bit, laziness (no tree where nothing tied), no stale tree across builds and mode switches, the give-up path."""
import ctypes as C

import numpy as np
import pytest

from tests import _oracle
from tests.test_kd_gpu import _tie_order_cases   # (the module's autouse fixture belongs to its own tests, not to this helper)
from avoid_mpc_amd import synth

pytestmark = pytest.mark.gpu
OUT = ("indices", "sqdist", "pts", "counts")
NO_TREE = 0   # amk__kd_exact_nodes of a scene whose tree has not been built for the current cloud (AMK_TIES_AUTO)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test needs a GPU"
    return torch


def _handle(torch, clouds, mode, kd=None):
    """clouds: [S, n, 3] float32 -> a KdBatch in tie-order `mode`, built (an existing handle: switched and rebuilt)."""
    from avoid_mpc_amd.host import KdBatch
    clouds = np.ascontiguousarray(clouds, np.float32)
    if kd is None:
        kd = KdBatch(clouds.shape[0], clouds.shape[1])
    kd.set_tie_order(mode)
    kd.build(torch.from_numpy(clouds).cuda())
    return kd


def _search(torch, kd, qs, k):
    """qs [S, Q, 3] float64 -> dict of host arrays; sqdist as int64 bits (NaN-proof, sign-of-zero-proof equality)."""
    r = kd.search(torch.from_numpy(np.ascontiguousarray(qs, np.float64)).cuda(), k)
    torch.cuda.synchronize()
    res = {n: r[n].cpu().numpy() for n in OUT}
    res["sqdist"] = res["sqdist"].view(np.int64)
    return res


def _same(a, b, what):
    for n in OUT:
        assert np.array_equal(a[n], b[n]), (what, n, np.argwhere(a[n] != b[n])[:4].tolist())


def _nodes(kd):
    from avoid_mpc_amd import capi
    nn = np.zeros(kd.S, np.int32)
    assert capi.load().amk__kd_exact_nodes(kd.h, nn.ctypes.data_as(C.c_void_p)) == 0
    return nn


def _oracle_nodes(t):
    lib_o = _oracle.load_oracle(); lib_o.kdo_num_nodes.restype = C.c_int; lib_o.kdo_num_nodes.argtypes = [C.c_void_p]
    return lib_o.kdo_num_nodes(t.h)


def _same_status_where_the_tree_is_unavailable(st2, st1, what):
    """Status 1 / 2 (given up, too deep) must be the same account in both modes.  A scene that AUTO never built a tree for
    (NOT_NEEDED: none of its queries tied) has no tree to give up on; its answers are the bucketed ones either way."""
    from avoid_mpc_amd import capi
    for s, (a, b) in enumerate(zip(st2.tolist(), st1.tolist())):
        if a in (capi.AMK_EXACT_GAVE_UP, capi.AMK_EXACT_TOO_DEEP) or (b in (capi.AMK_EXACT_GAVE_UP, capi.AMK_EXACT_TOO_DEEP) and a != capi.AMK_EXACT_NOT_NEEDED):
            assert a == b, (what, s, a, b)
        assert a in (b, capi.AMK_EXACT_NOT_NEEDED), (what, s, a, b)


def test_auto_index_lists_are_the_references(torch_cuda, oracle):
    """The eleven clouds of the AMK_TIES_NANOFLANN test, k = 1, 3, 8, 10, one handle in AMK_TIES_AUTO: indices, sqdist (bits), pts
    and counts equal the oracle tree's search() and the reference's recorded answers (tests/golden/kd_ref_golden.npz); and
    every output array equals, bit for bit, that of a handle in AMK_TIES_NANOFLANN."""
    torch = torch_cuda
    from avoid_mpc_amd import capi
    lib = capi.load()
    built = 0
    for name, c, qs in _tie_order_cases():
        t = _oracle.kd_oracle(c)
        tr = _oracle.ref_answers("tie." + name, c)
        kd2, kd1 = _handle(torch, c[None], capi.AMK_TIES_AUTO), _handle(torch, c[None], capi.AMK_TIES_NANOFLANN)
        assert lib.amk_kd_set_tie_order(kd2.h, 7) == capi.AMK_ERR_UNSUPPORTED          # and the handle stays in AUTO
        assert kd2.exact_status().cpu().numpy().tolist() == [capi.AMK_EXACT_NOT_NEEDED]
        for k in (1, 3, 8, 10):
            r2, r1 = _search(torch, kd2, qs[None], k), _search(torch, kd1, qs[None], k)
            _same(r2, r1, (name, k))
            idx, d2, pt, cnt = (r2[n][0] for n in OUT)
            for i, q in enumerate(qs):
                ia, da, pa = t.search(q, k)                       # KDTreeTwo::SearchForNearest semantics, traversal tie order
                assert cnt[i] == len(ia), (name, k, i)
                assert np.array_equal(idx[i][:cnt[i]], ia), (name, k, i, idx[i], ia)
                assert np.array_equal(d2[i][:cnt[i]], da.view(np.int64))
                assert np.array_equal(pt[i][:cnt[i]], pa)
                assert np.array_equal(idx[i][:cnt[i]], tr.search(q, k)[0]), (name, k, i)
        st2, st1 = kd2.exact_status().cpu().numpy(), kd1.exact_status().cpu().numpy()
        _same_status_where_the_tree_is_unavailable(st2, st1, name)
        if st2[0] != capi.AMK_EXACT_NOT_NEEDED:
            built += 1
            assert _nodes(kd2)[0] == _oracle_nodes(t), name      # the lazily built tree is the reference's
        kd2.close(); kd1.close()
    assert built >= 4      # grid, lattice, dup, planar ... really tie: the tree path was exercised, not only the bucketed one


def test_auto_equals_nanoflann_mode_on_large_clouds(torch_cuda):
    """Every path of the device build behind the lazy trigger: 200 k continuous points, 50 k on a 5 cm lattice, a 20 k-point line;
    three orders of the cloud per batch.  One handle in mode 2 against one in mode 1: identical output arrays."""
    torch = torch_cuda
    from avoid_mpc_amd import capi
    rng = np.random.default_rng(3)
    for n, kind in ((200000, "continuous"), (50000, "lattice"), (20000, "line")):
        c = synth.make_cloud(n, 11)[0]
        if kind == "lattice":
            c = (np.round(c * 20) / 20).astype(np.float32)
        if kind == "line":
            c[:, 1] = 0.5; c[:, 2] = 1.0
        cl = np.stack([c, c[::-1].copy(), c[rng.permutation(n)]])
        qs = np.concatenate([c[rng.integers(0, n, 24)].astype(np.float64), rng.uniform(-5, 25, (24, 3))])
        qs = np.stack([qs] * len(cl))
        kd2, kd1 = _handle(torch, cl, capi.AMK_TIES_AUTO), _handle(torch, cl, capi.AMK_TIES_NANOFLANN)
        r2, r1 = _search(torch, kd2, qs, 8), _search(torch, kd1, qs, 8)
        _same(r2, r1, (n, kind))
        st2, st1 = kd2.exact_status().cpu().numpy(), kd1.exact_status().cpu().numpy()
        print(f"{kind} {n}: status AUTO {st2.tolist()}, NANOFLANN {st1.tolist()}")
        _same_status_where_the_tree_is_unavailable(st2, st1, (n, kind))
        nn2, nn1 = _nodes(kd2), _nodes(kd1)
        assert all(a == b for a, b, s in zip(nn2, nn1, st2) if s != capi.AMK_EXACT_NOT_NEEDED), (kind, nn2, nn1)
        if kind == "lattice":
            assert (st2 == capi.AMK_EXACT_IN_USE).all()
        kd2.close(); kd1.close()


def _lazy_batch(rng, n=4000):
    """8 scenes: continuous random clouds (even) interleaved with copies rounded to a 0.25 m lattice (odd); queries at cloud points."""
    cont = [rng.uniform(-5, 5, (n, 3)).astype(np.float32) for _ in range(4)]
    cl = np.stack([x for c in cont for x in (c, (np.round(c * 4) / 4).astype(np.float32))])
    qs = np.stack([c[rng.integers(0, n, 16)].astype(np.float64) for c in cl])
    return cl, qs


def test_auto_builds_a_tree_only_where_a_query_tied(torch_cuda, oracle):
    """What distinguishes AUTO from mode 1.  Before any search every scene reports NOT_NEEDED; after it the continuous scenes still
    do and hold no tree (amk__kd_exact_nodes: 0, the value of a scene whose tree was never built), the lattice scenes report
    IN_USE with the oracle's node count.  That the inputs are what they claim -- no flagged query in a continuous scene, at least
    one in every lattice scene -- is asserted from amk_kd_tie_flags (random float32 coordinates against exact lattice ties)."""
    torch = torch_cuda
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import kd_tie_flags
    cl, qs = _lazy_batch(np.random.default_rng(21))
    k = 8
    kd = _handle(torch, cl, capi.AMK_TIES_AUTO)
    assert (kd.exact_status().cpu().numpy() == capi.AMK_EXACT_NOT_NEEDED).all()
    assert (_nodes(kd) == NO_TREE).all()
    fl = kd_tie_flags(kd, torch.from_numpy(qs).cuda(), k).cpu().numpy()
    assert (fl[0::2].sum(axis=1) == 0).all() and (fl[1::2].sum(axis=1) >= 1).all(), fl.sum(axis=1)
    r = _search(torch, kd, qs, k)
    st, nn = kd.exact_status().cpu().numpy(), _nodes(kd)
    assert (st[0::2] == capi.AMK_EXACT_NOT_NEEDED).all() and (st[1::2] == capi.AMK_EXACT_IN_USE).all(), st
    assert (nn[0::2] == NO_TREE).all(), nn
    for s in range(len(cl)):
        t = _oracle.kd_oracle(cl[s])
        if s % 2:
            assert nn[s] == _oracle_nodes(t), (s, nn[s])
        for i, q in enumerate(qs[s]):
            ia, da, pa = t.search(q, k)
            assert np.array_equal(r["indices"][s, i], ia) and np.array_equal(r["sqdist"][s, i], da.view(np.int64)), (s, i)
            assert np.array_equal(r["pts"][s, i], pa)
    # the host entry point goes the same way
    h = kd.search_host(qs, k)
    assert np.array_equal(h["indices"], r["indices"]) and np.array_equal(h["sqdist"].view(np.int64), r["sqdist"])
    kd.close()


def test_auto_tree_is_never_stale(torch_cuda):
    """Lattice clouds, search (trees appear); the same handle rebuilt with continuous clouds: NOT_NEEDED again, answers of a fresh
    handle; then the reverse order; then one handle through LOWEST_INDEX -> AUTO -> NANOFLANN -> AUTO across builds, each search
    answering as a fresh handle in that mode."""
    torch = torch_cuda
    from avoid_mpc_amd import capi
    rng = np.random.default_rng(22)
    cl, qs = _lazy_batch(rng)
    lat, cont = cl[1::2], cl[0::2]
    q_lat, q_cont = qs[1::2], qs[0::2]
    k = 8

    def fresh(c, q, mode):
        kd = _handle(torch, c, mode)
        r = _search(torch, kd, q, k)
        kd.close()
        return r

    for first, second in (((lat, q_lat), (cont, q_cont)), ((cont, q_cont), (lat, q_lat))):
        kd = _handle(torch, first[0], capi.AMK_TIES_AUTO)
        _same(_search(torch, kd, first[1], k), fresh(*first, capi.AMK_TIES_AUTO), "first cloud")
        st_first = kd.exact_status().cpu().numpy()
        kd = _handle(torch, second[0], capi.AMK_TIES_AUTO, kd)
        assert (kd.exact_status().cpu().numpy() == capi.AMK_EXACT_NOT_NEEDED).all() and (_nodes(kd) == NO_TREE).all()
        # queries of the FIRST cloud's kind too: whatever tree the handle still holds must not be walked
        for q in (second[1], first[1]):
            _same(_search(torch, kd, q, k), fresh(second[0], q, capi.AMK_TIES_NANOFLANN), "second cloud")
        st_second = kd.exact_status().cpu().numpy()
        want_first = capi.AMK_EXACT_IN_USE if first[0] is lat else capi.AMK_EXACT_NOT_NEEDED
        assert (st_first == want_first).all(), st_first
        if second[0] is lat:
            assert (st_second == capi.AMK_EXACT_IN_USE).all(), st_second
        kd.close()

    kd = None
    clouds = (lat, cont[:, ::-1].copy(), lat[::-1].copy(), lat)
    for mode, c in zip((capi.AMK_TIES_LOWEST_INDEX, capi.AMK_TIES_AUTO, capi.AMK_TIES_NANOFLANN, capi.AMK_TIES_AUTO), clouds):
        kd = _handle(torch, c, mode, kd)
        _same(_search(torch, kd, q_lat, k), fresh(c, q_lat, mode), ("switch", mode))
    # the switch alone changes nothing before the next build (as for AMK_TIES_NANOFLANN): the bucketed index answers
    kd = _handle(torch, lat, capi.AMK_TIES_LOWEST_INDEX, kd)
    kd.set_tie_order(capi.AMK_TIES_AUTO)
    assert (kd.exact_status().cpu().numpy() == capi.AMK_EXACT_OFF).all()
    _same(_search(torch, kd, q_lat, k), fresh(lat, q_lat, capi.AMK_TIES_LOWEST_INDEX), "no build since the switch")
    kd = _handle(torch, lat, capi.AMK_TIES_AUTO, kd)
    _same(_search(torch, kd, q_lat, k), fresh(lat, q_lat, capi.AMK_TIES_NANOFLANN), "built after the switch")
    kd.close()


def test_auto_gives_up_cleanly_and_keeps_the_bucketed_answer(torch_cuda, oracle):
    """The ring of open nodes shrunk to 2 entries (amk__exact_set_queue_cap, as in the AMK_TIES_NANOFLANN test): the lazy build of
    the 50 k-point lattice scenes ends, reports GAVE_UP, and their tied queries keep the bucketed answer (lowest index among
    equal distances); the continuous scenes of the batch are untouched (NOT_NEEDED, the reference's lists).  With the shipped
    capacity the same batch gets its trees."""
    torch = torch_cuda
    from avoid_mpc_amd import capi
    lib = capi.load()
    n = 50000
    cont = [synth.make_cloud(n, 31 + s)[0] for s in range(2)]
    cl = np.stack([(np.round(cont[0] * 20) / 20).astype(np.float32), cont[0], (np.round(cont[1] * 20) / 20).astype(np.float32), cont[1]])
    rng = np.random.default_rng(5)
    qs = np.stack([np.concatenate([c[rng.integers(0, n, 8)].astype(np.float64), rng.uniform(-5, 25, (8, 3))]) for c in cl])
    trees = [_oracle.kd_oracle(c) for c in cl]
    try:
        for cap in (2, 0):
            assert lib.amk__exact_set_queue_cap(cap) == 0
            kd = _handle(torch, cl, capi.AMK_TIES_AUTO)
            r = _search(torch, kd, qs, 8)
            st, nn = kd.exact_status().cpu().numpy(), _nodes(kd)
            print(f"queue cap {cap}: status {st.tolist()}, nodes {nn.tolist()}")
            assert (st[1::2] == capi.AMK_EXACT_NOT_NEEDED).all(), st
            assert (st[0::2] == (capi.AMK_EXACT_GAVE_UP if cap == 2 else capi.AMK_EXACT_IN_USE)).all(), (cap, st)
            for s, t in enumerate(trees):
                gave_up = st[s] == capi.AMK_EXACT_GAVE_UP
                assert nn[s] == (-1 if gave_up else (NO_TREE if s % 2 else _oracle_nodes(t))), (cap, s, nn[s])
                for i, q in enumerate(qs[s]):
                    ia, da = t.bruteforce(q, 8) if gave_up else t.search(q, 8)[:2]
                    assert np.array_equal(r["sqdist"][s, i], da.view(np.int64)), (cap, s, i)
                    assert np.array_equal(r["indices"][s, i], ia), (cap, s, i)
            kd.close()
    finally:
        lib.amk__exact_set_queue_cap(0)


def test_auto_refusals(torch_cuda):
    """k + 1 > AMK_MAX_K (the rule of amk_kd_tie_flags), the keyframe sweep with either handle in AUTO, and an unknown mode: all
    AMK_ERR_UNSUPPORTED, and nothing is launched (outputs untouched)."""
    torch = torch_cuda
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import KdBatch
    lib = capi.load()
    rng = np.random.default_rng(2)
    c = rng.uniform(-2, 2, (2, 500, 3)).astype(np.float32)
    kd = _handle(torch, c, capi.AMK_TIES_AUTO)
    assert lib.amk_kd_set_tie_order(kd.h, 7) == capi.AMK_ERR_UNSUPPORTED and lib.amk_kd_set_tie_order(kd.h, 3) == capi.AMK_ERR_UNSUPPORTED
    q = torch.from_numpy(rng.uniform(-2, 2, (2, 4, 3))).cuda()
    K = capi.AMK_MAX_K
    out = dict(indices=torch.full((2, 4, K), -7, dtype=torch.int32, device="cuda"),
               sqdist=torch.full((2, 4, K), -7.0, dtype=torch.float64, device="cuda"),
               pts=torch.full((2, 4, K, 3), -7.0, dtype=torch.float32, device="cuda"),
               counts=torch.full((2, 4), -7, dtype=torch.int32, device="cuda"))
    st = lib.amk_kd_search(kd.h, capi.dptr(q), 4, K, capi.dptr(out["indices"]), capi.dptr(out["sqdist"]), capi.dptr(out["pts"]),
                           capi.dptr(out["counts"]), None)
    torch.cuda.synchronize()
    assert st == capi.AMK_ERR_UNSUPPORTED and all(bool((v == -7).all()) for v in out.values())
    assert kd.search(q, K - 1)["indices"].shape == (2, 4, K - 1)                     # k + 1 == AMK_MAX_K is served
    with pytest.raises(capi.AmkError):
        kd.search_host(q.cpu().numpy(), K)
    # the sweep: an AUTO handle as keyframe or as current frame
    other = _handle(torch, c[:, ::-1].copy(), capi.AMK_TIES_LOWEST_INDEX)
    outl = torch.full((2,), -7, dtype=torch.int32, device="cuda"); reb = outl.clone()
    for kf, cur in ((kd, other), (other, kd)):
        sizes = kf.sizes().copy()
        assert lib.amk_kd_keyframe_sweep(kf.h, cur.h, 0.1, 1, capi.dptr(outl), capi.dptr(reb), None) == capi.AMK_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert bool((outl == -7).all()) and bool((reb == -7).all()) and np.array_equal(kf.sizes(), sizes)
    # a handle in scan mode ignores the mode (as it ignores AMK_TIES_NANOFLANN)
    lib.amk__kd_set_mode(kd.h, 1)
    assert kd.search(q, K)["indices"].shape == (2, 4, K)
    torch.cuda.synchronize()
    kd.close(); other.close()


GATE_SIZES = (0, 11, 4097, 4200)   # empty / just above the 10-point leaf / just above kExactBigNode (4096): the build's path changes


def _gate_batch():
    """Four scenes of GATE_SIZES points: distinct points of a 0.25 m lattice (coordinates exact in float32, so equal distances are
    exact ties), drawn from the smallest cube that holds them; 16 queries per scene at its own points (the empty scene: at the
    origin's corner of the lattice)."""
    rng = np.random.default_rng(34)
    cap, Q = max(GATE_SIZES), 16
    cl, qs = np.zeros((len(GATE_SIZES), cap, 3), np.float32), np.zeros((len(GATE_SIZES), Q, 3), np.float64)
    for s, n in enumerate(GATE_SIZES):
        if n == 0:
            continue
        L = int(np.ceil(n ** (1 / 3)))
        L += L ** 3 < n
        ijk = np.stack(np.unravel_index(rng.permutation(L ** 3)[:n], (L, L, L)), axis=1)
        cl[s, :n] = ijk * 0.25
        qs[s] = cl[s, rng.integers(0, n, Q)]
    return cl, np.array(GATE_SIZES, np.int32), qs


def test_one_build_pair_template_serves_both_modes(torch_cuda):
    """The build kernels are one pair template whose gate decides which workgroups build (csrc/kd_exact.hip): every scene for a
    handle in AMK_TIES_NANOFLANN, the scenes with a tied query for one in AMK_TIES_AUTO.  GATE_SIZES in one batch, every non-empty
    scene on a lattice: before a search no AUTO scene holds a tree; after it every scene with a flagged query (amk_kd_tie_flags --
    asserted to be all the non-empty ones) holds the NANOFLANN handle's node count and returns its k = 5 index lists, a scene
    without one (the empty scene) still reports no tree; a second search finds the trees built and answers the same."""
    torch = torch_cuda
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import KdBatch, kd_tie_flags
    cl, counts, qs = _gate_batch()
    k = 5
    d_cl, d_counts, d_qs = torch.from_numpy(cl).cuda(), torch.from_numpy(counts).cuda(), torch.from_numpy(qs).cuda()
    kds = {}
    for mode in (capi.AMK_TIES_NANOFLANN, capi.AMK_TIES_AUTO):
        kds[mode] = KdBatch(*cl.shape[:2])
        kds[mode].set_tie_order(mode)
        kds[mode].build(d_cl, d_counts)
    kd1, kd2 = kds[capi.AMK_TIES_NANOFLANN], kds[capi.AMK_TIES_AUTO]
    assert (_nodes(kd2) == NO_TREE).all()
    tied = kd_tie_flags(kd2, d_qs, k).cpu().numpy().any(axis=1)
    assert tied.tolist() == [n > 0 for n in GATE_SIZES], tied
    r1, r2 = _search(torch, kd1, qs, k), _search(torch, kd2, qs, k)
    nn1, nn2 = _nodes(kd1), _nodes(kd2)
    print("nodes NANOFLANN", nn1.tolist(), "AUTO", nn2.tolist())
    assert nn1[0] == 0 and (nn1[1:] > 1).all(), nn1
    for s in range(len(GATE_SIZES)):
        if tied[s]:
            assert nn2[s] == nn1[s], (s, nn2, nn1)
            assert np.array_equal(r2["indices"][s], r1["indices"][s]), s
        else:
            assert nn2[s] == NO_TREE, (s, nn2)
    assert np.array_equal(r2["counts"], r1["counts"])
    again = _search(torch, kd2, qs, k)
    _same(again, r2, "second search")
    assert np.array_equal(_nodes(kd2), nn2)
    kd1.close(); kd2.close()
