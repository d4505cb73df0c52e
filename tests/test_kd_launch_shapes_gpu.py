"""GPU: the launch shape every search kernel shares -- the block -> (scene, query) map "scenes interleaved over the 8 XCDs, four
queries per block" (wave_slot, csrc/kd_device.h) and the grid size that has to agree with it (search_blocks) -- at scene and query
counts that are no multiple of 8 and 4, in every tie-order mode and the scan mode, which the other tests run almost only at S = 1.

S in {1, 7, 9} x Q in {1, 3, 5} x k in {1, 8}; 300 points per scene: odd scenes on a 5 cm lattice (drawn with repetition: every
row ties at k = 8, two in three at k = 1), even scenes random, scene 0 cut to k points (the count rule answers 0).  Every search and every
amk_kd_tie_flags call goes through the C ABI into buffers one scene's worth of rows longer than S Q k, filled with a sentinel: the
tail must be untouched (a grid with a block too many and a map that lets it through would write there).

What is compared: sqdist (bits) and counts are equal in all four modes; indices and pts are equal, bit for bit, between the default
and the scan mode and between AMK_TIES_NANOFLANN and AMK_TIES_AUTO; the NANOFLANN lists are the oracle tree's.  Between the two
tie orders indices and pts are compared on the rows amk_kd_tie_flags does not flag: on a tied lattice row the orders keep the
points of equal distance in different sequence (and, at the k-th slot, a different point of them) -- that is the difference the
modes exist for, and it shows on about three in four lattice rows at k = 8 -- so there each mode's pts are checked against
the cloud at its own indices instead."""
import numpy as np
import pytest

from tests import _oracle

pytestmark = pytest.mark.gpu
N_PTS = 300
SENT = -7654321          # int32 sentinel; the float buffers hold float(SENT)
MODES = ("default", "scan", "nanoflann", "auto")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test needs a GPU"
    return torch


_CLOUDS = {}


def _clouds(S):
    """[S, 300, 3] float32 (the same for every k: scene 0 is cut by its count), computed once."""
    if S not in _CLOUDS:
        rng = np.random.default_rng(100 + S)
        cl = rng.uniform(0.0, 0.3, (S, N_PTS, 3))
        cl[1::2] = np.round(cl[1::2] * 20) / 20          # 7 sites per axis, 300 draws: most points have a twin
        _CLOUDS[S] = cl.astype(np.float32)
    return _CLOUDS[S]


def _queries(S, Q):
    """[S, Q, 3] float64: cloud points (the first is one of scene 0's kept points whatever k), the last of Q > 1 off the cloud."""
    rng = np.random.default_rng(1000 * S + Q)
    cl = _clouds(S)
    qs = np.stack([c[np.concatenate([[0], rng.integers(0, N_PTS, Q - 1)])] for c in cl]).astype(np.float64)
    if Q > 1:
        qs[:, -1] = rng.uniform(-0.1, 0.4, (S, 3))
    return qs


def _guarded(torch, n, dtype):
    return torch.full((n,), SENT, dtype=dtype, device="cuda")


def _search(torch, lib, kd, qd, S, Q, k, what):
    """amk_kd_search into sentinel-filled buffers of (S + 1) Q rows -> host arrays of the S Q rows; the tail must be untouched."""
    from avoid_mpc_amd import capi
    rows, tail = S * Q, Q
    idx, d2 = _guarded(torch, (rows + tail) * k, torch.int32), _guarded(torch, (rows + tail) * k, torch.float64)
    pts, cnt = _guarded(torch, (rows + tail) * k * 3, torch.float32), _guarded(torch, rows + tail, torch.int32)
    capi.check(lib.amk_kd_search(kd.h, capi.dptr(qd), Q, k, capi.dptr(idx), capi.dptr(d2), capi.dptr(pts), capi.dptr(cnt), None),
               "amk_kd_search")
    torch.cuda.synchronize()
    idx, d2, pts, cnt = (t.cpu().numpy() for t in (idx, d2, pts, cnt))
    assert (idx[rows * k:] == SENT).all() and (cnt[rows:] == SENT).all(), (what, "int tail written")
    assert (d2[rows * k:] == float(SENT)).all() and (pts[rows * k * 3:] == float(SENT)).all(), (what, "float tail written")
    return dict(indices=idx[:rows * k].reshape(S, Q, k), sqdist=d2[:rows * k].view(np.int64).reshape(S, Q, k),
                pts=pts[:rows * k * 3].reshape(S, Q, k, 3), counts=cnt[:rows].reshape(S, Q))


def _tie_flags(torch, lib, kd, qd, S, Q, k, what):
    from avoid_mpc_amd import capi
    fl = _guarded(torch, (S + 1) * Q, torch.int32)
    capi.check(lib.amk_kd_tie_flags(kd.h, capi.dptr(qd), 3, Q, k, capi.dptr(fl), None), "amk_kd_tie_flags")
    torch.cuda.synchronize()
    fl = fl.cpu().numpy()
    assert (fl[S * Q:] == SENT).all(), (what, "flag tail written")
    assert np.isin(fl[:S * Q], (0, 1)).all(), what
    return fl[:S * Q].reshape(S, Q)


@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("S", [1, 7, 9])
def test_every_mode_answers_every_row_and_nothing_else(torch_cuda, oracle, S, k):
    torch = torch_cuda
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import KdBatch
    lib = capi.load()
    cl = _clouds(S)
    sizes = np.full(S, N_PTS, np.int32)
    sizes[0] = k
    trees = [_oracle.kd_oracle(cl[s][:sizes[s]]) for s in range(S)]
    xyz, counts = torch.from_numpy(cl).cuda(), torch.from_numpy(sizes).cuda()
    kds = {}
    for name, order in (("default", capi.AMK_TIES_LOWEST_INDEX), ("nanoflann", capi.AMK_TIES_NANOFLANN), ("auto", capi.AMK_TIES_AUTO)):
        kds[name] = KdBatch(S, N_PTS)
        kds[name].set_tie_order(order)
        kds[name].build(xyz, counts)
    ever_flagged = np.zeros(S, bool)
    for Q in (1, 3, 5):
        qs = _queries(S, Q)
        qd = torch.from_numpy(qs).cuda()
        r = {m: _search(torch, lib, kds[m], qd, S, Q, k, (m, S, Q, k)) for m in ("default", "nanoflann", "auto")}
        capi.check(lib.amk__kd_set_mode(kds["default"].h, 1))
        r["scan"] = _search(torch, lib, kds["default"], qd, S, Q, k, ("scan", S, Q, k))
        capi.check(lib.amk__kd_set_mode(kds["default"].h, 0))
        fl = {m: _tie_flags(torch, lib, kds[m], qd, S, Q, k, (m, S, Q, k)) for m in ("default", "nanoflann", "auto")}

        for m in MODES[1:]:
            for n in ("sqdist", "counts"):
                assert np.array_equal(r[m][n], r["default"][n]), (m, n, S, Q, k)
        for a, b in (("scan", "default"), ("auto", "nanoflann")):
            for n in ("indices", "pts"):
                assert np.array_equal(r[a][n], r[b][n]), (a, b, n, S, Q, k, np.argwhere(r[a][n] != r[b][n])[:4].tolist())
        # the two tie orders against each other: identical where nothing ties
        untied = fl["default"] == 0
        for n in ("indices", "pts"):
            assert np.array_equal(r["nanoflann"][n][untied], r["default"][n][untied]), (n, S, Q, k)
        # every mode's points are the cloud's at its own indices; empty slots: -1 and zeros
        for m in MODES:
            idx, pts = r[m]["indices"], r[m]["pts"]
            held = np.arange(k)[None, None, :] < r[m]["counts"][:, :, None]
            assert ((idx >= 0) == held).all() and (idx[~held] == -1).all(), (m, S, Q, k)
            want = np.where(held[..., None], cl[np.arange(S)[:, None, None], np.where(held, idx, 0)], np.float32(0))
            assert np.array_equal(pts, want), (m, S, Q, k)
        # AMK_TIES_NANOFLANN: the reference's lists
        assert (r["nanoflann"]["counts"][0] == 0).all()          # scene 0 holds exactly k points
        for s in range(S):
            for i in range(Q):
                ia, da, pa = trees[s].search(qs[s, i], k)
                c = r["nanoflann"]["counts"][s, i]
                assert c == len(ia) and (len(ia) == k or s == 0), (s, i, S, Q, k)
                assert np.array_equal(r["nanoflann"]["indices"][s, i, :c], ia), (s, i, S, Q, k)
                assert np.array_equal(r["nanoflann"]["sqdist"][s, i, :c], da.view(np.int64)), (s, i, S, Q, k)
                assert np.array_equal(r["nanoflann"]["pts"][s, i, :c], pa), (s, i, S, Q, k)

        # tie flags: the same from every handle; a row whose lists differ between the orders is flagged; the scenes AUTO has built
        # a tree for are the scenes that have had a flagged row (its search flags by the same test and builds where it flagged)
        assert np.array_equal(fl["default"], fl["nanoflann"]) and np.array_equal(fl["default"], fl["auto"]), (S, Q, k)
        differs = (r["auto"]["indices"] != r["default"]["indices"]).any(axis=2)
        assert (fl["default"][differs] == 1).all(), (S, Q, k)
        assert fl["default"][0].sum() == 0 and fl["default"][2::2].sum() == 0, (S, Q, k)     # no kept neighbours / random float32 points
        ever_flagged |= fl["auto"].any(axis=1)
        st = kds["auto"].exact_status().cpu().numpy()
        assert np.array_equal(st != capi.AMK_EXACT_NOT_NEEDED, ever_flagged), (S, Q, k, st.tolist(), ever_flagged.tolist())
    if S > 1:
        assert ever_flagged[1::2].any(), (S, k)          # (the tree path of AUTO was exercised, not only the bucketed one)
    for kd in kds.values():
        kd.close()
