"""GPU: the keyframe map's sweep (amk_kfmap_update -> kd_sweep_mapped, csrc/kd_sweep.hip) on the scripts of tests/_sweep_cases.py, in
every sweep target and query order setting: the hashed grid with the keyframe in grid order where it has one (the default), the hashed
grid in record order, the frames' own indices.  Finite frames only: the header leaves the map unspecified for the others.

After every period the map's counts, sizes and outliers and EVERY POINT of every query frame, bit for bit and in order, equal the
numpy map's (SweepMap: _sweep_np inside NumpyMap's deque and gate); after the last one a batch of GetNearestDistance queries equals
the brute-force minimum.  No tolerance anywhere: the three settings therefore agree with each other.  tests/test_kfmap_sweep_cases.py
proves on the CPU that the scripts reach the edges they name."""
import numpy as np
import pytest

from tests import _sweep_cases as sc
from tests.test_kfmap_deque_gpu import _pack, check_state

pytestmark = pytest.mark.gpu


def run_group(cap, th, th_count, cases):
    import torch
    from avoid_mpc_amd.host import KfMap
    S = len(cases)
    refs = [sc.reference(c["name"]) for c in cases]
    gmap = KfMap(S, cap, sc.ECAP, sc.MAX_FRAMES, th, th_count, sc.DEPTH_MIN, sc.TBC)
    try:
        for t in range(3):
            what = f"max_points {cap}, th {th}, th_count {th_count}, period {t}"
            frames = [(c["clouds"][t], c["clouds"][t][:sc.ECAP].copy(), sc.TWC) for c in cases]
            cl, ed, Tw, cn, en = _pack(frames, cap, sc.ECAP)
            gmap.add_vertex(cl, ed, Tw, counts=cn, edge_counts=en)
            gmap.update()
            check_state(gmap.state(), [r["rows"][t][:3] for r in refs], what)
            for s, (c, r) in enumerate(zip(cases, refs)):
                want = r["rows"][t][3]
                pts, sz = gmap.points(s)
                assert sz[:len(want)].tolist() == [len(f) for f in want] and (sz[len(want):] == -1).all(), (what, c["name"], sz)
                exp = np.concatenate(want) if want else np.zeros((0, 3), np.float32)
                assert pts.shape == exp.shape, (what, c["name"], pts.shape, exp.shape)
                same = (pts.view(np.int32) == exp.view(np.int32)).all(axis=1)
                assert same.all(), (what, c["name"], "first differing point", int(np.argmin(same)), pts[np.argmin(same)], exp[np.argmin(same)])
        q = np.stack([sc.distance_queries(c["name"]) for c in cases])
        d = gmap.nearest_distance(torch.from_numpy(q).cuda()).cpu().numpy()
        e = np.array([[sc.expected_distance(r["rows"][2][3], q[s, j]) for j in range(sc.NQ)] for s, r in enumerate(refs)])
        assert np.array_equal(d.view(np.int64), e.view(np.int64)), (cap, th, th_count, np.argwhere(d != e).tolist(), d[d != e], e[d != e])
    finally:
        gmap.close()


@pytest.mark.parametrize("target,order", [(1, 1), (1, 0), (0, 1)])
def test_map_sweep_equals_the_numpy_map(target, order):
    from avoid_mpc_amd import capi
    lib = capi.load()
    lib.amk__sweep_set_target(target); lib.amk__sweep_set_order(order)
    try:
        for (cap, th, th_count), cases in sc.groups().items():
            run_group(cap, th, th_count, cases)
    finally:
        lib.amk__sweep_set_target(1); lib.amk__sweep_set_order(1)
