"""GPU: amk_sim_clearance, amk_sim_segment_cast and amk_sim_path_cast against their numpy restatements (flight.world_clearance_ordered,
world_segment_cast_ordered, world_path_cast_ordered) bit for bit, the _host forms against the device calls byte for byte, and the path
cast against the reduction of the segment cast's own outputs -- on solid counts around the kernels' round of 64, ragged and clamped
counts, worlds without cylinders, without boxes and without either, every path length at which a block's waves divide the legs
differently, three strides, three radii, and hand-made legs and points on every edge the contract names."""
import ctypes as C

import numpy as np
import pytest

from avoid_mpc_amd import capi, flight

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
Z_TOP = 4.0


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _clamped(counts, S, n):
    return np.full(S, n) if counts is None else np.clip(counts, 0, n)


def _restated(cyl, ccnt, box, bcnt, path, radius, z_top=Z_TOP):
    """the three restatements, scene by scene, in the shapes of the device outputs"""
    S, P = path.shape[:2]
    nc, nb = _clamped(ccnt, S, cyl.shape[1]), _clamped(bcnt, S, box.shape[1])
    clear = dict(dist=np.zeros((S, P)), kind=np.zeros((S, P), np.int32), index=np.zeros((S, P), np.int32))
    seg = dict(hit=np.zeros((S, P - 1), np.int32), t=np.zeros((S, P - 1)), kind=np.zeros((S, P - 1), np.int32), index=np.zeros((S, P - 1), np.int32))
    whole = dict(stop=np.zeros(S, np.int32), leg=np.zeros(S, np.int32), t=np.zeros(S), free=np.zeros(S), pts=np.zeros((S, 3)),
                 kind=np.zeros(S, np.int32), index=np.zeros(S, np.int32))
    for s in range(S):
        c, b = cyl[s, :nc[s]], box[s, :nb[s]]
        clear["dist"][s], clear["kind"][s], clear["index"][s] = flight.world_clearance_ordered(c, b, path[s], z_top)
        seg["hit"][s], seg["t"][s], seg["kind"][s], seg["index"][s] = flight.world_segment_cast_ordered(c, b, path[s], radius, z_top)
        r = flight.world_path_cast_ordered(c, b, path[s], radius, z_top)
        for k in whole:
            whole[k][s] = r[k]
    return clear, seg, whole


def _device(torch, cyl, ccnt, box, bcnt, path, radius, z_top=Z_TOP):
    from avoid_mpc_amd.host import sim_clearance, sim_path_cast, sim_segment_cast
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    w = dict(cyl_counts=up(None if ccnt is None else ccnt.astype(np.int32)), box_counts=up(None if bcnt is None else bcnt.astype(np.int32)), z_top=z_top)
    cyl_d, box_d, path_d = up(cyl), up(box), up(path)
    out = [sim_clearance(cyl_d, box_d, path_d, **w), sim_segment_cast(cyl_d, box_d, path_d, radius, **w), sim_path_cast(cyl_d, box_d, path_d, radius, **w)]
    torch.cuda.synchronize()
    return [{k: v.cpu().numpy() for k, v in o.items()} for o in out]


def _host(lib, cyl, ccnt, box, bcnt, path, radius, z_top=Z_TOP):
    S, P, stride = path.shape
    mc, mb = cyl.shape[1], box.shape[1]
    cyl, box, path = (np.ascontiguousarray(a, np.float64) for a in (cyl, box, path))
    ccnt, bcnt = (None if a is None else np.ascontiguousarray(a, np.int32) for a in (ccnt, bcnt))
    head = (_vp(cyl) if mc else None, _vp(ccnt), mc, _vp(box) if mb else None, _vp(bcnt), mb, S, z_top)
    clear = dict(dist=np.zeros((S, P)), kind=np.zeros((S, P), np.int32), index=np.zeros((S, P), np.int32))
    seg = dict(hit=np.zeros((S, P - 1), np.int32), t=np.zeros((S, P - 1)), kind=np.zeros((S, P - 1), np.int32), index=np.zeros((S, P - 1), np.int32))
    whole = dict(stop=np.zeros(S, np.int32), leg=np.zeros(S, np.int32), t=np.zeros(S), free=np.zeros(S), pts=np.zeros((S, 3)),
                 kind=np.zeros(S, np.int32), index=np.zeros(S, np.int32))
    capi.check(lib.amk_sim_clearance_host(*head, _vp(path), stride, P, *[_vp(a) for a in clear.values()]), "amk_sim_clearance_host")
    capi.check(lib.amk_sim_segment_cast_host(*head, _vp(path), stride, P, radius, *[_vp(a) for a in seg.values()]), "amk_sim_segment_cast_host")
    capi.check(lib.amk_sim_path_cast_host(*head, _vp(path), stride, P, radius, *[_vp(a) for a in whole.values()]), "amk_sim_path_cast_host")
    return clear, seg, whole


def _check_all(torch, cyl, ccnt, box, bcnt, path, radius, z_top=Z_TOP, host=True):
    """device == restatement bit for bit, _host == device byte for byte, the path cast == the reduction of the segment cast's outputs"""
    want = _restated(cyl, ccnt, box, bcnt, path, radius, z_top)
    got = _device(torch, cyl, ccnt, box, bcnt, path, radius, z_top)
    for name, g, w in zip(("clearance", "segment_cast", "path_cast"), got, want):
        for k in w:
            assert _same(g[k], w[k]), (name, k, np.argwhere(_bits(g[k]) != _bits(w[k]))[:5], g[k], w[k])
    for s in range(path.shape[0]):                                             # the identity, on the device's own per-leg answers
        r = flight.path_cast_reduction(path[s], *[got[1][k][s] for k in ("hit", "t", "kind", "index")])
        for k in got[2]:
            assert _same(np.asarray(got[2][k][s]), np.asarray(r[k], got[2][k].dtype)), (s, k, got[2][k][s], r[k])
    if host:
        for name, g, h in zip(("clearance", "segment_cast", "path_cast"), got, _host(capi.load(), cyl, ccnt, box, bcnt, path, radius, z_top)):
            for k in g:
                assert g[k].tobytes() == h[k].tobytes(), (name, k)
    return got


def _world(rng, S, max_cyl, max_box):
    cyl = np.stack([rng.uniform(2.0, 30.0, (S, max_cyl)), rng.uniform(-8.0, 8.0, (S, max_cyl)), rng.uniform(0.1, 0.5, (S, max_cyl))], axis=2)
    yaw = rng.uniform(-1.0, 1.0, (S, max_box))
    box = np.stack([rng.uniform(2.0, 30.0, (S, max_box)), rng.uniform(-8.0, 8.0, (S, max_box)), rng.uniform(0.05, 1.0, (S, max_box)),
                    rng.uniform(0.05, 1.5, (S, max_box)), np.cos(yaw), np.sin(yaw), rng.uniform(0.0, 2.5, (S, max_box)),
                    rng.uniform(2.6, 4.0, (S, max_box))], axis=2)
    return cyl.reshape(S, max_cyl, 3), box.reshape(S, max_box, 8)


def _paths(rng, S, n_points, stride):
    """random walks along the corridor; the columns behind x y z hold NaN and noise: they are not read"""
    step = rng.normal([1.4, 0.0, 0.0], [0.4, 0.5, 0.25], (S, n_points, 3))
    step[:, 0] = np.stack([rng.uniform(-2.0, 8.0, S), rng.uniform(-6.0, 6.0, S), rng.uniform(0.6, 3.2, S)], axis=1)
    path = np.full((S, n_points, stride), NAN)
    path[:, :, 0:3] = np.cumsum(step, axis=1)
    path[:, :, 3::2] = rng.normal(size=path[:, :, 3::2].shape)
    return path


def _lib_consts():
    lib = capi.load()
    return lib.amk__sim_truth_chunk(), lib.amk__sim_truth_waves()


# (S, max_cyl, max_box, cylinder counts, box counts): 0, 1, 63, 64, 65, 130 around the round of 64; ragged; -3 and beyond the max
WORLDS = [(1, 0, 0, None, None), (1, 0, 5, None, None), (3, 7, 0, None, None), (1, 1, 1, None, None), (3, 63, 65, None, None),
          (1, 64, 64, None, None), (3, 65, 63, None, None), (1, 130, 130, None, None), (3, 130, 70, [0, 64, 130], [-3, 65, 999]),
          (3, 66, 130, [1, 999, 63], [130, 0, 64]), (3, 0, 0, None, None)]
# (n_points or None = one above a multiple of the block's waves, in legs AND in points; stride; radius)
SHAPES = [(2, 3, 0.0), (5, 10, 0.25), (21, 14, 0.25), (None, 3, 3.0), (4, 14, 0.6)]


@pytest.mark.parametrize("wi", range(len(WORLDS)))
def test_the_three_kernels_are_their_restatements_bit_for_bit(wi):
    import torch
    chunk, waves = _lib_consts()
    assert chunk == 64
    S, mc, mb, ccnt, bcnt = WORLDS[wi]
    rng = np.random.default_rng(900 + wi)
    cyl, box = _world(rng, S, mc, mb)
    ccnt, bcnt = (None if a is None else np.array(a, np.int32) for a in (ccnt, bcnt))
    seen = set()
    for si, (n_points, stride, radius) in enumerate(SHAPES):
        for n in ([3 * waves + 1, 3 * waves + 2] if n_points is None else [n_points]):
            path = _paths(rng, S, n, stride)
            got = _check_all(torch, cyl, ccnt, box, bcnt, path, radius, host=si in (1, 3))
            seen |= set(got[1]["kind"].reshape(-1).tolist())
    if mc >= 63 and mb >= 63:
        assert {-1, 0, 1, 2} <= seen, seen                                    # every kind of solid answered somewhere, and some leg was free


def test_clearance_of_a_single_point_and_of_the_odometry_layout():
    """n_points = 1 (the monitor's call: x as [S, 1, 10]), with and without counts, and every output alone (the others NULL)."""
    import torch
    from avoid_mpc_amd.host import sim_clearance
    rng = np.random.default_rng(77)
    cyl, box = _world(rng, 3, 70, 9)
    x = rng.normal(size=(3, 1, 10)); x[:, 0, 0:3] = [[5.0, 0.0, 1.0], [12.0, -3.0, 2.5], [20.0, 4.0, 0.2]]
    ccnt = np.array([70, 3, 65], np.int32)
    for counts in (None, ccnt):
        want = _restated(cyl, counts, box, None, np.concatenate([x, x], axis=1), 0.0)[0]
        up = lambda a: torch.from_numpy(a).cuda()
        got = sim_clearance(up(cyl), up(box), up(x), cyl_counts=None if counts is None else up(counts))
        for k in got:
            assert _same(got[k].cpu().numpy(), want[k][:, :1]), k
        for only in got:                                                        # one output at a time: the others are not written
            out = {k: (torch.full_like(v, 7) if k == only else None) for k, v in got.items()}
            sim_clearance(up(cyl), up(box), up(x), cyl_counts=None if counts is None else up(counts), out=out)
            assert _same(out[only].cpu().numpy(), want[only][:, :1]), only


# ---- hand-made legs -----------------------------------------------------------------------------------------------------------------
CYL = np.array([[[10.0, 0.0, 0.5], [10.0, 3.0, 0.25]]])                          # cylinder 0 on the x axis, cylinder 1 beside it
BOX = np.array([[[20.0, 0.0, 0.5, 2.0, 1.0, 0.0, 0.0, 4.0],                       # box 0: a wall, x in [19.5, 20.5], |y| <= 2, full height
                 [30.0, 0.0, 0.5, 1.5, 1.0, 0.0, 2.5, 4.0],                       # box 1: a lintel over the x axis, z in [2.5, 4]
                 [40.0, 0.0, 1.0, 1.0, np.cos(0.5), np.sin(0.5), 0.5, 1.5]]])     # box 2: yawed and floating


def _legs(torch, legs, radius, cyl=CYL, box=BOX, z_top=Z_TOP):
    """independent legs [(a, b), ...] as ONE path a_0, b_0, a_1, b_1, ...: the even legs -> their (hit, t, kind, index), every kernel checked"""
    path = np.array([p for leg in legs for p in leg], np.float64)[None]
    got = _check_all(torch, cyl, None, box, None, path, radius, z_top)
    return [tuple(got[1][k][0, 2 * i].item() for k in ("hit", "t", "kind", "index")) for i in range(len(legs))]


def test_legs_level_vertical_degenerate_and_parallel_to_each_slab():
    import torch
    r = _legs(torch, [((0, 0, 1), (9, 0, 1)),          # level, stops short of cylinder 0's mantle at x = 9.5
                      ((0, 0, 1), (16, 0, 1)),         # level, through cylinder 0: enters at 9.5 / 16
                      ((15, 0, 3), (15, 0, -1)),       # vertical, down into the ground: t = 3 / 4
                      ((10, 0, 6), (10, 0, 3)),        # vertical, down onto cylinder 0's top: z_top = 4 at t = 2 / 3
                      ((15, 1, 1), (15, 1, 1)),        # degenerate, in free space
                      ((10, 0.25, 1), (10, 0.25, 1)),  # degenerate, inside cylinder 0
                      ((18, 1, 1), (22, 1, 1)),        # d_y = d_z = 0: parallel to the y and z slabs of box 0, inside both: enters at x = 19.5
                      ((18, 3, 1), (22, 3, 1)),        # the same beside the wall (|y| > 2): parallel and outside the y slab, missed
                      ((20, -4, 1), (20, 4, 1)),       # d_x = d_z = 0 inside the x slab: enters at y = -2, t = 1 / 4
                      ((20.25, 1, 6), (20.25, 1, 2))], # d_x = d_y = 0: down onto the wall's top, z = 4 at t = 1 / 2
              0.0)
    assert r[0] == (0, 1.0, -1, -1) and r[1] == (1, 9.5 / 16, 1, 0) and r[2] == (1, 0.75, 0, -1) and r[3] == (1, 2.0 / 3.0, 1, 0)
    assert r[4] == (0, 1.0, -1, -1) and r[5] == (1, 0.0, 1, 0)
    assert r[6] == (1, 1.5 * (1.0 / 4.0), 2, 0) and r[7] == (0, 1.0, -1, -1) and r[8] == (1, 2.0 * (1.0 / 8.0), 2, 0) and r[9] == (1, 0.5, 2, 0)


def test_legs_that_start_inside_each_kind_of_solid_touch_at_zero():
    import torch
    for radius in (0.0, 0.25):
        r = _legs(torch, [((5, 0, -0.5), (5, 0, 2)),      # under the ground, going up
                          ((10, 0.1, 1), (14, 0, 1)),     # inside cylinder 0, going out
                          ((20, 0, 1), (25, 0, 1)),       # inside the wall
                          ((30, 0, 3), (30, 0, 1)),       # inside the lintel, going down
                          ((5, 0, 0.2), (6, 0, 0.2))],    # 0.2 m over the ground: inside it only for the inflated ground
                  radius)
        assert [x[:3] for x in r[:4]] == [(1, 0.0, 0), (1, 0.0, 1), (1, 0.0, 2), (1, 0.0, 2)] and r[3][3] == 1
        assert r[4] == ((1, 0.0, 0, -1) if radius > 0.2 else (0, 1.0, -1, -1))


def test_legs_that_end_on_a_face_and_one_double_short_of_it():
    import torch
    short = np.nextafter(19.5, 0.0)
    r = _legs(torch, [((18.5, 0, 1), (19.5, 0, 1)),        # ends exactly on the wall's face: t == 1 counts
                      ((18.5, 0, 1), (short, 0, 1)),       # one double short of it: free
                      ((5, 0, 2), (5, 0, 0)),              # ends exactly on the ground
                      ((5, 0, 1), (5, 0, 2.0 ** -52))], 0.0)      # d_z = -(1 - 2^-52) exactly: one ulp of the leg short of the ground
    assert r[0] == (1, 1.0, 2, 0) and r[1] == (0, 1.0, -1, -1) and r[2] == (1, 1.0, 0, -1) and r[3] == (0, 1.0, -1, -1)


def test_legs_under_a_lintel_through_it_and_grazing_an_edge():
    import torch
    r = _legs(torch, [((28, 0, 1), (32, 0, 1)),            # under the lintel (z0 = 2.5): free
                      ((28, 0, 3), (32, 0, 3)),            # through it: enters at x = 29.5, t = 1.5 / 4
                      ((28, 0, 2.5), (32, 0, 2.5)),        # along its lower face: parallel to the z slab and within it (z0 <= a_z): touched
                      ((29, -1, 3), (30, -2, 3))],         # across the corner (29.5, -1.5) only: tn == tf, a grazing leg counts
              0.0)
    assert r[0] == (0, 1.0, -1, -1) and r[1] == (1, 1.5 * 0.25, 2, 1) and r[2] == (1, 1.5 * 0.25, 2, 1)
    assert r[3] == (1, 0.5, 2, 1)
    r = _legs(torch, [((28, 0, 1), (32, 0, 1)), ((28, 0, 2.3), (32, 0, 2.3))], 0.25)   # the inflated lintel reaches down to 2.25
    assert r[0] == (0, 1.0, -1, -1) and r[1] == (1, 1.25 * 0.25, 2, 1)


def test_equal_t_on_two_solids_the_order_decides():
    """Two identical cylinders, two identical boxes, and a cylinder and a box met at the same t: the earlier one in the order ground,
    cylinders, boxes keeps it -- whatever lane it sits in."""
    import torch
    cyl = np.zeros((1, 70, 3)); cyl[0, :, 0] = 1000.0; cyl[0, :, 2] = 0.1           # far away, except:
    cyl[0, 3] = cyl[0, 68] = [10.0, 0.0, 0.5]
    box = np.zeros((1, 70, 8)); box[0, :] = [1000.0, 0.0, 0.1, 0.1, 1.0, 0.0, 0.0, 1.0]
    box[0, 5] = box[0, 66] = [20.0, 0.0, 0.5, 2.0, 1.0, 0.0, 0.0, 4.0]
    box[0, 2] = [10.0, 5.0, 0.5, 0.5, 1.0, 0.0, 0.0, 4.0]                            # its face x = 9.5, as cylinder 3's mantle on the axis
    legs = [((0, 0, 1), (16, 0, 1)), ((15, 0, 1), (25, 0, 1)), ((0, 5, 1), (16, 5, 1)), ((0, 0, 1), (16, 0, -1))]
    r = _legs(torch, legs, 0.0, cyl, box)
    assert r[0] == (1, 9.5 / 16, 1, 3) and r[1] == (1, 4.5 * 0.1, 2, 5) and r[2] == (1, 9.5 * (1.0 / 16.0), 2, 2)
    assert r[3][2] == 0 and r[3][1] == 0.5                                           # the ground at t = 1 / 2, ahead of the cylinder
    two = np.array([[[0, 0, 1.0], [16, 0, 1.0], [0, 5, 1.0]]])                       # and the box moved onto the axis: cylinder 3 first
    box[0, 2, 1] = 0.0
    got = _check_all(torch, cyl, None, box, None, two, 0.0)
    assert (got[1]["hit"][0, 0], got[1]["kind"][0, 0], got[1]["index"][0, 0]) == (1, 1, 3)


def test_a_nan_in_an_endpoint_no_hit_in_the_cast_stop_two_in_the_path():
    import torch
    for bad in (NAN, INF, -INF):
        for col in range(3):
            path = np.array([[[0, 0, 1.0], [4, 0, 1.0], [8, 0, 1.0], [12, 0, 1.0], [16, 0, 1.0]]])
            path[0, 2, col] = bad
            got = _check_all(torch, CYL, None, BOX, None, path, 0.25)
            assert got[1]["hit"][0].tolist() == [0, 0, 0, 0]
            assert got[1]["hit"][0, 1] == 0 and got[1]["hit"][0, 2] == 0 and got[1]["t"][0, 1] == 1.0
            assert (got[2]["stop"][0], got[2]["leg"][0], got[2]["t"][0], got[2]["free"][0], got[2]["kind"][0]) == (2, 1, 0.0, 4.0, -1)
    path = np.array([[[0, 0, 1.0], [4, 0, 1.0], [12, 0, 1.0], [NAN, 0, 1.0]]])       # a contact in front of the NaN: stop 1
    got = _check_all(torch, CYL, None, BOX, None, path, 0.25)
    assert (got[2]["stop"][0], got[2]["leg"][0], got[2]["kind"][0], got[2]["index"][0]) == (1, 1, 1, 0)
    assert got[2]["t"][0] == 5.25 / 8 and got[2]["free"][0] == 4.0 + (5.25 / 8) * 8.0 and got[2]["pts"][0].tolist() == [4.0 + (5.25 / 8) * 8.0, 0.0, 1.0]
    big = np.array([[[-1e308, 0, 1.0], [1e308, 0, 1.0], [0, 0, 1.0]]])               # finite endpoints, d overflows: unjudgeable as well
    got = _check_all(torch, CYL, None, BOX, None, big, 0.25)
    assert got[1]["hit"][0, 0] == 0 and got[2]["stop"][0] == 2


def test_a_nan_in_each_entry_of_a_solid_that_solid_answers_nothing():
    import torch
    path = np.array([[[0, 0, 1.0], [16, 0, 1.0], [25, 0, 1.0], [10, 0.1, 1.0], [20, 0.2, 3.0]]])
    base = _check_all(torch, CYL, None, BOX, None, path, 0.25)
    assert base[1]["kind"][0].tolist()[:2] == [1, 2] and base[0]["kind"][0].tolist()[3:] == [1, 2]
    for e in range(3):
        cyl = CYL.copy(); cyl[0, 0, e] = NAN
        got = _check_all(torch, cyl, None, BOX, None, path, 0.25, host=e == 0)
        assert not ((got[1]["kind"] == 1) & (got[1]["index"] == 0)).any() and not ((got[0]["kind"] == 1) & (got[0]["index"] == 0)).any()
        assert got[1]["hit"][0, 0] == 0 and got[1]["kind"][0, 1] == 2               # leg 0 is free now; the wall still answers leg 1
    for e in range(8):
        box = BOX.copy(); box[0, 0, e] = NAN
        got = _check_all(torch, CYL, None, box, None, path, 0.25, host=e == 0)
        assert not ((got[1]["kind"] == 2) & (got[1]["index"] == 0)).any() and not ((got[0]["kind"] == 2) & (got[0]["index"] == 0)).any()
        assert got[1]["kind"][0, 0] == 1 and got[1]["hit"][0, 1] == 0               # the cylinder still answers leg 0; leg 1 is free now


def test_points_on_a_face_inside_each_kind_over_a_cylinder_below_ground_and_under_a_floating_box():
    import torch
    pts = np.array([[[19.5, 1.0, 1.0],       # on the wall's face: 0
                     [9.5, 0.0, 1.0],        # on cylinder 0's mantle: 0
                     [10.0, 0.1, 1.0],       # inside cylinder 0: -(0.5 - 0.1)
                     [20.1, 0.0, 1.0],       # inside the wall: -(0.5 - 0.1)
                     [30.0, 0.0, 3.0],       # inside the lintel: 0.5 from every x face and from z0
                     [10.0, 0.0, 5.5],       # above z_top over cylinder 0: 1.5 to its top
                     [10.0, 1.0, 7.0],       # above and beside it: to the rim
                     [5.0, 5.0, -0.75],      # below the ground
                     [30.0, 0.0, 2.0],       # under the lintel: 0.5 to its lower face, nearer than the ground
                     [40.0, 0.0, 0.3],       # under the floating box: 0.2 to it, 0.3 to the ground
                     [41.5, 0.0, 0.2],       # beside it from below: the ground is nearer
                     [NAN, 0.0, 1.0], [3.0, 0.0, NAN], [3.0, 0.0, INF], [3.0, 0.0, -INF]]])
    got = _check_all(torch, CYL, None, BOX, None, pts, 0.0)[0]
    d, k, i = got["dist"][0], got["kind"][0], got["index"][0]
    assert d[0] == 0.0 and (k[0], i[0]) == (2, 0) and d[1] == 0.0 and (k[1], i[1]) == (1, 0)
    assert d[2] == 0.1 - 0.5 and (k[2], i[2]) == (1, 0) and d[3] == (20.1 - 20.0) - 0.5 and (k[3], i[3]) == (2, 0)
    assert d[4] == -0.5 and (k[4], i[4]) == (2, 1) and d[5] == 1.5 and (k[5], i[5]) == (1, 0)
    assert d[6] == np.sqrt(0.5 * 0.5 + 3.0 * 3.0) and (k[6], i[6]) == (1, 0)
    assert d[7] == -0.75 and (k[7], i[7]) == (0, -1) and d[8] == 0.5 and (k[8], i[8]) == (2, 1)
    assert d[9] == 0.5 - 0.3 and (k[9], i[9]) == (2, 2) and d[10] == 0.2 and (k[10], i[10]) == (0, -1)
    assert np.isnan(d[12]) and (k[12], i[12]) == (0, -1) and d[13] == INF and k[13] == 0 and d[14] == -INF and k[14] == 0


def test_a_radius_larger_than_the_gaps_and_an_infinite_one():
    import torch
    rng = np.random.default_rng(5)
    cyl, box = _world(rng, 3, 20, 6)
    path = _paths(rng, 3, 7, 10)
    path[:, :, 2] += 6.0                                                            # well above everything: only a large sphere reaches down
    free = _check_all(torch, cyl, None, box, None, path, 0.25)
    assert (free[2]["stop"] == 0).all() and (free[2]["leg"] == -1).all() and (free[2]["t"] == 1.0).all()
    big = _check_all(torch, cyl, None, box, None, path, 12.0)
    assert (big[2]["stop"] == 1).all() and (big[2]["leg"] == 0).all() and (big[2]["t"] == 0.0).all() and (big[2]["kind"] == 0).all()
    everything = _check_all(torch, cyl, None, box, None, path, INF)
    assert (everything[1]["hit"] == 1).all() and (everything[1]["t"] == 0.0).all() and (everything[1]["kind"] == 0).all()


# ---- NULL optional outputs: every entry, both forms -----------------------------------------------------------------------------------
def _null_output_cases(n):
    """each output alone, and each one missing"""
    alone = [tuple(j == k for j in range(n)) for k in range(n)]
    return alone + [tuple(not g for g in given) for given in alone]


def test_every_entry_and_both_forms_with_each_output_alone_and_with_one_missing():
    """amk_sim_clearance, amk_sim_segment_cast, amk_sim_path_cast and their _host forms with NULL optional outputs: every output alone and
    every output missing in turn.  The outputs given hold the bytes of the call with all outputs; a sentinel-filled buffer that is left
    out stays as it was (the _host forms give such an output no device storage and hand the kernel a null pointer)."""
    import torch
    lib = capi.load()
    rng = np.random.default_rng(321)
    S, P, stride, radius = 3, 6, 10, 0.25
    cyl, box = _world(rng, S, 70, 9)
    ccnt, bcnt = np.array([70, 3, 65], np.int32), np.array([9, 0, 4], np.int32)
    path = _paths(rng, S, P, stride)
    path[:, :, 3:] = 0.5
    full = _check_all(torch, cyl, ccnt, box, bcnt, path, radius)
    assert (full[1]["hit"] == 1).any() and (full[1]["hit"] == 0).any() and (full[2]["stop"] == 1).any()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dev_in = [up(a) for a in (cyl, ccnt, box, bcnt, path)]
    head_d = (capi.dptr(dev_in[0]), capi.dptr(dev_in[1]), 70, capi.dptr(dev_in[2]), capi.dptr(dev_in[3]), 9, S, Z_TOP, capi.dptr(dev_in[4]), stride, P)
    head_h = (_vp(cyl), _vp(ccnt), 70, _vp(box), _vp(bcnt), 9, S, Z_TOP, _vp(path), stride, P)
    entries = [("amk_sim_clearance", (), full[0]), ("amk_sim_segment_cast", (radius,), full[1]), ("amk_sim_path_cast", (radius,), full[2])]
    for name, extra, want in entries:
        keys = list(want)
        for given in _null_output_cases(len(keys)):
            bufs = {k: np.full_like(want[k], 7) for k in keys}
            dev = {k: up(bufs[k]) for k in keys}
            capi.check(getattr(lib, name)(*head_d, *extra, *[capi.dptr(dev[k]) if g else None for k, g in zip(keys, given)], None), name)
            torch.cuda.synchronize()
            host = {k: bufs[k].copy() for k in keys}
            capi.check(getattr(lib, name + "_host")(*head_h, *extra, *[_vp(host[k]) if g else None for k, g in zip(keys, given)]), name + "_host")
            for k, g in zip(keys, given):
                expect = want[k] if g else bufs[k]
                assert dev[k].cpu().numpy().tobytes() == expect.tobytes(), (name, given, k)
                assert host[k].tobytes() == expect.tobytes(), (name + "_host", given, k)
