"""CPU: amk_sim_clearance, amk_sim_segment_cast, amk_sim_path_cast (and their _host forms) without a device -- the symbols are declared,
listed, bound and exported; every argument rule is refused before the device is asked for, the outputs untouched; the header states
the contract; the new kernels use no scratch and live in sim_truth.hip's object.  And the three numpy restatements
(flight.world_clearance_ordered, world_segment_cast_ordered, world_path_cast_ordered) are held to independent formulations: the cast at
radius 0 to the sensor's restatement (render_world_ordered), the clearance to "norm of p minus its clamp into the solid" with matrix
products and to the two report helpers (box_clearance, FlightWorld.clearance), the contact to an independent inside test along the leg,
and the path cast to the reduction of the segment cast."""
import ctypes as C
import glob
import json
import os
import re

import numpy as np
import pytest

from avoid_mpc_amd import build as amk_build
from avoid_mpc_amd import capi, flight
from tests import _flight

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIX = ["amk_sim_clearance", "amk_sim_clearance_host", "amk_sim_segment_cast", "amk_sim_segment_cast_host", "amk_sim_path_cast",
       "amk_sim_path_cast_host"]
INTERNAL = ["amk__sim_truth_chunk", "amk__sim_truth_waves"]
BAD, UNSUPPORTED, NO_DEVICE = capi.AMK_ERR_INVALID_ARG, capi.AMK_ERR_UNSUPPORTED, capi.AMK_ERR_NO_DEVICE
U = 2.0 ** -53   # the unit roundoff of a double
NAN = float("nan")
MAX_BLOCKS = 2 ** 24 - 1   # blocks along a grid dimension at 256 threads: the dimension times the block size stays below 2^32


@pytest.fixture(scope="module")
def lib():
    amk_build.build()
    return capi.load()


def _section():
    hdr = open(os.path.join(ROOT, "include", "avoid_mpc_amd.h")).read()
    return hdr, hdr[hdr.index("Closed-loop simulation"):]


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def test_the_new_symbols_are_declared_listed_bound_and_exported(lib):
    hdr, section = _section()
    for name in SIX:
        assert re.search(r"^int " + name + r"\(", section, re.M), name       # declared, in the simulation's section
        assert name in capi.SYMBOLS                                          # listed
        fn = getattr(lib, name)                                              # exported
        assert fn.argtypes is not None and fn.restype is C.c_int, name       # bound
    assert capi.missing_symbols() == []
    assert [len(getattr(lib, n).argtypes) for n in SIX] == [15, 14, 17, 16, 20, 19]
    for name in INTERNAL:                                                    # the tests' own: exported and bound, not in the header
        assert getattr(lib, name).restype is C.c_int and name not in hdr and name not in capi.SYMBOLS
    assert lib.amk__sim_truth_chunk() == 64 and lib.amk__sim_truth_waves() >= 1


def _world():
    return dict(cyl=np.ones((2, 3, 3)), cnt=np.full(2, 3, np.int32), box=np.ones((2, 2, 8)), bcnt=np.full(2, 2, np.int32))


def _world_refusals(call):
    """what all three refuse about the world, through call(**overrides)"""
    assert call(cyl_=None) == BAD and call(box_=None) == BAD and call(mc=-1) == BAD and call(mb=-1) == BAD
    assert call(cyl_=None, mc=1) == BAD and call(box_=None, mb=1) == BAD
    assert call(S=0) == BAD and call(S=-2) == BAD
    assert call(zt=-1.0) == BAD and call(zt=NAN) == BAD and call(zt=-1e-300) == BAD
    assert call(mc=2 ** 31 - 1, mb=2 ** 31 - 1) == UNSUPPORTED and call(mc=2 ** 31 - 2, mb=1) == UNSUPPORTED


def _world_accepted(call):
    """good calls reach the device question and nothing else"""
    assert call() == NO_DEVICE and call(cnt_=None, bcnt_=None) == NO_DEVICE and call(zt=0.0) == NO_DEVICE and call(zt=float("inf")) == NO_DEVICE
    assert call(cyl_=None, mc=0) == NO_DEVICE and call(box_=None, mb=0) == NO_DEVICE
    assert call(cyl_=None, cnt_=None, mc=0, box_=None, bcnt_=None, mb=0) == NO_DEVICE


def test_clearance_refuses_bad_arguments_without_a_device(lib):
    w = _world()
    pts = np.ones((2, 4, 5)); dist = np.full((2, 4), 7.0); kind = np.full((2, 4), 7, np.int32); index = np.full((2, 4), 7, np.int32)
    for fn, tail in ((lib.amk_sim_clearance, (None,)), (lib.amk_sim_clearance_host, ())):
        call = lambda cyl_=_vp(w["cyl"]), cnt_=_vp(w["cnt"]), mc=3, box_=_vp(w["box"]), bcnt_=_vp(w["bcnt"]), mb=2, S=2, zt=4.0, p=_vp(pts), \
            stride=5, n=4, d=_vp(dist), k=_vp(kind), i=_vp(index): fn(cyl_, cnt_, mc, box_, bcnt_, mb, S, zt, p, stride, n, d, k, i, *tail)
        _world_refusals(call)
        assert call(p=None) == BAD and call(stride=2) == BAD and call(stride=0) == BAD and call(n=0) == BAD and call(n=-1) == BAD
        assert call(d=None, k=None, i=None) == BAD
        assert call(S=65536) == UNSUPPORTED
        assert call(n=4 * MAX_BLOCKS + 1) == UNSUPPORTED and call(n=2 ** 31 - 1) == UNSUPPORTED   # four points per block, 2^24 - 1 blocks
        if lib.amk_device_count() <= 0:
            _world_accepted(call)
            assert call(n=1) == NO_DEVICE and call(stride=3) == NO_DEVICE and call(d=None) == NO_DEVICE and call(d=None, k=None) == NO_DEVICE
            assert lib.amk_sim_clearance(None, None, 0, None, None, 0, 1, 4.0, _vp(pts), 3, 4 * MAX_BLOCKS, _vp(dist), None, None, None) == NO_DEVICE
    assert (dist == 7.0).all() and (kind == 7).all() and (index == 7).all()


def test_segment_cast_refuses_bad_arguments_without_a_device(lib):
    w = _world()
    path = np.ones((2, 4, 5)); hit = np.full((2, 3), 7, np.int32); t = np.full((2, 3), 7.0); kind = np.full((2, 3), 7, np.int32)
    index = np.full((2, 3), 7, np.int32)
    for fn, tail in ((lib.amk_sim_segment_cast, (None,)), (lib.amk_sim_segment_cast_host, ())):
        call = lambda cyl_=_vp(w["cyl"]), cnt_=_vp(w["cnt"]), mc=3, box_=_vp(w["box"]), bcnt_=_vp(w["bcnt"]), mb=2, S=2, zt=4.0, p=_vp(path), \
            stride=5, n=4, r=0.25, h=_vp(hit), t_=_vp(t), k=_vp(kind), i=_vp(index): fn(cyl_, cnt_, mc, box_, bcnt_, mb, S, zt, p, stride, n, r, h,
                                                                                          t_, k, i, *tail)
        _world_refusals(call)
        assert call(p=None) == BAD and call(stride=2) == BAD and call(n=1) == BAD and call(n=0) == BAD and call(n=-4) == BAD
        assert call(r=-1e-300) == BAD and call(r=-1.0) == BAD and call(r=NAN) == BAD
        assert call(h=None, t_=None, k=None, i=None) == BAD
        assert call(S=65536) == UNSUPPORTED
        assert call(n=4 * MAX_BLOCKS + 2) == UNSUPPORTED and call(n=2 ** 31 - 1) == UNSUPPORTED   # four legs per block, 2^24 - 1 blocks
        if lib.amk_device_count() <= 0:
            _world_accepted(call)
            assert call(n=2) == NO_DEVICE and call(r=0.0) == NO_DEVICE and call(r=float("inf")) == NO_DEVICE
            assert call(h=None, t_=None, k=None) == NO_DEVICE
            assert lib.amk_sim_segment_cast(None, None, 0, None, None, 0, 1, 4.0, _vp(path), 3, 4 * MAX_BLOCKS + 1, 0.0, _vp(hit), None, None, None, None) == NO_DEVICE
    assert (hit == 7).all() and (t == 7.0).all() and (kind == 7).all() and (index == 7).all()


def test_path_cast_refuses_bad_arguments_without_a_device(lib):
    w = _world()
    path = np.ones((2, 4, 5))
    outs = [np.full(2, 7, np.int32), np.full(2, 7, np.int32), np.full(2, 7.0), np.full(2, 7.0), np.full((2, 3), 7.0), np.full(2, 7, np.int32),
            np.full(2, 7, np.int32)]
    for fn, tail in ((lib.amk_sim_path_cast, (None,)), (lib.amk_sim_path_cast_host, ())):
        call = lambda cyl_=_vp(w["cyl"]), cnt_=_vp(w["cnt"]), mc=3, box_=_vp(w["box"]), bcnt_=_vp(w["bcnt"]), mb=2, S=2, zt=4.0, p=_vp(path), \
            stride=5, n=4, r=0.25, o=tuple(_vp(a) for a in outs): fn(cyl_, cnt_, mc, box_, bcnt_, mb, S, zt, p, stride, n, r, *o, *tail)
        _world_refusals(call)
        assert call(p=None) == BAD and call(stride=2) == BAD and call(n=1) == BAD and call(n=0) == BAD
        assert call(r=-1.0) == BAD and call(r=NAN) == BAD
        assert call(o=(None,) * 7) == BAD
        assert call(S=MAX_BLOCKS + 1) == UNSUPPORTED and call(S=2 ** 31 - 1) == UNSUPPORTED            # a block per scene
        if lib.amk_device_count() <= 0:
            _world_accepted(call)
            assert call(S=65536) == NO_DEVICE                                 # a block per scene: the scenes are the grid's first dimension
            assert lib.amk_sim_path_cast(None, None, 0, None, None, 0, MAX_BLOCKS, 4.0, _vp(path), 3, 2, 0.0, _vp(outs[0]), *[None] * 7) == NO_DEVICE
            for keep in range(7):
                assert call(o=tuple(_vp(a) if j == keep else None for j, a in enumerate(outs))) == NO_DEVICE
    for a in outs:
        assert (a == 7).all()


def test_the_header_states_the_truth_contract():
    section = re.sub(r"\s*\*?\s+", " ", _section()[1])                         # comment stars and line breaks out
    section = section[section.index("Ground truth against the simulated world"):]
    for sentence in ("Every entry begins with the world arguments of amk_sim_render_world, in that order and with those meanings",
                     "Counts are clamped into [0, max]", "with both zero the world is the ground alone",
                     "d_odom (stride 10, one point) and x0array (stride 14, N rows) go in as they are",
                     "fp64, no contraction, every sum left to right as written; division, reciprocal and square root are IEEE-correct",
                     "a two-operand select drops a NaN", "A solid with a NaN in any of its entries",
                     "answers nothing, in the clearance and in the casts", "every entry e is tested with e == e",
                     "the ground, then the cylinders in index order, then the boxes in index order",
                     "qr = sqrt(ox ox + oy oy) - r; qz = p_z - z_top", "dist = sqrt(mr mr + mz mz) + (m < 0 ? m : 0)",
                     "qx = |olx| - |hx|, qy = |oly| - |hy|", "dist = sqrt((mx mx + my my) + mz mz) + (m < 0 ? m : 0)",
                     "a NaN height stays NaN with kind 0", "ground: z <= radius", "cylinder: radius R = r + radius, cut at z_top + radius",
                     "half extents |hx| + radius, |hy| + radius, vertical extent [z0 - radius, z1 + radius]",
                     "superset of the true swept sphere", "at most (sqrt(3) - 1) radius", "radius == 0 is the centre line",
                     "bound = (h - a_z) inv_z", "a == 0: [-inf, +inf] when c <= 0, else [+inf, -inf]",
                     "[(-b - sqrt(disc)) / a, (-b + sqrt(disc)) / a]", "amk_sim_render_world's slab rule word for word",
                     "the solid is touched iff every axis has near <= far, and tn <= tf && tf >= 0 && tn <= 1; its t is tn > 0 ? tn : 0.0",
                     "A leg that starts inside a solid touches it at t = 0", "the one place the cast differs from the sensor",
                     "A degenerate leg (a == b) touches iff its start is inside", "has no contact here",
                     "0 free to the end, 1 contact, 2 unjudgeable leg", "((len_0 + len_1) + ...) + t len_leg",
                     "len_j = sqrt((d_x d_x + d_y d_y) + d_z d_z)", "the last term is left out when d_stop is 2", "a_i + t d_i",
                     "Identity: the answer equals this reduction applied to amk_sim_segment_cast's per-leg outputs on the same path, bit for bit",
                     "Every error is returned before anything is staged or launched, the outputs untouched",
                     "stream-ordered and allocate nothing", "more than 2^24 - 1 scenes (a block per scene)",
                     "more than 4 (2^24 - 1) points or legs per scene",
                     "Not offered: the exact rounded Minkowski sum, per-scene radii, several contacts per leg, moving solids, the casts inside the pipeline"):
        assert sentence in section, sentence


def test_the_new_kernels_use_no_scratch_and_live_in_one_object(lib):
    table = json.load(open(amk_build.RES))
    mine = {n: r for n, r in table.items() if "sim_truth_" in n}
    assert len(mine) == 3 and all(any(k in n for n in mine) for k in ("clearance_kernel", "segment_kernel", "path_kernel")), sorted(mine)
    for n, r in mine.items():
        print(n, r)
        assert r["scratch_bytes_per_lane"] == 0 and r["lds_bytes"] <= 1024 and r["occupancy"] >= 4, (n, r)
    per_object = {os.path.basename(p)[:-len(".o.res.json")]: list(json.load(open(p))) for p in glob.glob(os.path.join(amk_build.OBJ, "*.o.res.json"))}
    assert [u for u, ks in per_object.items() if any("sim_truth_" in k for k in ks)] == ["sim_truth"]


# ---- worlds and paths for the restatements -----------------------------------------------------------------------------------------
def _solids(seed, n_cyl=12, n_box=9):
    """cylinders and yawed boxes ahead of the origin, some boxes floating; box 0 axis-aligned"""
    rng = np.random.default_rng(seed)
    cyl = np.stack([rng.uniform(3.0, 20.0, n_cyl), rng.uniform(-6.0, 6.0, n_cyl), rng.uniform(0.1, 0.6, n_cyl)], axis=1)
    yaw = rng.uniform(-1.0, 1.0, n_box)
    box = np.stack([rng.uniform(3.0, 20.0, n_box), rng.uniform(-6.0, 6.0, n_box), rng.uniform(0.1, 1.5, n_box), rng.uniform(0.05, 1.5, n_box),
                    np.cos(yaw), np.sin(yaw), rng.uniform(0.0, 1.5, n_box), rng.uniform(2.0, 4.0, n_box)], axis=1)
    box[0, 4:6] = [1.0, 0.0]
    return cyl, box


def _cast_rays(cyl, box, a, b, radius, z_top):
    """Independent legs a_i -> b_i through ONE call: the path a_0, b_0, a_1, b_1, ... whose even legs they are -> (hit, t, kind, index)"""
    path = np.stack([a, b], axis=1).reshape(-1, 3)
    return tuple(v[0::2] for v in flight.world_segment_cast_ordered(cyl, box, path, radius, z_top))


def _scale(p, cyl, box):
    """The coordinates' scale per (point, solid): |p|_1 plus the solid's own entries -> ([P, n_cyl], [P, n_box])"""
    pn = np.abs(np.asarray(p)[..., 0:3]).sum(axis=-1)[:, None]
    return pn + np.abs(cyl).sum(axis=1) + 4.0, pn + np.abs(box[:, [0, 1, 2, 3, 6, 7]]).sum(axis=1)


# ---- (a) the cast at radius 0 against the sensor -------------------------------------------------------------------------------------
ROWS, COLS = 48, 64
CAM = dict(fx=32.0, fy=32.0, cx=31.7, cy=24.2)
RANGE = 64.0   # the sensor's max_range and the legs' length: a power of two, so that RANGE * d and t * RANGE are exact


def _pose(p, th=0.2):
    T = np.eye(4); T[:3, 3] = p
    T[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
    return T


def _rays(Twb, Tbc):
    """The sensor's own camera centre and rays, by render_world_ordered's lines (they are this comparison's INPUT, so both sides start
    from the same bits) -> (o [3], dir [rows * cols, 3])"""
    A, B = np.asarray(Twb, np.float64).reshape(4, 4), np.asarray(Tbc, np.float64).reshape(4, 4)
    M = np.empty((3, 4))
    for i in range(3):
        for j in range(4):
            M[i, j] = ((A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]) + A[i, 3] * B[3, j]
    v, u = np.meshgrid(np.arange(ROWS, dtype=np.float64), np.arange(COLS, dtype=np.float64), indexing="ij")
    dc0, dc1 = (u - CAM["cx"]) / CAM["fx"], (v - CAM["cy"]) / CAM["fy"]
    return M[:, 3].copy(), np.stack([((M[i, 0] * dc0 + M[i, 1] * dc1) + M[i, 2] * 1.0).reshape(-1) for i in range(3)], axis=1)


def _cast_tolerance(o, D0, D1, t, kind, index, cyl, box):
    """The per-pixel bound of test_the_cast_at_radius_zero_is_the_sensor (see there).  D0: the sensor's rays, D1: the cast's d / RANGE."""
    eps = np.abs(D1 - D0)
    tol = np.zeros(len(t))
    with np.errstate(all="ignore"):
        g = kind == flight.KIND_GROUND                                            # t = -o_z / d_z against (0 - o_z) (1 / d_z'): exactly
        tol[g] = t[g] * eps[g, 2] / np.abs(D1[g, 2]) + 8 * U * t[g]               # t (d_z' - d_z) / d_z' apart, plus three roundings (8 u t)
        for k in np.unique(index[kind == flight.KIND_CYLINDER]):
            m = (kind == flight.KIND_CYLINDER) & (index == k)
            ox, oy, r = o[0] - cyl[k, 0], o[1] - cyl[k, 1], cyl[k, 2]
            c = ox * ox + oy * oy - r * r
            side = []
            for D in (D0[m], D1[m]):
                a, b = D[:, 0] ** 2 + D[:, 1] ** 2, ox * D[:, 0] + oy * D[:, 1]
                side.append((a, b, np.sqrt(np.maximum(b * b - a * c, 0.0))))
            (a0, b0, s0), (a1, b1, s1) = side
            Ea = np.abs(a1 - a0) + 4 * U * (a0 + a1)                              # the two sides' a, b, disc as computed: their difference
            Eb = np.abs(b1 - b0) + 4 * U * (abs(ox) * (np.abs(D0[m, 0]) + np.abs(D1[m, 0])) + abs(oy) * (np.abs(D0[m, 1]) + np.abs(D1[m, 1])))
            Ed = (np.abs(b0) + np.abs(b1)) * Eb + abs(c) * Ea + 8 * U * (b0 * b0 + b1 * b1 + abs(c) * (a0 + a1))
            Es = Ed / np.maximum(s0 + s1, 1e-300) + 2 * U * (s0 + s1)             # |s1 - s0| = |disc1 - disc0| / (s0 + s1), exactly
            En = Eb + Es + 4 * U * (np.abs(b0) + s0)                              # the numerator -b - s
            tol[m] = 2 * (En + t[m] * Ea) / np.minimum(a0, a1) + 8 * U * t[m]
        for k in np.unique(index[kind == flight.KIND_BOX]):
            m = (kind == flight.KIND_BOX) & (index == k)
            bx, by, hx, hy, cs, sn, z0, z1 = box[k]
            R = np.array([[cs, sn, 0.0], [-sn, cs, 0.0], [0.0, 0.0, 1.0]])
            ol, lo, hi = R @ (o - np.array([bx, by, 0.0])), np.array([-hx, -hy, z0]), np.array([hx, hy, z1])
            dl0, dl1 = D0[m] @ R.T, D1[m] @ R.T
            near = np.minimum((lo - ol) / dl0, (hi - ol) / dl0)                   # the three slabs' entries: t is the largest of them
            Edl = eps[m] @ np.abs(R).T + 8 * U * (np.abs(D0[m]) @ np.abs(R).T)
            L = np.abs(o).sum() + abs(bx) + abs(by) + hx + hy + abs(z0) + abs(z1)
            # a slab's near = N / dl: N is the same number on both sides up to 16 u L (its roundings, as in test_sim_world_abi.py), dl differs by Edl
            each = 2 * (16 * U * L + np.abs(near) * Edl) / np.minimum(np.abs(dl0), np.abs(dl1)) + 8 * U * np.abs(near)
            each = np.where(np.isfinite(each), each, np.inf)
            active = near + each >= t[m][:, None]                                 # only a slab that can reach t can move the largest near
            tol[m] = np.where(active, each, 0.0).max(axis=1)
    return tol


@pytest.mark.parametrize("seed", [31, 32, 33])
def test_the_cast_at_radius_zero_is_the_sensor(seed):
    """world_segment_cast_ordered at radius 0 from the camera centre along every pixel's ray, RANGE = 64 m long, against
    render_world_ordered with max_range = RANGE, in three WallWorld corridors from three poses each (yaw 0.2, above the ground and
    below z_top), 48 x 64: 27 648 pixels, none left out.  The hit sets are identical, and t RANGE agrees with the sensor's t to a
    bound derived per pixel, not fitted.
    The leg of pixel i is a = o, b = fl(o + RANGE dir_i), d = fl(b - a).  RANGE is a power of two, so RANGE dir_i is exact and so is
    every scaling by it: the cast computes, operation for operation, what the sensor's formulas give for the ray D' = d / RANGE in
    place of dir -- |D' - dir| is known to the test, it is at most u (|o| / RANGE + 2 |dir|) per component -- except at the ground,
    where the cast takes (0 - o_z) (1 / d_z) for the sensor's -o_z / d_z.  So the two differ by the sensitivity of t to its ray:
      ground:    t - t' = t (d_z' - d_z) / d_z' exactly, and three roundings.
      a box:     t is the largest of three entries N / dl, N the same number on both sides up to its own roundings (at most 16 u L, L the
                 coordinates' scale), dl = R D differing by |R| |D' - dir| and its roundings; only a slab whose entry can reach t within
                 its own bound can move the largest.
      cylinder:  t = (-b - s) / a, s = sqrt(disc): both sides' a, b and disc are recomputed here and their differences bounded by the
                 differences seen plus the roundings of either side; |s' - s| = |disc' - disc| / (s + s') holds exactly, so the bound
                 stays valid at a silhouette, where it grows as it must.
    Each first-order step is doubled to cover the second order."""
    prm, _ = _flight.make_prm("C1")
    world = flight.WallWorld(seed, prm, 1000, cyl_per_m=1.5, x_first=3.0, length=60.0)
    cyl = np.stack([world.cx, world.cy, world.cr], axis=1)
    worst, pixels = 0.0, 0
    for p in ([0.3, -0.2, 1.1], [14.0, 2.0, 0.4], [30.5, -1.5, 3.1]):
        Twb = _pose(p)
        sensor = flight.render_world_ordered((world.cx, world.cy, world.cr), world.box, Twb, flight.TBC_YAML, ROWS, COLS, CAM["fx"], CAM["fy"],
                                             CAM["cx"], CAM["cy"], z_top=4.0, max_range=RANGE).reshape(-1)
        o, D0 = _rays(Twb, flight.TBC_YAML)
        assert 0.0 < o[2] < 4.0
        b = o + RANGE * D0
        hit, t, kind, index = _cast_rays(cyl, world.box, np.broadcast_to(o, b.shape), b, 0.0, 4.0)
        t = t * RANGE
        assert np.array_equal(hit != 0, sensor > 0), np.argwhere((hit != 0) != (sensor > 0))[:10]
        assert {0, 1, 2} <= set(kind[hit != 0].tolist())                            # the ground, cylinders and boxes are all in the images
        D1 = (b - o) / RANGE
        tol = _cast_tolerance(o, D0, D1, sensor, kind, index, cyl, world.box)
        both = hit != 0
        err = np.abs(t - sensor)
        worst = max(worst, (err[both] / sensor[both]).max()); pixels += len(D0)
        print("pose", p, "hits", both.sum(), "largest |dt| / tol", (err[both] / tol[both]).max(), "largest relative dt", (err[both] / sensor[both]).max())
        assert (err[both] <= tol[both]).all(), np.argwhere(both & (err > tol))[:10]
    print("pixels", pixels, "largest relative dt overall", worst)


# ---- (b) the clearance against a second formulation ----------------------------------------------------------------------------------
def _clearance_by_clamping(p, cyl, box, z_top):
    """The independent side: outside a solid the norm of p minus its clamp into the solid, inside the least face distance, the boxes'
    frames by matrix products -> (dist [P, 1 + n_cyl + n_box] in the order ground, cylinders, boxes)"""
    p = np.asarray(p, np.float64)[:, 0:3]
    cols = [p[:, 2]]
    for cx, cy, r in cyl:
        rho, z = np.linalg.norm(p[:, 0:2] - np.array([cx, cy]), axis=1), p[:, 2]
        out = np.hypot(rho - np.minimum(rho, r), z - np.minimum(z, z_top))
        cols.append(np.where((rho <= r) & (z <= z_top), -np.minimum(r - rho, z_top - z), out))
    for bx, by, hx, hy, c, s, z0, z1 in box:
        R = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
        q = (p - np.array([bx, by, 0.0])) @ R.T
        lo, hi = np.array([-abs(hx), -abs(hy), z0]), np.array([abs(hx), abs(hy), z1])
        out = np.linalg.norm(q - np.clip(q, lo, hi), axis=1)
        cols.append(np.where(((q >= lo) & (q <= hi)).all(axis=1), -np.minimum(q - lo, hi - q).min(axis=1), out))
    return np.stack(cols, axis=1)


@pytest.mark.parametrize("seed", [41, 42, 43])
def test_clearance_against_the_norm_of_p_minus_its_clamp(seed):
    """world_clearance_ordered against the clamp formulation on 4000 random points (a quarter of them drawn inside a solid): the same
    winner, and the value within 32 u L, L = |p|_1 plus the solid's entries.  Either side reaches its distance through at most a dozen
    roundings of numbers no larger than L (differences of coordinates, a 2 x 2 rotation, squares, a sum, a root), each at most u L
    in absolute terms once carried to the result: 2 x 12 u L, rounded up to 32."""
    cyl, box = _solids(seed)
    rng = np.random.default_rng(seed + 100)
    pts = np.stack([rng.uniform(0.0, 23.0, 4000), rng.uniform(-8.0, 8.0, 4000), rng.uniform(-0.5, 6.0, 4000)], axis=1)
    pts[:500, 0:2] = cyl[rng.integers(0, len(cyl), 500), 0:2] + rng.uniform(-0.1, 0.1, (500, 2))
    k = rng.integers(0, len(box), 500)
    pts[500:1000, 0:2] = box[k, 0:2] + rng.uniform(-0.04, 0.04, (500, 2)); pts[500:1000, 2] = rng.uniform(box[k, 6], box[k, 7])
    dist, kind, index = flight.world_clearance_ordered(cyl, box, pts, 4.0)
    ref = _clearance_by_clamping(pts, cyl, box, 4.0)
    win = np.where(kind == 0, 0, np.where(kind == 1, 1 + index, 1 + len(cyl) + index))
    assert np.array_equal(win, ref.argmin(axis=1)), np.argwhere(win != ref.argmin(axis=1))[:10]
    assert {0, 1, 2} <= set(kind.tolist()) and (dist[kind == 1] < 0).any() and (dist[kind == 2] < 0).any() and (dist[kind == 0] < 0).any()
    Lc, Lb = _scale(pts, cyl, box)
    L = np.concatenate([np.abs(pts).sum(axis=1)[:, None], Lc, Lb], axis=1)[np.arange(len(pts)), win]
    err = np.abs(dist - ref.min(axis=1))
    print("largest |d - ref| / (u L):", (err / (U * L)).max())
    assert (err <= 32 * U * L).all()
    # per solid, not only the winner's: the two per-solid tables agree everywhere
    table = np.concatenate([pts[:, 2:3], flight.cylinder_distance_ordered(pts, cyl, 4.0), flight.box_distance_ordered(pts, box)], axis=1)
    Lall = np.concatenate([np.abs(pts).sum(axis=1)[:, None], Lc, Lb], axis=1)
    assert (np.abs(table - ref) <= 32 * U * Lall).all()


def test_clearance_reproduces_the_two_report_helpers():
    """For points level with full-height boxes and below z_top the three-dimensional distances ARE the report helpers' horizontal ones,
    exactly: with q_z < 0 the vertical term adds mz mz = 0 to the sum under the root, and the inside term is max(qx, qy) whenever that
    is >= q_z (WallWorld's walls are 0.1 m thick, the points at least 1 m from a box's top and bottom; the cylinders' q_z is -496 m under
    a z_top of 500 m).  sqrt(q q) is |q| exactly."""
    prm, _ = _flight.make_prm("C1")
    world = flight.WallWorld(7, prm, 1000, cyl_per_m=1.5, x_first=3.0, length=60.0)
    rng = np.random.default_rng(8)
    pts = np.stack([rng.uniform(0.0, 60.0, 3000), rng.uniform(-8.0, 8.0, 3000), rng.uniform(1.0, 2.4, 3000)], axis=1)
    full = world.box[world.box[:, 6] == 0.0]                                     # the piers: [0, 4]
    assert len(full) >= 8 and (full[:, 7] == 4.0).all()
    d3 = flight.box_distance_ordered(pts, full).min(axis=1)
    assert np.array_equal(d3, flight.box_clearance(pts, full)) and (d3 < 0).any() and (d3 > 0).any()
    cyl = np.stack([world.cx, world.cy, world.cr], axis=1)
    dc = flight.cylinder_distance_ordered(pts, cyl, 500.0).min(axis=1)
    assert np.array_equal(dc, world.clearance(pts)) and (dc < 0).any() and (dc > 0).any()
    dist, kind, index = flight.world_clearance_ordered(cyl, full, pts, 500.0)    # and the scan takes the least of the three
    assert np.array_equal(dist, np.minimum(np.minimum(pts[:, 2], dc), d3))
    assert np.array_equal(kind, np.where(pts[:, 2] <= np.minimum(dc, d3), 0, np.where(dc <= d3, 1, 2)))


# ---- (c) points along a leg ----------------------------------------------------------------------------------------------------------
def _inflated(cyl, box, radius):
    cyl, box = cyl.copy(), box.copy()
    cyl[:, 2] += radius
    box[:, 2] = np.abs(box[:, 2]) + radius; box[:, 3] = np.abs(box[:, 3]) + radius; box[:, 6] -= radius; box[:, 7] += radius
    return cyl, box


@pytest.mark.parametrize("seed,radius", [(51, 0.0), (52, 0.25), (53, 0.6)])
def test_points_ahead_of_the_contact_are_outside_and_the_contact_is_on_a_boundary(seed, radius):
    """600 random legs through a world of cylinders and boxes.  The independent inside test is the clamp formulation on the INFLATED
    solids (the centre against z <= radius, r + radius cut at z_top + radius, half extents + radius): its signed distance is > 0 outside.
    Ahead of the contact (t s for s in 0 .. 0.999, and the whole leg when there is none) every point lies outside every inflated
    solid, up to the bound; at the contact (t > 0) the winning solid's signed distance is 0 within the bound; a contact at t = 0 starts inside.
    The bound, for a point a + t d: the point itself carries 2 u (|a|_1 + t |d|_1); the clamp formulation's own distance 16 u L
    (as above); and t's error moves the point along d.  On a face or the ground t = N / dl with N off by at most 8 u L: the point is off
    by that along the normal.  On a mantle t is a root of a t^2 + 2 b t + c; the computed disc is off by at most 4 u (b b + |a c| + |disc|),
    the root by 2 u s more, -b - s by 2 u (|b| + s), so rho^2 - R^2 = -2 s dt at the root is off by at most
    E = (4 u (b b + |a c| + |disc|) / (2 s) + 2 u s + 2 u (|b| + s)) 2 s / a . a = 4 u (b b + |a c| + |disc|) + 4 u s (|b| + 2 s) -- the 1 / s cancels --
    and rho by E / (2 R) (E / rho_min more generally).  The asserted bound is 64 u (L + |d|_1) + E / R, each first-order step doubled."""
    z_top = 4.0
    cyl, box = _solids(seed)
    rng = np.random.default_rng(seed + 100)
    a = np.stack([rng.uniform(-1.0, 22.0, 600), rng.uniform(-7.0, 7.0, 600), rng.uniform(0.7, 4.5, 600)], axis=1)
    d = rng.normal(0.0, 4.0, (600, 3)); d[:, 2] *= 0.3
    d[:40, 2] = 0.0; d[40:60, 0:2] = 0.0                                         # level legs and vertical ones among them
    icyl, ibox = _inflated(cyl, box, radius)
    hit, t, kind, index = _cast_rays(cyl, box, a, a + d, radius, z_top)
    dd = (a + d) - a                                                              # the legs' d as the cast formed it
    assert 100 < hit.sum() < 590 and (t[hit != 0] == 0).any() and {0, 1, 2} <= set(kind[hit != 0].tolist())
    Lmax = np.abs(a).sum(axis=1) + np.abs(dd).sum(axis=1) + 40.0
    for s in (0.0, 0.25, 0.5, 0.75, 0.999):
        ahead = a + (np.where(hit != 0, t, 1.0) * s)[:, None] * dd
        sd = _clearance_by_clamping(ahead, icyl, ibox, z_top + radius); sd[:, 0] -= radius
        free = (hit == 0) | (t > 0)
        assert (sd[free].min(axis=1) > -64 * U * Lmax[free]).all(), (s, sd[free].min())
    on = (hit != 0) & (t > 0)
    pts = a + t[:, None] * dd
    sd = _clearance_by_clamping(pts, icyl, ibox, z_top + radius); sd[:, 0] -= radius
    win = np.where(kind == 0, 0, np.where(kind == 1, 1 + index, 1 + len(cyl) + index))
    at = np.abs(sd[np.arange(600), np.where(hit != 0, win, 0)])
    tol = 64 * U * Lmax
    m = on & (kind == 1)
    ox, oy, R = a[m, 0] - icyl[index[m], 0], a[m, 1] - icyl[index[m], 1], icyl[index[m], 2]
    qa, qb, qc = dd[m, 0] ** 2 + dd[m, 1] ** 2, ox * dd[m, 0] + oy * dd[m, 1], ox * ox + oy * oy - R * R
    disc = np.maximum(qb * qb - qa * qc, 0.0); sq = np.sqrt(disc)
    tol[m] += 2 * (4 * U * (qb * qb + np.abs(qa * qc) + disc) + 4 * U * sq * (np.abs(qb) + 2 * sq)) / R
    print("contacts", on.sum(), "of them on a mantle", m.sum(), "largest |signed distance| / tol", (at[on] / tol[on]).max())
    assert (at[on] <= tol[on]).all(), np.argwhere(on & (at > tol))[:10]
    inside0 = (hit != 0) & (t == 0)                                               # a contact at t = 0: the leg starts inside (or on) that solid
    sd0 = _clearance_by_clamping(a, icyl, ibox, z_top + radius); sd0[:, 0] -= radius
    assert (sd0[np.arange(600), np.where(hit != 0, win, 0)][inside0] <= 64 * U * Lmax[inside0]).all()


# ---- (d) the path restatement, and the NaN rules -------------------------------------------------------------------------------------
def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("seed", [61, 62, 63, 64])
def test_the_path_restatement_is_the_reduction_of_the_segment_restatement(seed):
    """world_path_cast_ordered walks the legs one at a time and stops; path_cast_reduction reduces world_segment_cast_ordered's answers for
    the whole path at once.  Bit for bit the same, on free paths, stopped paths and paths with a non-finite point in front of, at and
    behind the stop leg."""
    cyl, box = _solids(seed)
    rng = np.random.default_rng(seed)
    seen = set()
    for trial in range(40):
        n = int(rng.integers(2, 12))
        path = np.cumsum(np.concatenate([[[rng.uniform(-4.0, 1.0), rng.uniform(-6.0, 6.0), rng.uniform(0.8, 3.0)]],
                                         rng.normal([0.9, 0.0, 0.0], [0.3, 0.4, 0.1], (n - 1, 3))]), axis=0)
        path = np.concatenate([path, rng.normal(size=(n, 4))], axis=1)            # stride 7: the rest of a row is not read
        if trial % 4 == 1:
            path[rng.integers(0, n), rng.integers(0, 3)] = [NAN, np.inf, -np.inf][trial % 3]
        if trial % 7 == 3:
            path[1] = path[0]                                                      # a degenerate first leg
        radius = [0.0, 0.25, 0.6][trial % 3]
        got = flight.world_path_cast_ordered(cyl, box, path, radius)
        want = flight.path_cast_reduction(path, *flight.world_segment_cast_ordered(cyl, box, path, radius))
        assert sorted(got) == sorted(want)
        for key in got:
            assert _same(got[key], want[key]), (trial, key, got, want)
        seen.add(got["stop"])
        if got["stop"] == 0:
            assert got["leg"] == -1 and got["t"] == 1.0 and got["kind"] == -1 and not got["pts"].any()
        if got["stop"] == 2:
            assert got["t"] == 0.0 and got["kind"] == -1 and np.isfinite(got["free"])
    assert seen == {0, 1, 2}


def test_a_solid_with_a_nan_entry_answers_nothing_and_non_finite_points_follow_the_formulas():
    cyl, box = _solids(71, 4, 4)
    pts = np.array([[cyl[1, 0], cyl[1, 1], 1.0], [box[2, 0], box[2, 1], 0.5 * (box[2, 6] + box[2, 7])], [9.0, 1.0, 2.0]])
    path = np.array([[cyl[1, 0] - 3.0, cyl[1, 1], 1.0], [cyl[1, 0] + 3.0, cyl[1, 1], 1.0], [box[2, 0], box[2, 1], 0.5 * (box[2, 6] + box[2, 7])]])
    base = flight.world_clearance_ordered(cyl, box, pts)
    assert base[1].tolist()[:2] == [1, 2] and base[2].tolist()[:2] == [1, 2]      # inside cylinder 1, inside box 2
    for e in range(3):                                                             # every entry of a cylinder
        c = cyl.copy(); c[1, e] = NAN
        got = flight.world_clearance_ordered(c, box, pts)
        want = flight.world_clearance_ordered(np.delete(cyl, 1, axis=0), box, pts)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and not ((got[1] == 1) & (got[2] == 1)).any()
        hit, t, kind, index = flight.world_segment_cast_ordered(c, box, path, 0.25)
        assert not ((kind == 1) & (index == 1)).any()
        w = flight.world_segment_cast_ordered(np.delete(cyl, 1, axis=0), box, path, 0.25)
        assert np.array_equal(hit, w[0]) and np.array_equal(t, w[1]) and np.array_equal(kind, w[2])
    for e in range(8):                                                             # every entry of a box
        b = box.copy(); b[2, e] = NAN
        got = flight.world_clearance_ordered(cyl, b, pts)
        want = flight.world_clearance_ordered(cyl, np.delete(box, 2, axis=0), pts)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and not ((got[1] == 2) & (got[2] == 2)).any()
        hit, t, kind, index = flight.world_segment_cast_ordered(cyl, b, path, 0.25)
        assert not ((kind == 2) & (index == 2)).any()
        w = flight.world_segment_cast_ordered(cyl, np.delete(box, 2, axis=0), path, 0.25)
        assert np.array_equal(hit, w[0]) and np.array_equal(t, w[1]) and np.array_equal(kind, w[2])
    d, kd, ix = flight.world_clearance_ordered(cyl, box, [[1.0, 2.0, NAN], [NAN, 0.0, 1.0], [1.0, 1.0, np.inf], [1.0, 1.0, -np.inf]])
    assert np.isnan(d[0]) and (kd[0], ix[0]) == (0, -1)                           # a NaN height: the ground's NaN stays
    assert np.isfinite(d[1])                                                      # a NaN x is dropped by the selects: what the formulas give
    assert d[2] == np.inf and kd[2] == 0 and d[3] == -np.inf and kd[3] == 0      # (+inf is not < +inf: the ground keeps it)
    hit, t, kind, index = flight.world_segment_cast_ordered(cyl, box, [[0.0, 0.0, 1.0], [NAN, 0.0, 1.0], [5.0, 0.0, -1.0], [np.inf, 0.0, 1.0]], 0.25)
    assert hit.tolist() == [0, 0, 0] and t.tolist() == [1.0, 1.0, 1.0] and kind.tolist() == [-1, -1, -1] and index.tolist() == [-1, -1, -1]
