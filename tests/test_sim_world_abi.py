"""CPU: amk_sim_render_world and amk_sim_vehicle_step_att (and their _host variants) without a device -- the symbols are declared,
listed, bound and exported; every argument rule is refused before the device is asked for; the header states the contract; the new
kernels use no scratch and live in sim.hip's object; and the numpy restatements (flight.render_world_ordered,
flight.vehicle_attitude_ordered) are held to render_depth_ordered (zero boxes, bit for bit), to an independent six-face-plane
formulation of the boxes, and to numpy's straightforward acc2rotmat."""
import ctypes as C
import glob
import json
import os
import re

import numpy as np
import pytest

from avoid_mpc_amd import build as amk_build
from avoid_mpc_amd import capi, flight
from avoid_mpc_amd.host import depth_params
from tests import _flight
from tests import test_sim_abi as parent_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOUR = ["amk_sim_render_world", "amk_sim_render_world_host", "amk_sim_vehicle_step_att", "amk_sim_vehicle_step_att_host"]
BAD, UNSUPPORTED, NO_DEVICE = capi.AMK_ERR_INVALID_ARG, capi.AMK_ERR_UNSUPPORTED, capi.AMK_ERR_NO_DEVICE
U = 2.0 ** -53   # the unit roundoff of a double


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
    for name in FOUR:
        assert re.search(r"^int " + name + r"\(", section, re.M), name       # declared, in the simulation's section
        assert name in capi.SYMBOLS                                          # listed
        fn = getattr(lib, name)                                              # exported
        assert fn.argtypes is not None and fn.restype is C.c_int, name       # bound
    assert len(lib.amk_sim_render_world.argtypes) == 16 and len(lib.amk_sim_render_world_host.argtypes) == 15
    assert len(lib.amk_sim_vehicle_step_att.argtypes) == 9 and len(lib.amk_sim_vehicle_step_att_host.argtypes) == 8
    for name in ("amk__sim_render_world_t", "amk__sim_world_chunk"):         # the tests' own: exported and bound, not in the header
        assert getattr(lib, name).restype is C.c_int and name not in hdr and name not in capi.SYMBOLS
    assert lib.amk__sim_world_chunk() >= 2
    assert re.search(r"^#define AMK_SIM_ATT_YAW\s+0\b", section, re.M) and re.search(r"^#define AMK_SIM_ATT_ACCEL\s+1\b", section, re.M)
    assert (capi.AMK_SIM_ATT_YAW, capi.AMK_SIM_ATT_ACCEL) == (0, 1) == (flight.ATT_YAW, flight.ATT_ACCEL)


def test_render_world_refuses_bad_arguments_without_a_device(lib):
    p = depth_params(pixel2meter=1e-3)
    cyl = np.ones((2, 3, 3)); cnt = np.full(2, 3, np.int32); box = np.ones((2, 2, 8)); bcnt = np.full(2, 2, np.int32)
    T = np.tile(np.eye(4), (2, 1, 1)); img = np.full((2, 4, 5), 7, np.uint16)
    U16, F32 = capi.AMK_DEPTH_U16, capi.AMK_DEPTH_F32
    for fn, tail in ((lib.amk_sim_render_world, (None,)), (lib.amk_sim_render_world_host, ())):
        call = lambda cyl_=_vp(cyl), cnt_=_vp(cnt), mc=3, box_=_vp(box), bcnt_=_vp(bcnt), mb=2, S=2, zt=4.0, mr=60.0, pp=C.byref(p), rows=4, \
            cols=5, T_=_vp(T), out=_vp(img), kind=U16: fn(cyl_, cnt_, mc, box_, bcnt_, mb, S, zt, mr, pp, rows, cols, T_, out, kind, *tail)
        for mb in (2, 0):                                                      # amk_sim_render_depth's rules, with and without boxes
            assert call(cyl_=None, mb=mb) == BAD and call(T_=None, mb=mb) == BAD and call(out=None, mb=mb) == BAD and call(pp=None, mb=mb) == BAD
            assert call(rows=0, mb=mb) == BAD and call(cols=0, mb=mb) == BAD and call(rows=-3, mb=mb) == BAD
            assert call(mc=-1, mb=mb) == BAD and call(S=0, mb=mb) == BAD and call(S=-2, mb=mb) == BAD
            assert call(zt=-1.0, mb=mb) == BAD and call(zt=float("nan"), mb=mb) == BAD
            assert call(mr=-0.5, mb=mb) == BAD and call(mr=float("nan"), mb=mb) == BAD
            assert call(kind=2, mb=mb) == BAD and call(kind=-1, mb=mb) == BAD and call(kind=7, mb=mb) == BAD
            assert call(pp=C.byref(depth_params(pixel2meter=0.0)), mb=mb) == BAD
            assert call(rows=1 << 20, cols=1 << 20, S=2, mb=mb) == UNSUPPORTED
            assert call(rows=46341, cols=46341, S=256, mb=mb) == UNSUPPORTED
            assert call(S=65536, mb=mb) == UNSUPPORTED
        assert call(mb=-1) == BAD and call(box_=None) == BAD and call(box_=None, mb=1) == BAD       # the box list's own rules
        if lib.amk_device_count() <= 0:                                        # a good call reaches the device question and nothing else
            assert call() == NO_DEVICE and call(cnt_=None, bcnt_=None) == NO_DEVICE and call(kind=F32) == NO_DEVICE
            assert call(box_=None, mb=0) == NO_DEVICE and call(box_=None, bcnt_=None, mb=0, cyl_=None, mc=0) == NO_DEVICE
            assert call(cyl_=None, mc=0) == NO_DEVICE
    assert (img == 7).all()


def test_vehicle_att_refuses_bad_arguments_without_a_device(lib):
    ABc = np.zeros(150); cmd = np.zeros((2, 3)); x = np.full((2, 10), 3.0); T = np.full((2, 16), 5.0)
    for fn, tail in ((lib.amk_sim_vehicle_step_att, (None,)), (lib.amk_sim_vehicle_step_att_host, ())):
        call = lambda m=_vp(ABc), c=_vp(cmd), x_=_vp(x), T_=_vp(T), S=2, q=1e6, att=1, gz=9.81: fn(m, c, x_, T_, S, q, att, gz, *tail)
        for att in (0, 1):                                                     # amk_sim_vehicle_step's rules in both modes
            assert call(m=None, att=att) == BAD and call(c=None, att=att) == BAD and call(x_=None, att=att) == BAD
            assert call(S=0, att=att) == BAD and call(S=-1, att=att) == BAD and call(q=-1.0, att=att) == BAD and call(q=float("nan"), att=att) == BAD
            assert call(gz=-1e-300, att=att) == BAD and call(gz=float("nan"), att=att) == BAD
        assert call(att=2) == BAD and call(att=-1) == BAD
        if lib.amk_device_count() <= 0:
            assert call() == NO_DEVICE and call(att=0) == NO_DEVICE and call(T_=None) == NO_DEVICE and call(gz=0.0) == NO_DEVICE
    assert (x == 3.0).all() and (T == 5.0).all()


def test_the_header_states_the_world_contract():
    section = re.sub(r"\s*\*?\s+", " ", _section()[1])                         # comment stars and line breaks out
    section = section[section.index("amk_sim_render_world:"):]
    for sentence in ("A camera inside a box gets no return from that box", "A grazing ray counts",
                     "the ray is parallel to it. near = -inf, far = +inf when lo <= o && o <= hi: the slab imposes no bound",
                     "Otherwise near = +inf, far = -inf: the box is missed",
                     "Order: the ground, then the cylinders in index order, then the boxes in index order",
                     "inv = 1.0 / d, t1 = (lo - o) inv, t2 = (hi - o) inv, near = t1 < t2 ? t1 : t2, far = t1 < t2 ? t2 : t1",
                     "a hit at t = tn when n_x <= f_x && n_y <= f_y && n_z <= f_z && tn > 0 && tn <= tf",
                     "it is not cut at z_top", "does not renormalise them", "A negative half extent", "z1 < z0", "A NaN anywhere",
                     "Every error is returned before anything is launched", "allocates nothing",
                     "Unless n > 0 && m > 0 the rotation falls back to Rz(yaw)", "n = sqrt((T_0 T_0 + T_1 T_1) + T_2 T_2)",
                     "y' = (0.0 - zb_2 sn, zb_2 cs, zb_0 sn - zb_1 cs)", "exactly the identity"):
        assert sentence in section, sentence
    assert section.count("allocates nothing") >= 2                             # both new calls say so


def test_the_new_kernels_use_no_scratch_and_live_in_one_object(lib):
    table = json.load(open(amk_build.RES))
    world = {n: r for n, r in table.items() if "16sim_world_kernel" in n}
    att = {n: r for n, r in table.items() if "19sim_attitude_kernel" in n}
    assert len(world) == 3 and len(att) == 1, (sorted(world), sorted(att))      # U16, F32, the tests' fp64 t; the attitude
    for n, r in {**world, **att}.items():
        print(n, r)
        assert r["scratch_bytes_per_lane"] == 0, (n, r)
    for n, r in world.items():
        assert r["occupancy"] >= 8 and r["lds_bytes"] <= 8192, (n, r)           # fp64 VALU bound, as sim_render_kernel: eight waves per SIMD
    per_object = {os.path.basename(p)[:-len(".o.res.json")]: list(json.load(open(p))) for p in glob.glob(os.path.join(amk_build.OBJ, "*.o.res.json"))}
    assert [u for u, ks in per_object.items() if any("sim_world_kernel" in k or "sim_attitude_kernel" in k for k in ks)] == ["sim"]


@pytest.mark.parametrize("seed", parent_abi.SEEDS)
def test_zero_boxes_is_render_depth_ordered_bit_for_bit(seed):
    """render_world_ordered with an empty box list against render_depth_ordered on test_sim_abi.py's poses and cylinder selection:
    the same fp64 t, bit for bit -- the ground and cylinder lines are the same lines."""
    c = _flight.DEPTH_CAM
    world, xs = parent_abi._poses(seed)
    for x in xs:
        _, Twb = _flight._depth_frame(world, x, c)
        sel = (world.cx > x[0] - 2.0) & (world.cx < x[0] + 40.0)
        args = ((world.cx[sel], world.cy[sel], world.cr[sel]), Twb, c["Tbc"], c["rows"], c["cols"], c["fx"], c["fy"], c["cx"], c["cy"])
        old = flight.render_depth_ordered(*args)
        new = flight.render_world_ordered(args[0], np.zeros((0, 8)), *args[1:])
        assert (old > 0).any() and np.array_equal(old.view(np.uint64), new.view(np.uint64))


# ---- the boxes against six face planes ---------------------------------------------------------------------------------------------
ROWS, COLS = 48, 64
CAM = dict(fx=32.0, fy=32.0, cx=31.7, cy=24.2)
EDGE = 1e-9   # [m]: a ray this close to a box edge (by the independent side's own account) may fall on either side of it


def _six_faces(box, Twb, Tbc):
    """The independent side: Twc and the rays by matrix products, every box as six face planes in its own frame (a 3 x 3 rotation
    applied with @), the ground as a seventh plane.  -> (t [rows, cols] (inf: no hit), |d| along the winning face's normal, the
    winning surface's coordinate scale L, the ray's |d|_1, near_edge [rows, cols])"""
    Twc = np.asarray(Twb) @ np.asarray(Tbc)
    o = Twc[:3, 3]
    v, u = np.meshgrid(np.arange(ROWS, dtype=np.float64), np.arange(COLS, dtype=np.float64), indexing="ij")
    D = np.stack([(u - CAM["cx"]) / CAM["fx"], (v - CAM["cy"]) / CAM["fy"], np.ones_like(u)], -1) @ Twc[:3, :3].T
    best, dn, scale = np.full((ROWS, COLS), np.inf), np.ones((ROWS, COLS)), np.ones((ROWS, COLS))
    near_edge = np.zeros((ROWS, COLS), bool)
    with np.errstate(all="ignore"):
        tg = -o[2] / D[..., 2]
        ok = (D[..., 2] < 0) & (tg > 0)
        best, dn, scale = np.where(ok, tg, best), np.where(ok, np.abs(D[..., 2]), dn), np.where(ok, abs(o[2]), scale)
        for bx, by, hx, hy, c, s, z0, z1 in box:
            R = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
            ol, dl = R @ (o - np.array([bx, by, 0.0])), D @ R.T
            lo, hi = np.array([-hx, -hy, z0]), np.array([hx, hy, z1])
            L = np.abs(o).sum() + abs(bx) + abs(by) + hx + hy + abs(z0) + abs(z1)
            if np.all((ol >= lo) & (ol <= hi)):
                continue                                                        # the camera is inside: no return from this box
            for ax in range(3):
                oth = [i for i in range(3) if i != ax]
                for bound in (lo[ax], hi[ax]):
                    t = (bound - ol[ax]) / dl[..., ax]
                    q = ol[oth] + t[..., None] * dl[..., oth]
                    outside = np.maximum(lo[oth] - q, q - hi[oth]).max(axis=-1)  # > 0: the plane is met outside the face
                    near_edge |= (t > 0) & (np.abs(outside) < EDGE)
                    ok = (t > 0) & (outside <= 0) & (t < best)       # the first face met within its rectangle
                    best, dn, scale = np.where(ok, t, best), np.where(ok, np.abs(dl[..., ax]), dn), np.where(ok, L, scale)
    return best, dn, scale, np.abs(D).sum(axis=-1), near_edge


def _box_world(seed, n=9):
    """n yawed boxes ahead of the origin, some floating; box 0 axis-aligned"""
    rng = np.random.default_rng(seed)
    yaw = rng.uniform(-1.0, 1.0, n)
    box = np.stack([rng.uniform(3.0, 20.0, n), rng.uniform(-6.0, 6.0, n), rng.uniform(0.1, 1.5, n), rng.uniform(0.05, 1.5, n), np.cos(yaw),
                    np.sin(yaw), rng.uniform(0.0, 1.5, n), rng.uniform(2.0, 4.0, n)], axis=1)
    box[0, 4:6] = [1.0, 0.0]
    return box


def _yawed_pose(p, th):
    T = np.eye(4); T[:3, 3] = p
    T[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
    return T


@pytest.mark.parametrize("seed,pose", [(5, _yawed_pose([0.3, -0.2, 1.1], 0.2)), (6, _yawed_pose([1.0, 2.0, 0.4], -0.5)),
                                       (7, _yawed_pose([-2.0, 0.5, 3.1], 0.05))])
def test_the_boxes_against_six_face_planes(seed, pose):
    """render_world_ordered (slabs, one reciprocal each, written-out sums) against six face planes per box with matrix products.
    The hit sets are identical and t agrees to a bound derived per pixel, not fitted: both sides compute t = N / d with N = bound - o
    along the winning face's normal in the box's frame and d the ray's component along it.
      N: the camera position (a 4-term dot product: 7 roundings), minus the centre (1), rotated (2 products and a sum: 3 on the
         ordered side, 5 for a 3-term row on the other), bound - o (1): at most 14 roundings a side, each at most u times the
         coordinates' scale L = |o|_1 + |cx| + |cy| + hx + hy + |z0| + |z1|  ->  |dN| <= 32 u L between the two sides.
      d: dc (2), the camera rotation (5), the box rotation (5): 12 a side at u times D = |d|_1  ->  |dd| <= 32 u D.
      t = N / d: dt <= (dN + t dd) / |d| to first order, plus the final operations themselves -- a reciprocal and a product on one
         side, a division on the other, and the same again to cover the first-order step: 8 u t.
    tol = 32 u (L + t D) / |d| + 8 u t, with |d| the independent side's own value for its winning face.  Pixels whose ray meets a
    face plane within 1e-9 m of that face's edge by the independent side's account are left out; at most 1 % may be."""
    box = _box_world(seed)
    t = flight.render_world_ordered(([], [], []), box, pose, flight.TBC_YAML, ROWS, COLS, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], max_range=1e9)
    ref, dn, L, D, near_edge = _six_faces(box, pose, flight.TBC_YAML)
    assert near_edge.mean() <= 0.01, near_edge.sum()
    keep = ~near_edge
    hit, hit_ref = t > 0, np.isfinite(ref)
    assert np.array_equal(hit[keep], hit_ref[keep]), np.argwhere((hit != hit_ref) & keep)[:10]
    both = keep & hit
    ground_only = flight.render_world_ordered(([], [], []), np.zeros((0, 8)), pose, flight.TBC_YAML, ROWS, COLS, CAM["fx"], CAM["fy"], CAM["cx"],
                                              CAM["cy"], max_range=1e9)
    assert (t != ground_only).sum() > 100                                       # the boxes are in the image
    tol = 32 * U * (L + ref * D) / dn + 8 * U * ref
    err = np.abs(t - ref)
    print("pixels", both.sum(), "left out", near_edge.sum(), "largest |dt| / tol", (err[both] / tol[both]).max(), "largest relative dt", (err[both] / ref[both]).max())
    assert (err[both] <= tol[both]).all(), np.argwhere(both & (err > tol))[:10]


def test_parallel_slabs_and_a_camera_inside_a_box():
    """A level camera at yaw 0 with an integer principal point: the centre column has d_y == 0 and the centre row d_z == 0, exactly.
    An axis-aligned box whose near face is at x = 4.5 then returns 4.5 - 0.05 = 4.45 m down the centre column (Tbc puts the camera
    0.05 m ahead of the body) from the box's top edge (row 17) to where the ground comes nearer (row 32), and along the centre row; and a camera inside a box gets no return from it."""
    args = (flight.TBC_YAML, ROWS, COLS, 32.0, 32.0, 32.0, 24.0)
    T = np.eye(4); T[:3, 3] = [0.0, 0.0, 1.0]
    free = flight.render_world_ordered(([], [], []), np.zeros((0, 8)), T, *args, max_range=1e9)
    t = flight.render_world_ordered(([], [], []), [[5.0, 0.0, 0.5, 0.5, 1.0, 0.0, 0.0, 2.0]], T, *args, max_range=1e9)
    assert np.array_equal(t[17:32, 32], np.full(15, 4.45)) and np.array_equal(t[24, 29:36], np.full(7, 4.45))
    beside = flight.render_world_ordered(([], [], []), [[5.0, 3.0, 0.5, 0.5, 1.0, 0.0, 0.0, 2.0]], T, *args, max_range=1e9)
    assert np.array_equal(beside[:, 32], free[:, 32])                           # parallel and outside the slab: missed
    inside = flight.render_world_ordered(([], [], []), [[0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 2.0]], T, *args, max_range=1e9)
    assert np.array_equal(inside, free)
    nan = flight.render_world_ordered(([], [], []), [[5.0, 0.0, np.nan, 0.5, 1.0, 0.0, 0.0, 2.0], [5.0, 0.0, 0.5, 0.5, 1.0, 0.0, 0.0, 2.0]], T, *args,
                                      max_range=1e9)
    assert np.array_equal(nan, t)                                               # a NaN entry: no hit from that box, the next one is seen


# ---- the attitude ------------------------------------------------------------------------------------------------------------------
def _acc2rotmat(a, yaw, gz=flight.GZ):
    """numpy's straightforward acc2rotmat (mpc_obstacle_casadi.py:253-264): thrust direction, np.cross, np.linalg.norm"""
    zb = np.array([a[0], a[1], a[2] + gz]); zb = zb / np.linalg.norm(zb)
    xc = np.array([np.cos(yaw), np.sin(yaw), 0.0])
    yb = np.cross(zb, xc); yb = yb / np.linalg.norm(yb)
    return np.stack([np.cross(yb, zb), yb, zb], axis=1)


def _plant():
    prm, _ = _flight.make_prm("C1")
    A, B, c = flight.affine_plant(prm.tau, prm.dt)
    return np.concatenate([A.reshape(-1), B.reshape(-1), c])


def test_attitude_is_the_identity_at_hover_and_falls_back():
    ABc = np.zeros(150); ABc[:100] = np.eye(10).reshape(-1)                     # x+ = x: the new acceleration is the given one
    x = np.zeros((4, 10)); x[:, 0:3] = [[1.0, 2.0, 3.0]] * 4
    x[1, 7:10] = [0.0, 0.0, -flight.GZ]                                         # free fall: n == 0
    x[2, 7:10] = [np.nan, 0.0, 0.0]
    x[3, 3], x[3, 7:10] = 0.7, [0.0, 0.0, -flight.GZ]
    xn, T = flight.vehicle_attitude_ordered(ABc, x, np.zeros((4, 3)), 0.0)
    _, Ty = flight.vehicle_step_ordered(ABc, x, np.zeros((4, 3)), 0.0)
    assert np.array_equal(T[0], Ty[0]) and np.array_equal(T[0, :3, :3], np.eye(3)) and not np.signbit(T[0, :3, :3]).any()
    assert np.array_equal(T[1:], Ty[1:], equal_nan=True) and np.array_equal(xn[[0, 1, 3]], x[[0, 1, 3]])   # (0 * NaN: scene 2 is all NaN)
    assert np.array_equal(flight.vehicle_attitude_ordered(ABc, x, np.zeros((4, 3)), 0.0, flight.ATT_YAW)[1], Ty, equal_nan=True)


def test_attitude_is_orthonormal_and_is_acc2rotmat():
    """On 200 random accelerations (|a| <= 6 m/s^2 per axis: the thrust stays within 40 degrees or so of the vertical) and yaws:
    R^T R = I and R = numpy's acc2rotmat (np.cross, np.linalg.norm) to a derived bound.  Every entry of R is a unit vector's
    component, at most 1 in magnitude.  zb carries 3 roundings relative to itself (the norm's sum and root, the division), y' 2 more
    per component, yb 3 more, xb 3 more: at most 11 u relative on entries of magnitude <= 1, on either side, in different orders
    (np.linalg.norm sums by dot) -- so two such matrices differ entry-wise by at most 22 u, and a product of two rows of three such
    entries is off by at most 3 * 2 * 11 u plus its own 5 roundings: 71 u.  The asserted bounds are 32 u and 96 u.  cos / sin are
    numpy's on both sides."""
    rng = np.random.default_rng(12)
    ABc = np.zeros(150); ABc[:100] = np.eye(10).reshape(-1)
    x = np.zeros((200, 10)); x[:, 7:10] = rng.uniform(-6.0, 6.0, (200, 3)); x[:, 3] = rng.uniform(-3.0, 3.0, 200); x[:50, 3] = 0.0
    _, T = flight.vehicle_attitude_ordered(ABc, x, np.zeros((200, 3)), 0.0)
    R = T[:, :3, :3]
    ortho = np.abs(np.einsum("nji,njk->nik", R, R) - np.eye(3)).max()
    ref = np.stack([_acc2rotmat(x[i, 7:10], x[i, 3]) for i in range(200)])
    print("largest |R^T R - I| / u:", ortho / U, " largest |R - acc2rotmat| / u:", np.abs(R - ref).max() / U)
    assert ortho <= 96 * U and np.abs(R - ref).max() <= 32 * U
    assert (np.linalg.det(R) > 0.999).all() and (R[:, 2, 2] > 0.3).all()        # a rotation, thrust upwards
    assert np.abs(R[:, 2, 0]).max() > 0.2                                        # and really tilted
    cmd = rng.uniform(-3.0, 12.0, (200, 3))
    xn, T2 = flight.vehicle_attitude_ordered(_plant(), x, cmd, 1e6)               # the real plant: the state and p' are the yaw mode's
    xs, Ts = flight.vehicle_step_ordered(_plant(), x, cmd, 1e6)
    assert np.array_equal(xn, xs) and np.array_equal(T2[:, :3, 3], Ts[:, :3, 3]) and np.array_equal(T2[:, 3], Ts[:, 3])
    assert not np.array_equal(T2[:, :3, :3], Ts[:, :3, :3])
