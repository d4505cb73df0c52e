"""GPU: amk_sim_render_depth against flight.render_depth_ordered -- the fp64 ray parameter of every pixel bit for bit (through the
tests' amk__sim_render_t), both pixel types against flight.quantise_depth -- over image sizes, cylinder counts around the LDS chunk,
poses and the contract's edges; the round trip through amk_depth_to_clouds; and amk_sim_vehicle_step against
flight.vehicle_step_ordered.  S = 3 scenes per case."""
import ctypes as C

import numpy as np
import pytest

from avoid_mpc_amd import flight

pytestmark = pytest.mark.gpu

Z_TOP, MAX_RANGE = 4.0, 60.0
MAX_CYL = 110


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _cam(rows, cols, pixel2meter=1.0, resize_scale=1.0, integer_centre=False):
    """A camera of the yaml's shape at any size: 90 degrees wide; the principal point off the pixel grid unless asked otherwise"""
    cx, cy = (float(cols // 2), float(rows // 2)) if integer_centre else (cols / 2.0 - 0.3, rows / 2.0 + 0.2)
    return dict(rows=rows, cols=cols, pixel2meter=pixel2meter, depth_min=0.1, depth_max=MAX_RANGE, resize_scale=resize_scale, fx=cols / 2.0,
                fy=cols / 2.0, cx=cx, cy=cy, Tbc=flight.TBC_YAML)


def _params(c):
    from avoid_mpc_amd.host import depth_params
    return depth_params(c["pixel2meter"], c["depth_min"], c["depth_max"], c["resize_scale"], c["fx"], c["fy"], c["cx"], c["cy"], c["Tbc"])


def _pose(p, yaw=0.0, pitch=0.0):
    """Twb = [Rz(yaw) Ry(pitch) | p]; pitch > 0 looks down"""
    cy_, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    T = np.eye(4)
    T[:3, :3] = np.array([[cy_, -sy, 0.0], [sy, cy_, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]])
    T[:3, 3] = p
    return T


LOOK_DOWN = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])   # Ry(90 degrees), exact: the optical axis is world -z


def _world(seed, S=3, n=MAX_CYL):
    """S corridors of n cylinders ahead of the origin (flight.FlightWorld's ranges, denser)"""
    rng = np.random.default_rng(seed)
    return np.stack([np.stack([np.sort(rng.uniform(1.0, 40.0, n)), rng.uniform(-8.0, 8.0, n), rng.uniform(0.1, 0.5, n)], axis=1) for _ in range(S)])


def _reference(cyl, counts, Twb, c, z_top=Z_TOP, max_range=MAX_RANGE):
    out = []
    for s in range(len(Twb)):
        n = cyl.shape[1] if counts is None else int(counts[s])
        out.append(flight.render_depth_ordered((cyl[s, :n, 0], cyl[s, :n, 1], cyl[s, :n, 2]), Twb[s], c["Tbc"], c["rows"], c["cols"], c["fx"],
                                               c["fy"], c["cx"], c["cy"], z_top, max_range))
    return np.stack(out)


def _render(torch, cyl, counts, Twb, c, dtype, z_top=Z_TOP, max_range=MAX_RANGE):
    from avoid_mpc_amd.host import sim_render_depth
    out = sim_render_depth(torch.from_numpy(np.ascontiguousarray(cyl)).cuda(), torch.from_numpy(np.ascontiguousarray(Twb)).cuda(), _params(c),
                           c["rows"], c["cols"], counts=None if counts is None else torch.from_numpy(np.asarray(counts, np.int32)).cuda(),
                           z_top=z_top, max_range=max_range, dtype=dtype)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _assert_t_bits(got, ref, what):
    same = got.view(np.uint64) == ref.view(np.uint64)
    if not same.all():
        for s, r, q in np.argwhere(~same)[:10]:
            print(f"{what} scene {s} pixel ({r}, {q}): device t = {got[s, r, q]!r}, ordered numpy t = {ref[s, r, q]!r}")
    assert same.all(), (what, int((~same).sum()), same.size)


def _check_all_types(torch, cyl, counts, Twb, c, what, **kw):
    """fp64 t bit for bit, then both pixel types against the quantisation rule on that t; -> the reference t"""
    ref = _reference(cyl, counts, Twb, c, **kw)
    _assert_t_bits(_render(torch, cyl, counts, Twb, c, torch.float64, **kw), ref, what)
    f32 = _render(torch, cyl, counts, Twb, c, torch.float32, **kw)
    assert np.array_equal(f32.view(np.uint32), flight.quantise_depth(ref, c["pixel2meter"], np.float32).view(np.uint32)), what
    u16 = _render(torch, cyl, counts, Twb, c, torch.int16, **kw).view(np.uint16)
    assert np.array_equal(u16, flight.quantise_depth(ref, c["pixel2meter"], np.uint16)), what
    return ref


def _chunk():
    from avoid_mpc_amd import capi
    return capi.load().amk__sim_chunk()


# poses: identity, yawed, pitched down onto the ground, above z_top, inside a cylinder (placed in the test: it needs the world)
POSES = dict(identity=_pose([0.0, 0.0, 1.5]), yawed=_pose([2.0, -1.0, 1.2], yaw=0.4), down=_pose([1.0, 0.5, 2.0], pitch=0.6),
             above=_pose([3.0, 0.0, 6.5], yaw=-0.2, pitch=0.5), yaw_pitch=_pose([0.5, 2.0, 0.8], yaw=-0.7, pitch=-0.15))


def _inside(cyl_scene, k=3):
    """a camera inside cylinder k of a scene, off its axis"""
    cx, cy, r = cyl_scene[k]
    return _pose([cx - 0.05 - 0.3 * r, cy + 0.2 * r, 1.0], yaw=0.3)


@pytest.mark.parametrize("rows,cols,pixel2meter", [(5, 7, 1.0), (24, 32, 1e-3), (48, 64, 1e-3)])
def test_render_matches_the_ordered_restatement(torch_cuda, rows, cols, pixel2meter):
    """Ragged counts 0 / 1 / 7, one chunk / chunk + 1 / max_cyl, and max_cyl everywhere (no counts); every pose"""
    torch = torch_cuda
    ch = _chunk()
    assert 7 < ch and ch + 1 < MAX_CYL
    c = _cam(rows, cols, pixel2meter)
    cyl = _world(rows)
    cases = [((0, 1, 7), ("identity", "yawed", "down")), ((ch, ch + 1, MAX_CYL), ("above", "inside", "yaw_pitch")),
             ((7, MAX_CYL, ch), ("inside", "identity", "down")), (None, ("yawed", "above", "identity"))]
    for counts, poses in cases:
        Twb = np.stack([_inside(cyl[s]) if p == "inside" else POSES[p] for s, p in enumerate(poses)])
        ref = _check_all_types(torch, cyl, counts, Twb, c, (rows, cols, counts, poses))
        if counts is not None and counts[0] == 0 and rows > 5:
            assert (ref[0] > 0).any() and (ref[0] == 0).any()        # the empty scene: ground below the horizon, nothing above it
        if rows > 5:
            assert all((ref[s] > 0).any() for s in range(3)), (counts, poses)
    assert len({k for _, ps in cases for k in ps}) == 6


def test_render_one_full_size_scene(torch_cuda):
    """480 x 640, one scene, a count behind the first chunk: 1200 blocks, a grid of more than one block row of the image"""
    torch = torch_cuda
    c = _cam(480, 640, 1e-3)
    cyl = _world(480, S=1, n=_chunk() + 6)
    ref = _check_all_types(torch, cyl, None, POSES["yaw_pitch"][None], c, "480 x 640")
    assert 0.3 < (ref > 0).mean() < 1.0


def test_a_vertical_ray_and_a_camera_over_a_cylinder(torch_cuda):
    """The camera looks straight down with the principal point on a pixel: that pixel's ray has a == 0 exactly, and every cylinder
    term is NaN or -inf there -- no hit; the ground answers with the camera's height.  One scene hovers above a cylinder's top."""
    torch = torch_cuda
    c = _cam(5, 7, integer_centre=True)
    cyl = _world(5, n=7)
    Twb = np.tile(np.eye(4), (3, 1, 1))
    Twb[:, :3, :3] = LOOK_DOWN
    Twb[0, :3, 3] = [cyl[0, 4, 0] - cyl[0, 4, 2] - 0.3, cyl[0, 4, 1], 3.0]   # beside cylinder 4 of scene 0: slanted rays meet its wall
    Twb[1, :3, 3] = [cyl[1, 2, 0] - 0.01, cyl[1, 2, 1], 5.0]     # over cylinder 2 of scene 1, above z_top
    Twb[2, :3, 3] = [cyl[2, 0, 0] - 0.01, cyl[2, 0, 1], 2.0]     # INSIDE cylinder 0 of scene 2, looking down its axis direction
    ref = _check_all_types(torch, cyl, None, Twb, c, "vertical")
    for s in range(3):
        o_z = Twb[s, 2, 3] + ((LOOK_DOWN[2, 0] * 0.05 + LOOK_DOWN[2, 1] * 0.0) + LOOK_DOWN[2, 2] * 0.01)
        assert ref[s, 2, 3] == pytest.approx(o_z, abs=1e-12)        # the centre pixel: the ground, whatever stands around the ray
    assert ((ref[0] > 0) & (ref[0] < ref[0, 2, 3] - 0.5)).any()     # (the same image has wall hits: the cylinder terms did run)


def test_two_cylinders_at_exactly_equal_t(torch_cuda):
    """Two cylinders mirrored about the optical axis at dyadic coordinates: on the image's centre column both give the same t, bit for
    bit (each alone renders it), and the image is the same whichever comes first -- the strict < keeps the earlier one."""
    torch = torch_cuda
    c = _cam(5, 7, integer_centre=True)
    pair = np.array([[4.0, 1.0, 1.5], [4.0, -1.0, 1.5]])
    cyl = np.stack([pair, pair[::-1], pair])
    counts = (2, 2, 1)
    Twb = np.stack([_pose([0.0, 0.0, 1.0])] * 3)
    ref = _check_all_types(torch, cyl, counts, Twb, c, "equal t")
    alone = _reference(np.stack([pair[1:], pair[1:], pair[1:]]), (1, 1, 1), Twb, c)
    col = 3
    assert np.array_equal(ref[2, :, col], alone[2, :, col]) and (ref[2, :, col] > 0).all() and (ref[2, :, col] < 4.0).all()   # equal t: a tie
    assert np.array_equal(ref[0], ref[1])


def test_a_hit_at_exactly_max_range_and_one_float_beyond(torch_cuda):
    """Looking straight down, every ray has d_z = -1 exactly, so every pixel's t is the camera's height o_z: max_range = o_z keeps the
    whole image, the next double below it empties it."""
    torch = torch_cuda
    c = _cam(5, 7)
    Twb = np.tile(np.eye(4), (3, 1, 1)); Twb[:, :3, :3] = LOOK_DOWN; Twb[:, :3, 3] = [[0.0, 0.0, 3.0], [1.0, 2.0, 7.3], [5.0, -1.0, 0.7]]
    cyl = np.zeros((3, 0, 3))
    free = _reference(cyl, None, Twb, c, max_range=1e9)
    for s in range(3):
        o_z = free[s, 0, 0]
        assert (free[s] == o_z).all() and o_z > 0
        one = (np.zeros((1, 0, 3)), None, Twb[s:s + 1], c)
        kept = _check_all_types(torch, *one, "at max_range", max_range=float(o_z))
        gone = _check_all_types(torch, *one, "beyond max_range", max_range=float(np.nextafter(o_z, 0.0)))
        assert (kept == o_z).all() and (gone == 0).all()


def test_round_trip_through_depth_to_clouds(torch_cuda):
    """render (U16, millimetres) -> amk_depth_to_clouds at resize_scale 1 -> every obstacle point lies on a cylinder or on the ground.
    Bound, derived: the point is o + R (dc d) for the quantised depth d where the hit is o + R (dc t); R is orthonormal, so the two
    are |dc| |d - t| apart with |dc| <= |dc|_max over the image.  |d - t| <= half a depth quantum (pixel2meter / 2) plus four
    float32 roundings at most max_range (t -> float32, its quotient, the product back, 1 / (1 / d) in float32: 2^-24 relative
    each).  The cloud's coordinates are float32: each of the three is off by at most 2^-24 of the largest coordinate, at most
    |o|_inf + max_range |dc|_max.  A point that far from the hit is at most that far from the hit's surface."""
    torch = torch_cuda
    from avoid_mpc_amd.host import depth_to_clouds, sim_render_depth
    c = _cam(48, 64, 1e-3)
    cyl = _world(77, n=40)
    counts = np.array([40, 7, 23], np.int32)
    Twb = np.stack([POSES["identity"], POSES["yawed"], POSES["down"]])
    p = _params(c)
    cyl_d, Twb_d = torch.from_numpy(cyl).cuda(), torch.from_numpy(Twb).cuda()
    depth = sim_render_depth(cyl_d, Twb_d, p, 48, 64, counts=torch.from_numpy(counts).cuda(), z_top=Z_TOP, max_range=MAX_RANGE, dtype=torch.int16)
    Twc = torch.from_numpy(np.stack([T @ flight.TBC_YAML for T in Twb])).cuda()
    cloud, n, _, _ = depth_to_clouds(depth, p, Twb_d, Twc)
    torch.cuda.synchronize()
    cloud, n = cloud.cpu().numpy().astype(np.float64), n.cpu().numpy()
    u, v = np.meshgrid(np.arange(64.0), np.arange(48.0))
    dc_max = np.sqrt(((u - c["cx"]) / c["fx"]) ** 2 + ((v - c["cy"]) / c["fy"]) ** 2 + 1.0).max()
    eps = 2.0 ** -24
    bound = dc_max * (c["pixel2meter"] / 2 + 4 * eps * MAX_RANGE) + np.sqrt(3.0) * eps * (np.abs(Twb[:, :3, 3]).max() + 0.06 + MAX_RANGE * dc_max)
    print("round trip bound [m]:", bound)
    assert bound < 1e-3
    for s in range(3):
        assert n[s] > 1000, (s, n[s])
        P = cloud[s, :n[s]]
        k = counts[s]
        wall = np.abs(np.sqrt((P[:, 0:1] - cyl[s, :k, 0]) ** 2 + (P[:, 1:2] - cyl[s, :k, 1]) ** 2) - cyl[s, :k, 2])   # [points, cylinders]
        wall = np.where((P[:, 2:3] >= -bound) & (P[:, 2:3] <= Z_TOP + bound), wall, np.inf).min(axis=1)
        off = np.minimum(wall, np.abs(P[:, 2]))
        print("scene", s, "points", n[s], "largest distance to a surface [m]:", off.max(), "on cylinders:", int((wall <= bound).sum()))
        assert off.max() <= bound, (s, off.max(), bound)
        assert (wall <= bound).sum() > 50 and (np.abs(P[:, 2]) <= bound).sum() > 50     # both kinds of surface were seen


# ---- the vehicle -----------------------------------------------------------------------------------------------------------------
YAWS = np.array([0.0, np.pi / 2, -np.pi / 2, np.pi, 0.1, -2.5, 1e-3, 3 * np.pi / 4, 1.0])


def _vehicle(torch, ABc, x, cmd, q, want_twb=True):
    from avoid_mpc_amd.host import sim_vehicle_step
    xd, cd = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(cmd).cuda()
    Td = torch.full((len(x), 4, 4), 9.0, dtype=torch.float64, device="cuda") if want_twb else None
    sim_vehicle_step(ABc, cd, xd, Td, pose_quantum=q)
    torch.cuda.synchronize()
    return xd.cpu().numpy(), Td.cpu().numpy() if want_twb else None


def _states(seed, yaws):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-20.0, 20.0, (len(yaws), 10)); x[:, 3] = yaws
    return x, rng.uniform(-3.0, 12.0, (len(yaws), 3))


@pytest.mark.parametrize("model", ["mpc", "dense"])
@pytest.mark.parametrize("q", [0.0, 1e6])
def test_vehicle_state_and_position_bit_for_bit(torch_cuda, model, q):
    """x+ and the pose's translation against the numpy sum order, for the MPC's own model (sparse: its yaw row is the identity) and
    for a dense random (A, B, c) in which every term of every sum counts; pose_quantum 0 and 1e6; yaw = 0: the identity exactly."""
    torch = torch_cuda
    from avoid_mpc_amd import synth
    from avoid_mpc_amd.host import plant_model
    ABc = plant_model(synth.DEFAULT_TAU, 0.033) if model == "mpc" else np.random.default_rng(8).uniform(-1.5, 1.5, 150)
    x, cmd = _states(3, np.zeros(3) if model == "mpc" else YAWS[:3])
    xn, T = _vehicle(torch, ABc, x, cmd, q)
    rx, rT = flight.vehicle_step_ordered(ABc, x, cmd, q)
    assert np.array_equal(xn.view(np.uint64), rx.view(np.uint64)), np.abs(xn - rx).max()
    assert np.array_equal(T[:, :3, 3].view(np.uint64), rT[:, :3, 3].view(np.uint64))
    assert np.array_equal(T[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (3, 1))) and np.array_equal(T[:, 2, :3], np.tile([0.0, 0.0, 1.0], (3, 1)))
    if model == "mpc":
        assert (xn[:, 3] == 0).all()
        assert np.array_equal(T.view(np.uint64), rT.view(np.uint64))                          # the whole pose, signs of the zeros included
        assert np.array_equal(T[:, :3, :3], np.tile(np.eye(3), (3, 1, 1))) and not np.signbit(T[:, :3, :3]).any()
        if q:
            assert np.array_equal(T[:, :3, 3], np.round(xn[:, 0:3], 6))
        x2, none = _vehicle(torch, ABc, x, cmd, q, want_twb=False)                            # d_Twb is optional
        assert none is None and np.array_equal(x2, xn)


def test_vehicle_rotation_against_numpy_cos_sin(torch_cuda):
    """yaw != 0: the pose's rotation entries are the device's cos / sin; against numpy's over a ladder of yaws with +-pi/2 and pi in
    it.  Both libraries document errors of an ulp or two (the device's fp64 sin / cos: 2 ulp; the host's: under 1), so two results
    are at most 3 ulp apart and the assertion is 4.  Measured: CHANGELOG.md."""
    torch = torch_cuda
    from avoid_mpc_amd import synth
    from avoid_mpc_amd.host import plant_model
    ABc = plant_model(synth.DEFAULT_TAU, 0.033)
    x, cmd = _states(4, YAWS)
    xn, T = _vehicle(torch, ABc, x, cmd, 0.0)
    assert np.array_equal(xn[:, 3], YAWS)                                # the model's yaw row is the identity and yaw_dot = 0
    cs, sn = np.cos(YAWS), np.sin(YAWS); cs[0], sn[0] = 1.0, 0.0
    worst = 0.0
    for name, got, want in (("cos", T[:, 0, 0], cs), ("-sin", T[:, 0, 1], 0.0 - sn), ("sin", T[:, 1, 0], sn), ("cos", T[:, 1, 1], cs)):
        ulp = np.abs(got - want) / np.spacing(np.abs(want))
        print(name, "disagreement in ulp per yaw:", ulp)
        worst = max(worst, ulp.max())
    print("largest disagreement with numpy's cos / sin [ulp]:", worst)
    assert worst <= 4.0
    assert np.array_equal(T[:, 0, 0], T[:, 1, 1]) and np.array_equal(T[:, 0, 1], 0.0 - T[:, 1, 0])
