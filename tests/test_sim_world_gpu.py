"""GPU: amk_sim_render_world against flight.render_world_ordered -- the fp64 ray parameter of every pixel bit for bit (through the
tests' amk__sim_render_world_t), both pixel types against flight.quantise_depth -- over image sizes, box counts around the LDS chunk
and the contract's named edges; the world entry with zero boxes against amk_sim_render_depth; the round trip through
amk_depth_to_clouds; and amk_sim_vehicle_step_att against amk_sim_vehicle_step and flight.vehicle_attitude_ordered.  The cameras,
poses and cylinder worlds are tests/test_sim_gpu.py's."""
import numpy as np
import pytest

from avoid_mpc_amd import capi, flight
from tests.test_sim_gpu import LOOK_DOWN, MAX_CYL, MAX_RANGE, POSES, YAWS, Z_TOP, _assert_t_bits, _cam, _params, _pose, _states, _world

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _chunk():
    return capi.load().amk__sim_world_chunk()


def _boxes(seed, S=3, n=8):
    """S scenes of n boxes ahead of the origin: yawed, a third of them floating, a few thin like walls; box 0 of a scene axis-aligned"""
    rng = np.random.default_rng([seed, 0xB0])
    yaw = rng.uniform(-1.2, 1.2, (S, n))
    box = np.stack([rng.uniform(2.0, 30.0, (S, n)), rng.uniform(-7.0, 7.0, (S, n)), rng.uniform(0.02, 1.5, (S, n)), rng.uniform(0.05, 2.5, (S, n)),
                    np.cos(yaw), np.sin(yaw), np.where(rng.uniform(size=(S, n)) < 0.33, rng.uniform(0.5, 2.5, (S, n)), 0.0),
                    rng.uniform(2.6, 5.0, (S, n))], axis=2)
    box[:, 0, 4:6] = [1.0, 0.0]
    return box


def _clamped(counts, n, S):
    return [n] * S if counts is None else [min(max(int(k), 0), n) for k in counts]


def _reference(cyl, ccounts, box, bcounts, Twb, c, z_top=Z_TOP, max_range=MAX_RANGE):
    S = len(Twb)
    nc, nb = _clamped(ccounts, cyl.shape[1], S), _clamped(bcounts, box.shape[1], S)
    return np.stack([flight.render_world_ordered((cyl[s, :nc[s], 0], cyl[s, :nc[s], 1], cyl[s, :nc[s], 2]), box[s, :nb[s]], Twb[s], c["Tbc"], c["rows"],
                                                 c["cols"], c["fx"], c["fy"], c["cx"], c["cy"], z_top, max_range) for s in range(S)])


def _render(torch, cyl, ccounts, box, bcounts, Twb, c, dtype, z_top=Z_TOP, max_range=MAX_RANGE):
    from avoid_mpc_amd.host import sim_render_world
    dev = lambda a, t=np.float64: torch.from_numpy(np.ascontiguousarray(a, t)).cuda()
    out = sim_render_world(dev(cyl), dev(box), dev(Twb), _params(c), c["rows"], c["cols"], cyl_counts=None if ccounts is None else dev(ccounts, np.int32),
                           box_counts=None if bcounts is None else dev(bcounts, np.int32), z_top=z_top, max_range=max_range, dtype=dtype)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_all_types(torch, cyl, ccounts, box, bcounts, Twb, c, what, **kw):
    """fp64 t bit for bit, then both pixel types against the quantisation rule on that t; -> the reference t"""
    ref = _reference(cyl, ccounts, box, bcounts, Twb, c, **kw)
    _assert_t_bits(_render(torch, cyl, ccounts, box, bcounts, Twb, c, torch.float64, **kw), ref, what)
    f32 = _render(torch, cyl, ccounts, box, bcounts, Twb, c, torch.float32, **kw)
    assert np.array_equal(f32.view(np.uint32), flight.quantise_depth(ref, c["pixel2meter"], np.float32).view(np.uint32)), what
    u16 = _render(torch, cyl, ccounts, box, bcounts, Twb, c, torch.int16, **kw).view(np.uint16)
    assert np.array_equal(u16, flight.quantise_depth(ref, c["pixel2meter"], np.uint16)), what
    return ref


NO_CYL, NO_BOX = np.zeros((3, 0, 3)), np.zeros((3, 0, 8))


@pytest.mark.parametrize("rows,cols,pixel2meter", [(5, 7, 1.0), (24, 32, 1e-3), (48, 64, 1e-3)])
def test_world_matches_the_ordered_restatement(torch_cuda, rows, cols, pixel2meter):
    """Box counts 0 / 1 / chunk - 1, chunk / chunk + 1 / max_box, ragged, outside [0, max_box] (clamped), max_box everywhere; with
    ragged cylinders, with max_cyl == 0, and max_box == 0 with cylinders; every pose of tests/test_sim_gpu.py."""
    torch = torch_cuda
    ch = _chunk()
    mb = ch + 6
    c = _cam(rows, cols, pixel2meter)
    cyl, box = _world(rows), _boxes(rows, n=mb)
    some = cyl[:, :12]
    cases = [(some, (7, 0, 12), box, (0, 1, ch - 1), ("identity", "yawed", "down")),
             (some, None, box, (ch, ch + 1, mb), ("above", "yaw_pitch", "identity")),
             (cyl, (MAX_CYL, 3, 65), box, (ch + 1, 5, ch), ("yawed", "down", "yaw_pitch")),
             (some, (12, 12, 12), box, (-3, mb + 5, 2), ("identity", "yawed", "above")),
             (some, None, box, None, ("down", "identity", "yawed")),
             (NO_CYL, None, box, (3, mb, 1), ("identity", "yaw_pitch", "down")),
             (cyl, (5, 64, MAX_CYL), NO_BOX, None, ("yawed", "identity", "down"))]
    seen = 0
    for cyl_, cc, box_, bc, poses in cases:
        Twb = np.stack([POSES[p] for p in poses])
        ref = _check_all_types(torch, cyl_, cc, box_, bc, Twb, c, (rows, cols, cc, bc, poses))
        if box_.shape[1]:
            seen += int((ref != _reference(cyl_, cc, NO_BOX, None, Twb, c)).sum())
    assert seen > (0 if rows == 5 else 500)                       # (the boxes are in the images)


def test_world_one_full_size_scene(torch_cuda):
    """480 x 640, one scene: 1200 blocks, a grid of more than one block row of the image"""
    torch = torch_cuda
    c = _cam(480, 640, 1e-3)
    cyl, box = _world(480, S=1, n=6), _boxes(480, S=1, n=5)
    ref = _check_all_types(torch, cyl, None, box, None, POSES["yaw_pitch"][None], c, "480 x 640")
    assert (ref != _reference(cyl, None, NO_BOX[:1], None, POSES["yaw_pitch"][None], c)).mean() > 0.02


def test_zero_boxes_is_amk_sim_render_depth(torch_cuda):
    """The world entry with max_box == 0 (amk_sim_render_depth's own launch) and with boxes allocated but every count 0 (the world
    kernel's own ground and cylinder lines) against amk_sim_render_depth on the same inputs: identical images, both pixel types."""
    torch = torch_cuda
    from avoid_mpc_amd.host import sim_render_depth
    c = _cam(48, 64, 1e-3)
    cyl, counts = _world(21), np.array([MAX_CYL, 64, 9], np.int32)
    Twb = np.stack([POSES["yawed"], POSES["down"], POSES["yaw_pitch"]])
    for dtype in (torch.int16, torch.float32):
        old = sim_render_depth(torch.from_numpy(cyl).cuda(), torch.from_numpy(Twb).cuda(), _params(c), 48, 64, counts=torch.from_numpy(counts).cuda(),
                               z_top=Z_TOP, max_range=MAX_RANGE, dtype=dtype).cpu().numpy()
        assert (old != 0).mean() > 0.3
        assert np.array_equal(_render(torch, cyl, counts, NO_BOX, None, Twb, c, dtype), old)
        assert np.array_equal(_render(torch, cyl, counts, _boxes(21), (0, 0, 0), Twb, c, dtype), old)


# ---- the contract's named cases ----------------------------------------------------------------------------------------------------
DYADIC = dict(rows=6, cols=8, pixel2meter=1.0, depth_min=0.1, depth_max=MAX_RANGE, resize_scale=1.0, fx=4.0, fy=4.0, cx=4.0, cy=3.0,
              Tbc=flight.TBC_YAML)   # every camera-frame ray component a multiple of 1 / 4
AT_ORIGIN = _pose([-0.05, 0.0, 0.99])   # Tbc puts the camera 0.05 m ahead of the body: o = (0, 0, 1.0), level, looking along +x
UNIT = [5.0, 0.0, 0.5, 0.5, 1.0, 0.0, 0.0, 2.0]   # the box [4.5, 5.5] x [-0.5, 0.5] x [0, 2]


def _one_box_scenes(rows):
    return np.array(rows, np.float64).reshape(len(rows), 1, 8)


def test_axis_aligned_yawed_thin_and_floating_boxes(torch_cuda):
    """One box per scene: axis-aligned; yawed by 0.5 rad; a wall 0.8 mm thin; a beam floating at [2.2, 2.6] m seen from below (the
    camera pitched up under it); the same beam from the side (level, above the camera's height); and a camera inside a box, whose
    image is the empty world's."""
    torch = torch_cuda
    c = _cam(24, 32, 1e-3, integer_centre=True)
    beam = [4.0, 0.0, 0.3, 6.0, 1.0, 0.0, 2.2, 2.6]
    box = _one_box_scenes([UNIT, [5.0, 0.5, 0.5, 1.0, np.cos(0.5), np.sin(0.5), 0.0, 2.0], [6.0, 0.0, 4e-4, 3.0, np.cos(0.1), np.sin(0.1), 0.0, 3.0],
                           beam, beam, [0.0, 0.0, 1.0, 1.0, np.cos(0.3), np.sin(0.3), 0.0, 2.0]])
    Twb = np.stack([POSES["identity"], POSES["identity"], POSES["identity"], _pose([3.0, 0.0, 1.0], pitch=-0.9), _pose([0.0, 0.0, 1.5]),
                    _pose([0.1, -0.2, 1.0], yaw=0.4)])
    cyl = np.zeros((6, 0, 3))
    ref = _check_all_types(torch, cyl, None, box, None, Twb, c, "named boxes")
    free = _reference(cyl, None, np.zeros((6, 0, 8)), None, Twb, c)
    changed = (ref != free).reshape(6, -1).sum(axis=1)
    print("pixels each box changes:", changed)
    assert (changed[:5] > 0).all() and changed[2] > 50 and changed[5] == 0
    assert ((ref[3] != free[3]) & (free[3] == 0)).any()             # from below: the beam stands against the sky
    seen = ref[4] != free[4]
    assert seen[:12].any() and not seen[12:].any()                  # from the side: above the horizon only (the beam floats over the camera)
    assert np.abs(ref[2][ref[2] != free[2]] - 6.0).max() < 1.5      # the thin wall is seen where it stands


def test_parallel_rays_a_grazing_ray_and_equal_t(torch_cuda):
    """The dyadic camera at o = (0, 0, 1), level: the ray of pixel (v, u) is (1, (4 - u) / 4, (3 - v) / 4) exactly, so column 4 has
    d_y == 0 and row 3 has d_z == 0.  TALL is the unit box raised to z1 = 8, so that the rows above the horizon meet it too.
      scene 0: TALL: the rays of column 4, parallel to its y slab (and, in row 3, to its z slab as well), return 4.5 exactly.
      scene 1: TALL 3 m to the side: the parallel rays of column 4 lie outside its y slab and miss it; slanted rays still find it.
      scene 2: a box whose near corner (4, 1) lies on the ray of pixel (3, 3), d = (1, 1/4, 0): it enters the x slab and leaves the
               y slab at t = 4 exactly: tn == tf, a grazing ray, a hit at 4.0.  Its neighbour (3, 2) passes the corner outside.
      scene 3: a camera ON a slab's boundary with a parallel ray: the box's y slab is [0, 1] and o_y = 0: lo <= o holds, column 4 hits.
      scenes 4, 5, 6: a cylinder (5, 0, 0.5) whose front is at x = 4.5, the unit box whose face is there, and both: the centre
               pixel holds 4.5 in all three -- which of the two wins the tie cannot be seen, that the pixel holds that t can."""
    torch = torch_cuda
    c = DYADIC
    TALL = UNIT[:7] + [8.0]
    box = _one_box_scenes([TALL, [5.0, 3.0, 0.5, 0.5, 1.0, 0.0, 0.0, 8.0], [5.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 4.0], [5.0, 0.5, 0.5, 0.5, 1.0, 0.0, 0.0, 8.0],
                           UNIT, UNIT, UNIT])
    cyl = np.tile([[[5.0, 0.0, 0.5]]], (7, 1, 1))
    Twb = np.stack([AT_ORIGIN] * 7)
    ref = _check_all_types(torch, cyl, (0, 0, 0, 0, 1, 0, 1), box, (1, 1, 1, 1, 0, 1, 1), Twb, c, "parallel, grazing, equal t", max_range=1e9)
    free = _reference(cyl[:1], (0,), box[:1], (0,), Twb[:1], c, max_range=1e9)[0]
    assert (free[:4] == 0).all() and (free[4] == 4.0).all() and (free[5] == 2.0).all()   # sky on and above the horizon, ground below
    assert (ref[0, :4, 4] == 4.5).all() and ref[0, 4, 4] == 4.0 and ref[0, 3, 3] == 0
    assert np.array_equal(ref[1, :, 4], free[:, 4]) and (ref[1] != free).any()
    assert ref[2, 3, 3] == 4.0 and ref[2, 3, 2] == 0.0 and ref[2, 3, 4] == 4.0
    assert (ref[3, :4, 4] == 4.5).all()
    assert ref[4, 3, 4] == 4.5 and ref[5, 3, 4] == 4.5 and ref[6, 3, 4] == 4.5
    assert np.array_equal(ref[6], np.where((ref[4] > 0) & ((ref[5] == 0) | (ref[4] < ref[5])), ref[4], ref[5]))


def test_a_box_hit_at_exactly_max_range_and_one_double_beyond(torch_cuda):
    """Looking straight down onto a roof that fills the view (z1 = 2): every ray has d_z = -1 exactly, so every pixel's t is o_z - 2:
    max_range = that t keeps the whole image, the next double below it empties it (the ground lies beyond it too)."""
    torch = torch_cuda
    c = _cam(5, 7)
    Twb = np.tile(np.eye(4), (3, 1, 1)); Twb[:, :3, :3] = LOOK_DOWN; Twb[:, :3, 3] = [[0.0, 0.0, 3.0], [1.0, 2.0, 7.3], [5.0, -1.0, 2.7]]
    roof = _one_box_scenes([[0.0, 0.0, 50.0, 50.0, np.cos(0.3), np.sin(0.3), 0.5, 2.0]] * 3)
    free = _reference(NO_CYL, None, roof, None, Twb, c, max_range=1e9)
    for s in range(3):
        t = free[s, 0, 0]
        assert (free[s] == t).all() and 0 < t < Twb[s, 2, 3] - 1.9
        one = (NO_CYL[:1], None, roof[s:s + 1], None, Twb[s:s + 1], c)
        kept = _check_all_types(torch, *one, "at max_range", max_range=float(t))
        gone = _check_all_types(torch, *one, "beyond max_range", max_range=float(np.nextafter(t, 0.0)))
        assert (kept == t).all() and (gone == 0).all()


def test_a_nan_box_entry_is_no_hit(torch_cuda):
    """Eight scenes: box 0 has a NaN in entry s, box 1 is the unit box.  The image is that of the unit box alone: a NaN anywhere in a
    box is no hit from that box, and the box behind it in the list is still seen."""
    torch = torch_cuda
    c = _cam(24, 32, 1e-3)
    box = np.tile(np.array([[4.0, 0.2, 0.4, 0.6, np.cos(0.2), np.sin(0.2), 0.0, 3.0], UNIT]), (8, 1, 1))
    box[np.arange(8), 0, np.arange(8)] = np.nan
    cyl = _world(24, S=8, n=5)
    Twb = np.stack([POSES["identity"]] * 8)
    ref = _check_all_types(torch, cyl, None, box, None, Twb, c, "NaN entries")
    alone = _reference(cyl, None, box[:, 1:], None, Twb, c)
    assert np.array_equal(ref, alone) and (alone != _reference(cyl, None, box[:, :0], None, Twb, c)).any()


def _box_distance(P, box):
    """|signed distance| from points P [n, 3] to the surface of each box [m, 8] -> [n, m]"""
    ox, oy = P[:, 0:1] - box[:, 0], P[:, 1:2] - box[:, 1]
    q = np.stack([np.abs(box[:, 4] * ox + box[:, 5] * oy) - box[:, 2], np.abs(box[:, 4] * oy - box[:, 5] * ox) - box[:, 3],
                  np.abs(P[:, 2:3] - (box[:, 6] + box[:, 7]) / 2) - (box[:, 7] - box[:, 6]) / 2], axis=-1)
    return np.abs(np.sqrt((np.maximum(q, 0.0) ** 2).sum(axis=-1)) + np.minimum(q.max(axis=-1), 0.0))


def test_round_trip_through_depth_to_clouds(torch_cuda):
    """render (U16, millimetres) -> amk_depth_to_clouds at resize_scale 1 -> every obstacle point lies on the ground, a cylinder or a
    box face.  The bound is tests/test_sim_gpu.py's, derived the same way and with nothing in it that depends on the primitive: the
    point is o + R (dc d) for the quantised depth d where the hit is o + R (dc t), |dc| |d - t| apart with |d - t| <= half a depth
    quantum plus four float32 roundings at most max_range; the cloud's float32 coordinates add 2^-24 of the largest coordinate each."""
    torch = torch_cuda
    from avoid_mpc_amd.host import depth_to_clouds, sim_render_world
    c = _cam(48, 64, 1e-3)
    cyl, box = _world(78, n=20), _boxes(78, n=12)
    ccounts, bcounts = np.array([20, 7, 0], np.int32), np.array([12, 5, 9], np.int32)
    Twb = np.stack([POSES["identity"], POSES["yawed"], POSES["down"]])
    p = _params(c)
    dev = lambda a: torch.from_numpy(a).cuda()
    depth = sim_render_world(dev(cyl), dev(box), dev(Twb), p, 48, 64, cyl_counts=dev(ccounts), box_counts=dev(bcounts), z_top=Z_TOP,
                             max_range=MAX_RANGE, dtype=torch.int16)
    cloud, n, _, _ = depth_to_clouds(depth, p, dev(Twb), dev(np.stack([T @ flight.TBC_YAML for T in Twb])))
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
        k = ccounts[s]
        wall = np.abs(np.sqrt((P[:, 0:1] - cyl[s, :k, 0]) ** 2 + (P[:, 1:2] - cyl[s, :k, 1]) ** 2) - cyl[s, :k, 2])
        wall = np.where((P[:, 2:3] >= -bound) & (P[:, 2:3] <= Z_TOP + bound), wall, np.inf).min(axis=1, initial=np.inf)
        face = _box_distance(P, box[s, :bcounts[s]]).min(axis=1)
        off = np.minimum(np.minimum(wall, face), np.abs(P[:, 2]))
        print("scene", s, "points", n[s], "largest distance to a surface [m]:", off.max(), "on boxes:", int((face <= bound).sum()))
        assert off.max() <= bound, (s, off.max(), bound)
        assert (face <= bound).sum() > 50 and (np.abs(P[:, 2]) <= bound).sum() > 50     # boxes and the ground were seen


# ---- the vehicle -----------------------------------------------------------------------------------------------------------------
def _vehicle(torch, ABc, x, cmd, q, attitude, gz=flight.GZ, want_twb=True):
    from avoid_mpc_amd.host import sim_vehicle_step_att
    xd, cd = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(cmd).cuda()
    Td = torch.full((len(x), 4, 4), 9.0, dtype=torch.float64, device="cuda") if want_twb else None
    sim_vehicle_step_att(ABc, cd, xd, Td, pose_quantum=q, attitude=attitude, gz=gz)
    torch.cuda.synchronize()
    return xd.cpu().numpy(), Td.cpu().numpy() if want_twb else None


def _mpc_plant():
    from avoid_mpc_amd import synth
    from avoid_mpc_amd.host import plant_model
    return plant_model(synth.DEFAULT_TAU, 0.033)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("q", [0.0, 1e6])
def test_yaw_mode_is_amk_sim_vehicle_step(torch_cuda, q):
    """AMK_SIM_ATT_YAW against amk_sim_vehicle_step on the same inputs, every yaw of the ladder: x and Twb bit for bit."""
    torch = torch_cuda
    from avoid_mpc_amd.host import sim_vehicle_step
    ABc = _mpc_plant()
    x, cmd = _states(6, YAWS)
    xd, cd = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(cmd).cuda()
    Td = torch.full((len(x), 4, 4), 9.0, dtype=torch.float64, device="cuda")
    sim_vehicle_step(ABc, cd, xd, Td, pose_quantum=q)
    torch.cuda.synchronize()
    xn, T = _vehicle(torch, ABc, x, cmd, q, capi.AMK_SIM_ATT_YAW)
    assert np.array_equal(_bits(xn), _bits(xd.cpu().numpy())) and np.array_equal(_bits(T), _bits(Td.cpu().numpy()))
    x2, none = _vehicle(torch, ABc, x, cmd, q, capi.AMK_SIM_ATT_ACCEL, want_twb=False)          # d_Twb is optional in both modes
    assert none is None and np.array_equal(_bits(x2), _bits(xn))


@pytest.mark.parametrize("model", ["mpc", "dense"])
def test_accel_mode_at_yaw_zero_bit_for_bit(torch_cuda, model):
    """AMK_SIM_ATT_ACCEL against flight.vehicle_attitude_ordered at yaw == 0: no transcendental on either side, so x and the whole
    pose agree bit for bit; for the MPC's own model and for a dense random one whose yaw row is cleared, and for two values of gz."""
    torch = torch_cuda
    ABc = _mpc_plant() if model == "mpc" else np.random.default_rng(8).uniform(-1.5, 1.5, 150)
    if model == "dense":
        ABc[30:40] = 0.0; ABc[100 + 12:100 + 16] = 0.0; ABc[143] = 0.0                          # yaw+ = 0
    x, cmd = _states(9, np.zeros(16))
    x[0, 7:10], cmd[0] = 0.0, [0.0, 0.0, flight.GZ]                                              # hover
    for gz in (flight.GZ, 3.5):
        xn, T = _vehicle(torch, ABc, x, cmd, 1e6, capi.AMK_SIM_ATT_ACCEL, gz)
        rx, rT = flight.vehicle_attitude_ordered(ABc, x, cmd, 1e6, flight.ATT_ACCEL, gz)
        assert (rx[:, 3] == 0).all() and np.array_equal(_bits(xn), _bits(rx))
        assert np.array_equal(_bits(T), _bits(rT)), np.abs(T - rT).max()
        assert np.abs(rT[:, 2, 0]).max() > 0.05                                                  # really tilted
        R = T[:, :3, :3]
        assert np.abs(np.einsum("nji,njk->nik", R, R) - np.eye(3)).max() <= 96 * 2.0 ** -53     # (the bound tests/test_sim_world_abi.py derives)


def test_accel_mode_at_other_yaws(torch_cuda):
    """yaw != 0.  (a) With the device's OWN cos / sin -- read from the yaw-mode pose of the same inputs, which the kernel takes them
    from too -- the restatement matches bit for bit at every yaw.  (b) Against numpy's cos / sin every rotation entry, of magnitude
    at most 1, lies within 4 * 2^-52 of the numpy restatement: the 4 ulp test_vehicle_rotation_against_numpy_cos_sin asserts of the
    device's cos / sin.  Why it holds with room: the two libraries' cos / sin differ by an ulp at a few yaws (measured there), and
    that difference reaches an entry through y' = zb x (cs, sn, 0), a division by m >= zb_2 -- the thrust's vertical share, which the
    test's states keep above 1/2 -- and one more cross product, none of which amplifies it by more than 2 sqrt(2)."""
    torch = torch_cuda
    ABc = _mpc_plant()
    x, cmd = _states(4, YAWS)
    x[:, 7:10] = np.clip(x[:, 7:10], -4.0, 4.0); cmd[:, 0:2] = np.clip(cmd[:, 0:2], -4.0, 4.0); cmd[:, 2] = np.clip(cmd[:, 2], 6.0, 12.0)
    _, Ty = _vehicle(torch, ABc, x, cmd, 0.0, capi.AMK_SIM_ATT_YAW)
    xn, T = _vehicle(torch, ABc, x, cmd, 0.0, capi.AMK_SIM_ATT_ACCEL)
    rx, rT = flight.vehicle_attitude_ordered(ABc, x, cmd, 0.0, cs_sn=(Ty[:, 0, 0], Ty[:, 1, 0]))
    assert np.array_equal(xn[:, 3], YAWS) and np.array_equal(_bits(xn), _bits(rx))
    assert np.array_equal(_bits(T), _bits(rT)), np.abs(T - rT).max()
    _, nT = flight.vehicle_attitude_ordered(ABc, x, cmd, 0.0)
    assert (nT[:, 2, 2] > 0.5).all()
    err = np.abs(T[:, :3, :3] - nT[:, :3, :3]).max()
    print("largest |R - numpy's| / 2^-52:", err * 2.0 ** 52)
    assert err <= 4 * 2.0 ** -52
    assert np.array_equal(T[:, :, 3], Ty[:, :, 3]) and np.array_equal(T[:, 3], Ty[:, 3])


def test_accel_mode_falls_back_to_the_yaw_rotation(torch_cuda):
    """x+ = x (an identity model), so the new acceleration is the given one.  Free fall (n == 0), thrust along the heading
    (m == 0), thrust that overflows (n = inf: zb = 0, m == 0) and a NaN state: the pose is the yaw mode's, bit for bit; the scenes
    beside them tilt."""
    torch = torch_cuda
    ABc = np.zeros(150); ABc[:100] = np.eye(10).reshape(-1)
    x = np.zeros((6, 10)); x[:, 0:3] = [1.0, -2.0, 3.0]; x[:, 3] = [0.0, 0.0, 0.7, 0.0, 0.3, 0.0]
    x[0, 7:10] = [0.0, 0.0, -flight.GZ]
    x[1, 7:10] = [3.0, 0.0, -flight.GZ]
    x[2, 7:10] = [1e200, 1e200, 1e200]
    x[3, 7:10] = [np.nan, 0.0, 0.0]
    x[4, 7:10] = [2.0, -1.0, 0.5]
    x[5, 7:10] = [2.0, -1.0, 0.5]
    cmd = np.zeros((6, 3))
    _, Ty = _vehicle(torch, ABc, x, cmd, 0.0, capi.AMK_SIM_ATT_YAW)
    xn, T = _vehicle(torch, ABc, x, cmd, 0.0, capi.AMK_SIM_ATT_ACCEL)
    assert np.array_equal(_bits(T[:4]), _bits(Ty[:4]))
    assert np.array_equal(T[[0, 1]], np.tile(np.eye(4) + np.array([[0, 0, 0, 1.0], [0, 0, 0, -2.0], [0, 0, 0, 3.0], [0, 0, 0, 0]]), (2, 1, 1)))
    assert np.isnan(xn[3]).all() and np.array_equal(xn[[0, 1, 2, 4, 5]], x[[0, 1, 2, 4, 5]])
    _, rT = flight.vehicle_attitude_ordered(ABc, x, cmd, 0.0, cs_sn=(Ty[:, 0, 0], Ty[:, 1, 0]))
    assert np.array_equal(_bits(T[[0, 1, 2, 4, 5]]), _bits(rT[[0, 1, 2, 4, 5]]))
    assert (T[4:, 2, 0] != 0).all() and not np.array_equal(T[4, :3, :3], Ty[4, :3, :3])


# ---- the _host forms ---------------------------------------------------------------------------------------------------------------
def _vp(a):
    import ctypes as C
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_the_host_forms_equal_the_device_calls(torch_cuda):
    """amk_sim_render_world_host and amk_sim_vehicle_step_att_host on host arrays against the device calls on the same inputs: the same
    bytes.  Ragged counts of both kinds, both pixel types; NULL counts; a NULL box list with max_box == 0; a NULL h_Twb."""
    import ctypes as C
    torch = torch_cuda
    lib = capi.load()
    c = _cam(24, 32, 1e-3)
    p = _params(c)
    cyl, box = _world(31, n=9), _boxes(31, n=7)
    Twb = np.stack([POSES["yawed"], POSES["down"], POSES["identity"]])
    for cyl_, cc, box_, bc in ((cyl, np.array([9, 2, 5], np.int32), box, np.array([7, 0, 3], np.int32)), (cyl, None, box, None),
                               (cyl, np.array([4, 9, 0], np.int32), NO_BOX, None), (NO_CYL, None, box, np.array([1, 7, 2], np.int32))):
        for kind, dtype, npt in ((capi.AMK_DEPTH_U16, torch.int16, np.int16), (capi.AMK_DEPTH_F32, torch.float32, np.float32)):
            out = np.full((3, 24, 32), 7, npt)
            cyl_h, box_h = np.ascontiguousarray(cyl_), np.ascontiguousarray(box_)
            capi.check(lib.amk_sim_render_world_host(_vp(cyl_h) if cyl_h.size else None, _vp(cc), cyl_h.shape[1], _vp(box_h) if box_h.size else None,
                                                     _vp(bc), box_h.shape[1], 3, Z_TOP, MAX_RANGE, C.byref(p), 24, 32, _vp(Twb), _vp(out), kind),
                       "amk_sim_render_world_host")
            dev = _render(torch, cyl_, cc, box_, bc, Twb, c, dtype)
            assert (dev != 0).any() and np.array_equal(out.view(np.uint8), dev.view(np.uint8)), (cyl_.shape, cc, box_.shape, bc, kind)
    ABc = _mpc_plant()
    x, cmd = _states(11, YAWS)
    for attitude in (capi.AMK_SIM_ATT_YAW, capi.AMK_SIM_ATT_ACCEL):
        xd, Td = _vehicle(torch, ABc, x, cmd, 1e6, attitude, 3.5)
        for want_twb in (True, False):
            xh, Th = x.copy(), np.full((len(x), 4, 4), 9.0)
            capi.check(lib.amk_sim_vehicle_step_att_host(_vp(ABc), _vp(cmd), _vp(xh), _vp(Th) if want_twb else None, len(x), 1e6, attitude, 3.5),
                       "amk_sim_vehicle_step_att_host")
            assert np.array_equal(_bits(xh), _bits(xd))
            assert np.array_equal(_bits(Th), _bits(Td)) if want_twb else (Th == 9.0).all()
