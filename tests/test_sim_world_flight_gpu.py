"""GPU: closed-loop flights through a corridor with walls, gates and cylinders (flight.WallWorld), flown by a vehicle that tilts into
its thrust (AMK_SIM_ATT_ACCEL), sensor and vehicle on the device (tests/_sim_world.py device_world_flights) against the same pipeline
with numpy's restatements between the periods (host_twin_world_flights): four robots, a 48 x 64 sensor, 12 periods, with and without
a keyframe map.  The flights hold yaw at 0, so the tilted pose has no transcendental in it, the frames agree pixel for pixel, and
the two loops agree bit for bit in the state, the step's control, its flags and the published command."""
import numpy as np
import pytest

from avoid_mpc_amd import flight
from tests import _flight, _sim_world

pytestmark = pytest.mark.gpu

SEEDS, PERIODS = [2000, 2001, 2002, 2003], 12
WORLD = dict(cyl_per_m=1.5, x_first=3.0, length=60.0)   # tests/test_sim_flight_gpu.py's corridor, with WallWorld's walls from 9 m on


@pytest.mark.parametrize("keyframes", [None, dict(max_frame_count=3, th_dist=0.1, th_count=10)], ids=["single_frame", "keyframe_map"])
def test_device_loop_equals_the_host_twin_with_walls_and_tilt(keyframes):
    import torch
    assert torch.cuda.is_available()
    d = _sim_world.device_world_flights(SEEDS, "C1", PERIODS, world_kw=WORLD, keyframes=keyframes)
    h = _sim_world.host_twin_world_flights(SEEDS, "C1", PERIODS, world_kw=WORLD, keyframes=keyframes)
    prm, _ = _flight.make_prm("C1")
    print("\ndevice loop:", _flight.flight_stats(d, prm))
    print("least clearance per robot [m]: cylinders", d["clearance"].min(axis=1), " box faces", d["box_clearance"].min(axis=1))   # a finding, not gated
    print("largest tilt per robot [rad]:", np.arccos(np.clip(d["Twb"][:, :, 2, 2], -1.0, 1.0)).max(axis=1))
    assert (d["x"][:, :, 3] == 0).all()                                       # yaw = 0 throughout: Command.yaw = 0 holds the heading
    assert (d["flags"][:, :, 1] > 0).any() and np.abs(d["cmd"]).max() > 0     # the step solved and something was published
    assert (d["x"][:, -1, 0] - d["x"][:, 0, 0] > 0.5).all()                    # and the fleet flew
    assert (d["Twb"][:, :, 2, 0] != 0).any(axis=1).all()                       # every camera really tilted in some period
    for key in ("x", "u", "cmd", "Twb"):
        same = d[key].view(np.uint64) == h[key].view(np.uint64)
        assert same.all(), (key, np.argwhere(~same)[:5], np.abs(d[key] - h[key]).max())
    assert np.array_equal(d["flags"], h["flags"])
    c = _sim_world.SIM_CAM                                                     # some frame really saw a box: the same poses without the boxes
    with_boxes = _sim_world.host_frames(d["cyl"], d["cyl_counts"], d["box"], d["Twb"][:, -1], c)
    without = _sim_world.host_frames(d["cyl"], d["cyl_counts"], d["box"][:, :0], d["Twb"][:, -1], c)
    print("pixels of the last frame that a box answers, per robot:", (with_boxes != without).reshape(len(SEEDS), -1).sum(axis=1))
    assert (with_boxes != without).any()
    if keyframes:                                                              # the map was in the loop, and it is the same map
        print("keyframes / query frames / map points per robot:", d["n_keyframes"], d["n_query_frames"], d["map_points"])
        for key in ("n_keyframes", "n_query_frames", "map_points"):
            assert np.array_equal(d[key], h[key]), key


def test_yaw_attitude_in_the_walled_world():
    """AMK_SIM_ATT_YAW in the walled world: every pose stays level, and the device loop equals its host twin bit for bit in that
    mode too (2 robots, 6 periods)."""
    d = _sim_world.device_world_flights(SEEDS[:2], "C1", 6, world_kw=WORLD, attitude=flight.ATT_YAW)
    h = _sim_world.host_twin_world_flights(SEEDS[:2], "C1", 6, world_kw=WORLD, attitude=flight.ATT_YAW)
    assert np.array_equal(d["Twb"][:, :, :3, :3], np.tile(np.eye(3), (2, 7, 1, 1)))
    for key in ("x", "u", "cmd", "Twb"):
        assert np.array_equal(d[key].view(np.uint64), h[key].view(np.uint64)), key
    assert np.array_equal(d["flags"], h["flags"])
