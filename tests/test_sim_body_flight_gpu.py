"""GPU: closed-loop flights through flight.WallWorld flown by the rigid-body vehicle (tests/_sim_body.py): three robots, the 48 x 64
camera, 8 periods, with and without a keyframe map.  The device loop -- render, submit, amk_sim_vehicle_step_body, no host copy in
between -- equals the same pipeline with numpy's restatements of sensor and vehicle between the periods bit for bit in the state, the
step's control, its flags, the published command, the pose and the vehicle's hidden state; with the commanded yaw's (cs, sn) = (1, 0)
there is no transcendental anywhere in the flight.  The flight is NOT tests/_sim_world.py's: the plant disagrees with the MPC's
prediction, and the camera's tilt lags the acceleration it would follow at once under AMK_SIM_ATT_ACCEL."""
import numpy as np
import pytest

from avoid_mpc_amd import flight
from tests import _sim_body, _sim_world
from tests.test_sim_world_flight_gpu import WORLD

pytestmark = pytest.mark.gpu

SEEDS, PERIODS = [2000, 2001, 2002], 8
KEYFRAMES = dict(max_frame_count=3, th_dist=0.1, th_count=10)


@pytest.mark.parametrize("keyframes", [None, KEYFRAMES], ids=["single_frame", "keyframe_map"])
def test_the_body_device_loop_equals_its_host_twin(keyframes):
    import torch
    assert torch.cuda.is_available()
    d = _sim_body.device_body_flights(SEEDS, "C1", PERIODS, world_kw=WORLD, keyframes=keyframes)
    h = _sim_body.host_twin_body_flights(SEEDS, "C1", PERIODS, world_kw=WORLD, keyframes=keyframes)
    assert (d["x"][:, :, 3] == 0).all()                                       # the yaw is never written
    assert (d["flags"][:, :, 1] > 0).any() and np.abs(d["cmd"]).max() > 0     # the step solved and something was published
    assert (d["x"][:, -1, 0] - d["x"][:, 0, 0] > 0.3).all()                    # and the fleet flew
    for key in ("x", "u", "cmd", "Twb", "body"):
        same = d[key].view(np.uint64) == h[key].view(np.uint64)
        assert same.all(), (key, np.argwhere(~same)[:5], np.abs(d[key] - h[key]).max())
    assert np.array_equal(d["flags"], h["flags"])
    assert (d["body"][:, -1, flight.BODY_HELD] == flight.COG_MAX).all() and (d["body"][:, 1:, 58:] == 0).all()
    if keyframes:
        print("keyframes / query frames / map points per robot:", d["n_keyframes"], d["n_query_frames"], d["map_points"])
        for key in ("n_keyframes", "n_query_frames", "map_points"):
            assert np.array_equal(d[key], h[key]), key
        return
    # not the affine vehicle's flight: from the first period on the plant disagrees with the model the MPC predicts with
    a = _sim_world.device_world_flights(SEEDS, "C1", PERIODS, world_kw=WORLD)
    assert np.array_equal(a["x"][:, 0], d["x"][:, 0]) and np.array_equal(a["cmd"][:, 0], d["cmd"][:, 0])   # the same start, the same first command
    assert (np.abs(a["x"][:, 1] - d["x"][:, 1]).max(axis=1) > 0).all() and not np.array_equal(a["u"][:, 1:], d["u"][:, 1:])
    # and the camera lags.  (a) The pose of period t + 1 is not acc2rotmat of that period's acceleration state, which is what
    # AMK_SIM_ATT_ACCEL shows at once.  Without drag the specific force lies along the body's z, so the IMU's acceleration points along
    # the attitude itself and (a) differs in the roundings only; what the attitude lags is (b) its COMMAND: at the end of a period the
    # body's z has not reached the direction of the thrust that period commanded.
    lag = np.zeros((len(SEEDS), PERIODS))
    for t in range(PERIODS):
        zd = d["cmd"][:, t] / np.linalg.norm(d["cmd"][:, t], axis=1, keepdims=True)
        lag[:, t] = np.linalg.norm(np.cross(zd, d["Twb"][:, t + 1, :3, 2]), axis=1)
    print("sine of the angle between the body's z and the commanded thrust, per robot and period:\n", lag)
    assert (lag.max(axis=1) > 1e-6).all()                                      # (rounding would be 1e-16)
    _, T_att = flight.vehicle_attitude_ordered(np.concatenate([np.eye(10).reshape(-1), np.zeros(50)]), d["x"][:, 1:].reshape(-1, 10),
                                               np.zeros((len(SEEDS) * PERIODS, 3)))          # (an identity model: acc2rotmat of x as logged)
    differs = (T_att[:, :3, :3].reshape(len(SEEDS), PERIODS, 9) != d["Twb"][:, 1:, :3, :3].reshape(len(SEEDS), PERIODS, 9)).any(axis=2)
    print("periods in which the pose is not acc2rotmat of the acceleration state, per robot:", differs.sum(axis=1), "of", PERIODS)
    assert differs.any(axis=1).all()
    assert (d["Twb"][:, 1:, 2, 0] != 0).any(axis=1).all()                      # while really tilting
