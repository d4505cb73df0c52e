"""GPU: closed-loop flights through flight.WallWorld that see it through a noisy sensor (tests/_sim_noise.py): three robots, the
48 x 64 camera, 8 periods, with and without a keyframe map.  The device loop -- render, amk_sim_depth_noise, submit, vehicle, no host
copy in between -- equals the same pipeline with numpy's restatements of sensor, noise and vehicle between the periods bit for bit in
the state, the step's control, its flags, the published command and the pose, under a noise setting that exercises every stage.  With
every stage off the noisy loop is tests/_sim_world.py's device_world_flights bit for bit."""
import numpy as np
import pytest

from tests import _sim_noise, _sim_world
from tests.test_sim_world_flight_gpu import WORLD

pytestmark = pytest.mark.gpu

SEEDS, PERIODS = [2000, 2001, 2002], 8
KEYFRAMES = dict(max_frame_count=3, th_dist=0.1, th_count=10)


def _same_flight(a, b):
    for key in ("x", "u", "cmd", "Twb"):
        same = a[key].view(np.uint64) == b[key].view(np.uint64)
        assert same.all(), (key, np.argwhere(~same)[:5], np.abs(a[key] - b[key]).max())
    assert np.array_equal(a["flags"], b["flags"])


@pytest.mark.parametrize("keyframes", [None, KEYFRAMES], ids=["single_frame", "keyframe_map"])
def test_the_noisy_device_loop_equals_its_host_twin(keyframes):
    import torch
    assert torch.cuda.is_available()
    d = _sim_noise.device_noisy_flights(SEEDS, _sim_noise.EVERY_STAGE, "C1", PERIODS, world_kw=WORLD, keyframes=keyframes, scene_id0=5)
    h = _sim_noise.host_twin_noisy_flights(SEEDS, _sim_noise.EVERY_STAGE, "C1", PERIODS, world_kw=WORLD, keyframes=keyframes, scene_id0=5)
    print("\npixels the noise altered per period (of %d):" % (len(SEEDS) * 48 * 64), h["changed"])
    assert (h["changed"] > 100).all()                                          # the sensor really was noisy, every period
    assert (d["flags"][:, :, 1] > 0).any() and np.abs(d["cmd"]).max() > 0      # the step solved and something was published
    assert (d["x"][:, -1, 0] - d["x"][:, 0, 0] > 0.3).all()                    # and the fleet flew
    _same_flight(d, h)
    if keyframes:
        print("keyframes / query frames / map points per robot:", d["n_keyframes"], d["n_query_frames"], d["map_points"])
        for key in ("n_keyframes", "n_query_frames", "map_points"):
            assert np.array_equal(d[key], h[key]), key


def test_with_every_stage_off_the_noisy_loop_is_the_clean_one():
    n = _sim_noise.device_noisy_flights(SEEDS, dict(seed=9), "C1", PERIODS, world_kw=WORLD, keyframes=KEYFRAMES)
    c = _sim_world.device_world_flights(SEEDS, "C1", PERIODS, world_kw=WORLD, keyframes=KEYFRAMES)
    _same_flight(n, c)
    for key in ("n_keyframes", "n_query_frames", "map_points"):
        assert np.array_equal(n[key], c[key]), key
    noisy = _sim_noise.device_noisy_flights(SEEDS, _sim_noise.EVERY_STAGE, "C1", PERIODS, world_kw=WORLD, keyframes=KEYFRAMES)
    assert not np.array_equal(noisy["u"], c["u"])                              # and the noise does reach the step
