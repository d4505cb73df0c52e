"""GPU: closed-loop depth flights with the sensor and the vehicle on the device (tests/_sim_flight.py device_depth_flights) against the
same pipeline with numpy's restatements between the periods (host_twin_depth_flights): four robots, a 48 x 64 sensor, 12 periods,
with and without a keyframe map.  At yaw = 0 the vehicle's pose has no transcendental in it, the frames agree pixel for pixel, and
so the two loops agree bit for bit in the state, the step's control, its flags and the published command."""
import numpy as np
import pytest

from tests import _flight, _sim_flight

pytestmark = pytest.mark.gpu

SEEDS, PERIODS = [2000, 2001, 2002, 2003], 12
WORLD = dict(cyl_per_m=1.5, x_first=3.0, length=60.0)   # the keyframe flights' corridor (tests/test_kfmap_gpu.py): obstacles from the start


@pytest.mark.parametrize("keyframes", [None, dict(max_frame_count=3, th_dist=0.1, th_count=10)], ids=["single_frame", "keyframe_map"])
def test_device_loop_equals_the_host_twin(keyframes):
    import torch
    assert torch.cuda.is_available()
    d = _sim_flight.device_depth_flights(SEEDS, "C1", PERIODS, world_kw=WORLD, keyframes=keyframes)
    h = _sim_flight.host_twin_depth_flights(SEEDS, "C1", PERIODS, world_kw=WORLD, keyframes=keyframes)
    prm, _ = _flight.make_prm("C1")
    print("\ndevice loop:", _flight.flight_stats(d, prm))
    assert (d["x"][:, :, 3] == 0).all()                                       # yaw = 0 throughout: Command.yaw = 0 holds the heading
    assert (d["flags"][:, :, 1] > 0).any() and np.abs(d["cmd"]).max() > 0     # the step solved and something was published
    assert (d["x"][:, -1, 0] - d["x"][:, 0, 0] > 1.0).all()                    # and the fleet flew
    for key in ("x", "u", "cmd"):
        same = d[key].view(np.uint64) == h[key].view(np.uint64)
        assert same.all(), (key, np.argwhere(~same)[:5], np.abs(d[key] - h[key]).max())
    assert np.array_equal(d["flags"], h["flags"])
    if keyframes:                                                              # the map was in the loop, and it is the same map
        print("keyframes / query frames / map points per robot:", d["n_keyframes"], d["n_query_frames"], d["map_points"])
        assert d["n_query_frames"].max() >= 3, "the flights never had a multi-frame map"   # (as tests/test_kfmap_gpu.py asks of its flights)
        for key in ("n_keyframes", "n_query_frames", "map_points"):
            assert np.array_equal(d[key], h[key]), key


def test_the_ring_keeps_the_newest_periods():
    """A log ring shorter than the flight holds the newest periods, bit for bit what the full log holds there."""
    full = _sim_flight.device_depth_flights(SEEDS[:2], "C1", 6, world_kw=WORLD)
    ring = _sim_flight.device_depth_flights(SEEDS[:2], "C1", 6, world_kw=WORLD, ring=2)
    for key in ("u", "cmd", "flags"):
        assert np.array_equal(ring[key][:, 4:], full[key][:, 4:]) and not ring[key][:, :4].any(), key
    assert np.array_equal(ring["x"][:, 5:], full["x"][:, 5:])
