"""GPU: the ground-truth monitor beside a closed-loop flight (tests/_sim_truth.py device_truth_flights): four robots, a 48 x 64 sensor,
12 periods through flight.WallWorld with a vehicle that tilts (AMK_SIM_ATT_ACCEL), with and without a keyframe map.  The monitor --
the pipeline's audit in AMK_AUDIT_REPORT, amk_sim_clearance on the state and amk_sim_path_cast on the plan, every period, on the
device -- changes nothing: the flight is tests/_sim_world.py's device_world_flights bit for bit.  And what it logged is what the numpy
restatements give for the logged states and plans, bit for bit.  How often the two verdicts differ is printed, not asserted: that is
a finding about the planner and its map."""
import numpy as np
import pytest

from tests import _sim_truth, _sim_world
from tests.test_sim_world_flight_gpu import PERIODS, SEEDS, WORLD

pytestmark = pytest.mark.gpu


def _bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


@pytest.mark.parametrize("keyframes", [None, dict(max_frame_count=3, th_dist=0.1, th_count=10)], ids=["single_frame", "keyframe_map"])
def test_the_monitor_changes_nothing_and_logs_the_restatements(keyframes):
    import torch
    assert torch.cuda.is_available()
    m = _sim_truth.device_truth_flights(SEEDS, "C1", PERIODS, world_kw=WORLD, keyframes=keyframes)
    d = _sim_world.device_world_flights(SEEDS, "C1", PERIODS, world_kw=WORLD, keyframes=keyframes)
    for key in ("x", "u", "cmd", "Twb"):                                        # (Twb: the pose of every period)
        same = m[key].view(np.uint64) == d[key].view(np.uint64)
        assert same.all(), (key, np.argwhere(~same)[:5])
    assert np.array_equal(m["flags"], d["flags"])
    assert (m["flags"][:, :, 1] > 0).any() and (m["x"][:, -1, 0] - m["x"][:, 0, 0] > 0.5).all()   # the step solved and the fleet flew
    want = _sim_truth.truth_answers_ordered(m)
    for key, w in want.items():
        assert m[key].dtype == w.dtype and np.array_equal(_bits(m[key]), _bits(w)), (key, np.argwhere(_bits(m[key]) != _bits(w))[:5])
    assert m["n_legs"] == m["x0array"].shape[2] - 1 and (m["truth_free"] > 0).any() and np.isfinite(m["truth_clear_dist"]).all()
    truth, audit = m["truth_stop"] != 0, m["audit_stop"] != 0
    print("\n(robot, period) pairs:", truth.size, " truth stops, audit free:", int((truth & ~audit).sum()), " audit stops, truth free:",
          int((~truth & audit).sum()), " both stop:", int((truth & audit).sum()), " both free:", int((~truth & ~audit).sum()))
    print("least true clearance per robot [m]:", m["truth_clear_dist"].min(axis=1), " of kind", np.take_along_axis(
        m["truth_clear_kind"], m["truth_clear_dist"].argmin(axis=1)[:, None], axis=1)[:, 0])


def test_the_monitor_with_fewer_legs_than_the_horizon():
    """An audit over the first four legs only: the monitor hands the truth cast a copy of the plan's leading five rows per scene (a
    scene must start every n_points rows).  Two robots, six periods: still the unmonitored flight, still the restatements."""
    m = _sim_truth.device_truth_flights(SEEDS[:2], "C1", 6, world_kw=WORLD, n_legs=4)
    d = _sim_world.device_world_flights(SEEDS[:2], "C1", 6, world_kw=WORLD)
    for key in ("x", "u", "cmd", "Twb"):
        assert np.array_equal(m[key].view(np.uint64), d[key].view(np.uint64)), key
    assert np.array_equal(m["flags"], d["flags"]) and m["n_legs"] == 4 < m["x0array"].shape[2] - 1
    for key, w in _sim_truth.truth_answers_ordered(m).items():
        assert m[key].dtype == w.dtype and np.array_equal(_bits(m[key]), _bits(w)), key
    assert (m["truth_leg"] < 4).all() and (m["audit_leg"] < 4).all()
