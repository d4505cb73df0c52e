"""GPU: the pipeline obtains one hardware queue per slot by itself when the runtime's pool (GPU_MAX_HW_QUEUES, 4 by default) is
smaller than its slot count: the slots' streams run side by side, amk_pipeline_queue_mode tells how each was created, the results
are the pooled streams' bit for bit, and a creation call that fails leaves the slot with a pooled stream.

The runtime fixes its queue pool at the first HIP call, so every case runs in a fresh child process that is given
GPU_MAX_HW_QUEUES explicitly; a child is started once per configuration and shared by the tests that read it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from avoid_mpc_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# What automatic mode creates when the pool is too small (csrc/pipeline.hip: amk__pipeline_queue_policy)
SHIPPED, SHIPPED_NAME = capi.AMK_QUEUES_PRIORITY, "priority"
PROBE_SLOTS = 6          # more than the pool of 4: pooled streams must share
PROBE_ITERS = 75000      # dependent integer steps of the probe's kernel, 20 ns each on an MI355X: 1.5 ms

CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, ROOT)
import numpy as np
import torch
from avoid_mpc_amd import capi, synth, fsm
from avoid_mpc_amd.host import Pipeline
what, out_npz, iters = sys.argv[1].split(","), sys.argv[2], int(sys.argv[3])
lib = capi.load()
prm = synth.MpcParams(T=0.33, K=3)
res = {}
if "inject" in what:
    assert lib.amk__pipeline_inject_failure(None, 3) == capi.AMK_OK
pl = Pipeline(6, 2, 512, 512, prm)            # the smallest shape that creates a pipeline: the queues do not depend on it
res["modes"] = [pl.queue_mode(i) for i in range(6)]
res["no_slot"] = [pl.queue_mode(-1), pl.queue_mode(6)]
if "probe" in what:
    t = np.zeros((6, 2), np.uint64)
    capi.check(lib.amk__pipeline_overlap_probe(pl.h, iters, t.ctypes.data_as(C.c_void_p)), "amk__pipeline_overlap_probe")
    res["start_end"] = [[int(a), int(b)] for a, b in t]
pl.close()
if "bits" in what:   # 3 slots x gang 2, 4 scenes, 2 000-point clouds, N = 10, K = 3, 6 frames of the cold workload
    S, n, ne = 4, 2000, 200
    pl = Pipeline(3, S, n, ne, prm, gang=2)
    res["bits_modes"] = [pl.queue_mode(i) for i in range(3)]
    keep, tickets = [], []
    for f in range(6):
        scenes = [synth.make_scene(n, 7100 + 13 * f + s, prm) for s in range(S)]
        sq = np.stack([fsm.state_quads(sc["pos"], sc["vel"], sc["acc"], sc["yaw"], prm.decay, prm.max_iter) for sc in scenes])
        fr = [torch.from_numpy(np.stack([sc["cloud"] for sc in scenes])).cuda(), torch.from_numpy(np.stack([sc["edge"][:ne] for sc in scenes])).cuda(),
              torch.from_numpy(sq).cuda(), torch.from_numpy(np.array([sc["pos"][0] for sc in scenes])).cuda(),
              torch.from_numpy(np.stack([sc["ref_path"] for sc in scenes])).cuda()]
        keep.append(fr)
        tickets.append(pl.submit(*fr))
    pl.drain()
    arrays = {}
    for f, t in enumerate(tickets):
        for k, v in pl.outputs(t).items():
            arrays["%s_%d" % (k, f)] = v
    np.savez(out_npz, **arrays)
    res["tickets"] = tickets
    pl.close()
print("RESULT " + json.dumps(res))
"""


def _child(tmp, what, hw_queues, knob):
    env = {k: v for k, v in os.environ.items() if k != "AMK_PIPELINE_QUEUES"}
    env["GPU_MAX_HW_QUEUES"] = str(hw_queues)
    if knob:
        env["AMK_PIPELINE_QUEUES"] = knob
    npz = os.path.join(str(tmp), "bits_%s_%s.npz" % (hw_queues, knob or "auto"))
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + CHILD, what, npz, str(PROBE_ITERS)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    res["npz"] = npz
    return res


@pytest.fixture(scope="module")
def auto4(tmp_path_factory):
    return _child(tmp_path_factory.mktemp("queues"), "probe,bits", 4, None)


@pytest.fixture(scope="module")
def pooled4(tmp_path_factory):
    return _child(tmp_path_factory.mktemp("queues"), "probe,bits", 4, "pooled")


def _intervals(res):
    t = np.array(res["start_end"], dtype=np.int64)
    t0 = t[:, 0].min()
    return t, "start / end in us after the first start (100 MHz clock): " + ", ".join(
        "[%.0f, %.0f]" % ((a - t0) / 100.0, (b - t0) / 100.0) for a, b in t)


def test_slots_overlap(auto4, pooled4):
    """Six slots on a pool of four queues: one fixed-length single-block kernel per slot, launched back to back.  In automatic mode
    every pair of the six [start, end] intervals intersects.  The same with AMK_PIPELINE_QUEUES=pooled is printed, not asserted:
    there two streams share a queue and serialise, which is the runtime's property, not this library's."""
    tp, line = _intervals(pooled4)
    print("pooled:   ", line, "; latest start %s earliest end" % ("<" if tp[:, 0].max() < tp[:, 1].min() else ">="))
    t, line = _intervals(auto4)
    print("automatic:", line)
    assert (t[:, 1] > t[:, 0]).all()
    assert t[:, 0].max() < t[:, 1].min(), line


def test_mode_report(auto4, pooled4, tmp_path):
    assert auto4["modes"] == [SHIPPED] * PROBE_SLOTS and auto4["no_slot"] == [-1, -1]
    assert pooled4["modes"] == [capi.AMK_QUEUES_POOLED] * PROBE_SLOTS
    wide = _child(tmp_path, "modes", 8, None)   # pool >= slots + 1: the documented configuration keeps its pooled streams
    assert wide["modes"] == [capi.AMK_QUEUES_POOLED] * PROBE_SLOTS


def test_same_bits(auto4, pooled4, tmp_path):
    """u, x0array, flags and ref_path of every ticket, automatic mode against pooled streams: identical bits.  Three slots fit
    a pool of four, so automatic mode keeps pooled streams there; the same frames with the knob at `priority` -- the streams
    automatic mode creates when the pool is too small -- must give those bits too."""
    forced = _child(tmp_path, "bits", 4, SHIPPED_NAME)
    assert auto4["bits_modes"] == [capi.AMK_QUEUES_POOLED] * 3 and pooled4["bits_modes"] == [capi.AMK_QUEUES_POOLED] * 3
    assert forced["bits_modes"] == [SHIPPED] * 3
    b = np.load(pooled4["npz"])
    assert len(b.files) == 4 * 6 and len(set(pooled4["tickets"])) == 6
    assert any(np.abs(b["u_%d" % f]).max() > 0 for f in range(6))   # (the steps ran)
    for res in (auto4, forced):
        a = np.load(res["npz"])
        assert res["tickets"] == pooled4["tickets"] and sorted(a.files) == sorted(b.files)
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def test_fallback(tmp_path):
    """Every non-pooled creation call of the next amk_pipeline_create fails: creation succeeds, the slots report pooled streams."""
    res = _child(tmp_path, "inject", 4, SHIPPED_NAME)
    assert res["modes"] == [capi.AMK_QUEUES_POOLED] * PROBE_SLOTS
