"""GPU: changes to how the solve's values TRAVEL (the forward roll's ring of prefetched gains waited for load by load, wave
reductions advanced side by side) and not to how they are computed must return, BIT FOR BIT, what the library before them
returned.

tests/golden/mpc_riccati_transport.npz holds inputs (ref_states per scene) and that earlier library's outputs on the GPU
(tools/record_riccati_transport.py): u, the warm start w = [X_0, U_0, ..., X_N] and info[4] of MpcBatch.Solve, and u / x0array /
flags / ref_path of one amk_step_batch.  Cases: the baked horizons 20, 10, 30; the generic kernel at N = 7 (no multiple of the
forward roll's prefetch depth) and at N = 3 and N = 2 (shorter than the prefetch depth: every load of the ring's last turn is
one nobody uses; 2 is the smallest horizon there is); K = 8 and K = 3; zero start and, for n20k8, a second solve from the first
one's warm start; fp64 and fp32.  Three or more of the n20k8 scenes regularise (info[2] > 0): their inertia loop runs the
backward sweep several times per iteration.

So that the fixture cannot hide a fault of the library it was recorded from, every fp64 case is also compared with the CPU
oracle under the tolerances of tests/test_mpc_gpu.py: same info and |u - u_oracle|, |w - w_oracle| <= 1e-6 scene by scene; a
scene whose counts differ by a rounding-level branch flip must be converged on both sides and agree to 1e-4, one per case at
the most.  fp32 has no oracle twin: its cases pin the bits only (tests/test_mpc_fp32_gpu.py states its accuracy)."""
import os

import numpy as np
import pytest

from tests import _oracle
from avoid_mpc_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-6
DT = 0.033
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mpc_riccati_transport.npz")
# name -> (N, K, scenes, solves recorded)
CASES = {"n20k8": (20, 8, 6, 2), "n10k3": (10, 3, 6, 1), "n30k3": (30, 3, 4, 1), "n7k3": (7, 3, 4, 1), "n3k3": (3, 3, 4, 1),
         "n2k8": (2, 8, 4, 1)}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def _params(N, K):
    prm = synth.MpcParams(T=N * DT + 1e-4, K=K)
    assert prm.N == N
    return prm


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _solve_all(torch, golden, name, bits):
    """The case's solves on one MpcBatch -> [(u, w, info)] per solve."""
    from avoid_mpc_amd.host import MpcBatch
    N, K, S, n_solves = CASES[name]
    prm = _params(N, K)
    gpu = MpcBatch(prm.T, prm.dt, prm.K, S); gpu.configure(prm); gpu.set_precision(bits)
    assert gpu.N == N
    out = []
    for i in range(n_solves):
        ref = golden[f"{name}_ref{i}"]
        assert ref.shape == (S, gpu.ref_len)
        u, _x0, info = gpu.Solve(torch.from_numpy(ref).cuda(), faster=(i == 0))
        torch.cuda.synchronize()
        out.append((u.cpu().numpy(), gpu.get_warm_start().cpu().numpy(), info.cpu().numpy()))
    gpu.close()
    return out


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("name", list(CASES))
def test_solve_returns_the_recorded_bits(name, bits, torch_cuda, golden):
    got = _solve_all(torch_cuda, golden, name, bits)
    for i, (u, w, info) in enumerate(got):
        tag = f"{name}_fp{bits}_s{i}_"
        print(tag, "info", info.tolist())
        assert np.array_equal(info, golden[tag + "info"]), (tag, info.tolist(), golden[tag + "info"].tolist())
        assert np.array_equal(_bits(u), _bits(golden[tag + "u"])), (tag, np.abs(u - golden[tag + "u"]).max())
        assert np.array_equal(_bits(w), _bits(golden[tag + "w"])), (tag, np.abs(w - golden[tag + "w"]).max())


def test_bench_like_scenes_retry_the_backward_sweep(golden):
    """The zero-start n20k8 scenes were picked on the oracle so that several of them regularise; the recorded solves did."""
    reg = golden["n20k8_fp64_s0_info"][:, 2]
    print("n20k8 zero start: regularisations per scene", reg.tolist())
    assert (reg > 0).sum() >= 3 and reg.max() >= 5


@pytest.mark.parametrize("name", list(CASES))
def test_solve_matches_oracle(name, torch_cuda, golden):
    N, K, S, _n = CASES[name]
    prm = _params(N, K)
    got = _solve_all(torch_cuda, golden, name, 64)
    cpu = [_oracle.MpcOracle(prm.T, prm.dt, prm.K) for _ in range(S)]
    for m in cpu:
        m.configure(prm)
    worst, flipped = 0.0, 0
    for i, (u, w, info) in enumerate(got):
        ref = golden[f"{name}_ref{i}"]
        for s in range(S):
            if i > 0:   # both sides start the second solve from the same point: the recorded warm start
                cpu[s].warm_start[:] = got[i - 1][1][s]
            uc, _xc, ic = cpu[s].Solve(ref[s], i == 0)
            d = max(np.abs(u[s] - uc).max(), np.abs(w[s] - cpu[s].warm_start).max())
            if np.array_equal(info[s], ic):
                worst = max(worst, d)
            else:   # rounding-level branch flip: same optimum, different counts
                flipped += 1
                assert info[s][0] == 0 and ic[0] == 0 and d <= 1e-4, (name, i, s, info[s], ic, d)
    print(f"{name}: max |gpu - oracle| = {worst:.3e}, scenes with flipped counts: {flipped}/{S * len(got)}")
    assert worst <= TOL and flipped <= 1


def test_step_returns_the_recorded_bits(torch_cuda, golden):
    """The n20k8 scenes through amk_step_batch, mpc_max_iter = 3: kNN queries -> pack -> solve, up to three passes."""
    torch = torch_cuda
    from avoid_mpc_amd.host import KdBatch, MpcBatch, step_batch
    N, K, S, _n = CASES["n20k8"]
    prm = _params(N, K); prm.max_iter = 3
    n = int(golden["step_cloud_points"])
    scenes = [synth.make_scene(n, int(seed), prm) for seed in golden["n20k8_seeds"]]
    import hashlib
    h = hashlib.sha256()
    for sc in scenes:
        h.update(np.ascontiguousarray(sc["cloud"]).tobytes()); h.update(np.ascontiguousarray(sc["edge"]).tobytes())
    assert np.array_equal(np.frombuffer(h.digest(), np.uint8), golden["step_cloud_sha256"]), \
        "the synthetic clouds are not the ones the fixture was recorded on"
    cl = np.stack([sc["cloud"] for sc in scenes]); ed = np.stack([sc["edge"] for sc in scenes])
    kd_o, kd_e = KdBatch(S, cl.shape[1]), KdBatch(S, ed.shape[1])
    kd_o.build(torch.from_numpy(cl).cuda()); kd_e.build(torch.from_numpy(ed).cuda())
    mpc = MpcBatch(prm.T, prm.dt, prm.K, S); mpc.configure(prm)
    sq = np.stack([_oracle.scene_state_quads(sc, prm) for sc in scenes])
    ref = torch.from_numpy(np.stack([sc["ref_path"] for sc in scenes])).cuda()
    pos_x = torch.from_numpy(np.array([sc["pos"][0] for sc in scenes])).cuda()
    out = step_batch(kd_o, kd_e, mpc, prm, torch.from_numpy(sq).cuda(), pos_x, ref)
    torch.cuda.synchronize()
    got = dict(u=out["u"].cpu().numpy(), x0array=out["x0array"].cpu().numpy(), flags=out["flags"].cpu().numpy(),
               ref_path=ref.cpu().numpy())
    print("step flags", got["flags"].tolist())
    assert got["flags"][:, 1].min() >= 2        # every scene re-planned: solves from a zero AND from a warm start
    for key in ("flags", "u", "x0array", "ref_path"):
        assert np.array_equal(_bits(got[key]), _bits(golden["step_" + key])), key
