"""Records tests/golden/mpc_riccati_transport.npz: inputs and outputs of MpcBatch.Solve and of one amk_step_batch for
tests/test_mpc_riccati_transport_gpu.py, which pins a library bit for bit to the one that recorded them.

  python tools/record_riccati_transport.py --inputs FILE    (CPU) picks the scenes on the oracle, writes the inputs
  python tools/record_riccati_transport.py --record FILE    (GPU) runs the built library on them, adds the outputs

The fixture in the tree was recorded from the library of the commit BEFORE the forward roll's prefetch ring and the wave
reductions were rescheduled; record it again only from a library whose results are meant to become the new pin.

Solve cases (name: N, K, scenes): every one from a zero warm start (faster = True), `n20k8` also a second solve on the second
re-plan pass's problem from the first solve's warm start; each in fp64 and fp32.  The n20k8 scenes are chosen so that at least
three of them regularise (info[2] > 0 on the oracle): their inertia loop runs the backward sweep more than once per iteration.
The step case runs the n20k8 scenes (clouds regenerated from the seeds by avoid_mpc_amd.synth) through amk_step_batch."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from avoid_mpc_amd import synth  # noqa: E402
from tests import _oracle  # noqa: E402

DT = 0.033
# name -> (N, K, scenes, cloud points, first seed to try)
CASES = {"n20k8": (20, 8, 6, 20000, 200), "n10k3": (10, 3, 6, 5000, 200), "n30k3": (30, 3, 4, 5000, 200),
         "n7k3": (7, 3, 4, 5000, 400), "n3k3": (3, 3, 4, 5000, 400), "n2k8": (2, 8, 4, 5000, 400)}
STEP_CASE = "n20k8"


def params(N, K):
    prm = synth.MpcParams(T=N * DT + 1e-4, K=K)
    assert prm.N == N
    return prm


def scene_log(n, seed, prm):
    """The P vectors (ref_states) of every re-plan pass of the oracle's own control step on the scene."""
    sc = synth.make_scene(n, seed, prm)
    kd, ke = _oracle.kd_oracle(sc["cloud"]), _oracle.kd_oracle(sc["edge"])
    mpc = _oracle.MpcOracle(prm.T, prm.dt, prm.K); mpc.configure(prm)
    r = _oracle.step_oracle(kd, ke, mpc, prm, _oracle.scene_state_quads(sc, prm), sc["pos"][0], sc["ref_path"].copy(),
                            want_log=True)
    return sc, r["ref_log"][:r["flags"][1]]


def cloud_digest(scenes):
    h = hashlib.sha256()
    for sc in scenes:
        h.update(np.ascontiguousarray(sc["cloud"]).tobytes()); h.update(np.ascontiguousarray(sc["edge"]).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def make_inputs(path):
    out = {}
    for name, (N, K, S, n, seed0) in CASES.items():
        prm = params(N, K)
        picked, seed = [], seed0
        want_reg = 3 if name == STEP_CASE else 0
        while len(picked) < S:
            sc, log = scene_log(n, seed, prm)
            seed += 1
            if len(log) < 2:
                continue
            m = _oracle.MpcOracle(prm.T, prm.dt, prm.K); m.configure(prm)
            _u, _x, info = m.Solve(log[0], True)
            reg = info[2] > 0
            have_reg = sum(p[3] for p in picked)
            if not reg and S - len(picked) <= want_reg - have_reg:
                continue   # the remaining places are for scenes that regularise
            picked.append((seed - 1, sc, log, bool(reg), info.copy()))
            print(name, "seed", seed - 1, "passes", len(log), "oracle info", info, flush=True)
        assert sum(p[3] for p in picked) >= want_reg
        out[name + "_seeds"] = np.array([p[0] for p in picked], np.int64)
        out[name + "_ref0"] = np.stack([p[2][0] for p in picked])
        if name == STEP_CASE:
            out[name + "_ref1"] = np.stack([p[2][1] for p in picked])
            out["step_cloud_points"] = np.int64(n)
            out["step_cloud_sha256"] = cloud_digest([p[1] for p in picked])
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


def record(path):
    import torch
    from avoid_mpc_amd.host import KdBatch, MpcBatch, step_batch
    z = dict(np.load(path))
    for name, (N, K, S, n, _seed0) in CASES.items():
        prm = params(N, K)
        for bits in (64, 32):
            gpu = MpcBatch(prm.T, prm.dt, prm.K, S); gpu.configure(prm); gpu.set_precision(bits)
            refs = [z[name + "_ref0"]] + ([z[name + "_ref1"]] if name == STEP_CASE else [])
            for i, ref in enumerate(refs):
                u, _x0, info = gpu.Solve(torch.from_numpy(ref).cuda(), faster=(i == 0))
                torch.cuda.synchronize()
                tag = f"{name}_fp{bits}_s{i}_"
                z[tag + "u"] = u.cpu().numpy(); z[tag + "info"] = info.cpu().numpy()
                z[tag + "w"] = gpu.get_warm_start().cpu().numpy()
                print(tag, "info", z[tag + "info"].tolist(), flush=True)
            gpu.close()
    # one control step of the n20k8 scenes, three re-plan passes at the most
    N, K, S, n, _ = CASES[STEP_CASE]
    prm = params(N, K); prm.max_iter = 3
    scenes = [synth.make_scene(n, int(s), prm) for s in z[STEP_CASE + "_seeds"]]
    assert np.array_equal(cloud_digest(scenes), z["step_cloud_sha256"])
    got = run_step(torch, scenes, prm)
    for k, v in got.items():
        z["step_" + k] = v
    print("step flags", got["flags"].tolist())
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path), "bytes")


def run_step(torch, scenes, prm):
    from avoid_mpc_amd.host import KdBatch, MpcBatch, step_batch
    S = len(scenes)
    cl = np.stack([sc["cloud"] for sc in scenes]); ed = np.stack([sc["edge"] for sc in scenes])
    kd_o, kd_e = KdBatch(S, cl.shape[1]), KdBatch(S, ed.shape[1])
    kd_o.build(torch.from_numpy(cl).cuda()); kd_e.build(torch.from_numpy(ed).cuda())
    mpc = MpcBatch(prm.T, prm.dt, prm.K, S); mpc.configure(prm)
    sq = np.stack([_oracle.scene_state_quads(sc, prm) for sc in scenes])
    ref = torch.from_numpy(np.stack([sc["ref_path"] for sc in scenes])).cuda()
    pos_x = torch.from_numpy(np.array([sc["pos"][0] for sc in scenes])).cuda()
    out = step_batch(kd_o, kd_e, mpc, prm, torch.from_numpy(sq).cuda(), pos_x, ref)
    torch.cuda.synchronize()
    return dict(u=out["u"].cpu().numpy(), x0array=out["x0array"].cpu().numpy(), flags=out["flags"].cpu().numpy(),
                ref_path=ref.cpu().numpy())


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--inputs":
        make_inputs(sys.argv[2])
    elif len(sys.argv) == 3 and sys.argv[1] == "--record":
        record(sys.argv[2])
    else:
        sys.exit(__doc__)
