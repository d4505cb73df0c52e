"""Two builds of the library on the same inputs, bit for bit: the MPC's solve, control step and NLP evaluation.

    python tools/experiments/mpc_host_bits.py --parent scratch/ab/libA.so [--branch avoid_mpc_amd/libavoid_mpc_amd.so] [--out FILE]

Each library is loaded in a child process of its own (one HIP runtime, one library per process) and fed the same inputs: 16 scenes at
C1 (N = 10, its own instantiation) and at N = 7 (the generic one), the solve and the step in fp64 and in fp32.  The parent runs twice.
  amk_mpc_solve (u, x0array, info, warm start) and one amk_step_batch step (u, x0array, flags, ref_path, the packed scene records):
      branch == parent, np.array_equal.
  amk_mpc_eval and amk_mpc_eval_gamma: an output the parent reproduces bit for bit against itself must be bit-equal on the branch; one it
      does not (evaluate accumulates through LDS) is held to tests/test_mpc_eval_gpu.py's RTOL of the largest entry.
  the tau block of grad_p gamma is exempt from bit equality (its derivative part may move in the last bit when the model's RK4 changes
      `* (1.0 / 6)` for `/ 6`): tests/test_casadi_plugin_gpu.py's 1e-5 for grad_gamma_p, relative to the block's largest entry.
Exit status 1 when any of that fails."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
S = 16
RTOL_EVAL, RTOL_TAU = 1e-9, 1e-5


def shapes():
    from avoid_mpc_amd import synth
    c1 = synth.CONFIGS["C1"]
    return {"C1": synth.MpcParams(T=c1["T"], K=c1["K"]), "N7": synth.MpcParams(T=7 * 0.033 + 1e-4, K=3)}


def child(lib_path, out_path):
    from avoid_mpc_amd import capi
    capi.LIB_PATH = os.path.abspath(lib_path)
    import ctypes as C
    import torch
    from avoid_mpc_amd import synth
    from avoid_mpc_amd.host import KdBatch, MpcBatch, step_batch
    from tests import _oracle
    from tests.test_mpc_eval_gpu import _points_at
    out = {}
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for tag, prm in shapes().items():
        N, K = prm.N, prm.K
        _, W, R = _points_at(prm, S, 21)
        scenes = [synth.make_scene(5000, 900 + i, prm) for i in range(S)]
        nmax, emax = max(len(sc["cloud"]) for sc in scenes), max(max(len(sc["edge"]) for sc in scenes), 1)
        cl = np.zeros((S, nmax, 3), np.float32); ed = np.zeros((S, emax, 3), np.float32)
        cn = np.array([len(sc["cloud"]) for sc in scenes], np.int32); en = np.array([len(sc["edge"]) for sc in scenes], np.int32)
        for s, sc in enumerate(scenes):
            cl[s, :cn[s]] = sc["cloud"]; ed[s, :en[s]] = sc["edge"]
        sq = np.stack([_oracle.scene_state_quads(sc, prm) for sc in scenes])
        for bits in (64, 32):
            key = f"{tag}/fp{bits}/"
            m = MpcBatch(prm.T, prm.dt, prm.K, S); m.configure(prm); m.set_precision(bits)
            u, x0, info = m.Solve(torch.from_numpy(R).cuda(), faster=True)
            w = m.get_warm_start()
            torch.cuda.synchronize()
            out.update({key + "solve.u": u.cpu().numpy(), key + "solve.x0array": x0.cpu().numpy(), key + "solve.info": info.cpu().numpy(),
                        key + "solve.warm_start": w.cpu().numpy()})
            kd_o, kd_e = KdBatch(S, nmax), KdBatch(S, emax)
            kd_o.build(torch.from_numpy(cl).cuda(), torch.from_numpy(cn).cuda()); kd_e.build(torch.from_numpy(ed).cuda(), torch.from_numpy(en).cuda())
            m2 = MpcBatch(prm.T, prm.dt, prm.K, S); m2.configure(prm); m2.set_precision(bits)
            ref = torch.from_numpy(np.stack([sc["ref_path"] for sc in scenes])).cuda()
            pos_x = torch.from_numpy(np.array([sc["pos"][0] for sc in scenes])).cuda()
            st = step_batch(kd_o, kd_e, m2, prm, torch.from_numpy(sq).cuda(), pos_x, ref)
            torch.cuda.synchronize()
            out.update({key + "step." + k: st[k].cpu().numpy() for k in ("u", "x0array", "flags")})
            out[key + "step.ref_path"] = ref.cpu().numpy()
            out[key + "step.ref_states"] = np.asarray(m2.ref_states())
            if bits == 32:
                continue   # the evaluation kernels are fp64 whatever the solve's arithmetic
            lam_f = np.linspace(0.5, 2.0, S); lam_g = np.random.default_rng(22).normal(size=(S, 10 + 10 * N))
            ev = m.eval(torch.from_numpy(W).cuda(), torch.from_numpy(R).cuda(), torch.from_numpy(lam_f).cuda())
            torch.cuda.synchronize()
            out.update({f"{tag}/eval.{k}": v.cpu().numpy() for k, v in ev.items()})
            gx = np.zeros((S, 10 + 14 * N)); gp = np.zeros((S, R.shape[1] + 34))
            assert m.lib.amk_mpc_eval_gamma_host(m.h, vp(W), vp(R), vp(lam_f), vp(lam_g), vp(gx), vp(gp)) == 0
            out[f"{tag}/gamma.grad_x"] = gx
            out[f"{tag}/gamma.grad_p.tau"] = gp[:, -30:-26].copy()
            gp[:, -30:-26] = 0.0
            out[f"{tag}/gamma.grad_p.rest"] = gp
    np.savez(out_path, **out)


def run_child(lib, path):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, path], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.exit(f"child on {lib} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return dict(np.load(path))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.path.join(ROOT, "scratch", "ab", "libA.so"))
    ap.add_argument("--branch", default=os.path.join(ROOT, "avoid_mpc_amd", "libavoid_mpc_amd.so"))
    ap.add_argument("--out")
    ap.add_argument("--child", nargs=2)
    a = ap.parse_args()
    if a.child:
        return child(*a.child)
    with tempfile.TemporaryDirectory() as d:
        p1, p2, br = (run_child(lib, os.path.join(d, f"{i}.npz")) for i, lib in enumerate((a.parent, a.parent, a.branch)))
    lines, bad = [f"parent {a.parent}  branch {a.branch}  {S} scenes per shape; max |branch - parent| / max |parent| where not 0"], 0
    for k in sorted(p1):
        same = np.array_equal(p1[k], br[k], equal_nan=True)
        scale = max(np.abs(p1[k]).max(), 1e-300) if p1[k].dtype.kind == "f" else 1
        rel = 0.0 if same else float(np.abs(br[k].astype(np.float64) - p1[k]).max() / scale)
        if "solve." in k or "step." in k:
            ok, rule = same, "bit-equal"
        elif k.endswith("grad_p.tau"):
            ok, rule = rel <= RTOL_TAU, f"exempt, <= {RTOL_TAU:g}"
        elif np.array_equal(p1[k], p2[k], equal_nan=True):
            ok, rule = same, "parent reproduces itself: bit-equal"
        else:
            ok, rule = rel <= RTOL_EVAL, f"parent does not reproduce itself: <= {RTOL_EVAL:g}"
        bad += not ok
        lines.append(f"{'ok  ' if ok else 'FAIL'} {k:34s} {str(p1[k].shape):16s} {'identical' if same else f'rel {rel:.3e}':16s} ({rule})")
    lines.append(f"{len(p1)} outputs, {bad} failed")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
