"""Cost of the three tie orders side by side (amk_kd_set_tie_order: 0 lowest index, 1 nanoflann's tree at every build, 2 AUTO =
the tree only where a query tied), 256 scenes:
  (a) index build and the 21-query, k = 8 search of a control-step pass at 3072 and 50 000 points per scene, tie-free clouds;
  (b) the same on clouds rounded to a 5 cm lattice (exact ties everywhere: AUTO builds every tree, behind its first search);
  (c) the whole single-frame step (both index builds + amk_step_batch, C2 size, K = 8, cold start) on tie-free scenes.
A cycle = build + search (or builds + step) is what a frame costs; AUTO pays for its trees inside the search, so cycles are the
comparable figure.  Wall clock around work that ends in a device synchronise, REPS repetitions after a warm-up, the modes
alternated inside every repetition; mode 0 is measured three times per section (its spread is the run-to-run noise of the box).
Usage: python tools/experiments/tie_auto_cost.py [output file]   (default profiles/tie_auto_cost.txt)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from avoid_mpc_amd import capi, fsm, synth
from avoid_mpc_amd.host import KdBatch, MpcBatch, kd_build_pair, step_batch

S, REPS, WARM = 256, 12, 3
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def med(v):
    return float(np.median(v))


def kd_section(n, lattice):
    base = torch.from_numpy(synth.make_cloud(n, 7)[0]).cuda()
    cl = torch.stack([base[torch.randperm(n, device="cuda")] for _ in range(S)]).contiguous()
    qs = torch.rand((S, 21, 3), dtype=torch.float64, device="cuda") * torch.tensor([20.0, 6.0, 3.0], dtype=torch.float64, device="cuda")
    if lattice:
        cl = (torch.round(cl * 20) / 20).contiguous()
        qs = cl[:, :21, :].to(torch.float64).contiguous()   # queries at cloud points, as the control step's snapped points are
    legs = [("0", 0), ("0'", 0), ("0''", 0), ("1", 1), ("2", 2)]
    kds, outs = {}, {}
    for name, mode in legs:
        kd = KdBatch(S, n); kd.set_tie_order(mode); kd.build(cl)
        outs[name] = kd.search(qs, 8); kds[name] = kd
    torch.cuda.synchronize()
    t = {name: dict(build=[], search=[], cycle=[]) for name, _ in legs}
    for rep in range(WARM + REPS):
        for name, _ in legs:
            kd, r = kds[name], outs[name]
            cyc = timed(lambda: (kd.build(cl), kd.search(qs, 8, out=r)))
            b = timed(lambda: kd.build(cl))
            kd.search(qs, 8, out=r)                         # (AUTO: the trees of this cloud exist from here on)
            s = timed(lambda: kd.search(qs, 8, out=r))
            if rep >= WARM:
                t[name]["build"].append(b); t[name]["search"].append(s); t[name]["cycle"].append(cyc)
    status = kds["2"].exact_status().cpu().numpy()
    flagged = int((status != capi.AMK_EXACT_NOT_NEEDED).sum())
    same = all(torch.equal(outs["2"][k], outs["1"][k]) for k in ("indices", "sqdist", "pts", "counts"))
    say(f"n = {n} x {S} scenes, {'5 cm lattice' if lattice else 'tie-free'} clouds; AUTO built a tree for {flagged}/{S} scenes; "
        f"AUTO == mode 1 bit for bit: {same}")
    say("  mode   build ms   search ms (steady)   build + search ms (median of %d; min .. max of the cycle)" % REPS)
    for name, _ in legs:
        v = t[name]
        say(f"  {name:<5} {med(v['build']):9.3f} {med(v['search']):12.3f} {med(v['cycle']):22.3f}   ({min(v['cycle']):.3f} .. {max(v['cycle']):.3f})")
    c0 = [med(t[nm]["cycle"]) for nm in ("0", "0'", "0''")]
    spread = (max(c0) - min(c0)) / med(c0)
    say(f"  run-to-run spread (three mode-0 legs, cycle medians): {100 * spread:.1f} %;  AUTO / mode 0 = {med(t['2']['cycle']) / med(c0):.3f},  "
        f"AUTO / mode 1 = {med(t['2']['cycle']) / med(t['1']['cycle']):.3f},  mode 1 / mode 0 = {med(t['1']['cycle']) / med(c0):.3f}")
    say()
    for kd in kds.values():
        kd.close()
    return dict(spread=spread, auto_over_1=med(t["2"]["cycle"]) / med(t["1"]["cycle"]))


def step_section():
    c = synth.CONFIGS["C2"]
    n = c["n"]
    prm = synth.MpcParams(T=c["T"], K=c["K"])
    dev = torch.device("cuda"); N = prm.N
    clouds, edges = synth.make_clouds_torch(n, S, 4242, dev)
    sq = np.zeros((S, prm.max_iter, 10)); ref0 = np.zeros((S, N, 10)); posx = np.zeros(S)
    for s in range(S):
        pos, vel, acc, yaw = synth.make_odom(4242 + s, prm)
        sq[s] = fsm.state_quads(pos, vel, acc, yaw, prm.decay, prm.max_iter)
        ref0[s] = synth.make_ref_path(pos, prm); posx[s] = pos[0]
    sq = torch.from_numpy(sq).to(dev); ref0 = torch.from_numpy(ref0).to(dev); posx = torch.from_numpy(posx).to(dev)
    legs = [("0", 0), ("0'", 0), ("0''", 0), ("1", 1), ("2", 2)]
    st = {}
    for name, mode in legs:
        kd_o, kd_e = KdBatch(S, n), KdBatch(S, edges.shape[1])
        kd_o.set_tie_order(mode); kd_e.set_tie_order(mode)
        mpc = MpcBatch(prm.T, prm.dt, prm.K, S); mpc.configure(prm)
        out = dict(u=torch.empty((S, 4), dtype=torch.float64, device=dev), x0array=torch.empty((S, N, 14), dtype=torch.float64, device=dev),
                   flags=torch.empty((S, 4), dtype=torch.int32, device=dev))
        st[name] = dict(kd_o=kd_o, kd_e=kd_e, mpc=mpc, out=out, ref=ref0.clone(), cycle=[], step=[])

    def builds(x):
        kd_build_pair(x["kd_o"], clouds, x["kd_e"], edges)

    def step(x):
        x["ref"].copy_(ref0); x["mpc"].reset_warm_start()      # cold: every repetition solves the same problem
        step_batch(x["kd_o"], x["kd_e"], x["mpc"], prm, sq, posx, x["ref"], out=x["out"])

    for rep in range(WARM + REPS):
        for name, _ in legs:
            x = st[name]
            cyc = timed(lambda: (builds(x), step(x)))
            builds(x); torch.cuda.synchronize()
            s_ = timed(lambda: step(x))
            if rep >= WARM:
                x["cycle"].append(cyc); x["step"].append(s_)
    same0 = all(torch.equal(st["2"]["out"][k], st["0"]["out"][k]) for k in ("u", "x0array", "flags"))
    need = int((st["2"]["kd_o"].exact_status() != capi.AMK_EXACT_NOT_NEEDED).sum()) + int((st["2"]["kd_e"].exact_status() != capi.AMK_EXACT_NOT_NEEDED).sum())
    say(f"single-frame step, {S} scenes, C2 ({n}-point clouds, N = {N}, K = {prm.K}), cold start, tie-free scenes; AUTO built {need} trees; "
        f"AUTO == mode 0 bit for bit: {same0}")
    say("  mode   step ms (after the builds)   builds + step ms (median of %d; min .. max)   scenes/s of the cycle" % REPS)
    for name, _ in legs:
        x = st[name]
        say(f"  {name:<5} {med(x['step']):12.3f} {med(x['cycle']):28.3f}   ({min(x['cycle']):.3f} .. {max(x['cycle']):.3f}) {S / med(x['cycle']) * 1e3:14.0f}")
    c0 = [med(st[nm]["cycle"]) for nm in ("0", "0'", "0''")]; s0 = [med(st[nm]["step"]) for nm in ("0", "0'", "0''")]
    spread = (max(c0) - min(c0)) / med(c0)
    say(f"  run-to-run spread (three mode-0 legs, cycle medians): {100 * spread:.1f} %")
    say(f"  cycle: AUTO / mode 0 = {med(st['2']['cycle']) / med(c0):.3f},  AUTO / mode 1 = {med(st['2']['cycle']) / med(st['1']['cycle']):.3f},  mode 1 / mode 0 = {med(st['1']['cycle']) / med(c0):.3f}")
    say(f"  step alone: AUTO / mode 0 = {med(st['2']['step']) / med(s0):.3f},  AUTO / mode 1 = {med(st['2']['step']) / med(st['1']['step']):.3f}")
    say()


def main():
    assert torch.cuda.is_available(), "this measurement needs the GPU: there is no CPU fallback"
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "tie_auto_cost.txt")
    say(f"tie order cost, {torch.cuda.get_device_name(0)}; wall clock around synchronised work, median of {REPS} after {WARM} warm-up repetitions")
    say()
    say("(a) tie-free clouds")
    for n in (3072, 50000):
        kd_section(n, False)
    say("(b) clouds on a 5 cm lattice")
    for n in (3072, 50000):
        kd_section(n, True)
    say("(c) the control step")
    step_section()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
