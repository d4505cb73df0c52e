"""Cost of amk_kfmap_set_tie_order(AMK_TIES_NANOFLANN): one control period of a keyframe map -- add_vertex + update + step -- in the
default mode and in the mode, legs alternating period by period on two maps fed the same frames.
  shape A   256 scenes x 3072-point frames (the reference's frame size), max_frame_count 100
  shape B   256 scenes x 50 k-point frames, max_frame_count 3 -- skipped when amk_kfmap_tie_order_bytes + amk_kfmap_pool_bytes of the
            two maps exceed the free memory
Frames: uniform boxes that move 0.3 m per period (every sweep rebuilds its keyframe); the clouds are tie-free, so both modes compute
the same step: the difference is the price of the trees (built behind every AddVertex and every rebuilding sweep) and of the
traversals.  HIP events around each period, median over the periods after warm-up; one process.
usage: python tools/experiments/kfmap_tie_cost.py [--out FILE]"""
import ctypes as C
import sys
sys.path.insert(0, ".")
import numpy as np, torch
from avoid_mpc_amd import capi, synth
from avoid_mpc_amd.host import KfMap, MpcBatch

S, PERIODS, WARM, STEP = 256, 24, 6, 0.3
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
dev = torch.device("cuda")
lib = capi.load()
Tbc = np.eye(4); Tbc[:3, :3] = [[0, 0, 1], [-1, 0, 0], [0, -1, 0]]        # the camera looks along body +x
cam = capi.FrameCamera(32.0, 32.0, 32.0, 24.0, 10.0, 64, 48)
prm = synth.MpcParams(T=0.66, K=8, max_iter=3)
lines = ["keyframe map, cost of AMK_TIES_NANOFLANN; one MI355X, HIP events around add_vertex + update + step of one period, "
         f"median of {PERIODS - WARM} periods after {WARM}, the two modes alternating period by period, one process"]


def shape(n, ne, max_frames):
    need, pool = C.c_longlong(), C.c_longlong()
    lib.amk_kfmap_tie_order_bytes(S, n, ne, max_frames, C.byref(need)); lib.amk_kfmap_pool_bytes(S, n, ne, max_frames, C.byref(pool))
    free = torch.cuda.mem_get_info()[0]
    head = f"S = {S} x {n}-point frames, max_frame_count {max_frames}: pools {pool.value / 2**30:.2f} GiB per map, the mode's trees {need.value / 2**30:.2f} GiB"
    if 2 * pool.value + need.value > 0.9 * free:
        lines.append(head + f" -- skipped, {free / 2**30:.1f} GiB free")
        return
    maps = {0: KfMap(S, n, ne, max_frames, 0.1, 10, 0.1, Tbc), 1: KfMap(S, n, ne, max_frames, 0.1, 10, 0.1, Tbc)}
    maps[1].set_tie_order(capi.AMK_TIES_NANOFLANN)
    mpcs = {m: MpcBatch(prm.T, prm.dt, prm.K, S) for m in maps}
    for m in mpcs.values():
        m.configure(prm)
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    box = lambda k, d: (torch.rand((S, k, 3), generator=g, device=dev) * torch.tensor([20.0, 20.0, 5.0], device=dev)
                        + torch.tensor([d + 2.0, -10.0, 0.0], device=dev)).contiguous()
    scs = [synth.make_scene(100, 1 + s, prm) for s in range(S)]
    from tests import _oracle
    times = {0: [], 1: []}
    for t in range(PERIODS):
        d = STEP * t
        cloud, edge = box(n, d), box(ne, d)
        Twc = np.tile(Tbc, (S, 1, 1)); Twc[:, 0, 3] = d; Twc[:, 2, 3] = 1.5
        Tw = torch.from_numpy(Twc).to(dev)
        sq = np.stack([_oracle.scene_state_quads(sc, prm) for sc in scs]); sq[:, :, 0] += d
        ref = np.stack([sc["ref_path"] for sc in scs]); ref[:, :, 0] += d
        px = np.array([sc["pos"][0] + d for sc in scs])
        dsq, dpx = torch.from_numpy(sq).to(dev), torch.from_numpy(px).to(dev)
        for mode in ((0, 1) if t % 2 == 0 else (1, 0)):
            dref = torch.from_numpy(ref.copy()).to(dev)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            maps[mode].add_vertex(cloud, edge, Tw)
            maps[mode].update()
            maps[mode].step(mpcs[mode], prm, dsq, dpx, dref, cam=cam)
            b.record(); b.synchronize()
            if t >= WARM:
                times[mode].append(a.elapsed_time(b))
    st = maps[1].exact_status()
    nq = maps[1].state()["n_query_frames"]
    in_use = int((st["obs"] == capi.AMK_EXACT_IN_USE).sum()), int((st["obs"] != capi.AMK_EXACT_OFF).sum())
    m0, m1 = np.median(times[0]), np.median(times[1])
    lines.append(head + f"; {nq.min()} .. {nq.max()} query frames per scene, {in_use[0]} of {in_use[1]} present obstacle frames answer from their tree")
    lines.append(f"  default        {m0:8.3f} ms per period   ({min(times[0]):.3f} .. {max(times[0]):.3f})")
    lines.append(f"  AMK_TIES_NANOFLANN {m1:8.3f} ms per period   ({min(times[1]):.3f} .. {max(times[1]):.3f})   {m1 / m0:.2f} x")
    for m in maps.values():
        m.close()


shape(3072, 512, 100)
shape(50000, 5000, 3)
text = "\n".join(lines)
print(text)
if out_path:
    open(out_path, "w").write(text + "\n")
