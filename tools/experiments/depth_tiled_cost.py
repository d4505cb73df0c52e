"""Cost of amk_depth_to_clouds (both clouds; above AMK_EDGE_MAX_PIXELS on the tiled kernels, one workgroup per band of rows) against
amk_depth_to_cloud alone (the obstacle cloud only, one workgroup per scene) -- the only part of the work that ran above 16 000 pixels
before the tiled kernels -- and, at the reference's own 64 x 48, of the dispatch as built (the two one-block kernels) against the tiled
kernels forced by amk__depth_set_band_rows: the evidence for or against moving small frames to the tiled path.
  shape A   S = 1,   480 x 640 at scale 1    (307 200 pixels)
  shape B   S = 256, 240 x 320 at scale 1    (76 800 pixels, the frame of a 50 k-point cloud)
  shape C   S = 256 and S = 1, 480 x 640 at scale 10 (3 072 pixels)
Images: a wall at 20 m with noise, a near box, 2 % invalid pixels (uint16 millimetres).  Outputs and workspace are allocated once;
device events around a block of back-to-back calls (40 at shapes A and B, 400 at shape C: 10 ms and more per block), every side of a
shape warmed up first, the sides alternating block by block, one process; the figure is the median block over its calls.
usage: python tools/experiments/depth_tiled_cost.py [--out FILE]"""
import ctypes as C
import sys
sys.path.insert(0, ".")
import numpy as np, torch
from avoid_mpc_amd import capi
from avoid_mpc_amd.host import depth_params

BLOCKS, WARM = 9, 3
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = torch.device("cuda")
lib = capi.load()
lines = [f"amk_depth_to_clouds vs amk_depth_to_cloud; one MI355X, device events around a block of back-to-back calls, median of {BLOCKS} blocks "
         f"per side after {WARM} warm-up calls of every side, sides alternating block by block, one process; us per call (min .. max)"]


def images(S, rows, cols, seed):
    rng = np.random.default_rng(seed)
    out = np.empty((S, rows, cols), np.uint16)
    for s in range(S):
        d = np.full((rows, cols), 20.0) + rng.normal(0, 0.02, (rows, cols))
        r0, c0 = rng.integers(2, rows // 2), rng.integers(2, cols // 2)
        d[r0:r0 + rows // 3, c0:c0 + cols // 3] = rng.uniform(2, 8)
        d[rng.random((rows, cols)) < 0.02] = 0.0
        out[s] = np.round(d * 1000)
    return out


def shape(name, S, rows, cols, scale, calls, sides):
    """sides: list of (label, kind, band_rows) with kind 'obstacle' (amk_depth_to_cloud) or 'both' (amk_depth_to_clouds)"""
    p = depth_params(pixel2meter=1e-3, resize_scale=scale, fx=cols / 2.0, fy=cols / 2.0, cx=cols / 2.0, cy=rows / 2.0)
    w, h, nbytes = C.c_int(), C.c_int(), C.c_longlong()
    capi.check(lib.amk_depth_out_size(rows, cols, scale, C.byref(w), C.byref(h)), "amk_depth_out_size")
    capi.check(lib.amk_depth_clouds_work_bytes(rows, cols, scale, S, C.byref(nbytes)), "amk_depth_clouds_work_bytes")
    cap = w.value * h.value
    img = torch.from_numpy(images(min(S, 8), rows, cols, 7).view(np.int16)).to(dev).repeat((S + 7) // 8, 1, 1)[:S].contiguous()
    T = torch.eye(4, dtype=torch.float64, device=dev).repeat(S, 1, 1).contiguous()
    cloud = torch.zeros((S, cap, 3), dtype=torch.float32, device=dev); edge = torch.zeros_like(cloud)
    cnt = torch.zeros(S, dtype=torch.int32, device=dev); ecnt = torch.zeros_like(cnt)
    work = torch.empty((nbytes.value + 7) // 8, dtype=torch.int64, device=dev)
    st = capi.stream_ptr(None)
    d = capi.dptr

    def call(kind, band):
        lib.amk__depth_set_band_rows(band)
        if kind == "obstacle":
            rc = lib.amk_depth_to_cloud(d(img), capi.AMK_DEPTH_U16, rows, cols, rows * cols, S, C.byref(p), d(T), d(cloud), 3, cap * 3, d(cnt), st)
        else:
            rc = lib.amk_depth_to_clouds(d(img), capi.AMK_DEPTH_U16, rows, cols, rows * cols, S, C.byref(p), d(T), d(T), d(cloud), cap * 3,
                                         d(cnt), d(edge), cap * 3, d(ecnt), 3, d(work), work.numel() * 8, st)
        capi.check(rc, kind)

    try:
        for _, kind, band in sides:
            for _ in range(WARM):
                call(kind, band)
        torch.cuda.synchronize()
        times = [[] for _ in sides]
        for b in range(BLOCKS):
            order = range(len(sides)) if b % 2 == 0 else reversed(range(len(sides)))
            for i in order:
                a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(calls):
                    call(sides[i][1], sides[i][2])
                z.record(); z.synchronize()
                times[i].append(a.elapsed_time(z) * 1e3 / calls)
    finally:
        lib.amk__depth_set_band_rows(0)
    lines.append(f"{name}: S = {S}, {rows} x {cols} at scale {scale:g} -> {w.value} x {h.value} = {cap} pixels; "
                 f"{int(cnt.sum())} obstacle and {int(ecnt.sum())} edge points; {calls} calls per block")
    base = np.median(times[0])
    for (label, _, _), t in zip(sides, times):
        lines.append(f"  {label:<58s} {np.median(t):10.1f} us   ({min(t):.1f} .. {max(t):.1f})   {np.median(t) / base:.2f} x")


OBST = ("amk_depth_to_cloud (obstacle cloud only, one workgroup/scene)", "obstacle", 0)
shape("A", 1, 480, 640, 1.0, 40, [OBST, ("amk_depth_to_clouds (both clouds, tiled, bands of 16 rows)", "both", 0)])
shape("B", 256, 240, 320, 1.0, 40, [OBST, ("amk_depth_to_clouds (both clouds, tiled, bands of 16 rows)", "both", 0)])
for S in (256, 1):
    shape("C", S, 480, 640, 10.0, 400, [("amk_depth_to_clouds as built (the two one-block kernels)", "both", 0),
                                        ("amk_depth_to_clouds forced tiled, bands of 16 rows", "both", 16),
                                        ("amk_depth_to_clouds forced tiled, bands of 4 rows", "both", 4), OBST])
text = "\n".join(lines)
print(text)
if out_path:
    open(out_path, "w").write(text + "\n")
