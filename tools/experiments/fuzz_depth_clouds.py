"""Randomised cross-check of amk_depth_to_clouds (csrc/depth.hip: both clouds of a depth frame, tiled into bands of rows above
AMK_EDGE_MAX_PIXELS or when amk__depth_set_band_rows says so) against oracle/depth_oracle.c: random image sizes (odd, tiny, wide,
640 x 480 at scale 1 and 2), resize scales, pixel types, holes / out-of-range / non-finite pixels, empty scenes and scenes whose only
valid pixels lie in a few rows, random band heights (0 = the dispatch as built), Twc != Twb, stride 3 / 4; both clouds must have the
oracle's count, order and float bits.
usage: python tools/experiments/fuzz_depth_clouds.py [seed] [seconds]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from tests import _oracle
from avoid_mpc_amd import capi
from avoid_mpc_amd.host import depth_params, depth_to_clouds

rng = np.random.default_rng(int(sys.argv[1]) if len(sys.argv) > 1 else 1)
t_end = time.time() + (float(sys.argv[2]) if len(sys.argv) > 2 else 60.0)
lib = capi.load()
TBC = np.array([[0, 0, 1, 0.1], [-1, 0, 0, 0.0], [0, -1, 0, 0.05], [0, 0, 0, 1.0]])


def poses(S):
    th = rng.uniform(-np.pi, np.pi, S)
    T = np.zeros((S, 4, 4))
    for s in range(S):
        T[s] = [[np.cos(th[s]), -np.sin(th[s]), 0, rng.uniform(-50, 50)], [np.sin(th[s]), np.cos(th[s]), 0, rng.uniform(-50, 50)],
                [0, 0, 1, rng.uniform(0.5, 3)], [0, 0, 0, 1]]
    return T


it = bad = frames = tiled = 0
try:
    while time.time() < t_end:
        it += 1
        rows, cols = int(rng.integers(1, 200)), int(rng.integers(1, 260))
        if rng.random() < 0.15:
            rows, cols = 480, 640
        scale = float(rng.choice([1.0, 2.0, 2.5, 3.0, 4.0, 7.3, 10.0]))
        W, H = int(cols / scale), int(rows / scale)
        if H < 1 or W < 1:
            continue
        dtype = np.uint16 if rng.random() < 0.5 else np.float32
        S = int(rng.integers(1, 5))
        far = float(rng.choice([5.0, 30.0, 90.0]))
        imgs = []
        for s in range(S):
            d = rng.uniform(0.05, far, (rows, cols))
            if rng.random() < 0.6:   # piecewise-constant walls: real edges for Canny
                d = np.kron(rng.uniform(0.3, far, (rows // 16 + 1, cols // 16 + 1)), np.ones((16, 16)))[:rows, :cols]
            d[rng.random((rows, cols)) < 0.1] = 0.0
            d[rng.random((rows, cols)) < 0.05] = 150.0
            u = rng.random()
            if u < 0.1:
                d[:] = 0.0                                        # an empty scene
            elif u < 0.25:
                keep = int(rng.integers(0, rows))                 # valid pixels in a few rows only
                d[:keep] = 0.0; d[keep + int(rng.integers(1, 4)):] = 0.0
            if dtype == np.uint16:
                imgs.append(np.round(np.minimum(d, 65.0) * 1000).astype(np.uint16))
            else:
                d = d.astype(np.float32)
                m = rng.random((rows, cols))
                d[m < 0.01] = np.nan; d[(m >= 0.01) & (m < 0.02)] = np.inf; d[(m >= 0.02) & (m < 0.03)] = -1.0
                imgs.append(d)
        imgs = np.stack(imgs)
        Twb, Twc = poses(S), poses(S)
        prm = dict(pixel2meter=1e-3 if dtype == np.uint16 else 1.0, depth_min=float(rng.choice([0.1, 0.5])), depth_max=float(rng.choice([10.0, 100.0])),
                   resize_scale=scale, fx=float(rng.uniform(100, 400)), fy=float(rng.uniform(100, 400)), cx=cols / 2.0 + rng.uniform(-3, 3),
                   cy=rows / 2.0 + rng.uniform(-3, 3), Tbc=TBC)
        band = int(rng.choice([0, 0, 1, 2, 3, 4, 5, 7, 8, 16, 17, 64]))
        tiled += band > 0 or W * H > 16000
        lib.amk__depth_set_band_rows(band)
        dev = torch.from_numpy(imgs.view(np.int16) if dtype == np.uint16 else imgs).cuda()
        cloud, counts, edge, ecounts = depth_to_clouds(dev, depth_params(**prm), torch.from_numpy(Twb).cuda(), torch.from_numpy(Twc).cuda(),
                                                       point_stride=int(rng.choice([3, 4])))
        torch.cuda.synchronize()
        cloud, counts, edge, ecounts = (t.cpu().numpy() for t in (cloud, counts, edge, ecounts))
        for s in range(S):
            frames += 1
            ref, _ = _oracle.depth_oracle(imgs[s], prm, Twb[s])
            eref = _oracle.depth_edge_oracle(imgs[s], prm, Twc[s])[0] if len(ref) else ref[:0]
            ok = counts[s] == len(ref) and np.array_equal(cloud[s, :counts[s], :3].view(np.uint32), ref.view(np.uint32))
            oke = ecounts[s] == len(eref) and np.array_equal(edge[s, :ecounts[s], :3].view(np.uint32), eref.view(np.uint32))
            if not (ok and oke):
                bad += 1
                print("MISMATCH", it, rows, cols, scale, dtype.__name__, "band", band, "scene", s, "cloud", ok, counts[s], len(ref),
                      "edge", oke, ecounts[s], len(eref), flush=True)
finally:
    lib.amk__depth_set_band_rows(0)
print("fuzz iterations", it, "tiled", tiled, "frames checked", frames, "mismatches", bad)
sys.exit(1 if bad else 0)
