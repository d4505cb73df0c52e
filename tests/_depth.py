"""What the depth tests share (tests/test_depth_gpu.py, tests/test_depth_clouds_gpu.py): the camera mounting, random poses and the
wall-with-a-box scene.  Every function draws from the caller's generator, in a fixed order."""
import numpy as np

TBC = np.array([[0, 0, 1, 0.1], [-1, 0, 0, 0.0], [0, -1, 0, 0.05], [0, 0, 0, 1.0]])


def poses(rng, S):
    out = np.zeros((S, 4, 4))
    for s in range(S):
        th = rng.uniform(-np.pi, np.pi)
        out[s] = [[np.cos(th), -np.sin(th), 0, rng.uniform(-5, 5)], [np.sin(th), np.cos(th), 0, rng.uniform(-5, 5)],
                  [0, 0, 1, rng.uniform(0.5, 3)], [0, 0, 0, 1]]
    return out


def wall_scene(rng, shape, dtype):
    """A wall at 20 m with noise, a near box, 2 % invalid pixels; uint16 millimetres or float32 metres."""
    rows, cols = shape
    d = np.full(shape, 20.0) + rng.normal(0, 0.02, shape)
    r0, c0 = rng.integers(2, rows // 2), rng.integers(2, cols // 2)
    d[r0:r0 + rows // 3, c0:c0 + cols // 3] = rng.uniform(2, 8)
    d[rng.random(shape) < 0.02] = 0.0
    return np.round(d * 1000).astype(np.uint16) if dtype == np.uint16 else d.astype(np.float32)
