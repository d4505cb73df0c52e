"""CPU: the host-side half of amk_depth_to_clouds -- the workspace query is host arithmetic (no device), monotone in the scenes and
the rows and rejects bad arguments; without a GPU the host call refuses with AMK_ERR_NO_DEVICE instead of computing anything."""
import ctypes as C

import numpy as np
import pytest

from avoid_mpc_amd import build as amk_build
from avoid_mpc_amd import capi


@pytest.fixture(scope="module")
def lib():
    amk_build.build()
    return capi.load()


def _bytes(lib, rows, cols, scale, S):
    b = C.c_longlong(-1)
    assert lib.amk_depth_clouds_work_bytes(rows, cols, scale, S, C.byref(b)) == capi.AMK_OK
    return b.value


def test_work_bytes_answers_without_a_device(lib):
    assert _bytes(lib, 480, 640, 1.0, 1) >= 8 * 480          # {obstacle, edge} count of every band, bands of one row included
    assert _bytes(lib, 480, 640, 10.0, 256) >= 8 * 48 * 256
    assert _bytes(lib, 1, 1, 1.0, 1) > 0


def test_work_bytes_is_monotone_in_scenes_and_rows(lib):
    by_scenes = [_bytes(lib, 240, 320, 1.0, S) for S in (1, 2, 3, 16, 256, 257)]
    assert by_scenes == sorted(by_scenes) and by_scenes[0] < by_scenes[-1]
    by_rows = [_bytes(lib, rows, 320, 2.0, 4) for rows in (2, 3, 4, 5, 48, 240, 480, 481, 4800)]
    assert by_rows == sorted(by_rows) and by_rows[0] < by_rows[-1]


def test_work_bytes_rejects_bad_arguments(lib):
    b = C.c_longlong(-1)
    bad = capi.AMK_ERR_INVALID_ARG
    assert lib.amk_depth_clouds_work_bytes(0, 640, 1.0, 1, C.byref(b)) == bad
    assert lib.amk_depth_clouds_work_bytes(480, -1, 1.0, 1, C.byref(b)) == bad
    assert lib.amk_depth_clouds_work_bytes(480, 640, 0.0, 1, C.byref(b)) == bad
    assert lib.amk_depth_clouds_work_bytes(480, 640, float("nan"), 1, C.byref(b)) == bad
    assert lib.amk_depth_clouds_work_bytes(4, 4, 10.0, 1, C.byref(b)) == bad       # (the down-scaled image has no pixel)
    assert lib.amk_depth_clouds_work_bytes(480, 640, 1.0, 0, C.byref(b)) == bad
    assert lib.amk_depth_clouds_work_bytes(480, 640, 1.0, 1, None) == bad
    assert b.value == -1


def test_host_call_without_a_gpu_refuses(lib):
    if lib.amk_device_count() > 0:
        pytest.skip("GPU present")
    from avoid_mpc_amd.host import depth_params
    p = depth_params(resize_scale=2.0)
    img = np.ones((60, 80), np.float32); T = np.eye(4)
    cloud = np.full((1200, 3), -7, np.float32); edge = cloud.copy(); cnt = np.full(1, -7, np.int32); ecnt = cnt.copy()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    st = lib.amk_depth_to_clouds_host(vp(img), capi.AMK_DEPTH_F32, 60, 80, 4800, 1, C.byref(p), vp(T), vp(T), vp(cloud), 3600, vp(cnt),
                                      vp(edge), 3600, vp(ecnt), 3)
    assert st == capi.AMK_ERR_NO_DEVICE
    assert (cloud == -7).all() and (edge == -7).all() and cnt[0] == -7 and ecnt[0] == -7
    assert lib.amk_depth_to_clouds_host(None, capi.AMK_DEPTH_F32, 60, 80, 4800, 1, C.byref(p), vp(T), vp(T), vp(cloud), 3600, vp(cnt),
                                        vp(edge), 3600, vp(ecnt), 3) == capi.AMK_ERR_INVALID_ARG
    assert lib.amk_depth_to_clouds_host(vp(img), 7, 60, 80, 4800, 1, C.byref(p), vp(T), vp(T), vp(cloud), 3600, vp(cnt),
                                        vp(edge), 3600, vp(ecnt), 3) == capi.AMK_ERR_UNSUPPORTED
