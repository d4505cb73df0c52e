"""CPU: the interface of amk_kfmap_set_tie_order -- the three calls are in the header and in capi, and amk_kfmap_tie_order_bytes is
host arithmetic (it needs no device) that equals a restatement of what the setter allocates."""
import ctypes as C
import os

import pytest

from avoid_mpc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("amk_kfmap_set_tie_order", "amk_kfmap_tie_order_bytes", "amk_kfmap_exact_status_host")


def tie_order_bytes(S, max_points, max_edge_points, max_frame_count):
    """the tree's arrays (amk::ExactStore, csrc/kd_exact.hip) for both pools of (max_frame_count + 2) * S scenes, and the edge pool's planes"""
    scenes = (max_frame_count + 2) * S

    def tree(mp):
        cap = (mp + 255) // 256 * 256 + 1024          # amk_kd_create
        nodes = cap // 2 + 64                         # ex_max_nodes
        per_point = 4 + 4 + 4 + 12                    # vAcc_, the two lists of planeSplit, the coordinates in vAcc_ order
        per_node = 4 * 4 + 8 * 2 + 8 * 6              # left, right, feat, child; divlow, divhigh; the node's box
        return cap * per_point + nodes * per_node + 8 * 6 + 4, cap
    obs, _ = tree(max_points)
    edge, ecap = tree(max_edge_points)
    return scenes * (obs + edge + 12 * ecap)


@pytest.mark.parametrize("shape", [(1, 100, 100, 1), (256, 3072, 512, 100), (512, 50000, 5000, 3)])
def test_tie_order_bytes_is_host_arithmetic(shape):
    lib = capi.load()
    b = C.c_longlong(0)
    assert lib.amk_kfmap_tie_order_bytes(*shape, C.byref(b)) == capi.AMK_OK
    assert b.value == tie_order_bytes(*shape)
    assert lib.amk_kfmap_tie_order_bytes(*shape, None) == capi.AMK_ERR_INVALID_ARG
    assert lib.amk_kfmap_tie_order_bytes(0, 100, 100, 3, C.byref(b)) == capi.AMK_ERR_INVALID_ARG
    assert lib.amk_kfmap_tie_order_bytes(4, 100, 100, 0, C.byref(b)) == capi.AMK_ERR_INVALID_ARG


def test_the_new_calls_are_in_the_header_and_in_capi():
    header = open(os.path.join(ROOT, "include", "avoid_mpc_amd.h")).read()
    lib = capi.load()
    for name in NEW:
        assert f"int {name}(" in header, name
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    assert not capi.missing_symbols()
    assert "the keyframe map's own pool handles stay in the default mode" not in header
