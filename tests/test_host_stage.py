"""CPU: where the *_host entry points' staging block (csrc/host_stage.h, HostStage) puts a call's slots, through amk__stage_layout --
the host-only entry that runs the same stage_next loop.  No device."""
import ctypes as C

import numpy as np
import pytest

from avoid_mpc_amd import capi

ALIGN = 256   # what separate hipMallocs gave the kernels before the slots shared a block


def layout(sizes):
    lib = capi.load()
    lib.amk__stage_layout.restype = C.c_int
    lib.amk__stage_layout.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_longlong)]
    b = np.array(sizes, np.int64)
    off = np.full(len(sizes), -1, np.int64)
    total = C.c_longlong(-1)
    st = lib.amk__stage_layout(b.ctypes.data_as(C.c_void_p) if len(sizes) else None, len(sizes),
                               off.ctypes.data_as(C.c_void_p) if len(sizes) else None, C.byref(total))
    return st, off.tolist(), total.value


CASES = [
    [1],
    [256], [257], [255, 1, 256, 4096],
    [24, 24, 12, 4, 36],                    # amk_kd_search_host: one scene, one query, k = 3
    [0, 8], [8, 0], [8, 0, 0, 8], [0], [0, 0],   # zero-byte slots: a max_points == 0 handle, an output nobody asked for
    [300 * 12 + 17 * 12, 8],                # an odd cloud and its counts
    [(1 << 32) + 1, 3, 1 << 33],            # past 32 bits
]


@pytest.mark.parametrize("sizes", CASES, ids=lambda s: "-".join(map(str, s)))
def test_slots_are_aligned_ordered_and_disjoint(sizes):
    st, off, total = layout(sizes)
    assert st == capi.AMK_OK
    end = 0
    for b, o in zip(sizes, off):
        assert o % ALIGN == 0
        assert o >= end                      # in call order, behind everything before it
        assert o - end < ALIGN               # and no further than the alignment asks
        if b:
            end = o + b
    assert total == end                      # the block ends with its last slot that holds anything


@pytest.mark.parametrize("sizes,at", [([8, 0, 8], 1), ([0, 8], 0), ([300, 0, 0, 5], 1), ([8, 0], 1)])
def test_a_zero_byte_slot_takes_no_room(sizes, at):
    _, off, total = layout(sizes)
    _, off_without, total_without = layout(sizes[:at] + sizes[at + 1:])
    assert off[:at] + off[at + 1:] == off_without and total == total_without
    if at + 1 < len(sizes):
        assert off[at] == off[at + 1]        # the next slot starts where the empty one stands


def test_no_slots_need_no_block():
    assert layout([]) == (capi.AMK_OK, [], 0)


def test_refusals():
    lib = capi.load()
    assert layout([8, -1])[0] == capi.AMK_ERR_INVALID_ARG
    total = C.c_longlong(0)
    lib.amk__stage_layout.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_longlong)]
    assert lib.amk__stage_layout(None, 1, None, C.byref(total)) == capi.AMK_ERR_INVALID_ARG
    assert lib.amk__stage_layout(None, -1, None, C.byref(total)) == capi.AMK_ERR_INVALID_ARG
    assert lib.amk__stage_layout(None, 0, None, None) == capi.AMK_ERR_INVALID_ARG
