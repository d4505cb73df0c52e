"""CPU: the pipeline's hardware-queue policy (csrc/pipeline.hip: amk__pipeline_queue_policy), a pure function of the runtime's pool
size, the slot count and the number of stream priority classes -> the mode and the class of every slot."""
import ctypes as C

import numpy as np
import pytest

from avoid_mpc_amd import capi

POOLED, PRIORITY = capi.AMK_QUEUES_POOLED, capi.AMK_QUEUES_PRIORITY
CAP = capi.AMK_PIPELINE_MAX_OWN_QUEUES
SLOTS = [1, 4, 5, 10, 12, 13, 16, 24, 30]
CLASSES = 3            # what hipDeviceGetStreamPriorityRange spans on this runtime: 0 high, 1 normal, 2 low
CYCLE = [1, 2, 0]      # normal, low, high


def policy(pool, n_slots, n_classes=CLASSES, forced=-1):
    lib = capi.load()
    mode = np.full(n_slots, -7, np.int32); cls = np.full(n_slots, -7, np.int32)
    own = lib.amk__pipeline_queue_policy(pool, n_slots, n_classes, forced, mode.ctypes.data_as(C.c_void_p), cls.ctypes.data_as(C.c_void_p))
    assert own == int((mode != POOLED).sum())
    assert set(mode) <= {POOLED, PRIORITY} and ((cls >= 0) & (cls < n_classes)).all()
    assert (mode[:own] == PRIORITY).all()          # the leading slots get queues of their own, the ones beyond share
    assert (cls[own:] == (n_classes - 1) // 2).all()   # (a pooled stream is of the normal class)
    return mode, cls, own


def check_priority(cls, own, pool, n_slots):
    assert own == min(n_slots, CLASSES * pool, CAP)    # never more than 24 queues of the pipeline's own
    per_class = np.bincount(cls[:own], minlength=CLASSES)
    assert per_class.max() <= pool                     # nobody above the per-class limit
    assert (cls[:own] == np.array(CYCLE)[np.arange(own) % CLASSES]).all()
    assert per_class[1] >= per_class[2] >= per_class[0]   # the high class never holds more slots than another


@pytest.mark.parametrize("n_slots", SLOTS)
@pytest.mark.parametrize("pool", [4, 32])
def test_automatic(pool, n_slots):
    mode, cls, own = policy(pool, n_slots)
    if pool >= n_slots + 1 or pool >= CAP:     # the pool suffices (today's streams), or nothing may be added to it
        assert own == 0
    else:
        check_priority(cls, own, pool, n_slots)


@pytest.mark.parametrize("n_slots", SLOTS)
@pytest.mark.parametrize("pool", [4, 32])
def test_forced(pool, n_slots):
    assert policy(pool, n_slots, forced=POOLED)[2] == 0
    mode, cls, own = policy(pool, n_slots, forced=PRIORITY)
    check_priority(cls, own, pool, n_slots)
    assert (policy(pool, n_slots, forced=2)[0] == policy(pool, n_slots)[0]).all()   # an unknown mode: automatic


def test_edges():
    mode, cls, own = policy(4, 10, n_classes=1, forced=PRIORITY)   # a device with one class: four slots of their own, six share
    assert list(mode) == [PRIORITY] * 4 + [POOLED] * 6 and (cls == 0).all()
    mode, cls, own = policy(4, 10, n_classes=5)                    # normal, the two lower classes, then the two higher ones
    assert list(cls) == [2, 3, 4, 1, 0, 2, 3, 4, 1, 0]
    lib = capi.load()
    buf = (C.c_int * 4)()
    assert lib.amk__pipeline_queue_policy(0, 4, 3, -1, buf, buf) == -1
    assert lib.amk__pipeline_queue_policy(4, 0, 3, -1, buf, buf) == -1
    assert lib.amk__pipeline_queue_policy(4, 4, 3, -1, None, buf) == -1
