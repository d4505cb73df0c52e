"""CPU: the reference-shaped tree has one home (csrc/kd_exact.hip) and ONE build pair template, kd_exact_build_top_kernel<GATE> /
kd_exact_build_kernel<GATE> (one instantiation per caller: every scene, AMK_TIES_AUTO's lazy scenes, the keyframe map's rows), in
place of three hand-written copies; one status kernel; the device build (kd_exact_build.h) is compiled by that unit alone, and
kd_grid_build_kernel by kd_sweep.hip alone.  No compute calls (tests/test_kd_gpu.py, tests/test_kd_tie_auto_gpu.py and
tests/test_kfmap_tie_order_gpu.py run the pair on the device for its three callers)."""
import glob
import json
import os

import pytest

from avoid_mpc_amd import build as amk_build

# kernel_resources.json of the commit before the merge (df25c26, the build's flags for gfx950): the same row for each of the three
# copies -- kd_exact_build_top_kernel / kd_auto_build_top_kernel / kd_pool_exact_build_top_kernel, and the three rest kernels.
PARENT = {
    "kd_exact_build_top_kernel": dict(vgprs=137, lds_bytes=928, occupancy=3),
    "kd_exact_build_kernel": dict(vgprs=73, lds_bytes=152088, occupancy=4),
}
RETIRED = ("kd_auto_build_top_kernel", "kd_auto_build_rest_kernel", "kd_pool_exact_build_top_kernel",
           "kd_pool_exact_build_rest_kernel", "kd_auto_status_kernel")
TREE_KERNELS = tuple(PARENT) + RETIRED[:4] + ("kd_exact_status_kernel", "kd_auto_status_kernel")


def _has(mangled, name):
    """`name` is the kernel's own identifier: Itanium mangling writes it behind its length (21kd_exact_build_kernel), so
    kd_exact_build_kernel is not found in kd_pool_exact_build_rest_kernel"""
    return mangled == name or f"{len(name)}{name}" in mangled


@pytest.fixture(scope="module")
def table():
    amk_build.build()
    return json.load(open(amk_build.RES))


@pytest.fixture(scope="module")
def per_object(table):
    """translation unit -> its kernels, from the per-object resource remarks the build leaves"""
    return {os.path.basename(p)[:-len(".o.res.json")]: list(json.load(open(p)))
            for p in glob.glob(os.path.join(amk_build.OBJ, "*.o.res.json"))}


def test_one_build_pair_template_and_one_status_kernel(table):
    for name, parent in PARENT.items():
        mine = sorted(n for n in table if _has(n, name))
        assert len(mine) == 3 and all(f"{name}ILi{g}EE" in n for g, n in enumerate(mine)), (name, mine)   # <kGateNone | Lazy | Rows>
        for n in mine:
            r = table[n]
            assert r["scratch_bytes_per_lane"] == 0, (n, r)
            assert r["vgprs"] <= parent["vgprs"], (n, r)
            assert r["lds_bytes"] == parent["lds_bytes"], (n, r)
            assert r["occupancy"] >= parent["occupancy"], (n, r)
    for name in RETIRED:
        assert not [n for n in table if _has(n, name)], name
    status = [n for n in table if "status_kernel" in n]
    assert len(status) == 1 and _has(status[0], "kd_exact_status_kernel"), status


def test_every_kernel_is_compiled_by_one_unit(per_object):
    assert "kd_exact" in per_object and "kd_sweep" in per_object, sorted(per_object)
    for unit, kernels in per_object.items():
        for n in kernels:
            if _has(n, "kd_grid_build_kernel"):
                assert unit == "kd_sweep", (unit, n)
            if any(_has(n, t) for t in TREE_KERNELS):
                assert unit == "kd_exact", (unit, n)
    assert any(_has(n, "kd_grid_build_kernel") for n in per_object["kd_sweep"])
    assert all(any(_has(n, t) for n in per_object["kd_exact"]) for t in PARENT)


def test_only_kd_exact_includes_the_device_build():
    assert os.path.exists(os.path.join(amk_build.CSRC, "kd_exact_build.h"))
    users = [os.path.basename(p) for p in amk_build.sources() if "kd_exact_build.h" in open(p).read()]
    assert users == ["kd_exact.hip"], users
    headers = [f for f in os.listdir(amk_build.CSRC) if f.endswith(".h") and f != "kd_exact_build.h"
               and "kd_exact_build.h\"" in open(os.path.join(amk_build.CSRC, f)).read()]
    assert not headers, headers   # (nor through another header)
