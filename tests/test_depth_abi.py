"""CPU: the three depth kernels of csrc/depth.hip (depth_to_cloud_kernel, depth_to_edge_kernel, depth_band_kernel<T, EMIT>) share one
statement of every rule of the reference (obstacle_depth, quantise, to_world, EdgeLayers); what the compiler makes of them stays what it
made of the three hand-written copies: the same eight kernels, compiled by the depth unit alone, no scratch, the same static LDS, eight
waves per SIMD, no more registers.  No compute calls (tests/test_depth_gpu.py and tests/test_depth_clouds_gpu.py run them)."""
import glob
import json
import os
import re

import pytest

from avoid_mpc_amd import build as amk_build

# kernel_resources.json of the commit before the helpers (a5bbe1d, the build's flags for gfx950); both pixel types have the same row
PARENT = {
    "depth_to_cloud_kernel": {"": dict(vgprs=52, lds_bytes=112)},
    "depth_to_edge_kernel": {"": dict(vgprs=56, lds_bytes=128)},
    "depth_band_kernel": {"Lb0E": dict(vgprs=34, lds_bytes=64), "Lb1E": dict(vgprs=62, lds_bytes=288)},   # EMIT = false, true
}
PIXELS = ("t", "f")   # unsigned short, float
VGPRS_AT_EIGHT_WAVES = 64


def _has(mangled, name):
    """`name` is the kernel's own identifier: Itanium mangling writes it behind its length"""
    return mangled == name or f"{len(name)}{name}" in mangled


@pytest.fixture(scope="module")
def table():
    amk_build.build()
    return json.load(open(amk_build.RES))


def test_the_eight_depth_kernels_keep_their_resources(table):
    mine = sorted(n for n in table if re.search(r"\d+depth_[a-z_]*kernel", n))   # every kernel whose own name starts with depth_
    want = {}
    for name, variants in PARENT.items():
        for emit, row in variants.items():
            for px in PIXELS:
                found = [n for n in mine if _has(n, name) and f"{name}I{px}{emit}E" in n]
                assert len(found) == 1, (name, px, emit, mine)
                want[found[0]] = row
    assert sorted(want) == mine and len(mine) == 8, mine   # exactly these eight
    for n, parent in want.items():
        r = table[n]
        print(n, r)
        assert r["scratch_bytes_per_lane"] == 0, (n, r)
        assert r["lds_bytes"] == parent["lds_bytes"], (n, r)
        assert r["occupancy"] >= 8, (n, r)
        assert r["vgprs"] <= parent["vgprs"] or r["vgprs"] <= VGPRS_AT_EIGHT_WAVES, (n, r)


def test_the_depth_unit_alone_compiles_them(table):
    per_object = {os.path.basename(p)[:-len(".o.res.json")]: list(json.load(open(p)))
                  for p in glob.glob(os.path.join(amk_build.OBJ, "*.o.res.json"))}
    assert "depth" in per_object, sorted(per_object)
    for unit, kernels in per_object.items():
        mine = [n for n in kernels if any(_has(n, name) for name in PARENT)]
        assert len(mine) == (8 if unit == "depth" else 0), (unit, mine)
