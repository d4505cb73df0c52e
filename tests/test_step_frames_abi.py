"""CPU: the multi-frame step's merge (csrc/step_frames.hip) is ONE kernel template, step_merge_plan_pack_kernel<EXACT, CPL, Trees>,
with its body written in it: eight instantiations, none with scratch memory, none with more vector registers than the kernels it
replaced.  No compute calls (tests/test_step_frames_edges_gpu.py and tests/test_kfmap_tie_order_gpu.py run every instantiation on
the device)."""
import json
import os
import re

import pytest

from avoid_mpc_amd import build as amk_build

# (EXACT, CPL, Trees) -> VGPRs.  From kernel_resources.json of the commit before the template (74da4a9, the build's flags for
# gfx950), where the two MapTrees instantiations were step_merge_plan_pack_map_kernel<0> and <4>.  CPL 0: the wide merge.
PARENT_VGPRS = {
    (0, 0, "FrameExact"): 63, (0, 1, "FrameExact"): 63, (0, 2, "FrameExact"): 63, (0, 4, "FrameExact"): 70,
    (0, 16, "FrameExact"): 202, (1, 16, "FrameExact"): 202,
    (1, 0, "MapTrees"): 81, (1, 4, "MapTrees"): 81,
}
MERGE = re.compile(r"step_merge_plan_pack_kernelILb([01])ELi(\d+)E(?:PKN3amk10(FrameExact)|N3amk8(MapTrees))EE")


@pytest.fixture(scope="module")
def table():
    amk_build.build()
    return json.load(open(amk_build.RES))


def test_the_merge_is_one_template_with_eight_instantiations(table):
    assert not [n for n in table if "step_merge_plan_pack_map_kernel" in n]
    mine = [n for n in table if "step_merge_plan_pack" in n]
    found = {}
    for n in mine:
        m = MERGE.search(n)
        assert m, n
        found[(int(m.group(1)), int(m.group(2)), m.group(3) or m.group(4))] = table[n]
    assert len(mine) == 8 and sorted(found) == sorted(PARENT_VGPRS), sorted(mine)
    for inst, r in found.items():
        assert r["scratch_bytes_per_lane"] == 0, (inst, r)
        assert r["vgprs"] <= PARENT_VGPRS[inst], (inst, r)


def test_the_text_include_is_gone():
    assert not os.path.exists(os.path.join(amk_build.CSRC, "step_merge_plan_pack_body.h"))
