"""CPU: the map's own queries (FrameKDMap::QueryNearest / GetNearestDistance / GetPtCloud, csrc/map_query.hip + csrc/kfmap.hip) are
declared in the header, bound in capi.py and exported by the built library, and the new kernel uses no scratch memory and no LDS
beyond the search's per-wavefront rows.  No compute calls (tests/test_kfmap_query_gpu.py and tests/test_kd_query_frames_gpu.py run
them on the device)."""
import json
import os
import re

import pytest

from avoid_mpc_amd import build as amk_build
from avoid_mpc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["amk_kfmap_query_nearest", "amk_kfmap_nearest_distance", "amk_kfmap_points_host", "amk_kd_query_frames",
       "amk_kd_nearest_distance_frames", "amk_kfmap_query_nearest_host", "amk_kfmap_nearest_distance_host", "amk_kd_query_frames_host"]


@pytest.fixture(scope="module")
def lib():
    amk_build.build()
    return capi.load()


def test_declared_bound_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "avoid_mpc_amd.h")).read()
    declared = set(re.findall(r"^int (amk_[a-z_0-9]+)\(", hdr, re.M))
    for name in NEW:
        assert name in declared, name
        assert name in capi.SYMBOLS, name
        fn = getattr(lib, name, None)
        assert fn is not None and fn.argtypes is not None, name
    # the arities of the header's declarations equal the bindings'
    for name in NEW:
        decl = re.search(r"^int " + name + r"\((.*?)\);", hdr, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(getattr(lib, name).argtypes), name


def test_the_query_kernel_uses_no_scratch_and_only_the_search_rows_of_lds(lib):
    table = json.load(open(amk_build.RES))
    mine = {n: r for n, r in table.items() if "map_query_kernel" in n}
    assert len(mine) == 4, sorted(mine)                 # map / handle list x k-NN / distance
    search = [r for n, r in table.items() if "kd_grid_search_kernel" in n][0]
    for n, r in mine.items():
        assert r["scratch_bytes_per_lane"] == 0, (n, r)
        assert r["lds_bytes"] == search["lds_bytes"], (n, r, search)   # four GridWaveLds, nothing else
        assert r["vgprs"] <= 128, (n, r)                                # four waves per SIMD at least


def test_argument_checks_need_no_device(lib):
    """NULL handles are refused before anything touches the device."""
    assert lib.amk_kfmap_query_nearest(None, None, None, 3, 1, 1, 0, None, None, None, None, None) == capi.AMK_ERR_INVALID_ARG
    assert lib.amk_kfmap_nearest_distance(None, None, 3, 1, None, None) == capi.AMK_ERR_INVALID_ARG
    assert lib.amk_kfmap_points_host(None, 0, None, 0, None, None) == capi.AMK_ERR_INVALID_ARG
    assert lib.amk_kd_query_frames(None, 1, None, None, None, 3, 1, 1, None, None, None, None, None) == capi.AMK_ERR_INVALID_ARG
    assert lib.amk_kd_nearest_distance_frames(None, 1, None, 3, 1, None, None) == capi.AMK_ERR_INVALID_ARG
