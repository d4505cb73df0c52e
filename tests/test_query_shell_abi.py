"""CPU: the layer around the index walks of the spatial queries (radius search, segment search, segment nearest, segment cast, path
cast; csrc/map_query.hip and the five csrc/kd_*.hip query files) states its frame walk (for_each_frame), its row output
(write_list_row, write_cast_row) and its entry rules (kd_query_handle_status, kd_order_behind_pending) once; what the compiler makes
of the 15 map kernels and the five handle kernels stays what it made of the copies: the same kernels, each compiled by its own
unit, the same VGPRs, AGPRs, scratch, LDS and occupancy.  No device calls (tests/test_kd_*_gpu.py and tests/test_kfmap_*_gpu.py run
them)."""
import glob
import json
import os

import pytest

from avoid_mpc_amd import build as amk_build

# kernel_resources.json of the commit before the helpers (074b6d7, the build's flags for gfx950): (vgprs, occupancy, lds_bytes),
# zero scratch and zero AGPRs in every row.  tag: what of the mangled template arguments follows the kernel's own name.
MAP_KERNELS = {
    ("map_query_exact_kernel", "E"): (63, 7, 9792),
    ("map_query_kernel", "ILb1ELb0EE"): (61, 7, 5184),    # <MAP, DIST>: a keyframe map, k-NN
    ("map_query_kernel", "ILb0ELb0EE"): (61, 7, 5184),
    ("map_query_kernel", "ILb1ELb1EE"): (55, 7, 5184),    # distance
    ("map_query_kernel", "ILb0ELb1EE"): (54, 7, 5184),
    ("map_radius_kernel", "ILb1EE"): (77, 6, 5184),
    ("map_radius_kernel", "ILb0EE"): (77, 6, 5184),
    ("map_segment_kernel", "ILb1EE"): (115, 4, 5184),
    ("map_segment_kernel", "ILb0EE"): (115, 4, 5184),
    ("map_segment_nearest_kernel", "ILb1EE"): (107, 4, 5184),
    ("map_segment_nearest_kernel", "ILb0EE"): (107, 4, 5184),
    ("map_segment_cast_kernel", "ILb1EE"): (106, 4, 5184),
    ("map_segment_cast_kernel", "ILb0EE"): (106, 4, 5184),
    ("map_path_cast_kernel", "ILb1ELi4EE"): (116, 4, 5504),
    ("map_path_cast_kernel", "ILb0ELi4EE"): (116, 4, 5504),
}
HANDLE_KERNELS = {   # kernel -> (its unit, the row)
    ("kd_radius_search_kernel", "N"): ("kd_radius", (54, 8, 5184)),
    ("kd_segment_search_kernel", "N"): ("kd_segment", (90, 5, 5184)),
    ("kd_segment_nearest_kernel", "N"): ("kd_segment_nearest", (84, 5, 5184)),
    ("kd_segment_cast_kernel", "N"): ("kd_segment_cast", (84, 5, 5184)),
    ("kd_path_cast_kernel", "ILi4EE"): ("kd_path_cast", (104, 4, 5504)),
}
QUERY_FILES = ("kd_radius.hip", "kd_segment.hip", "kd_segment_nearest.hip", "kd_segment_cast.hip", "kd_path_cast.hip")
SHARED_HEADER = "kd_device.h"


def _find(names, kernel, tag):
    """the one mangled name that holds `kernel` as an identifier of its own (Itanium mangling writes it behind its length) with
    `tag` straight behind it"""
    found = [n for n in names if f"{len(kernel)}{kernel}{tag}" in n]
    assert len(found) == 1, (kernel, tag, found)
    return found[0]


def _src(name):
    return open(os.path.join(amk_build.CSRC, name)).read()


@pytest.fixture(scope="module")
def table():
    amk_build.build()
    return json.load(open(amk_build.RES))


@pytest.fixture(scope="module")
def per_object(table):
    return {os.path.basename(p)[:-len(".o.res.json")]: list(json.load(open(p)))
            for p in glob.glob(os.path.join(amk_build.OBJ, "*.o.res.json"))}


def _check_row(table, name, row):
    r = table[name]
    print(name, r)
    vgprs, occupancy, lds = row
    assert (r["vgprs"], r["occupancy"], r["lds_bytes"]) == (vgprs, occupancy, lds), (name, r)
    assert r["scratch_bytes_per_lane"] == 0 and r["agprs"] == 0, (name, r)


def test_the_fifteen_map_kernels_keep_their_resources(table, per_object):
    mine = sorted(n for n in table if "_GLOBAL__N_1" in n and any(f"{len(k)}{k}" in n for k, _ in MAP_KERNELS))
    want = {_find(mine, kernel, tag): row for (kernel, tag), row in MAP_KERNELS.items()}
    assert sorted(want) == mine and len(mine) == 15, mine   # exactly these fifteen
    for name, row in want.items():
        _check_row(table, name, row)
    assert sorted(per_object["map_query"]) == mine          # and map_query.hip compiles them, nothing else


def test_the_five_handle_kernels_keep_their_resources(table, per_object):
    for (kernel, tag), (unit, row) in HANDLE_KERNELS.items():
        name = _find(list(table), kernel, tag)
        _check_row(table, name, row)
        assert per_object[unit] == [name], (unit, per_object[unit])   # one kernel per query file: its own


def test_the_frame_walk_and_the_row_output_are_written_once():
    map_query = _src("map_query.hip")
    assert map_query.count("pool_scene(") == 1
    assert "USER" not in map_query
    elsewhere = [f for f in sorted(os.listdir(amk_build.CSRC))
                 if f.endswith((".hip", ".h")) and f != "kd_index.hip" and not f.startswith("step")]
    assert sum(_src(f).count("out_pts[o * 3 + 0]") for f in elsewhere) == 1
    assert _src(SHARED_HEADER).count("out_pts[o * 3 + 0]") == 1


def test_the_handle_entries_order_behind_a_pending_build_in_one_place():
    assert sum(_src(f).count("async_pending = 0") for f in QUERY_FILES + (SHARED_HEADER,)) == 1
    assert _src(SHARED_HEADER).count("async_pending = 0") == 1
    for f in QUERY_FILES:
        text = _src(f)
        assert "kd_query_handle_status(" in text and "kd_order_behind_pending(" in text, f
        assert "0x7fffffff" not in text and "mode != 0" not in text, f   # the rules are kd_query_handle_status's
