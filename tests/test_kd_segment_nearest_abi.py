"""Segment nearest in the C ABI (amk_kd_segment_nearest and its host, keyframe-map and frame-list variants): declared in the header,
bound in capi.py and exported by the built library; the header states the contract's sentences, the two identities included; the new
kernels use no scratch memory and at most 128 VGPRs; the C++ adapters compile with the new methods (CPU) and answer like the brute
force (GPU, the one test marked so).  The compute tests are tests/test_kd_segment_nearest_gpu.py and
tests/test_kfmap_segment_nearest_gpu.py."""
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from avoid_mpc_amd import build as amk_build
from avoid_mpc_amd import capi
from tests import _segment_nearest as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["amk_kd_segment_nearest", "amk_kd_segment_nearest_host", "amk_kfmap_segment_nearest", "amk_kfmap_segment_nearest_host",
       "amk_kd_segment_nearest_frames", "amk_kd_segment_nearest_frames_host"]


@pytest.fixture(scope="module")
def lib():
    amk_build.build()
    return capi.load()


def header():
    return open(os.path.join(ROOT, "include", "avoid_mpc_amd.h")).read()


def test_declared_bound_and_exported(lib):
    hdr = header()
    declared = set(re.findall(r"^int (amk_[a-z_0-9]+)\(", hdr, re.M))
    for name in NEW:
        assert name in declared, name
        assert name in capi.SYMBOLS, name
        fn = getattr(lib, name, None)
        assert fn is not None and fn.argtypes is not None, name
        decl = re.search(r"^int " + name + r"\((.*?)\);", hdr, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(fn.argtypes), name
    assert not capi.missing_symbols()


def test_header_states_the_contract():
    text = " ".join(re.sub(r"^\s*\*", " ", line) for line in header().splitlines())
    text = re.sub(r"\s+", " ", text)
    for sentence in ["Segment nearest: the k map points closest to each leg of a path, with no radius to choose",
                     "are exactly those of \"Segment search\" above",
                     "the k usable points (d2 < DBL_MAX) with the smallest d2, ascending; equal d2 order by cloud index",
                     "d_t is the position of the closest approach along the leg",
                     "min(k, usable points of the scene)",
                     "Slots beyond the count hold -1 / DBL_MAX / 0.0 / (0,0,0)",
                     "or with a non-finite L2, gets count 0 and empty slots",
                     "a non-finite path point spoils only the legs that touch it",
                     "An empty or never-built scene answers 0",
                     "A degenerate leg (a == b) has t = 0",
                     "There is no radius, no size rule, no fast path and no PtIsInFrame",
                     "the exact tree is never consulted, and a handle in AMK_TIES_NANOFLANN / AMK_TIES_AUTO answers like the default",
                     "1 <= k <= AMK_MAX_K",
                     "Each output may be NULL, but not all of them",
                     "Every error is returned before anything is staged or launched, the outputs untouched",
                     "The call is stream-ordered and allocates nothing",
                     "The lists equal, bit for bit, those of amk_kd_segment_search called with radius_sq = +inf and max_results = k; "
                     "the count is min(k, that search's count)",
                     "A degenerate leg at a answers with the distances, indices and points of amk_kd_search(k) at a, in the default "
                     "tie order, for a scene holding more than k points",
                     "the size rule of SearchForNearest belongs to amk_kd_search and is absent here",
                     "The answer is the k nearest of all frames a scene holds",
                     "equal d2 keep the earlier frame, then the lower index within a frame",
                     "min(k, sum of the frames' usable points)",
                     "A map scene with no frame answers 0",
                     # and the segment search's own comment keeps its sentence
                     "Not offered: per-leg radii, uncapped result lists, an unbounded \"nearest point to the segment\" query, "
                     "segment queries inside amk_step_batch or the pipeline"]:
        assert sentence in text, sentence


def test_the_segment_nearest_kernels_meet_the_resource_limits(lib):
    table = json.load(open(amk_build.RES))
    mine = {n: r for n, r in table.items() if "kd_segment_nearest_kernel" in n or "map_segment_nearest_kernel" in n}
    assert len(mine) == 3, sorted(mine)                 # one handle; a keyframe map; a list of handles
    assert not [n for n in mine if "kd_segment_search_kernel" in n or "map_segment_kernel" in n]
    search = [r for n, r in table.items() if "kd_grid_search_kernel" in n][0]
    for n, r in mine.items():
        assert r["scratch_bytes_per_lane"] == 0, (n, r)
        assert r["lds_bytes"] == search["lds_bytes"], (n, r, search)   # four GridWaveLds, nothing else
        assert r["vgprs"] <= 128, (n, r)                                # four waves per SIMD at least


def test_argument_checks_need_no_device(lib):
    """NULL handles are refused before anything touches the device."""
    inv = capi.AMK_ERR_INVALID_ARG
    assert lib.amk_kd_segment_nearest(None, None, 3, 2, 1, None, None, None, None, None, None) == inv
    assert lib.amk_kd_segment_nearest_host(None, None, 3, 2, 1, None, None, None, None, None) == inv
    assert lib.amk_kfmap_segment_nearest(None, None, 3, 2, 1, 0, None, None, None, None, None, None) == inv
    assert lib.amk_kfmap_segment_nearest_host(None, None, 3, 2, 1, 0, None, None, None, None, None) == inv
    assert lib.amk_kd_segment_nearest_frames(None, 1, None, 3, 2, 1, None, None, None, None, None, None) == inv
    assert lib.amk_kd_segment_nearest_frames_host(None, 1, None, 3, 2, 1, None, None, None, None, None) == inv


def test_python_hosts_offer_segment_nearest():
    from avoid_mpc_amd import host
    assert callable(host.KdBatch.segment_nearest) and callable(host.KdBatch.segment_nearest_host)
    assert callable(host.KfMap.segment_nearest) and callable(host.segment_nearest_frames)


def compile_demo(tmp_path):
    """built the way tests/test_cpp_adapters_gpu.py builds its host"""
    exe = str(tmp_path / "segment_nearest_demo")
    libdir = os.path.join(ROOT, "avoid_mpc_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "segment_nearest_demo.cpp"), "-o", exe,
                           "-L", libdir, "-lavoid_mpc_amd", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_adapters_compile_with_the_new_methods(lib, tmp_path):
    hpp = open(os.path.join(ROOT, "include", "avoid_mpc_amd", "kd_tree_two.hpp")).read()
    assert "size_t SegmentNearest(num_t ax, num_t ay, num_t az, num_t bx, num_t by, num_t bz, int n)" in hpp
    fk = open(os.path.join(ROOT, "include", "avoid_mpc_amd", "frame_kd_map.hpp")).read()
    assert "size_t QuerySegmentNearest(const Vector3d &from, const Vector3d &to, int k" in fk
    assert os.path.exists(compile_demo(tmp_path))


@pytest.mark.gpu
def test_cpp_adapters_answer_like_the_brute_force(tmp_path):
    exe = compile_demo(tmp_path)
    rng = np.random.default_rng(23)
    n, nl, k = 3000, 12, 8
    cloud = (np.round(rng.random((n, 3)) * [6.0, 5.0, 3.0] * 8) / 8).astype(np.float32)   # quantised: equal distances occur
    legs = np.round(rng.random((nl, 2, 3)) * [6.0, 5.0, 3.0] * 8) / 8
    legs[:, 1] = legs[:, 0] + np.round((rng.random((nl, 3)) - 0.5) * 8) / 8               # legs of up to half a metre per axis
    legs[3, 1] = legs[3, 0]                                                               # and a degenerate one
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("3i", n, nl, k)); f.write(cloud.tobytes()); f.write(legs.tobytes())
    subprocess.check_call([exe, fin, fout])
    buf = open(fout, "rb").read()
    off = 0

    def take(dtype, cnt):
        nonlocal off
        a = np.frombuffer(buf, dtype=dtype, count=cnt, offset=off)
        off += a.nbytes
        return a

    for a, b in legs:                                    # KDTreeTwo::SegmentNearest
        count, c = (int(v) for v in take(np.int32, 2))
        e = N.nearest_brute(cloud, a, b, k)
        assert count == k and c == k and e["count"] == k
        assert np.array_equal(take(np.int32, c), e["indices"]) and np.array_equal(take(np.float64, c), e["sqdist"])
        assert np.array_equal(take(np.float64, c), e["t"])
        assert np.array_equal(take(np.float32, 3 * c).reshape(-1, 3), e["pts"])
    for a, b in legs:                                    # FrameKDMap::QuerySegmentNearest over [second half, first half]
        count, c = (int(v) for v in take(np.int32, 2))
        e = N.nearest_brute_frames([cloud[n // 2:], cloud[:n // 2]], a, b, k)
        assert count == k and c == k
        assert np.array_equal(take(np.float64, c), e["sqdist"]) and np.array_equal(take(np.float64, c), e["t"])
        assert np.array_equal(take(np.float64, 3 * c).reshape(-1, 3), e["pts"].astype(np.float64))
    assert off == len(buf)
