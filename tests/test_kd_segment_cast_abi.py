"""Segment cast in the C ABI (amk_kd_segment_cast and its host, keyframe-map and frame-list variants): declared in the header, bound
in capi.py and exported by the built library; the header states the contract's sentences; the new kernels use no scratch memory
and at most 128 VGPRs; the four cases done by hand hold in the numpy restatement (tests/_cast.py); the C++ adapters compile with
the new methods (CPU) and answer like the brute force (GPU, the one test marked so).  The compute tests are
tests/test_kd_segment_cast_gpu.py and tests/test_kfmap_segment_cast_gpu.py."""
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from avoid_mpc_amd import build as amk_build
from avoid_mpc_amd import capi
from tests import _cast as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["amk_kd_segment_cast", "amk_kd_segment_cast_host", "amk_kfmap_segment_cast", "amk_kfmap_segment_cast_host",
       "amk_kd_segment_cast_frames", "amk_kd_segment_cast_frames_host"]


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
        assert "max_results" not in decl and "radius_sq" in decl, name
    assert not capi.missing_symbols()


def test_header_states_the_contract():
    text = " ".join(re.sub(r"^\s*\*", " ", line) for line in header().splitlines())
    text = re.sub(r"\s+", " ", text)
    for sentence in ["Segment cast: the first contact of a moving sphere along each leg of a path",
                     "are exactly those of \"Segment search\" above",
                     "There is no max_results: one contact per leg",
                     "All arithmetic is fp64 with contraction off and sums left to right, as in \"Segment search\"",
                     "Per leg ab, L2 and inv = 1.0 / L2 are exactly those of the segment search",
                     "ap = p - a; q = (ap0*ap0 + ap1*ap1) + ap2*ap2",
                     "usable iff q < DBL_MAX",
                     "q < r2: contact at t = 0",
                     "dot = (ap0*ab0 + ap1*ab1) + ap2*ab2; c = q - r2; disc = dot*dot - L2*c",
                     "contact iff dot > 0 and disc > 0 and t < 1, with t = (dot - sqrt(disc)) * inv",
                     "Every test is a strict comparison, so NaN and inf - inf give no contact",
                     "A grazing pass (disc == 0) and a contact that would begin exactly at b (t == 1) do not count",
                     "in exact arithmetic, a cast hits if and only if the segment search's count is above 0",
                     "The answer of a leg is the usable point with the smallest t; equal t keeps the lower cloud index",
                     "A leg without contact holds 1.0",
                     "so t * |ab| is the free distance in both cases",
                     "the point touched, (0,0,0) if none",
                     "-1 if none",
                     "Each output may be NULL, but not all of them",
                     "A degenerate leg (a == b) has dot == 0 and never uses inv",
                     "It hits iff some usable point has q < r2, at t = 0, and returns the lowest such index, not the nearest such point",
                     "radius_sq >= DBL_MAX (after clamping) puts every usable point inside at the start",
                     "radius_sq == 0 is allowed and answers by the formula",
                     "has no contact; a non-finite path point spoils only the one or two legs that touch it",
                     "An empty or never-built scene answers no contact",
                     "The fp64 sqrt and the one division are correctly rounded on the device",
                     "there is one reciprocal per leg and no division per candidate",
                     "Every error is returned before anything is staged or launched, the outputs untouched",
                     "The call is stream-ordered and allocates nothing",
                     "the tie-order modes do not apply",
                     "equal t keeps the earlier frame, then the lower cloud index within a frame",
                     "the frame touched, its position in the query vector (0 = current frame), -1 if none",
                     "A map scene with no frame answers no contact",
                     "Scan-mode handles, tie-order handles in the frame list and n_frames > AMK_MAX_FRAMES return AMK_ERR_UNSUPPORTED "
                     "before anything is staged or launched",
                     "no map state changed"]:
        assert sentence in text, sentence


def test_the_segment_cast_kernels_meet_the_resource_limits(lib):
    table = json.load(open(amk_build.RES))
    mine = {n: r for n, r in table.items() if "kd_segment_cast_kernel" in n or "map_segment_cast_kernel" in n}
    assert len(mine) == 3, sorted(mine)                 # one handle; a keyframe map; a list of handles
    search = [r for n, r in table.items() if "kd_grid_search_kernel" in n][0]
    for n, r in mine.items():
        assert r["scratch_bytes_per_lane"] == 0, (n, r)
        assert r["lds_bytes"] == search["lds_bytes"], (n, r, search)   # four GridWaveLds, nothing else
        assert r["vgprs"] <= 128, (n, r)                                # four waves per SIMD at least


def test_argument_checks_need_no_device(lib):
    """NULL handles are refused before anything touches the device."""
    inv = capi.AMK_ERR_INVALID_ARG
    assert lib.amk_kd_segment_cast(None, None, 3, 2, 0.25, None, None, None, None, None) == inv
    assert lib.amk_kd_segment_cast_host(None, None, 3, 2, 0.25, None, None, None, None) == inv
    assert lib.amk_kfmap_segment_cast(None, None, 3, 2, 0.25, 0, None, None, None, None, None) == inv
    assert lib.amk_kfmap_segment_cast_host(None, None, 3, 2, 0.25, 0, None, None, None, None) == inv
    assert lib.amk_kd_segment_cast_frames(None, 1, None, 3, 2, 0.25, None, None, None, None, None) == inv
    assert lib.amk_kd_segment_cast_frames_host(None, 1, None, 3, 2, 0.25, None, None, None, None) == inv


def test_python_hosts_offer_segment_cast():
    from avoid_mpc_amd import host
    assert callable(host.KdBatch.segment_cast) and callable(host.KdBatch.segment_cast_host)
    assert callable(host.KfMap.segment_cast) and callable(host.segment_cast_frames)


def test_the_four_cases_done_by_hand_hold_in_the_restatement():
    a, b = np.array([0.0, 0.0, 0.0]), np.array([10.0, 0.0, 0.0])
    # first is not closest: the point nearest the line (index 1) stands behind the one met first
    e = K.cast_brute(np.array([[2.0, 0.375, 0.0], [6.0, 0.0, 0.0], [9.0, 5.0, 5.0]], np.float32), a, b, 0.25)
    assert e["hit"] == 1 and e["indices"] == 0 and e["pts"].tolist() == [2.0, 0.375, 0.0]
    assert e["t"] == (20.0 - np.sqrt(400.0 - 100.0 * (4.140625 - 0.25))) * (1.0 / 100.0) and abs(e["t"] - 0.16692810861169263) < 1e-15
    # a grazing pass does not count; a slightly wider sphere meets the first of the two
    pair = np.array([[3.0, 0.5, 0.0], [7.0, 0.5, 0.0]], np.float32)
    e = K.cast_brute(pair, a, b, 0.25)
    assert e["hit"] == 0 and e["t"] == 1.0 and e["indices"] == -1 and e["pts"].tolist() == [0.0, 0.0, 0.0]
    e = K.cast_brute(pair, a, b, 0.265625)
    assert e["hit"] == 1 and e["indices"] == 0 and e["t"] == (30.0 - np.sqrt(900.0 - 100.0 * (9.25 - 0.265625))) * (1.0 / 100.0)
    # a contact that would begin exactly at b
    e = K.cast_brute(np.array([[10.5, 0.0, 0.0]], np.float32), a, b, 0.25)
    assert e["hit"] == 0 and K.contacts(np.array([[10.5, 0.0, 0.0]], np.float32), a, b, 0.25)[1][0] == 1.0
    # the start on the sphere's surface: met at t = 0 heading in, missed heading out
    on = np.array([[0.5, 0.0, 0.0]], np.float32)
    e = K.cast_brute(on, a, b, 0.25)
    assert e["hit"] == 1 and e["t"] == 0.0 and e["indices"] == 0
    assert K.cast_brute(on, a, -b, 0.25)["hit"] == 0
    # over frames: an equal t keeps the earlier frame; a non-finite leg has no contact; +inf puts every usable point inside
    e = K.cast_brute_frames([on, on], a, b, 0.25)
    assert e["hit"] == 1 and e["frame"] == 0
    assert K.cast_brute(on, a, np.array([np.nan, 0.0, 0.0]), 0.25)["hit"] == 0
    e = K.cast_brute(np.array([[np.inf, 0.0, 0.0], [50.0, 50.0, 50.0]], np.float32), a, b, float("inf"))
    assert e["hit"] == 1 and e["indices"] == 1 and e["t"] == 0.0


def compile_demo(tmp_path):
    """built the way tests/test_cpp_adapters_gpu.py builds its host"""
    exe = str(tmp_path / "segment_cast_demo")
    libdir = os.path.join(ROOT, "avoid_mpc_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "segment_cast_demo.cpp"), "-o", exe,
                           "-L", libdir, "-lavoid_mpc_amd", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_adapters_compile_with_the_new_methods(lib, tmp_path):
    hpp = open(os.path.join(ROOT, "include", "avoid_mpc_amd", "kd_tree_two.hpp")).read()
    assert "bool SegmentCast(num_t ax, num_t ay, num_t az, num_t bx, num_t by, num_t bz, double radius_sq, double &t)" in hpp
    fk = open(os.path.join(ROOT, "include", "avoid_mpc_amd", "frame_kd_map.hpp")).read()
    assert "bool QuerySegmentCast(const Vector3d &from, const Vector3d &to, double radius_sq, Vector3d &point, double &t" in fk
    assert os.path.exists(compile_demo(tmp_path))


@pytest.mark.gpu
def test_cpp_adapters_answer_like_the_brute_force(tmp_path):
    exe = compile_demo(tmp_path)
    rng = np.random.default_rng(23)
    n, nl, r2 = 3000, 12, 0.0625
    cloud = (np.round(rng.random((n, 3)) * [6.0, 5.0, 3.0] * 8) / 8).astype(np.float32)   # quantised: equal t occur
    legs = np.round(rng.random((nl, 2, 3)) * [6.0, 5.0, 3.0] * 8) / 8
    legs[:6, 1] = legs[:6, 0] + np.round((rng.random((6, 3)) - 0.5) * 8) / 8              # half of them up to half a metre per axis
    legs[3, 1] = legs[3, 0]                                                               # and a degenerate one
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("2i", n, nl)); f.write(struct.pack("d", r2)); f.write(cloud.tobytes()); f.write(legs.tobytes())
    subprocess.check_call([exe, fin, fout])
    buf = open(fout, "rb").read()
    off = 0

    def take(dtype, cnt):
        nonlocal off
        a = np.frombuffer(buf, dtype=dtype, count=cnt, offset=off)
        off += a.nbytes
        return a

    hits = 0
    for a, b in legs:                                    # KDTreeTwo::SegmentCast
        hit, index = (int(v) for v in take(np.int32, 2))
        e = K.cast_brute(cloud, a, b, r2)
        assert hit == e["hit"] and index == e["indices"]
        assert take(np.float64, 1)[0] == e["t"] and np.array_equal(take(np.float32, 3), e["pts"])
        hits += hit
    assert 0 < hits < nl
    for a, b in legs:                                    # FrameKDMap::QuerySegmentCast over [second half, first half]
        hit = int(take(np.int32, 1)[0])
        e = K.cast_brute_frames([cloud[n // 2:], cloud[:n // 2]], a, b, r2)
        assert hit == e["hit"] and take(np.float64, 1)[0] == e["t"]
        assert np.array_equal(take(np.float64, 3), e["pts"].astype(np.float64))
    assert off == len(buf)
