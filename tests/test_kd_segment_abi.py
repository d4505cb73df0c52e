"""The segment searches in the C ABI (amk_kd_segment_search and its host, keyframe-map and frame-list variants): declared in the
header, bound in capi.py and exported by the built library; the header states the contract's sentences; the new kernels use no
scratch memory and at most 128 VGPRs; the C++ adapters compile with the new methods (CPU) and answer like the brute force (GPU, the
one test marked so).  The compute tests are tests/test_kd_segment_gpu.py and tests/test_kfmap_segment_gpu.py."""
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from avoid_mpc_amd import build as amk_build
from avoid_mpc_amd import capi
from tests import _segment as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["amk_kd_segment_search", "amk_kd_segment_search_host", "amk_kfmap_segment_search", "amk_kfmap_segment_search_host",
       "amk_kd_segment_search_frames", "amk_kd_segment_search_frames_host"]


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
    for sentence in ["A path is n_points >= 2 positions per scene",
                     "d_path[(s*n_points + j)*point_stride + {0,1,2}]",
                     "n_points = 2 is a lone segment",
                     "Every output is [S][n_legs = n_points - 1]",
                     "L2 = (ab0*ab0 + ab1*ab1) + ab2*ab2; inv = 1.0 / L2",
                     "t = dot > 0 ? dot*inv : 0; t = t < 1 ? t : 1",
                     "c = t < 1 ? a + t*ab (per component: one product, one sum) : b exactly",
                     "There is one reciprocal per leg, not a division per candidate",
                     "the leg answers exactly what amk_kd_radius_search answers at a, bit for bit",
                     "The test is strict: a result has d2 < radius_sq",
                     "the full number of results of the leg, never capped by max_results",
                     "or whose L2 is not finite, gets count 0 and empty slots",
                     "a non-finite path point spoils only the one or two legs that touch it",
                     "An empty or never-built scene answers 0",
                     "ascending by d2, equal d2 by cloud index",
                     "the earlier frame first, then the lower cloud index within a frame",
                     "max_results == 0 requires every list pointer NULL",
                     "No size rule, no fast path, no PtIsInFrame",
                     "Every error is returned before anything is launched, the outputs untouched",
                     "The call is stream-ordered and allocates nothing",
                     "Not offered: per-leg radii, uncapped result lists, an unbounded \"nearest point to the segment\" query, "
                     "segment queries inside amk_step_batch or the pipeline"]:
        assert sentence in text, sentence


def test_the_segment_kernels_use_no_scratch(lib):
    table = json.load(open(amk_build.RES))
    mine = {n: r for n, r in table.items() if "kd_segment_search_kernel" in n or "map_segment_kernel" in n}
    assert len(mine) == 3, sorted(mine)                 # one handle; a keyframe map; a list of handles
    search = [r for n, r in table.items() if "kd_grid_search_kernel" in n][0]
    for n, r in mine.items():
        assert r["scratch_bytes_per_lane"] == 0, (n, r)
        assert r["lds_bytes"] == search["lds_bytes"], (n, r, search)   # four GridWaveLds, nothing else
        assert r["vgprs"] <= 128, (n, r)                                # four waves per SIMD at least


def test_argument_checks_need_no_device(lib):
    """NULL handles are refused before anything touches the device."""
    inv = capi.AMK_ERR_INVALID_ARG
    assert lib.amk_kd_segment_search(None, None, 3, 2, 1.0, 1, None, None, None, None, None, None) == inv
    assert lib.amk_kd_segment_search_host(None, None, 3, 2, 1.0, 1, None, None, None, None, None) == inv
    assert lib.amk_kfmap_segment_search(None, None, 3, 2, 1.0, 1, 0, None, None, None, None, None, None) == inv
    assert lib.amk_kfmap_segment_search_host(None, None, 3, 2, 1.0, 1, 0, None, None, None, None, None) == inv
    assert lib.amk_kd_segment_search_frames(None, 1, None, 3, 2, 1.0, 1, None, None, None, None, None, None) == inv
    assert lib.amk_kd_segment_search_frames_host(None, 1, None, 3, 2, 1.0, 1, None, None, None, None, None) == inv


def test_python_hosts_offer_the_segment_search():
    from avoid_mpc_amd import host
    assert callable(host.KdBatch.segment_search) and callable(host.KdBatch.segment_search_host)
    assert callable(host.KfMap.segment_search) and callable(host.segment_search_frames)


def compile_demo(tmp_path):
    """built the way tests/test_cpp_adapters_gpu.py builds its host"""
    exe = str(tmp_path / "segment_demo")
    libdir = os.path.join(ROOT, "avoid_mpc_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "segment_demo.cpp"), "-o", exe,
                           "-L", libdir, "-lavoid_mpc_amd", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_adapters_compile_with_the_new_methods(lib, tmp_path):
    hpp = open(os.path.join(ROOT, "include", "avoid_mpc_amd", "kd_tree_two.hpp")).read()
    assert "size_t SegmentSearch(num_t ax, num_t ay, num_t az, num_t bx, num_t by, num_t bz, double radius_sq, int max_results)" in hpp
    assert "std::vector<double> segment_t;" in hpp
    fk = open(os.path.join(ROOT, "include", "avoid_mpc_amd", "frame_kd_map.hpp")).read()
    assert "size_t QuerySegment(const Vector3d &from, const Vector3d &to, double radius_sq, int max_results" in fk
    assert os.path.exists(compile_demo(tmp_path))


@pytest.mark.gpu
def test_cpp_adapters_answer_like_the_brute_force(tmp_path):
    exe = compile_demo(tmp_path)
    rng = np.random.default_rng(23)
    n, nl, k, r2 = 3000, 12, 8, 0.5
    cloud = (np.round(rng.random((n, 3)) * [6.0, 5.0, 3.0] * 8) / 8).astype(np.float32)   # quantised: equal distances occur
    legs = np.round(rng.random((nl, 2, 3)) * [6.0, 5.0, 3.0] * 8) / 8
    legs[:, 1] = legs[:, 0] + np.round((rng.random((nl, 3)) - 0.5) * 8) / 8               # legs of up to half a metre per axis
    legs[3, 1] = legs[3, 0]                                                               # and a degenerate one
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("3i", n, nl, k)); f.write(struct.pack("d", r2)); f.write(cloud.tobytes()); f.write(legs.tobytes())
    subprocess.check_call([exe, fin, fout])
    buf = open(fout, "rb").read()
    off = 0

    def take(dtype, cnt):
        nonlocal off
        a = np.frombuffer(buf, dtype=dtype, count=cnt, offset=off)
        off += a.nbytes
        return a

    seen = 0
    for a, b in legs:                                    # KDTreeTwo::SegmentSearch
        count, c = (int(v) for v in take(np.int32, 2))
        e = G.segment_brute(cloud, a, b, r2, k)
        assert count == e["count"] and c == min(count, k)
        assert np.array_equal(take(np.int32, c), e["indices"][:c]) and np.array_equal(take(np.float64, c), e["sqdist"][:c])
        assert np.array_equal(take(np.float64, c), e["t"][:c])
        assert np.array_equal(take(np.float32, 3 * c).reshape(-1, 3), e["pts"][:c])
        seen += count > k
    assert seen >= 3                                     # (the count does exceed the list)
    for a, b in legs:                                    # FrameKDMap::QuerySegment over [second half, first half]
        count, c = (int(v) for v in take(np.int32, 2))
        e = G.segment_brute_frames([cloud[n // 2:], cloud[:n // 2]], a, b, r2, k)
        assert count == e["count"] and c == min(count, k)
        assert np.array_equal(take(np.float64, c), e["sqdist"][:c]) and np.array_equal(take(np.float64, c), e["t"][:c])
        assert np.array_equal(take(np.float64, 3 * c).reshape(-1, 3), e["pts"][:c].astype(np.float64))
    assert off == len(buf)
