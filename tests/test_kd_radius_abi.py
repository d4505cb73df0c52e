"""The radius searches in the C ABI (amk_kd_radius_search and its host, keyframe-map and frame-list variants): declared in the header,
bound in capi.py and exported by the built library; the header states the contract's sentences; the new kernels use no scratch
memory; the C++ adapters compile with the new methods (CPU) and answer like the brute force (GPU, the one test marked so).
The compute tests are tests/test_kd_radius_gpu.py and tests/test_kfmap_radius_gpu.py."""
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from avoid_mpc_amd import build as amk_build
from avoid_mpc_amd import capi
from tests import _radius as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["amk_kd_radius_search", "amk_kd_radius_search_host", "amk_kfmap_radius_search", "amk_kfmap_radius_search_host",
       "amk_kd_radius_search_frames", "amk_kd_radius_search_frames_host"]


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
    for sentence in ["a SQUARED distance, as nanoflann's L2 radius is",
                     "The test is strict: a result has squared distance < radius_sq, a point at exactly radius_sq is not a result",
                     "The count is never capped: it is always the full number, whatever max_results",
                     "The size rule does not apply",
                     "a cloud of one point, or of exactly max_results points, answers normally",
                     "max_results == 0 requires every list pointer NULL",
                     "the tie-order modes do not apply",
                     "there is no fast path and no PtIsInFrame",
                     "equal distances keep the earlier frame, then the lower cloud index within a frame",
                     "The reference never calls it",
                     "per-query radii, uncapped result lists (a CSR output), radius queries inside amk_step_batch"]:
        assert sentence in text, sentence


def test_the_radius_kernels_use_no_scratch(lib):
    table = json.load(open(amk_build.RES))
    mine = {n: r for n, r in table.items() if "kd_radius_search_kernel" in n or "map_radius_kernel" in n}
    assert len(mine) == 3, sorted(mine)                 # one handle; a keyframe map; a list of handles
    search = [r for n, r in table.items() if "kd_grid_search_kernel" in n][0]
    for n, r in mine.items():
        assert r["scratch_bytes_per_lane"] == 0, (n, r)
        assert r["lds_bytes"] == search["lds_bytes"], (n, r, search)   # four GridWaveLds, nothing else
        assert r["vgprs"] <= 128, (n, r)                                # four waves per SIMD at least


def test_argument_checks_need_no_device(lib):
    """NULL handles are refused before anything touches the device."""
    inv = capi.AMK_ERR_INVALID_ARG
    assert lib.amk_kd_radius_search(None, None, 3, 1, 1.0, 1, None, None, None, None, None) == inv
    assert lib.amk_kd_radius_search_host(None, None, 3, 1, 1.0, 1, None, None, None, None) == inv
    assert lib.amk_kfmap_radius_search(None, None, 3, 1, 1.0, 1, 0, None, None, None, None, None) == inv
    assert lib.amk_kfmap_radius_search_host(None, None, 3, 1, 1.0, 1, 0, None, None, None, None) == inv
    assert lib.amk_kd_radius_search_frames(None, 1, None, 3, 1, 1.0, 1, None, None, None, None, None) == inv
    assert lib.amk_kd_radius_search_frames_host(None, 1, None, 3, 1, 1.0, 1, None, None, None, None) == inv


def test_python_hosts_offer_the_radius_search():
    from avoid_mpc_amd import host
    assert callable(host.KdBatch.radius_search) and callable(host.KdBatch.radius_search_host)
    assert callable(host.KfMap.radius_search) and callable(host.radius_search_frames)


def compile_demo(tmp_path):
    """built the way tests/test_cpp_adapters_gpu.py builds its host"""
    exe = str(tmp_path / "radius_demo")
    libdir = os.path.join(ROOT, "avoid_mpc_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "radius_demo.cpp"), "-o", exe,
                           "-L", libdir, "-lavoid_mpc_amd", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_adapters_compile_with_the_new_methods(lib, tmp_path):
    hpp = open(os.path.join(ROOT, "include", "avoid_mpc_amd", "kd_tree_two.hpp")).read()
    assert "size_t RadiusSearch(num_t x, num_t y, num_t z, double radius_sq, int max_results)" in hpp
    fk = open(os.path.join(ROOT, "include", "avoid_mpc_amd", "frame_kd_map.hpp")).read()
    assert "size_t QueryRadius(const Vector3d &point, double radius_sq, int max_results" in fk
    assert os.path.exists(compile_demo(tmp_path))


@pytest.mark.gpu
def test_cpp_adapters_answer_like_the_brute_force(tmp_path):
    exe = compile_demo(tmp_path)
    rng = np.random.default_rng(23)
    n, nq, k, r2 = 3000, 12, 8, 0.5
    cloud = (np.round(rng.random((n, 3)) * [6.0, 5.0, 3.0] * 8) / 8).astype(np.float32)   # quantised: equal distances occur
    qs = np.round(rng.random((nq, 3)) * [6.0, 5.0, 3.0] * 8) / 8
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("3i", n, nq, k)); f.write(struct.pack("d", r2)); f.write(cloud.tobytes()); f.write(qs.tobytes())
    subprocess.check_call([exe, fin, fout])
    buf = open(fout, "rb").read()
    off = 0

    def take(dtype, cnt):
        nonlocal off
        a = np.frombuffer(buf, dtype=dtype, count=cnt, offset=off)
        off += a.nbytes
        return a

    seen = 0
    for q in qs:                                         # KDTreeTwo::RadiusSearch
        count, c = (int(v) for v in take(np.int32, 2))
        e = R.radius_brute(cloud, q, r2, k)
        assert count == e["count"] and c == min(count, k)
        assert np.array_equal(take(np.int32, c), e["indices"][:c]) and np.array_equal(take(np.float64, c), e["sqdist"][:c])
        assert np.array_equal(take(np.float32, 3 * c).reshape(-1, 3), e["pts"][:c])
        seen += count > k
    assert seen >= 3                                     # (the count does exceed the list)
    for q in qs:                                         # FrameKDMap::QueryRadius over [second half, first half]
        count, c = (int(v) for v in take(np.int32, 2))
        e = R.radius_brute_frames([cloud[n // 2:], cloud[:n // 2]], q, r2, k)
        assert count == e["count"] and c == min(count, k)
        assert np.array_equal(take(np.float64, c), e["sqdist"][:c])
        assert np.array_equal(take(np.float64, 3 * c).reshape(-1, 3), e["pts"][:c].astype(np.float64))
    assert off == len(buf)
