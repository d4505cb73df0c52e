"""Path cast and the pipeline's audit in the C ABI (amk_kd_path_cast and its host, keyframe-map and frame-list variants,
amk_pipeline_set_path_audit, amk_pipeline_audit_outputs): declared in the header, bound in capi.py and exported by the built
library; the header states the contract's sentences; the new kernels use no scratch memory and at most 128 VGPRs; the case done by
hand holds in the numpy restatement (tests/_path_cast.py); the C++ adapters compile with the new methods (CPU) and answer like the
restatement (GPU, the one test marked so).  The compute tests are tests/test_kd_path_cast_gpu.py, tests/test_kfmap_path_cast_gpu.py
and tests/test_pipeline_audit_gpu.py."""
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from avoid_mpc_amd import build as amk_build
from avoid_mpc_amd import capi
from tests import _path_cast as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASTS = ["amk_kd_path_cast", "amk_kd_path_cast_host", "amk_kfmap_path_cast", "amk_kfmap_path_cast_host",
         "amk_kd_path_cast_frames", "amk_kd_path_cast_frames_host"]
NEW = CASTS + ["amk_pipeline_set_path_audit", "amk_pipeline_audit_outputs"]


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
        if name in CASTS:
            assert "max_results" not in decl and "radius_sq" in decl and "_stop" in decl and "_free" in decl, name
    assert not capi.missing_symbols()
    assert (capi.AMK_AUDIT_OFF, capi.AMK_AUDIT_REPORT, capi.AMK_AUDIT_SLOW_DOWN) == (0, 1, 2)
    for name, value in (("AMK_AUDIT_OFF", 0), ("AMK_AUDIT_REPORT", 1), ("AMK_AUDIT_SLOW_DOWN", 2)):
        assert re.search(r"^#define " + name + r" " + str(value) + r"\b", hdr, re.M), name


def test_header_states_the_contract():
    text = " ".join(re.sub(r"^\s*\*", " ", line) for line in header().splitlines())
    text = re.sub(r"\s+", " ", text)
    for sentence in ["Path cast: one answer per scene for a whole path -- the first leg that cannot be passed",
                     "are exactly those of \"Segment cast\" above, and so is every per-point formula",
                     "The stop leg of a scene is the first leg j, in leg order, for which one of these holds",
                     "the leg has a contact by the segment cast's rule",
                     "the least (t, index)",
                     "the leg is unjudgeable: it has a non-finite endpoint coordinate or a non-finite L2",
                     "an audit must not read a NaN trajectory as free",
                     "0 = free to the end, 1 = contact, 2 = unjudgeable leg",
                     "the stop leg, -1 when free",
                     "0.0 when d_stop is 2, 1.0 when free",
                     "((len_0 + len_1) + ... + len_{leg-1}) + t * len_leg with len_j = sqrt(L2_j)",
                     "fp64 with contraction off, summed left to right",
                     "term is left out when d_stop is 2",
                     "A free path gives its whole length",
                     "(0,0,0) unless d_stop is 1",
                     "-1 unless d_stop is 1",
                     "Each output may be NULL, but not all of them",
                     "A degenerate leg has length 0 and stops the path iff a usable point lies inside at its start",
                     "the answer equals this reduction applied to amk_kd_segment_cast's per-leg outputs on the same path, bit for bit",
                     "d_free is rebuilt from the path by the formula",
                     "The legs behind the stop leg are never walked",
                     "Every error is returned before anything is staged or launched, the outputs untouched",
                     "The call is stream-ordered and allocates nothing",
                     "the least (t, frame, index) over the frames its scene holds",
                     "the frame touched, -1 unless d_stop is 1",
                     "Scan-mode handles, tie-order handles in the frame list and n_frames > AMK_MAX_FRAMES return AMK_ERR_UNSUPPORTED "
                     "before anything is staged or launched",
                     "no map state changed",
                     # the pipeline's paragraph
                     "The trajectory audit, off by default",
                     "row 0 is X0, the state the step planned from",
                     "after the step and before the command is written",
                     "amk_kd_path_cast(the slot's obstacle index, x0array, 14, n_legs + 1, radius * radius, ...)",
                     "on the map as it stands after the period's AddVertex and update",
                     "publishes PubSlowDownCmd instead of u for a scene with flags[0] == 1 whose audit stops (d_stop != 0)",
                     "the verdict lives only in the audit outputs and the command",
                     "valid only while no frame is staged or in flight on any slot",
                     "else AMK_ERR_UNSUPPORTED",
                     "n_legs outside [0, N - 1]: AMK_ERR_INVALID_ARG",
                     "submit and launch allocate nothing more",
                     "AMK_AUDIT_OFF frees nothing and stops the stage",
                     "a frame that brings its own keyframe list (n_keyframes > 0) is refused at submit with AMK_ERR_UNSUPPORTED",
                     "Not offered: the audit inside amk_step_batch, amk_step_batch_frames or amk_kfmap_step"]:
        assert sentence in text, sentence


def test_the_path_cast_kernels_meet_the_resource_limits(lib):
    table = json.load(open(amk_build.RES))
    mine = {n: r for n, r in table.items() if "kd_path_cast_kernel" in n or "map_path_cast_kernel" in n}
    assert len(mine) == 3, sorted(mine)                 # one handle; a keyframe map; a list of handles
    search = [r for n, r in table.items() if "kd_grid_search_kernel" in n][0]
    for n, r in mine.items():
        waves = int(re.search(r"Li(\d+)E", n).group(1))  # the template's W: waves per block = legs per round
        assert r["scratch_bytes_per_lane"] == 0, (n, r)
        assert r["lds_bytes"] == waves * (search["lds_bytes"] // 4 + 2 * 40), (n, r, search)   # a GridWaveLds and two 40-byte leg records per wave
        assert r["vgprs"] <= 128, (n, r)                                                       # four waves per SIMD at least
    veto = [r for n, r in table.items() if "pipeline_audit_veto_kernel" in n]
    assert len(veto) == 1 and veto[0]["scratch_bytes_per_lane"] == 0 and veto[0]["lds_bytes"] == 0


def test_argument_checks_need_no_device(lib):
    """NULL handles are refused before anything touches the device."""
    inv = capi.AMK_ERR_INVALID_ARG
    n6 = [None] * 6
    assert lib.amk_kd_path_cast(None, None, 3, 2, 0.25, *n6, None) == inv
    assert lib.amk_kd_path_cast_host(None, None, 3, 2, 0.25, *n6) == inv
    assert lib.amk_kfmap_path_cast(None, None, 3, 2, 0.25, 0, *n6, None) == inv
    assert lib.amk_kfmap_path_cast_host(None, None, 3, 2, 0.25, 0, *n6) == inv
    assert lib.amk_kd_path_cast_frames(None, 1, None, 3, 2, 0.25, *n6, None) == inv
    assert lib.amk_kd_path_cast_frames_host(None, 1, None, 3, 2, 0.25, *n6) == inv
    assert lib.amk_pipeline_set_path_audit(None, 1, 0.5, 0) == inv
    assert lib.amk_pipeline_audit_outputs(None, 0, *n6) == inv


def test_python_hosts_offer_the_path_cast_and_the_audit():
    from avoid_mpc_amd import host
    assert callable(host.KdBatch.path_cast) and callable(host.KdBatch.path_cast_host)
    assert callable(host.KfMap.path_cast) and callable(host.path_cast_frames)
    assert callable(host.Pipeline.set_path_audit) and callable(host.Pipeline.audit_outputs)


def test_the_case_done_by_hand_holds_in_the_restatement():
    cloud = np.array([[2.0, 0.375, 0.0], [6.0, 0.0, 0.0], [9.0, 5.0, 5.0]], np.float32)
    path = np.array([[[-3.0, 0.0, 0.0], [0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [20.0, 0.0, 0.0]]])
    e = P.expected_batch([[cloud]], path, 0.25)
    t = (20.0 - np.sqrt(400.0 - 389.0625)) * (1.0 / 100.0)
    assert e["stop"].tolist() == [1] and e["leg"].tolist() == [1] and e["indices"].tolist() == [0] and e["pts"][0].tolist() == [2.0, 0.375, 0.0]
    assert e["t"][0] == t and e["free"][0] == 3.0 + t * 10.0
    # nothing within reach: free to the end, the whole length, summed left to right
    e = P.expected_batch([[cloud[[0, 2]]]], path, 0.0625)
    assert e["stop"].tolist() == [0] and e["leg"].tolist() == [-1] and e["t"].tolist() == [1.0] and e["free"][0] == (3.0 + 10.0) + 10.0
    assert e["indices"].tolist() == [-1] and (e["pts"] == 0).all()
    # a NaN in point 2 spoils legs 1 and 2: unjudgeable at leg 1, t 0, free = leg 0 alone, no point -- unless leg 0 stops first
    bad = path.copy(); bad[0, 2, 1] = np.nan
    e = P.expected_batch([[cloud]], bad, 0.25)
    assert e["stop"].tolist() == [2] and e["leg"].tolist() == [1] and e["t"].tolist() == [0.0] and e["free"].tolist() == [3.0]
    assert e["indices"].tolist() == [-1] and (e["pts"] == 0).all()
    e = P.expected_batch([[np.array([[-2.0, 0.25, 0.0]], np.float32)]], bad, 0.25)
    assert e["stop"].tolist() == [1] and e["leg"].tolist() == [0] and 0.0 < e["t"][0] < 1.0 and e["free"][0] == e["t"][0] * 3.0
    # over frames: an equal t keeps the earlier frame
    e = P.expected_batch([[cloud, cloud]], path, 0.25)
    assert e["stop"].tolist() == [1] and e["frame"].tolist() == [0]
    # the reduction of per-leg answers is the same function
    legs = P.K.expected_batch([[cloud]], path, 0.25)
    P.assert_bitwise(P.reduce_legs(legs, path), P.expected_batch([[cloud]], path, 0.25), P.KEYS, "reduction")


def compile_demo(tmp_path):
    """built the way tests/test_cpp_adapters_gpu.py builds its host"""
    exe = str(tmp_path / "path_cast_demo")
    libdir = os.path.join(ROOT, "avoid_mpc_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "path_cast_demo.cpp"), "-o", exe,
                           "-L", libdir, "-lavoid_mpc_amd", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_adapters_compile_with_the_new_methods(lib, tmp_path):
    hpp = open(os.path.join(ROOT, "include", "avoid_mpc_amd", "kd_tree_two.hpp")).read()
    assert "int PathCast(const double *path_xyz, int n_points, double radius_sq, int &leg, double &t, double &free_dist)" in hpp
    fk = open(os.path.join(ROOT, "include", "avoid_mpc_amd", "frame_kd_map.hpp")).read()
    assert "int QueryPathCast(const std::vector<Vector3d> &path, double radius_sq, int &leg, double &t, double &freeDist, Vector3d &point" in fk
    assert os.path.exists(compile_demo(tmp_path))


@pytest.mark.gpu
def test_cpp_adapters_answer_like_the_restatement(tmp_path):
    exe = compile_demo(tmp_path)
    rng = np.random.default_rng(23)
    n, npaths, npts, r2 = 400, 10, 7, 0.04
    cloud = (np.round(rng.random((n, 3)) * [6.0, 5.0, 3.0] * 8) / 8).astype(np.float32)   # quantised: equal t occur
    paths = np.round(rng.random((npaths, npts, 3)) * [6.0, 5.0, 3.0] * 8) / 8
    paths[:5, 1:] = paths[:5, :1] + np.cumsum(np.round((rng.random((5, npts - 1, 3)) - 0.5) * 4) / 8, axis=1)   # half of them in short legs
    paths[3, 2] = paths[3, 1]                                                             # with a degenerate leg
    paths[3, 6, 0] = np.nan                                                               # and an unjudgeable one behind it
    paths[9] += 100.0                                                                     # one far from everything
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("3i", n, npaths, npts)); f.write(struct.pack("d", r2)); f.write(cloud.tobytes()); f.write(paths.tobytes())
    subprocess.check_call([exe, fin, fout])
    buf = open(fout, "rb").read()
    off = 0

    def take(dtype, cnt):
        nonlocal off
        a = np.frombuffer(buf, dtype=dtype, count=cnt, offset=off)
        off += a.nbytes
        return a

    one = P.expected_batch([[cloud]] * npaths, paths, r2)
    two = P.expected_batch([[cloud[n // 2:], cloud[:n // 2]]] * npaths, paths, r2)
    for i in range(npaths):                              # KDTreeTwo::PathCast
        stop, leg, index = (int(v) for v in take(np.int32, 3))
        assert (stop, leg, index) == (one["stop"][i], one["leg"][i], one["indices"][i]), i
        t, free = take(np.float64, 2)
        assert t == one["t"][i] and free == one["free"][i] and np.array_equal(take(np.float32, 3), one["pts"][i]), i
    assert one["stop"].tolist() == [1, 1, 1, 2, 1, 1, 1, 1, 1, 0] and one["leg"].tolist() == [1, 3, 4, 5, 0, 0, 0, 0, 0, -1]
    assert two["frame"].tolist() == [0, 1, 1, -1, 0, 0, 0, 0, 1, -1]
    for i in range(npaths):                              # FrameKDMap::QueryPathCast over [second half, first half]
        stop, leg = (int(v) for v in take(np.int32, 2))
        assert (stop, leg) == (two["stop"][i], two["leg"][i]), i
        t, free = take(np.float64, 2)
        assert t == two["t"][i] and free == two["free"][i], i
        assert np.array_equal(take(np.float64, 3), two["pts"][i].astype(np.float64)), i
    assert off == len(buf)
