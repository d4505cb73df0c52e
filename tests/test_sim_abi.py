"""CPU: the closed-loop simulation's C ABI (amk_sim_render_depth, amk_sim_vehicle_step and their _host variants) without a device --
the symbols are declared, bound and exported; bad arguments are refused before the device is asked for; the header states the
contract; the kernels use no scratch; and the numpy restatement of the render's operation order (flight.render_depth_ordered)
gives the depth flights' frames (tests/_flight.py _depth_frame, on flight.render_depth) pixel for pixel."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from avoid_mpc_amd import build as amk_build
from avoid_mpc_amd import capi, flight
from avoid_mpc_amd.host import depth_params
from tests import _flight

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOUR = ["amk_sim_render_depth", "amk_sim_render_depth_host", "amk_sim_vehicle_step", "amk_sim_vehicle_step_host"]
BAD, UNSUPPORTED = capi.AMK_ERR_INVALID_ARG, capi.AMK_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def lib():
    amk_build.build()
    return capi.load()


def _header():
    return open(os.path.join(ROOT, "include", "avoid_mpc_amd.h")).read()


def test_the_four_symbols_are_declared_bound_and_exported(lib):
    hdr = _header()
    for name in FOUR:
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name          # declared
        assert name in capi.SYMBOLS                                          # listed
        fn = getattr(lib, name)                                              # exported
        assert fn.argtypes is not None and fn.restype is C.c_int, name       # bound
    assert len(lib.amk_sim_render_depth.argtypes) == 13 and len(lib.amk_sim_render_depth_host.argtypes) == 12
    assert len(lib.amk_sim_vehicle_step.argtypes) == 7 and len(lib.amk_sim_vehicle_step_host.argtypes) == 6
    section = hdr[hdr.index("Closed-loop simulation"):]
    assert all(name in section for name in FOUR)                             # a section of their own at the header's end
    assert "amk_depth_to_clouds_host(" not in section


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def test_render_refuses_bad_arguments_without_a_device(lib):
    p = depth_params(pixel2meter=1e-3)
    cyl = np.ones((2, 3, 3)); cnt = np.full(2, 3, np.int32); T = np.tile(np.eye(4), (2, 1, 1)); img = np.full((2, 4, 5), 7, np.uint16)
    U16, F32 = capi.AMK_DEPTH_U16, capi.AMK_DEPTH_F32
    for fn, tail in ((lib.amk_sim_render_depth, (None,)), (lib.amk_sim_render_depth_host, ())):
        call = lambda cyl_=_vp(cyl), cnt_=_vp(cnt), mc=3, S=2, zt=4.0, mr=60.0, pp=C.byref(p), rows=4, cols=5, T_=_vp(T), out=_vp(img), kind=U16: \
            fn(cyl_, cnt_, mc, S, zt, mr, pp, rows, cols, T_, out, kind, *tail)
        assert call(cyl_=None) == BAD and call(T_=None) == BAD and call(out=None) == BAD and call(pp=None) == BAD
        assert call(rows=0) == BAD and call(cols=0) == BAD and call(rows=-3) == BAD
        assert call(mc=-1) == BAD and call(S=0) == BAD and call(S=-2) == BAD
        assert call(zt=-1.0) == BAD and call(zt=float("nan")) == BAD and call(mr=-0.5) == BAD and call(mr=float("nan")) == BAD
        assert call(kind=2) == BAD and call(kind=-1) == BAD and call(kind=7) == BAD
        q = depth_params(pixel2meter=0.0)
        assert call(pp=C.byref(q)) == BAD
        assert call(rows=1 << 20, cols=1 << 20, S=2) == UNSUPPORTED            # 2^33 blocks of 256 pixels
        assert call(rows=46341, cols=46341, S=256) == UNSUPPORTED              # 2^31 / 256 tiles and a bit, times 256 scenes
        assert call(S=65536) == UNSUPPORTED
        if lib.amk_device_count() <= 0:                                        # a good call reaches the device question and nothing else
            assert call() == capi.AMK_ERR_NO_DEVICE and call(cnt_=None) == capi.AMK_ERR_NO_DEVICE
            assert call(cyl_=None, mc=0) == capi.AMK_ERR_NO_DEVICE and call(kind=F32) == capi.AMK_ERR_NO_DEVICE
    assert (img == 7).all()


def test_vehicle_refuses_bad_arguments_without_a_device(lib):
    ABc = np.zeros(150); cmd = np.zeros((2, 3)); x = np.full((2, 10), 3.0); T = np.full((2, 16), 5.0)
    for fn, tail in ((lib.amk_sim_vehicle_step, (None,)), (lib.amk_sim_vehicle_step_host, ())):
        call = lambda m=_vp(ABc), c=_vp(cmd), x_=_vp(x), T_=_vp(T), S=2, q=1e6: fn(m, c, x_, T_, S, q, *tail)
        assert call(m=None) == BAD and call(c=None) == BAD and call(x_=None) == BAD
        assert call(S=0) == BAD and call(S=-1) == BAD and call(q=-1.0) == BAD and call(q=float("nan")) == BAD
        if lib.amk_device_count() <= 0:
            assert call() == capi.AMK_ERR_NO_DEVICE and call(T_=None) == capi.AMK_ERR_NO_DEVICE and call(q=0.0) == capi.AMK_ERR_NO_DEVICE
    assert (x == 3.0).all() and (T == 5.0).all()


def test_the_header_states_the_contract():
    section = _header()
    section = re.sub(r"\s*\*?\s+", " ", section[section.index("Closed-loop simulation"):])   # comment stars and line breaks out
    for sentence in ("The comparison is a strict <", "the ground and then the lower cylinder index keep it",
                     "rounded to the nearest integer, ties to even, clamped to [0, 65535]", "rint(t / pixel2meter)",
                     "allocates nothing", "Every error is returned before anything is launched",
                     "every sum left to right in index order", "At yaw == 0 the rotation is exactly the identity",
                     "x+_i = ((sum_j A_ij x_j) + (sum_j B_ij u_j)) + c_i", "HOST pointer to 150 doubles"):
        assert sentence in section, sentence
    assert section.count("allocates nothing") >= 2   # both calls say so


def test_the_sim_kernels_use_no_scratch(lib):
    table = json.load(open(amk_build.RES))
    render = {n: r for n, r in table.items() if "17sim_render_kernel" in n}
    vehicle = {n: r for n, r in table.items() if "18sim_vehicle_kernel" in n}
    assert len(render) == 3 and len(vehicle) == 1, (sorted(render), sorted(vehicle))   # U16, F32, the tests' fp64 t; the vehicle
    for n, r in {**render, **vehicle}.items():
        print(n, r)
        assert r["scratch_bytes_per_lane"] == 0, (n, r)
    for n, r in render.items():
        assert r["occupancy"] >= 8 and r["lds_bytes"] <= 4096, (n, r)   # fp64 VALU bound: the full eight waves per SIMD, chunks of a few KB
    per_object = {os.path.basename(p)[:-len(".o.res.json")]: list(json.load(open(p)))
                  for p in __import__("glob").glob(os.path.join(amk_build.OBJ, "*.o.res.json"))}
    assert [u for u, ks in per_object.items() if any("sim_render_kernel" in k or "sim_vehicle_kernel" in k for k in ks)] == ["sim"]


SEEDS, PERIODS = (3, 11, 29), 5


def _poses(seed):
    """(world, the states whose poses _depth_frame renders): a flight's start, then five periods under a constant command that climbs
    and drifts sideways, so that no position is a round number"""
    prm, _ = _flight.make_prm("C1")
    world = flight.FlightWorld(seed, prm, 1000)
    x, _ = flight.initial_state(seed, prm)
    xs = []
    for _t in range(PERIODS):
        xs.append(x.copy())
        x = flight.apply_command(x[None], np.array([[1.3, -0.7, flight.GZ + 0.4]]), prm)[0]
    return world, xs


@pytest.mark.parametrize("seed", SEEDS)
def test_the_ordered_restatement_renders_the_depth_flights_frames(seed):
    """flight.render_depth_ordered + quantise_depth against _depth_frame (flight.render_depth, matrix products in numpy's order) on
    _depth_frame's own poses and cylinder selection: identical uint16 images, millimetres.  The two differ in the order of a few
    fp64 sums, i.e. by ulps of t; a pixel changes only if such an ulp straddles a rounding boundary of the float32 conversion.  The
    allowed share of such pixels is 0 on these inputs -- any that differ are listed with both fp64 values."""
    c = _flight.DEPTH_CAM
    world, xs = _poses(seed)
    for t, x in enumerate(xs):
        img, Twb = _flight._depth_frame(world, x, c)
        sel = (world.cx > x[0] - 2.0) & (world.cx < x[0] + 40.0)
        cyl = (world.cx[sel], world.cy[sel], world.cr[sel])
        args = (cyl, Twb, c["Tbc"], c["rows"], c["cols"], c["fx"], c["fy"], c["cx"], c["cy"])
        t_ord = flight.render_depth_ordered(*args)
        mine = flight.quantise_depth(t_ord, c["pixel2meter"], np.uint16)
        assert mine.dtype == np.uint16 and mine.shape == img.shape
        assert (img > 0).sum() > 0.3 * img.size and sel.sum() >= 8                     # (a frame with a scene in it)
        diff = np.argwhere(mine != img)
        if len(diff):
            old = flight.render_depth(*args).astype(np.float64)
            for r, q in diff[:20]:
                print(f"seed {seed} period {t} pixel ({r}, {q}): ordered t = {t_ord[r, q]!r} -> {mine[r, q]}, render_depth = {old[r, q]!r} -> {img[r, q]}")
        assert len(diff) == 0, (seed, t, len(diff))
        f32 = flight.quantise_depth(t_ord, 1.0, np.float32)
        assert f32.dtype == np.float32 and np.array_equal(f32, t_ord.astype(np.float32))   # pixel2meter 1: the float32 depth itself


def test_vehicle_restatement_is_the_affine_plant():
    """flight.vehicle_step_ordered on (A, B, c) of flight.affine_plant is the plant of apply_command to rounding (the model is exactly
    affine; the two sum in different orders): 1e-12 on states of order 10."""
    prm, _ = _flight.make_prm("C1")
    A, B, c = flight.affine_plant(prm.tau, prm.dt)
    ABc = np.concatenate([A.reshape(-1), B.reshape(-1), c])
    rng = np.random.default_rng(5)
    x = rng.uniform(-10, 10, (6, 10)); x[:, 3] = 0.0; cmd = rng.uniform(-3, 12, (6, 3))
    xn, T = flight.vehicle_step_ordered(ABc, x, cmd, 1e6)
    assert np.abs(xn - flight.apply_command(x, cmd, prm)).max() < 1e-12
    assert np.array_equal(T[:, :3, :3], np.tile(np.eye(3), (6, 1, 1))) and not np.signbit(T[:, :3, :3]).any()
    assert np.array_equal(T[:, :3, 3], np.round(xn[:, 0:3], 6))
    assert np.array_equal(flight.vehicle_step_ordered(ABc, x, cmd, 0.0)[1][:, :3, 3], xn[:, 0:3])
