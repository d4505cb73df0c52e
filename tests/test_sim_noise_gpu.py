"""GPU: amk_sim_depth_noise against its numpy restatement (flight.depth_noise_ordered) bit for bit, for both pixel types, on images
of one pixel, one row, one column, sizes that are no multiple of the block, rows that straddle a block and exactly one block and one
pixel more, with scene strides larger than the image (the padding untouched); every stage alone and all together, every probability
at 0 and at 1; the stream itself (amk__sim_noise_words) against flight.noise_words; the _host form against the device call byte for
byte; every argument error with the output left unwritten; the scene_id0 split identity; a non-default stream."""
import ctypes as C

import numpy as np
import pytest

from avoid_mpc_amd import capi, flight
from tests import _sim_noise

pytestmark = pytest.mark.gpu

P2M = _sim_noise.P2M
BAD, UNSUPPORTED = capi.AMK_ERR_INVALID_ARG, capi.AMK_ERR_UNSUPPORTED
NAN = float("nan")
EDGE = dict(seed=21, edge_jump=0.25)
# every stage alone, every probability at 0 and at 1, the two edge outcomes filling [0, 1], and all together
SETTINGS = {
    "off": {},
    "seed only": dict(seed=5, focal_baseline=3.0),
    "axial": dict(seed=1, sigma0=0.004, sigma2=0.0025), "axial sigma0": dict(seed=2, sigma0=0.02), "axial sigma2": dict(seed=3, sigma2=0.01),
    "drop": dict(seed=4, p_drop=0.3), "drop 1": dict(seed=4, p_drop=1.0),
    "edge 0 0": dict(EDGE), "edge drop": dict(EDGE, p_edge_drop=0.5), "edge drop 1": dict(EDGE, p_edge_drop=1.0),
    "edge fly": dict(EDGE, p_edge_fly=0.5), "edge fly 1": dict(EDGE, p_edge_fly=1.0), "edge sum 1": dict(EDGE, p_edge_drop=0.4, p_edge_fly=0.6),
    "edge wide": dict(EDGE, edge_jump=30.0, p_edge_fly=1.0),                     # only missing neighbours make an edge: no partner anywhere
    "disparity": dict(focal_baseline=38.0, disparity_quantum=0.125), "disparity coarse": dict(focal_baseline=5.0, disparity_quantum=1.0),
    "range": dict(z_min=0.3, z_max=25.0), "range min": dict(z_min=2.0),
    "all": _sim_noise.EVERY_STAGE, "all harsh": dict(_sim_noise.EVERY_STAGE, seed=77, p_drop=0.2, sigma2=0.02, p_edge_drop=0.5, p_edge_fly=0.5),
}
# (S, rows, cols, scene stride or None = rows cols)
SHAPES = [(1, 1, 1, None), (2, 1, 7, None), (2, 7, 1, None), (3, 17, 19, None), (2, 3, 300, None), (1, 2, 256, None), (2, 2, 257, None),
          (2, 17, 19, 17 * 19 + 5), (3, 3, 300, 1024)]
FILL = {np.uint16: 0xA5A5, np.float32: np.array(0xA5A5A5A5, np.uint32).view(np.float32)}   # what an unwritten output pixel holds


def _kind(dtype):
    return capi.AMK_DEPTH_F32 if np.dtype(dtype) == np.float32 else capi.AMK_DEPTH_U16


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _strided(img, stride, fill):
    """[S, rows, cols] -> flat [S * stride] with `fill` between the images"""
    S, rows, cols = img.shape
    flat = np.full(S * stride, fill, img.dtype)
    flat.reshape(S, stride)[:, :rows * cols] = img.reshape(S, -1)
    return flat


def _params(setting):
    from avoid_mpc_amd.host import sim_noise_params
    return sim_noise_params(setting)


def _device(torch, img, setting, frame, scene_id0=0, stride=None, stream=None):
    """amk_sim_depth_noise on a flat, possibly strided buffer -> the whole output buffer (flat), numpy"""
    S, rows, cols = img.shape
    stride = stride or rows * cols
    as_torch = lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
    d_in, d_out = as_torch(_strided(img, stride, FILL[img.dtype.type])), as_torch(np.full(S * stride, FILL[img.dtype.type], img.dtype))
    capi.check(capi.load().amk_sim_depth_noise(capi.dptr(d_in), capi.dptr(d_out), _kind(img.dtype), rows, cols, stride, S, P2M, C.byref(_params(setting)),
                                               scene_id0, frame, capi.stream_ptr(stream)), "amk_sim_depth_noise")
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    return d_out.cpu().numpy().view(img.dtype)


def _host(img, setting, frame, scene_id0=0, stride=None):
    S, rows, cols = img.shape
    stride = stride or rows * cols
    h_in, h_out = _strided(img, stride, FILL[img.dtype.type]), np.full(S * stride, FILL[img.dtype.type], img.dtype)
    capi.check(capi.load().amk_sim_depth_noise_host(h_in.ctypes.data_as(C.c_void_p), h_out.ctypes.data_as(C.c_void_p), _kind(img.dtype), rows, cols,
                                                    stride, S, P2M, C.byref(_params(setting)), scene_id0, frame), "amk_sim_depth_noise_host")
    return h_out


@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=["u16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_the_kernel_is_the_restatement_bit_for_bit(shape, dtype):
    import torch
    S, rows, cols, stride = shape
    img = _sim_noise.noise_images(31, S, rows, cols, dtype)
    frame, scene_id0 = 3 + rows, 1000 * cols
    seen = dict(zeroed=0, changed=0, flown=0)
    for name, setting in SETTINGS.items():
        parts = {}
        want = flight.depth_noise_ordered(img, setting, P2M, frame, scene_id0, parts=parts)
        got = _device(torch, img, setting, frame, scene_id0, stride)
        full = _strided(want, stride or rows * cols, FILL[dtype])                 # the padding between the images is left as it was
        assert np.array_equal(_bits(got), _bits(full)), (name, np.argwhere(_bits(got) != _bits(full))[:5])
        if name in ("off", "seed only"):
            assert want.tobytes() == img.tobytes()
        if name in ("all", "edge fly 1", "disparity", "range"):                   # the _host form, byte for byte, padding included
            assert _host(img, setting, frame, scene_id0, stride).tobytes() == got.tobytes(), name
        seen["zeroed"] += int(((want == 0) & (img != 0)).sum()); seen["changed"] += int((_bits(want) != _bits(img)).sum())
        seen["flown"] += int(parts["flown"].sum())
    if rows * cols >= 300:                                                        # the settings did something to these images
        assert seen["zeroed"] > 50 and seen["changed"] > 500 and seen["flown"] > 20, seen


def test_the_images_hold_what_the_stages_must_meet():
    """the interior edge, edges on every border and corner, missing blocks and pixels, the clamp, both range gates, odd float32 pixels"""
    jump = 0.25
    for dtype in (np.uint16, np.float32):
        img = _sim_noise.noise_images(31, 3, 17, 19, dtype)
        parts = {}
        flight.depth_noise_ordered(img, dict(seed=1, edge_jump=jump, p_edge_fly=1.0), P2M, 0, parts=parts)
        disc, valid, z = parts["disc"], parts["valid"], parts["z_in"]
        border = [disc[:, 0, :], disc[:, -1, :], disc[:, :, 0], disc[:, :, -1]]
        assert all(b.any() for b in border) and disc[:, 1:-1, 1:-1].any()
        assert any(disc[s, r, c] for s in range(3) for r in (0, -1) for c in (0, -1))
        assert (~valid).sum() > 30 and parts["flown"].sum() > 30 and (disc & ~parts["partner"]).any()
        assert (valid & (z < 0.3)).any() and (valid & (z > 25.0)).any() and (z == np.float32(0.3)).any()
        if dtype == np.uint16:
            assert (img == 65535).any() and (img == 0).any()
        else:
            assert np.isnan(img).any() and np.isposinf(img).any() and np.isneginf(img).any() and (img < 0).any() and (z > 65.535).any()


def test_the_clamp_of_the_u16_store_is_reached():
    """depths near 65.535 m pushed past the last count by the axial stage come back as 65535, on the device as in numpy"""
    import torch
    img = np.full((1, 4, 70), 65500, np.uint16)
    setting = dict(seed=6, sigma0=0.05)
    want = flight.depth_noise_ordered(img, setting, P2M, 0)
    assert (want == 65535).sum() > 20 and (want < 65500).any()
    assert np.array_equal(_device(torch, img, setting, 0).reshape(img.shape), want)


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 300), (3, 17, 19), (1, 2, 257)], ids=lambda s: "x".join(str(v) for v in s))
def test_the_words_are_the_restatements(shape):
    import torch
    S, rows, cols = shape
    lib = capi.load()
    for seed, scene_id0, frame in ((0, 0, 0), (7, 255, 5), (2 ** 64 - 1, -2, 2 ** 63 + 1)):
        out = torch.zeros((S, rows, cols, 3), dtype=torch.int64, device="cuda")
        capi.check(lib.amk__sim_noise_words(capi.dptr(out), rows, cols, S, seed, scene_id0, frame, capi.stream_ptr()), "amk__sim_noise_words")
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), flight.noise_words(seed, scene_id0, frame, S, rows, cols)), (seed, scene_id0, frame)


def test_a_split_fleet_draws_the_same_stream_on_the_device():
    import torch
    for dtype in (np.uint16, np.float32):
        img = _sim_noise.noise_images(32, 4, 17, 19, dtype)
        whole = _device(torch, img, _sim_noise.EVERY_STAGE, 9, scene_id0=40).reshape(img.shape)
        part = _device(torch, img[2:], _sim_noise.EVERY_STAGE, 9, scene_id0=42).reshape(2, 17, 19)
        assert whole[2:].tobytes() == part.tobytes()
        assert whole[:2].tobytes() != _device(torch, img[:2], _sim_noise.EVERY_STAGE, 9, scene_id0=42).tobytes()
        assert whole.tobytes() != _device(torch, img, _sim_noise.EVERY_STAGE, 10, scene_id0=40).tobytes()        # another frame
        assert whole.tobytes() != _device(torch, img, dict(_sim_noise.EVERY_STAGE, seed=1), 9, scene_id0=40).tobytes()


def test_a_non_default_stream_and_the_python_wrapper():
    import torch
    from avoid_mpc_amd.host import sim_depth_noise
    img = _sim_noise.noise_images(33, 3, 48, 64, np.uint16)
    want = flight.depth_noise_ordered(img, _sim_noise.EVERY_STAGE, P2M, 4, 7)
    side = torch.cuda.Stream()
    assert np.array_equal(_device(torch, img, _sim_noise.EVERY_STAGE, 4, 7, stream=side).reshape(img.shape), want)
    depth = torch.from_numpy(img.view(np.int16)).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        out = sim_depth_noise(depth, _sim_noise.EVERY_STAGE, P2M, 4, scene_id0=7)                               # torch's current stream
    again = sim_depth_noise(depth, _sim_noise.EVERY_STAGE, P2M, 4, scene_id0=7, out=torch.zeros_like(depth), stream=side)
    side.synchronize()
    assert out.dtype == depth.dtype and out.data_ptr() != depth.data_ptr()
    assert np.array_equal(out.cpu().numpy().view(np.uint16), want) and np.array_equal(again.cpu().numpy().view(np.uint16), want)
    assert np.array_equal(depth.cpu().numpy().view(np.uint16), img)                                                  # out of place
    f32 = torch.from_numpy(_sim_noise.noise_images(33, 2, 17, 19, np.float32)).cuda()
    got = sim_depth_noise(f32, dict(seed=3, sigma0=0.01), P2M, 0)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and np.array_equal(_bits(got.cpu().numpy()), _bits(flight.depth_noise_ordered(f32.cpu().numpy(), dict(seed=3, sigma0=0.01), P2M, 0)))


def test_every_argument_error_leaves_the_output_unwritten():
    import torch
    from avoid_mpc_amd.host import sim_noise_params
    lib = capi.load()
    src = torch.full((2, 4, 6), 2000, dtype=torch.int16, device="cuda"); dst = torch.full((2, 4, 6), 7, dtype=torch.int16, device="cuda")
    big = torch.full((96,), 7, dtype=torch.int16, device="cuda")
    h_src = np.full((2, 4, 6), 2000, np.uint16); h_dst = np.full((2, 4, 6), 7, np.uint16)
    p_src, p_dst, p_big = src.data_ptr(), dst.data_ptr(), big.data_ptr()
    for fn, tail, a, b in ((lib.amk_sim_depth_noise, (None,), p_src, p_dst), (lib.amk_sim_depth_noise_host, (), h_src.ctypes.data, h_dst.ctypes.data)):
        def call(i=a, o=b, kind=capi.AMK_DEPTH_U16, rows=4, cols=6, stride=24, S=2, p2m=1e-3, null_prm=False, **kw):
            return fn(i, o, kind, rows, cols, stride, S, p2m, None if null_prm else C.byref(sim_noise_params(kw)), 0, 0, *tail)
        assert call(i=None) == BAD and call(o=None) == BAD and call(null_prm=True) == BAD
        assert call(o=a) == BAD and call(i=b, o=b) == BAD                         # in place
        assert call(i=a, o=a + 2 * 47) == BAD and call(i=a + 2 * 47, o=a) == BAD  # 48 pixels each, 47 apart
        assert call(i=b + 2 * 10, o=b, stride=30) == BAD
        assert call(rows=0) == BAD and call(cols=0) == BAD and call(S=0) == BAD and call(cols=-6) == BAD
        assert call(stride=23) == BAD and call(stride=-1) == BAD
        assert call(p2m=0.0) == BAD and call(p2m=-1.0) == BAD and call(p2m=NAN) == BAD
        for name in ("p_drop", "p_edge_drop", "p_edge_fly"):
            assert call(**{name: -1e-9}) == BAD and call(**{name: 1.0 + 1e-9}) == BAD and call(**{name: NAN}) == BAD, name
        assert call(p_edge_drop=0.6, p_edge_fly=0.5) == BAD
        for name in ("sigma0", "sigma2", "edge_jump", "disparity_quantum", "z_min", "z_max"):
            assert call(**{name: -1e-300}) == BAD and call(**{name: NAN}) == BAD, name
        assert call(disparity_quantum=0.1) == BAD and call(disparity_quantum=0.1, focal_baseline=0.0) == BAD and call(disparity_quantum=0.1, focal_baseline=NAN) == BAD
        assert call(kind=2) == BAD and call(kind=-1) == BAD
        assert call(o=a + (1 << 40), S=65536) == UNSUPPORTED                      # (refused: the far address is never touched)
        assert call(o=a + (1 << 50), S=1, rows=1 << 16, cols=1 << 16, stride=1 << 32) == UNSUPPORTED
    torch.cuda.synchronize()
    assert (dst == 7).all().item() and (big == 7).all().item() and (src == 2000).all().item() and (h_dst == 7).all() and (h_src == 2000).all()
    # back-to-back images do not overlap: the two halves of one buffer of 96 pixels are a good call
    big[:48] = 1234
    assert lib.amk_sim_depth_noise(p_big, p_big + 2 * 48, capi.AMK_DEPTH_U16, 4, 6, 24, 2, 1e-3, C.byref(sim_noise_params({})), 0, 0, None) == capi.AMK_OK
    torch.cuda.synchronize()
    assert (big == 1234).all().item()
