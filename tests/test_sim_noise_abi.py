"""CPU: amk_sim_depth_noise without a device -- the symbols are declared, listed, bound and exported, every argument rule is refused
before the device is asked for with the output untouched, the header states the contract, the new kernels use no scratch and no LDS.
And the numpy restatement (flight.noise_words, flight.depth_noise_ordered) is held to independent formulations: the stream to a
pure-Python big-integer mix, the discontinuity classification and the partner to a padded-array formulation, each stage alone to the
property it must have, and the stream's statistics to their expectations within five standard errors."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from avoid_mpc_amd import build as amk_build
from avoid_mpc_amd import capi, flight
from tests import _sim_noise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, UNSUPPORTED, NO_DEVICE = capi.AMK_ERR_INVALID_ARG, capi.AMK_ERR_UNSUPPORTED, capi.AMK_ERR_NO_DEVICE
NAN = float("nan")
M64 = (1 << 64) - 1
G_MAX = 3.4642          # the contract's bound on |g|
P2M = _sim_noise.P2M
# what the U16 store and the read back may move a depth by: half a count from rintf, and four float32 roundings (the depth, pixel2meter,
# the quotient, the read) of at most 2^-24 relative each on values below 65 536 counts: 4 * 2^-24 * 2^16 = 2^-6 of a count
U16_SLACK = (0.5 + 2.0 ** -6) * P2M


@pytest.fixture(scope="module")
def lib():
    amk_build.build()
    return capi.load()


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _prm(**kw):
    p = flight.noise_params(kw)
    return capi.SimNoiseParams(int(p.seed), *[float(getattr(p, n)) for n in flight.NOISE_FIELDS[1:]])


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_declared_listed_bound_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "avoid_mpc_amd.h")).read()
    section = hdr[hdr.index("Ground truth against the simulated world"):]
    for name, n_args in (("amk_sim_depth_noise", 12), ("amk_sim_depth_noise_host", 11)):
        assert re.search(r"^int " + name + r"\(", section, re.M), name       # declared, after the ground truth's section
        assert name in capi.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args, name
    assert capi.missing_symbols() == []
    assert lib.amk__sim_noise_words.restype is C.c_int and "amk__sim_noise_words" not in hdr and "amk__sim_noise_words" not in capi.SYMBOLS
    fields = re.search(r"typedef struct amk_sim_noise_params \{(.*?)\} amk_sim_noise_params;", hdr, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip() for decl in fields.split(";") if decl.strip() for n in decl.replace("unsigned long long", "").replace("double", "").split(",")]
    assert tuple(names) == flight.NOISE_FIELDS == tuple(n for n, _ in capi.SimNoiseParams._fields_)
    assert C.sizeof(capi.SimNoiseParams) == 8 * len(flight.NOISE_FIELDS)


def test_bad_arguments_are_refused_before_the_device_is_asked(lib):
    src = np.full((2, 4, 6), 2000, np.uint16); dst = np.full((2, 4, 6), 7, np.uint16)
    big = np.full(2 * 30 + 24, 7, np.uint16)
    for fn, tail in ((lib.amk_sim_depth_noise, (None,)), (lib.amk_sim_depth_noise_host, ())):
        def call(i=_vp(src), o=_vp(dst), kind=capi.AMK_DEPTH_U16, rows=4, cols=6, stride=24, S=2, p2m=1e-3, prm=None, null_prm=False, **kw):
            p = None if null_prm else C.byref(prm if prm is not None else _prm(**kw))
            return fn(i, o, kind, rows, cols, stride, S, p2m, p, 0, 0, *tail)
        assert call(i=None) == BAD and call(o=None) == BAD and call(null_prm=True) == BAD
        assert call(o=_vp(src)) == BAD                                          # in place
        assert call(i=_vp(big), o=C.c_void_p(big.ctypes.data + 2 * 47)) == BAD  # 48 pixels each, 47 apart
        assert call(i=C.c_void_p(big.ctypes.data + 2 * 10), o=_vp(big), stride=30) == BAD   # 54 pixels each with the stride, 10 apart
        assert call(rows=0) == BAD and call(cols=0) == BAD and call(S=0) == BAD and call(rows=-1) == BAD and call(S=-3) == BAD
        assert call(stride=23) == BAD and call(stride=0) == BAD and call(stride=-24) == BAD
        assert call(p2m=0.0) == BAD and call(p2m=-1e-3) == BAD and call(p2m=NAN) == BAD
        for name in ("p_drop", "p_edge_drop", "p_edge_fly"):
            assert call(**{name: -1e-9}) == BAD and call(**{name: 1.0 + 1e-9}) == BAD and call(**{name: NAN}) == BAD, name
        assert call(p_edge_drop=0.6, p_edge_fly=0.5) == BAD and call(p_edge_drop=1.0, p_edge_fly=1e-9) == BAD
        for name in ("sigma0", "sigma2", "edge_jump", "disparity_quantum", "z_min", "z_max"):
            assert call(**{name: -1e-300}) == BAD and call(**{name: NAN}) == BAD, name
        assert call(disparity_quantum=0.1) == BAD and call(disparity_quantum=0.1, focal_baseline=-1.0) == BAD
        assert call(disparity_quantum=0.1, focal_baseline=NAN) == BAD
        assert call(kind=2) == BAD and call(kind=-1) == BAD
        far = C.c_void_p(src.ctypes.data + (1 << 40))                           # (never touched: the call is refused)
        assert call(o=far, S=65536, stride=24) == UNSUPPORTED
        assert call(o=C.c_void_p(src.ctypes.data + (1 << 50)), S=1, rows=1 << 16, cols=1 << 16, stride=1 << 32) == UNSUPPORTED   # 2^24 tiles
        if lib.amk_device_count() <= 0:                                         # good calls reach the device question and nothing else
            assert call() == NO_DEVICE and call(**_sim_noise.EVERY_STAGE) == NO_DEVICE and call(kind=capi.AMK_DEPTH_F32, rows=2) == NO_DEVICE
            assert call(p_edge_drop=0.5, p_edge_fly=0.5) == NO_DEVICE and call(p_drop=1.0, p_edge_drop=1.0) == NO_DEVICE
            assert call(i=_vp(big), o=C.c_void_p(big.ctypes.data + 2 * 48)) == NO_DEVICE     # back to back
            assert call(focal_baseline=-1.0) == NO_DEVICE                       # (unused without a quantum)
    assert (dst == 7).all() and (big == 7).all() and (src == 2000).all()
    assert lib.amk__sim_noise_words(None, 4, 6, 1, 0, 0, 0, None) == BAD and lib.amk__sim_noise_words(_vp(big), 0, 6, 1, 0, 0, 0, None) == BAD
    assert lib.amk__sim_noise_words(_vp(big), 4, 6, 65536, 0, 0, 0, None) == UNSUPPORTED and (big == 7).all()


def test_the_header_states_the_noise_contract():
    hdr = open(os.path.join(ROOT, "include", "avoid_mpc_amd.h")).read()
    section = re.sub(r"\s*\*?\s+", " ", hdr[hdr.index("Sensor noise on the simulated depth frames"):])
    for sentence in ("z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) 0x94D049BB133111EB; return z ^ z >> 31",
                     "k = mix(mix(mix(seed) ^ (scene_id0 + s)) ^ frame)", "w_j = mix(k ^ (4 i + j))", "the position in the image, not in memory",
                     "g = (f0 + f1 + f2 + f3 - 131070) c", "c = 2.6428997921303014e-05 = 1 / sqrt((65536^2 - 1) / 3)", "|g| <= 3.4642",
                     "T(p) = p >= 1 ? 2^32 : (u64)(p 4294967296.0)", "(float)((double)(float)pixel pixel2meter)",
                     "is copied bit for bit; no stage sees it", "in the order left, right, up, down, are read from the INPUT image",
                     "z <- z + f (z_partner - z)", "z <- z + (sigma0 + (sigma2 z) z) g", "dq = rint(d / q) q", "z <- focal_baseline / dq",
                     "z not > 0, z < z_min, or (z_max > 0 and z > z_max)", "A call with everything off is a copy, for both pixel types",
                     "d_in == d_out or overlapping ranges", "p_edge_drop + p_edge_fly > 1", "allocates nothing and keeps no hidden state",
                     "Not offered: a calibrated model of any camera, spatially or temporally correlated noise"):
        assert sentence in section, sentence
    assert float("2.6428997921303014e-05") == flight.NOISE_SCALE == 1.0 / np.sqrt((65536.0 ** 2 - 1.0) / 3.0)
    assert 131070 * flight.NOISE_SCALE <= G_MAX


def test_the_new_kernels_use_no_scratch_and_no_lds(lib):
    table = json.load(open(amk_build.RES))
    mine = {n: r for n, r in table.items() if "sim_noise" in n}
    assert len(mine) == 3 and sum("sim_noise_kernel" in n for n in mine) == 2 and sum("sim_noise_words_kernel" in n for n in mine) == 1, sorted(mine)
    for n, r in mine.items():
        print(n, r)                                                             # (the VGPR counts are recorded in DESIGN.md, not gated)
        assert r["scratch_bytes_per_lane"] == 0 and r["lds_bytes"] == 0, (n, r)   # no tile is kept, so no LDS and no barrier


# ---- the stream ----------------------------------------------------------------------------------------------------------------------
def _mix_int(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def test_noise_words_equal_a_big_integer_restatement():
    rows, cols = 5, 9
    for seed, scene_id0, frame in ((0, 0, 0), (1, 255, 7), (M64, -3, M64 - 1), (0x0123456789ABCDEF, 2 ** 62, 2 ** 63 + 5)):
        w = flight.noise_words(seed, scene_id0, frame, 3, rows, cols)
        assert w.shape == (3, rows, cols, 3) and w.dtype == np.uint64
        for s in range(3):
            k = _mix_int(_mix_int(_mix_int(seed & M64) ^ ((scene_id0 + s) & M64)) ^ (frame & M64))
            want = [[_mix_int(k ^ (4 * i + j)) for j in range(3)] for i in range(rows * cols)]
            assert w[s].reshape(-1, 3).tolist() == want, (seed, scene_id0, frame, s)
    for z in (0, 1, M64, 0x8000000000000000, 12345678901234567890):                # the scalar form wraps too
        assert int(flight.noise_mix(np.uint64(z))) == _mix_int(z)


def test_seed_scene_and_frame_each_change_the_words_and_a_split_fleet_draws_the_same():
    base = flight.noise_words(5, 10, 3, 2, 6, 8)
    for other in (flight.noise_words(6, 10, 3, 2, 6, 8), flight.noise_words(5, 11, 3, 2, 6, 8), flight.noise_words(5, 10, 4, 2, 6, 8)):
        assert (other != base).mean() > 0.99
    assert np.array_equal(flight.noise_words(5, 11, 3, 1, 6, 8)[0], base[1])    # scene 1 of a call at 10 is scene 0 of a call at 11
    assert len(np.unique(base)) == base.size
    four = flight.noise_words(9, 0, 2, 4, 6, 8)
    assert np.array_equal(four[2:], flight.noise_words(9, 2, 2, 2, 6, 8))
    for dtype in (np.uint16, np.float32):                                       # and so do the frames
        img = _sim_noise.noise_images(3, 4, 17, 19, dtype)
        whole = flight.depth_noise_ordered(img, _sim_noise.EVERY_STAGE, P2M, 6)
        part = flight.depth_noise_ordered(img[2:], _sim_noise.EVERY_STAGE, P2M, 6, scene_id0=2)
        assert whole[2:].tobytes() == part.tobytes() and whole[:2].tobytes() != flight.depth_noise_ordered(img[:2], _sim_noise.EVERY_STAGE, P2M, 6, 2).tobytes()


def _variate(w0):
    f = [(w0 >> np.uint64(16 * j)) & np.uint64(0xffff) for j in range(4)]
    return (f[0].astype(np.int64) + f[1].astype(np.int64) + f[2].astype(np.int64) + f[3].astype(np.int64) - 131070) * flight.NOISE_SCALE


def test_the_streams_statistics_lie_within_five_standard_errors():
    """Per (seed, scene): 8 frames of 48 x 64.  Standard errors from the sample size N alone: the mean's is 1 / sqrt(N); a lag-1
    correlation is the mean of M products of independent unit-variance variates, 1 / sqrt(M); the variance's is sqrt(Var(g^2) / N) with
    Var(g^2) = E g^4 - 1 = 2 + (excess kurtosis of a discrete uniform on 65536 levels) / 4, the Irwin-Hall sum of four and not a
    normal's 2; the dropout rate's is binomial around T(p) / 2^32."""
    n = 65536.0
    var_g2 = 2.0 + (-(6.0 / 5.0) * (n * n + 1.0) / (n * n - 1.0)) / 4.0
    assert abs(var_g2 - 1.7) < 1e-9
    T = int(flight.noise_threshold(0.05))
    p = T / 2.0 ** 32
    assert abs(p - 0.05) < 2.0 ** -32
    worst = {}
    for seed in (0, 1, 7):
        for scene in (0, 1, 255):
            w = np.concatenate([flight.noise_words(seed, scene, frame, 1, 48, 64) for frame in range(8)])   # [8, 48, 64, 3]
            g = _variate(w[..., 0])
            N = g.size
            assert np.abs(g).max() <= G_MAX
            stats = {"mean": g.mean() * np.sqrt(N), "variance": (np.mean(g * g) - 1.0) / np.sqrt(var_g2 / N)}
            for name, a, b in (("horizontal", g[:, :, :-1], g[:, :, 1:]), ("vertical", g[:, :-1], g[:, 1:]), ("frame to frame", g[:-1], g[1:])):
                stats[name] = np.mean(a * b) * np.sqrt(a.size)
            stats["dropout"] = (np.mean((w[..., 1] >> np.uint64(32)) < np.uint64(T)) - p) / np.sqrt(p * (1.0 - p) / N)
            for name, v in stats.items():
                worst[name] = max(worst.get(name, 0.0), abs(float(v)))
                assert abs(v) <= 5.0, (seed, scene, name, v)
    print("\nlargest deviation in standard errors:", {k: round(v, 2) for k, v in worst.items()})


# ---- the stages ----------------------------------------------------------------------------------------------------------------------
def _z(img):
    return (img.astype(np.float32).astype(np.float64) * P2M).astype(np.float32).astype(np.float64)


def _padded_classification(z, jump):
    """The discontinuity stage written differently: the image padded by one pixel of +inf (neither a missing return nor a finite
    one), the four differences taken on the padded array at once -> (discontinuity pixel, index of the partner among left, right,
    up, down or -1)"""
    S, rows, cols = z.shape
    pad = np.pad(z, ((0, 0), (1, 1), (1, 1)), constant_values=np.inf)
    offsets = [(1, 0), (1, 2), (0, 1), (2, 1)]                                   # (row, column) starts of left, right, up, down
    nb = np.stack([pad[:, r:r + rows, c:c + cols] for r, c in offsets])          # [4, S, rows, cols]
    with np.errstate(invalid="ignore"):
        step = np.isfinite(nb) & (nb > 0) & (np.abs(nb - z) > jump)
        missing = ~(nb > 0)                                                      # NaN, 0, negative, -inf; never the padding
    disc = (step | missing).any(axis=0)
    partner = np.where(step.any(axis=0), step.argmax(axis=0), -1)
    return disc, partner, nb


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_the_discontinuity_stage_against_a_padded_formulation(dtype):
    jump = _sim_noise.EVERY_STAGE["edge_jump"]
    for rows, cols in ((17, 19), (1, 7), (7, 1), (1, 1), (3, 300)):
        img = _sim_noise.noise_images(11, 3, rows, cols, dtype)
        parts = {}
        out = flight.depth_noise_ordered(img, dict(seed=4, edge_jump=jump, p_edge_fly=1.0), P2M, 2, parts=parts)
        z = _z(img)
        disc, partner, nb = _padded_classification(z, jump)
        valid = np.isfinite(z) & (z > 0)
        assert np.array_equal(parts["valid"], valid)
        assert np.array_equal(parts["disc"], disc & valid) and np.array_equal(parts["partner"], (partner >= 0) & valid)
        zp = np.take_along_axis(nb, np.maximum(partner, 0)[None], axis=0)[0]
        has = valid & (partner >= 0)
        assert np.array_equal(parts["partner_z"][has], zp[has]) and np.array_equal(parts["flown"], has)   # p_edge_fly = 1: every one flies
        # a flown pixel lies between z and its partner (the store's rounding aside), a discontinuity pixel without a partner is dropped
        zo = _z(out)
        lo, hi = np.minimum(z, zp), np.maximum(z, zp)
        # the store: U16 rounds to half a count (no clamp: both ends are U16 depths); float32 rounds the depth, the quotient, the read back
        slack = np.full(z.shape, U16_SLACK) if dtype == np.uint16 else 3 * 2.0 ** -24 * hi
        assert (zo[has] >= lo[has] - slack[has]).all() and (zo[has] <= hi[has] + slack[has]).all()
        assert (out[valid & disc & (partner < 0)] == 0).all()
        same = ~has & ~(valid & disc & (partner < 0))
        assert img[same].tobytes() == out[same].tobytes()                        # everything else is copied
        if rows * cols > 100:
            assert has.sum() > 10 and (valid & disc & (partner < 0)).any() and (partner[has] > 0).any()


@pytest.mark.filterwarnings("ignore:invalid value:RuntimeWarning")     # (the invalid pixels' own z: masked out of every assertion)
def test_only_the_axial_stage_moves_a_pixel_within_its_bound():
    s0, s2 = 0.004, 0.0025
    for dtype in (np.uint16, np.float32):
        img = _sim_noise.noise_images(12, 3, 17, 19, dtype)
        out = flight.depth_noise_ordered(img, dict(seed=8, sigma0=s0, sigma2=s2), P2M, 1)
        z, zo = _z(img), _z(out)
        valid = np.isfinite(z) & (z > 0)
        assert img[~valid].tobytes() == out[~valid].tobytes()
        # rounding: the U16 store is within half a count (clamped pixels aside); float32 rounds the depth, the quotient and the read back
        ok = valid & (z + (s0 + s2 * z * z) * G_MAX < 65535 * P2M) if dtype == np.uint16 else valid
        round_off = U16_SLACK if dtype == np.uint16 else 3 * 2.0 ** -24 * (z + (s0 + s2 * z * z) * G_MAX)
        bound = (s0 + s2 * z * z) * G_MAX + round_off
        assert (np.abs(zo - z)[ok] <= bound[ok]).all() and ok.sum() > 100
        assert (out[ok] != img[ok]).mean() > 0.5                                 # and it does move them
        assert (out[valid & ~ok] > 0).all()


@pytest.mark.filterwarnings("ignore:divide by zero:RuntimeWarning", "ignore:invalid value:RuntimeWarning")   # (the same)
def test_only_the_disparity_stage_leaves_whole_disparities():
    fb, q = 38.0, 0.125
    for dtype in (np.uint16, np.float32):
        img = _sim_noise.noise_images(13, 3, 17, 19, dtype)
        out = flight.depth_noise_ordered(img, dict(focal_baseline=fb, disparity_quantum=q), P2M, 0)
        z, zo = _z(img), _z(out)
        valid = np.isfinite(z) & (z > 0)
        assert img[~valid].tobytes() == out[~valid].tobytes()
        steps = np.rint(fb / z / q)
        far = valid & (steps == 0)                                               # beyond the last disparity step: no return
        assert (out[far] == 0).all()
        kept = valid & ~far & (fb / (steps * q) < 65535 * P2M)
        n = fb / zo[kept] / q
        # zo = fb / (n q) up to the store: half a count in U16 (relative 0.5 P2M / z), three float32 roundings in F32
        rel = U16_SLACK / zo[kept] if dtype == np.uint16 else 3 * 2.0 ** -24
        assert (np.abs(n - steps[kept]) <= steps[kept] * rel * (1 + rel) + 1e-9).all() and kept.sum() > 100
        assert len(np.unique(steps[kept])) > 5


def test_everything_off_is_a_copy_and_each_gate_zeroes_what_it_names():
    for dtype in (np.uint16, np.float32):
        img = _sim_noise.noise_images(14, 3, 17, 19, dtype)
        assert flight.depth_noise_ordered(img, {}, P2M, 3).tobytes() == img.tobytes()
        assert flight.depth_noise_ordered(img, dict(seed=99, focal_baseline=5.0), P2M, 3).tobytes() == img.tobytes()
        if dtype == np.float32:
            assert np.isnan(img).any() and np.isinf(img).any() and (img < 0).any() and (img.view(np.uint32) == 0x7FC12345).any()
        z = _z(img)
        valid = np.isfinite(z) & (z > 0)
        out = flight.depth_noise_ordered(img, dict(z_min=0.3, z_max=25.0), P2M, 3)
        gone = valid & ((z < 0.3) | (z > 25.0))
        assert (out[gone] == 0).all() and out[~gone].tobytes() == img[~gone].tobytes() and gone.any() and (valid & (z == np.float32(0.3))).any()
        out = flight.depth_noise_ordered(img, dict(p_drop=1.0), P2M, 3)
        assert (out[valid] == 0).all() and out[~valid].tobytes() == img[~valid].tobytes()
        out = flight.depth_noise_ordered(img, dict(seed=1, p_drop=0.25), P2M, 3)
        assert 0.15 < (out[valid] == 0).mean() < 0.35 and out[out != 0].tobytes() == img[out != 0].tobytes()
        disc = _padded_classification(z, 0.25)[0] & valid
        out = flight.depth_noise_ordered(img, dict(edge_jump=0.25, p_edge_drop=1.0), P2M, 3)
        assert (out[disc] == 0).all() and out[~disc].tobytes() == img[~disc].tobytes() and disc.any()


def test_the_u16_read_and_write_round_trip_is_the_identity():
    pix = np.arange(65536, dtype=np.uint16).reshape(1, 256, 256)
    for p2m in (1.0, 0.001, 0.00025):
        z = (pix.astype(np.float32).astype(np.float64) * p2m).astype(np.float32).astype(np.float64)
        assert np.array_equal(flight.quantise_depth(z, p2m, np.uint16), pix), p2m
