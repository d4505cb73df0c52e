"""GPU: the primitives every interior-point iteration of the solve is made of -- fast_exp / fast_log / rcp_f64 of
csrc/fast_math.h, and fast_rcp, the softplus chain of collide_term, slacks, the DPP reduction ladders, seg_sum and
suffix_scan2 of csrc/mpc_device_impl.h in both arithmetics -- through the probes of csrc/solve_probe.hip, on the directed tables of
tests/_solve_math_cases.py, against mpmath and against the operation-for-operation restatements (which
tests/test_solve_math_cases.py holds against mpmath themselves: every limit below is the restatement's own worst error on
the same table, rounded up to the next 0.05).

Measured (CPU: the restatement against mpmath, which sets the limit; device: an MI355X):
  exp, normal results     CPU 0.9569 ulp (x = -4.4692), limit 1.0     device: the restatement's bits on all 36 500 arguments
  exp, denormal results   CPU 0.7257 quanta (x = -708.99), limit 0.75 device: the same bits
  log, normal arguments   CPU 0.7835 ulp (the double below sqrt 2), limit 0.8
                          device 0.7835 ulp, the restatement's bits on all 37 165 arguments; denormals 0.4688 ulp (1.4653e-317)
  slacks fp64 / fp32      CPU 1.198 / 0.718 eps, limits 1.2 / 0.75, on the device + 1 for its reciprocal: 2.2 / 1.75
                          device 1.198 / 0.664 eps, the small slack 0.689 / 0.644
  sg fp64 / fp32          CPU 1.296 / 1.567 eps, limits 1.3 / 1.6, on the device + 1 for its reciprocal: 2.3 / 2.6
                          device 1.323 eps (x = -6.847) / 1.428 eps (x = -8.905)
  g = log(1 + e^x)        against the exact log of the rounded 1 + e^x: CPU 0.7105 ulp (sexp, slog) / 2.3342 ulp (numpy's float32
                          exp and log), limits 0.75 / 2.35; device 0.7105 ulp (x = -0.5588) / 2.0661 ulp (x = 1.5513)
  rcp_f64                 limit 1 ulp (the header's contract); device: correctly rounded on 681 632 of 681 632, worst 0.5000 ulp
  fast_rcp fp32           limit 1 ulp; device: correctly rounded on 8 404 998 of 8 404 998 (every float of [1, 2) among them)
  log(1 + e^x) leaves 0   CPU and device alike at x = -36.73679713130388 (fp64), -16.635507583618164 (fp32)

Each check was seen to fail against a library with one value-level change (no address depends on any of them); the tests
that failed, none other did:
  Lg7 = 1.4898...e-01 (*)                               test_fast_log_normal_arguments
  the dk * ln2_lo term dropped                          test_fast_log_normal_arguments, test_fast_log_denormals_and_specials
  the branch constant 0.7071... set to 0.75             test_fast_log_normal_arguments
  rcp_f64's correction reduced to fma(e, r, r)          test_rcp_f64_true_error (10.2 ulp), test_fast_log_normal_arguments,
                                                        test_sg_is_the_sigmoid[fp64]
  DPP_MIRROR -> DPP_HALF_MIRROR in row_reduce           test_wave_reductions_are_the_numpy_tree[fp64], [fp32]
  the rows combined as ((r0 + r1) + r2) + r3            test_wave_reductions_are_the_numpy_tree[fp64], [fp32]
  half_shift_down's bound k + d < 32 -> k + d < 64      test_suffix_scan2[fp64], [fp32]
  the fp32 margin 0.6 -> 0.5 (the table's threshold)    test_the_chain_is_exactly_zero_where_the_pretest_skips_it[fp32]
  (*) Lg7's last printed digit is below the double's precision (any last digit gives the same double), and one ulp of Lg7
      moves no result: its term is <= 1.4e-12 of the logarithm.  The change taken is the third digit.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _solve_math_cases as K

pytestmark = pytest.mark.gpu
F64, F32 = K.F64, K.F32
BOTH = pytest.mark.parametrize("dt", [F64, F32], ids=["fp64", "fp32"])
INT = {F64: np.int64, F32: np.int32}
AMK_ERR_INVALID_ARG = 1


def bits(a):
    return np.ascontiguousarray(a).view(INT[a.dtype.type])


@functools.lru_cache(None)
def _lib():
    from avoid_mpc_amd import capi
    lib = capi.load()
    vp, i = C.c_void_p, C.c_int
    for suf in ("f64", "f32"):
        for name, args in (("scalar", [vp, vp, i, vp]), ("slacks", [vp, vp, vp, i, vp]), ("wave", [vp, vp, i, vp]),
                           ("scan", [vp, vp, vp, vp, vp, i, vp])):
            fn = getattr(lib, f"amk__solve_probe_{name}_{suf}")
            fn.restype, fn.argtypes = i, args
    lib.amk__solve_probe_wave_planes.restype, lib.amk__solve_probe_wave_planes.argtypes = i, []
    return lib


def _run(name, dt, ins, n, planes, per=1):
    """ins to the device, the probe, its [planes][n * per] output back"""
    import torch
    dev = [torch.from_numpy(np.ascontiguousarray(a, dt)).cuda() for a in ins]
    out = torch.full((planes, n * per), 7.0, dtype=torch.float64 if dt is F64 else torch.float32, device="cuda")
    fn = getattr(_lib(), f"amk__solve_probe_{name}_{'f64' if dt is F64 else 'f32'}")
    assert fn(*[C.c_void_p(d.data_ptr()) for d in dev], C.c_void_p(out.data_ptr()), n, None) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


def scalar(x, dt=F64):
    """-> exp, log (sign kept), reciprocal, g = log(1 + e^x), sg = e^x / (1 + e^x)"""
    return _run("scalar", dt, [x], len(x), 5)


def slacks(s, mu, dt):
    return _run("slacks", dt, [s, mu], len(s), 2)


WAVE_PLANES = ("row_sum", "wave_sum", "wave_min", "wave_max", "r2_sum", "r2_min", "r3_sum", "r3_min", "r3_max",
               "seg1", "seg2", "seg4", "seg8", "seg16", "seg32", "seg64")


def wave(v, dt):
    assert v.ndim == 2 and v.shape[1] == 64 and _lib().amk__solve_probe_wave_planes() == len(WAVE_PLANES)
    o = _run("wave", dt, [v], len(v), len(WAVE_PLANES), 64)
    return dict(zip(WAVE_PLANES, o.reshape(len(WAVE_PLANES), len(v), 64)))


def scan(x0, x1, a0, a1, dt):
    return _run("scan", dt, [x0, x1, a0, a1], len(x0), 2, 64).reshape(2, len(x0), 64)


def test_probes_refuse_null_and_empty():
    import torch
    lib, d = _lib(), torch.zeros(64, dtype=torch.float64, device="cuda")
    p = C.c_void_p(d.data_ptr())
    for suf in ("f64", "f32"):
        f = lambda name: getattr(lib, f"amk__solve_probe_{name}_{suf}")
        assert f("scalar")(None, p, 1, None) == f("scalar")(p, None, 1, None) == f("scalar")(p, p, 0, None) == AMK_ERR_INVALID_ARG
        assert f("slacks")(p, None, p, 1, None) == f("slacks")(p, p, p, -1, None) == AMK_ERR_INVALID_ARG
        assert f("wave")(None, p, 1, None) == f("wave")(p, p, 0, None) == AMK_ERR_INVALID_ARG
        assert f("scan")(p, p, p, None, p, 1, None) == f("scan")(p, p, p, p, p, 0, None) == AMK_ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------------ exp and log
def test_fast_exp_is_the_restatement_bit_for_bit_and_clamps():
    x = np.concatenate([K.exp_table(), K.EXP_SPECIAL])
    e = scalar(x)[0]
    ce, _ = K.restated_exp_log(x)
    assert np.array_equal(bits(e), bits(ce)), x[bits(e) != bits(ce)][:8]
    n = len(K.EXP_SPECIAL)
    as_ = scalar(K.EXP_SPECIAL_AS)[0]
    assert np.array_equal(bits(e[-n:]), bits(as_)) and np.isfinite(e).all()      # NaN, -inf -> exp(-745.2); +inf, 1e9 -> exp(709.7)
    assert 1.6e308 < as_[0] < 1.7e308 and as_[1] == 0.0                          # (e^709.7 = 1.65e308; e^-745.2 is under half a quantum)
    assert (e[x == 0.0] == 1.0).all() and np.signbit(x[x == 0.0]).any()


def test_fast_log_normal_arguments():
    x = K.log_normal()
    l = scalar(x)[1]
    _, cl = K.restated_exp_log(x)
    same = np.mean(bits(l) == bits(cl))
    off = np.abs(l - cl) / np.spacing(np.abs(cl))
    err = K.true_ulp_error(l, K.mp_log(x))
    print(f"fast_log: bit-identical to slog on {same:.6f}, at most {off.max():.0f} ulp off it; true error {err.max():.4f} ulp "
          f"at x = {x[err.argmax()]!r} (limit {K.LIMIT_LOG_ULP})")
    assert off.max() <= 1.0 and same >= 0.999
    assert err.max() <= K.LIMIT_LOG_ULP


def test_fast_log_denormals_and_specials():
    x = K.log_denormal()
    l = scalar(x)[1]
    err = K.true_ulp_error(l, K.mp_log(x))
    print(f"fast_log on denormals: true error {err.max():.4f} ulp at x = {x[err.argmax()]!r}")
    assert err.max() <= K.LIMIT_LOG_ULP
    s = scalar(K.LOG_SPECIAL)[1]          # 0, -0, inf, -inf, -1, -DBL_MIN, NaN, 1
    assert s[0] == -np.inf and s[1] == -np.inf and s[2] == np.inf
    assert np.isnan(s[3:7]).all()
    assert s[7] == 0.0 and not np.signbit(s[7])


# -------------------------------------------------------------------------------------------------------- reciprocal
def test_rcp_f64_true_error():
    x = K.rcp64_table()
    r = scalar(x)[2]
    share, worst, at = K.rcp_true_error(x, r)
    print(f"rcp_f64: correctly rounded on {share:.6f} of {len(x)}, worst true error {worst:.4f} ulp at x = {at!r}")
    assert worst <= K.LIMIT_RCP_ULP
    assert (r[x == 1.0] == 1.0).all() and np.array_equal(r[np.abs(x) == 2.0 ** -1022], [2.0 ** 1022])


def test_fast_rcp_f32_true_error_on_every_float_of_one_binade():
    x = K.rcp32_table()
    r = scalar(x, F32)[2]
    assert r.dtype == F32
    share, worst, at = K.rcp_true_error(x, r)
    print(f"fast_rcp fp32: correctly rounded on {share:.6f} of {len(x)}, worst true error {worst:.4f} ulp at x = {at!r}")
    assert worst <= K.LIMIT_RCP_ULP
    assert r[0] == 1.0


# ---------------------------------------------------------------------------------------------- the softplus chain
@BOTH
def test_the_chain_is_exactly_zero_where_the_pretest_skips_it(dt):
    x = K.dormancy_table(dt)
    o = scalar(x, dt)
    g = o[3]
    far = x <= dt(K.DORMANT_AT[dt])
    assert far.sum() >= 1 << 16
    assert (g[far] == 0.0).all() and not np.signbit(g[far]).any()          # the pre-test's claim, on the chain itself
    thr, (lo, hi) = K.threshold(x, g), K.THRESHOLD_IN[dt]
    print(f"{dt.__name__}: log(1 + e^x) != 0 from x = {thr!r}")
    assert lo < thr <= hi and (g[x >= thr] > 0).all()
    assert (o[4][far] > 0).all()                                            # (the slope is not zero there: e^x itself)
    if dt is F64:   # real_exp / real_log are fast_exp / fast_log: the chain is the two probed functions composed
        e = o[0]
        assert np.array_equal(bits(g), bits(scalar(1.0 + e)[1]))
        ce, _ = K.restated_exp_log(x)
        assert thr == K.threshold(x, K.restated_exp_log(1.0 + ce)[1])


@BOTH
def test_sg_is_the_sigmoid(dt):
    x = K.SG_X.astype(dt)
    sg = scalar(x, dt)[4]
    err = K.rel_error_eps(sg, K.mp_sigmoid(x), dt)
    print(f"sg {dt.__name__}: {err.max():.4f} eps at x = {x[err.argmax()]!r} (limit {K.DEVICE_LIMIT_SG_EPS[dt]})")
    assert sg.dtype == dt and err.max() <= K.DEVICE_LIMIT_SG_EPS[dt]


@BOTH
def test_the_chain_is_the_logarithm_of_the_rounded_sum(dt):
    """g against the reference program's formula: the exact log of the ROUNDED 1 + e^x, e^x being the device's own"""
    x = K.SG_X.astype(dt)
    o = scalar(x, dt)
    err = K.true_ulp_error(o[3], K.mp_softplus_of_rounded(o[0], dt), dt)
    print(f"chain {dt.__name__}: {err.max():.4f} ulp at x = {x[err.argmax()]!r} (limit {K.LIMIT_CHAIN_ULP[dt]})")
    assert (o[3] > 0).sum() > 1500 and err.max() <= K.LIMIT_CHAIN_ULP[dt]


# ------------------------------------------------------------------------------------------------------------ slacks
@BOTH
def test_slacks(dt):
    s, mu = K.slacks_table(dt)
    w1, w2 = slacks(s, mu, dt)
    lim = K.DEVICE_LIMIT_SLACKS_EPS[dt]
    assert w1.dtype == dt and (w1 > 0).all() and (w2 > 0).all() and np.isfinite(w1).all() and np.isfinite(w2).all()
    t1, t2 = K.slacks_mp(s, mu)
    e1, e2 = K.rel_error_eps(w1, t1, dt), K.rel_error_eps(w2, t2, dt)
    small, large = np.where(s > 0, e1, e2), np.where(s > 0, e2, e1)
    print(f"slacks {dt.__name__}: the large slack {large.max():.4f} eps, the small one {small.max():.4f} eps (limit {lim})")
    assert large.max() <= lim
    assert small.max() <= lim                                               # no cancellation in the small slack
    ld = np.longdouble                                                      # (the difference to 2^-64, not to 2^-53)
    assert np.all(np.abs((w1.astype(ld) - w2.astype(ld)) + 2 * s.astype(ld)) <= lim * K.EPS[dt] * (w1.astype(ld) + w2.astype(ld)))


# -------------------------------------------------------------------------------------------------- wave reductions
def _same_or_both_nan(a, b):
    return np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b)))


@BOTH
def test_wave_reductions_are_the_numpy_tree(dt):
    v = np.concatenate([K.wave_sum_table(), K.wave_minmax_table()]).astype(dt)
    n_fin = len(K.wave_sum_table())
    o = wave(v, dt)
    fin = slice(0, n_fin)
    want = {"wave_sum": K.tree(v), "wave_min": K.tree(v, np.fmin), "wave_max": K.tree(v, np.fmax), "row_sum": K.tree(v, seg=16)}
    want.update({f"seg{s}": K.tree(v, seg=s) for s in (1, 2, 4, 8, 16, 32, 64)})
    for name, w in want.items():
        assert w.dtype == dt
        # the sums of a wave that holds a NaN or both infinities are NaN: a NaN for a NaN, bits everywhere else
        assert np.array_equal(bits(o[name][fin]), bits(w[fin])), name
        assert _same_or_both_nan(o[name], w), name
    for name in ("wave_sum", "wave_min", "wave_max"):                       # all 64 lanes hold the same bits
        assert (bits(o[name][fin]) == bits(o[name][fin])[:, :1]).all(), name
    assert (bits(o["row_sum"][fin]).reshape(n_fin, 4, 16) == bits(o["row_sum"][fin]).reshape(n_fin, 4, 16)[:, :, :1]).all()
    for fused, plain in (("r2_sum", "wave_sum"), ("r2_min", "wave_min"), ("r3_sum", "wave_sum"), ("r3_min", "wave_min"), ("r3_max", "wave_max")):
        assert _same_or_both_nan(o[fused], o[plain]) and np.array_equal(bits(o[fused][fin]), bits(o[plain][fin])), fused
    # a one-hot wave returns its one value whichever lane held it (the first 64 waves: 1.0 in lane l; the next 64: 3.5)
    for blk, val in ((slice(0, 64), 1.0), (slice(64, 128), 3.5)):
        for name in ("wave_sum", "wave_max", "seg64", "r2_sum", "r3_sum", "r3_max"):
            assert (o[name][blk] == val).all(), name
        assert (o["wave_min"][blk] == 0.0).all()
    # fmin / fmax drop a NaN; all NaN gives NaN
    m = K.wave_minmax_table()
    for row, mn, mx in zip(m, o["wave_min"][n_fin:], o["wave_max"][n_fin:]):
        ok = row[~np.isnan(row)].astype(dt)
        if len(ok):
            assert (mn == ok.min()).all() and (mx == ok.max()).all()
        else:
            assert np.isnan(mn).all() and np.isnan(mx).all()


# -------------------------------------------------------------------------------------------------------------- scan
@BOTH
def test_suffix_scan2(dt):
    x0, x1, a0, a1, N = K.scan_table()
    x0, x1, a0, a1 = (a.astype(dt) for a in (x0, x1, a0, a1))
    o = scan(x0, x1, a0, a1, dt)
    for ch, (x, al) in enumerate(((x0, a0), (x1, a1))):
        vals, sums = K.scan_mp(x, al)
        got = o[ch]
        err = np.array([[float(abs(K.MP.mpf(float(g)) - t)) for g, t in zip(gr, tr)] for gr, tr in zip(got, vals)])
        assert np.isfinite(got).all() and np.all(err <= 64 * K.EPS[dt] * sums), (ch, np.max(err / np.maximum(sums, 1e-300)) / K.EPS[dt])
        exact = (al == 0) | (N == 1)
        assert exact.sum() >= 8 and np.array_equal(bits(got[exact]), bits(x[exact]))   # x_e = b_e, bit for bit
        assert (got[(np.arange(64) & 31) >= N[:, None]] == 0).all()              # at or beyond N: nothing to sum
    # a lane of one 32-lane half never sees the other half: other data there, the same bits here
    for keep in (slice(0, 32), slice(32, 64)):
        y0, y1 = 1e6 + x0[:, ::-1].copy(), -3.0 * x1[:, ::-1].copy() - 1.0
        y0[:, keep], y1[:, keep] = x0[:, keep], x1[:, keep]
        p = scan(y0, y1, a0, a1, dt)
        assert np.array_equal(bits(p[:, :, keep]), bits(o[:, :, keep]))
