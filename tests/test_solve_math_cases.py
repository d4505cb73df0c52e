"""CPU: the case tables of tests/_solve_math_cases.py hold what the GPU tests rely on, and the restatements the device is
compared with (oracle/mpc_oracle.c sexp / slog, the numpy slacks and reduction trees) are themselves held against mpmath:
that is where every LIMIT_* of the tables' module comes from."""
import math
import os
import re

import numpy as np

from tests import _solve_math_cases as K

F64, F32 = K.F64, K.F32


def _is_limit_of(worst, limit):
    """`limit` is `worst` rounded up to the next 0.05: a table or restatement that moved fails here, either way"""
    return worst <= limit and abs(K.round_up_005(worst) - limit) < 1e-9


# ------------------------------------------------------------------------------------------------------- the tables
def test_log_table_has_both_sides_of_every_branch_and_every_special():
    x = K.log_normal()
    m, _ = np.frexp(x)
    assert (m < K.SQRT_HALF).any() and (m >= K.SQRT_HALF).any()
    assert (m == K.SQRT_HALF).any() and (m == np.nextafter(K.SQRT_HALF, 0.0)).any()     # the two doubles the branch separates
    for c in (1.0, K.SQRT_HALF, math.sqrt(2.0), 0.5, 2.0):
        assert np.isin(K.neighbours(c, 64), x).all()
    j = np.arange(1, 54)
    assert np.isin(1.0 - 2.0 ** -j, x).all() and np.isin(1.0 + 2.0 ** -j[:52], x).all()
    assert np.isin(2.0 ** np.arange(-1022, 1024), x).all()
    assert np.isin([K.DBL_MIN, K.DBL_MAX], x).all()
    assert ((x > 1.0) & (x < 1.0 + 1e-15)).any() and ((x > 1.0 + math.exp(2.9)) & (x < 22.0)).any()   # 1 + e^x, both ends
    d = K.log_denormal()
    assert np.isin([K.DENORM_MAX, K.DENORM_MIN, 1e-310], d).all() and np.all((d > 0) & (d < K.DBL_MIN))
    s = K.LOG_SPECIAL
    bits = lambda v: np.array(v, F64).view(np.int64)
    for v in (0.0, -0.0, np.inf, -np.inf, -1.0, -K.DBL_MIN):
        assert (s.view(np.int64) == bits(v)).any(), v
    assert np.isnan(s).any()


def test_exp_table_has_ties_denormal_results_and_every_special():
    x = K.exp_table()
    assert x.min() == K.EXP_LO and x.max() == K.EXP_HI
    t = x * K.INV_LN2
    assert np.sum(np.abs(t - np.floor(t)) == 0.5) >= 100               # rint ties
    r = np.abs(x - np.rint(t) * K.LN2)
    assert r.max() > 0.34657 and (r == 0).sum() >= 1                    # |r| at its largest, ln2 / 2 = 0.346574
    k = np.rint(t)
    assert k.min() == -1075 and k.max() == 1024 and len(np.unique(k)) == 2100    # every exponent the clamp lets through
    with np.errstate(under="ignore"):
        e = np.exp(x)
    assert np.sum((e > 0) & (e < K.DBL_MIN)) >= 4000                   # denormal results
    assert np.isin([0.0, 1e-17, -1e-17, 5e-324, 709.0], x).all() and np.signbit(x[x == 0]).any()
    s = K.EXP_SPECIAL
    assert np.isin([np.inf, -np.inf, 1e9, -1e9], s).all() and np.isnan(s).any()
    assert (s < K.EXP_LO).any() and ((s > K.EXP_HI) & (s < 710)).any()


def test_reciprocal_tables_stay_inside_the_domain_and_cover_it():
    x = K.rcp64_table()
    e = np.frexp(np.abs(x))[1] - 1
    for want in (-1021, -1, 0, 1, 1021):
        assert np.sum(e == want) >= 2 * (1 << 16)
    assert (x < 0).sum() >= 5 * (1 << 16) and np.isin(2.0 ** np.arange(-1022, 1023), x).all()
    assert np.mean((x.view(np.int64) & 0xFF) != 0) > 0.9               # low mantissa bits are in use
    y = K.rcp32_table()
    assert len(np.unique(y[(y >= 1) & (y < 2)])) == 1 << 23             # every float of [1, 2)
    e32 = np.frexp(np.abs(y))[1] - 1
    assert (e32 == -126).sum() >= 8192 and (e32 == 125).sum() >= 8192 and (y < 0).any()


def test_dormancy_and_slack_and_wave_and_scan_tables():
    for dt in (F64, F32):
        x = K.dormancy_table(dt)
        at, (lo, hi) = K.DORMANT_AT[dt], K.THRESHOLD_IN[dt]
        assert x.dtype == dt and (x == dt(at)).any() and np.sum(x <= at) >= (1 << 16) and np.sum(x > at) >= (1 << 16)
        assert np.isin(K.neighbours(at, 64, dt), x).all()
        assert np.sum((x > lo) & (x <= hi)) > 1000 and (x > hi).any()
        s, mu = K.slacks_table(dt)
        assert s.dtype == dt and (s == 0).any() and (s > 0).any() and (s < 0).any()
        assert mu.min() < 1.1e-9 and mu.max() > 0.1 and len(np.unique(mu)) == 9
        ratio = np.abs(s[s != 0]).astype(F64) / mu[s != 0]
        assert ratio.min() < (1.1e-12 if dt is F64 else 1e-5) and ratio.max() > 0.9e12
    assert len(K.slacks_table(F64)[0]) == 9 * 51 and 200 < len(K.slacks_table(F32)[0]) < 9 * 51
    w = K.wave_sum_table()
    assert all((w == np.eye(64)[l]).all(axis=1).any() for l in range(64)) and (w == np.arange(64.0)).all(axis=1).any()
    assert np.isfinite(w).all()
    # waves whose sum depends on the tree: the tree and the left-to-right sum differ
    assert np.sum(K.tree(w)[:, 0] != np.cumsum(w, axis=1)[:, -1]) >= 4
    m = K.wave_minmax_table()
    n_nan = np.isnan(m).sum(axis=1)
    assert (n_nan == 1).any() and (n_nan == 64).any() and np.isposinf(m).any() and np.isneginf(m).any()
    assert not (m == 0).any()
    x0, x1, a0, a1, N = K.scan_table()
    assert set(N) == set(K.SCAN_N) and set(a0) == set(K.SCAN_ALPHA) and (a0 != a1).all()
    assert all(set(a0[N == n]) == set(K.SCAN_ALPHA) for n in K.SCAN_N)
    lane = np.arange(64) & 31
    for xx in (x0, x1):
        assert all((row[lane >= n] == 0).all() and (row[lane < n] != 0).all() for row, n in zip(xx, N))
        assert (xx[:, :32] != xx[:, 32:]).any(axis=1).all()


def test_the_margins_are_the_ones_the_solve_compiles():
    src = open(os.path.join(K._oracle.ROOT, "avoid_mpc_amd", "csrc", "mpc_device_impl.h")).read()
    m = re.search(r"far = radius \+ \(AMK_REAL_F32 \? RL\(([0-9.]+)\) : RL\(([0-9.]+)\)\)", src)
    assert m and float(m.group(1)) == K.FAR_MARGIN[F32] and float(m.group(2)) == K.FAR_MARGIN[F64]
    assert K.DORMANT_AT[F64] == -37.0 and K.DORMANT_AT[F32] == float(F32(-19.2))


# ------------------------------------------------------------------------------------- restatements against mpmath
def test_restated_exp_true_error():
    x = K.exp_table()
    e, _ = K.restated_exp_log(x)
    err = K.true_ulp_error(e, K.mp_exp(x))
    den = e < K.DBL_MIN
    wn, wd = err[~den].max(), err[den].max()
    print(f"sexp: normal results {wn:.4f} ulp at x = {x[~den][err[~den].argmax()]!r}; denormal results {wd:.4f} quanta "
          f"at x = {x[den][err[den].argmax()]!r}")
    assert den.sum() >= 4000
    assert _is_limit_of(wn, K.LIMIT_EXP_ULP) and _is_limit_of(wd, K.LIMIT_EXP_DENORMAL_QUANTA)
    es, _ = K.restated_exp_log(K.EXP_SPECIAL)
    ea, _ = K.restated_exp_log(K.EXP_SPECIAL_AS)
    assert np.array_equal(es.view(np.int64), ea.view(np.int64)) and np.isfinite(es).all()


def test_restated_log_true_error():
    x = K.log_normal()
    _, l = K.restated_exp_log(x)
    err = K.true_ulp_error(l, K.mp_log(x))
    print(f"slog: {err.max():.4f} ulp at x = {x[err.argmax()]!r}")
    assert _is_limit_of(err.max(), K.LIMIT_LOG_ULP)
    assert l[x == 1.0][0] == 0.0 and not np.signbit(l[x == 1.0][0])


def test_numpy_slacks_true_error():
    for dt in (F64, F32):
        s, mu = K.slacks_table(dt)
        w1, w2 = K.slacks_np(s, mu)
        assert w1.dtype == dt and (w1 > 0).all() and (w2 > 0).all()
        t1, t2 = K.slacks_mp(s, mu)
        e1, e2 = K.rel_error_eps(w1, t1, dt), K.rel_error_eps(w2, t2, dt)
        small = np.where(s > 0, e1, e2)
        print(f"slacks {dt.__name__}: worst {max(e1.max(), e2.max()):.4f} eps, the small slack {small.max():.4f} eps")
        assert _is_limit_of(max(e1.max(), e2.max()), K.LIMIT_SLACKS_EPS[dt])


def test_restated_sigmoid_true_error():
    """sg = e^x / (1 + e^x) with the restated exp (fp64) / numpy's float32 exp, a correctly rounded division"""
    for dt in (F64, F32):
        x = K.SG_X.astype(dt)
        ex = K.restated_exp_log(x)[0] if dt is F64 else np.exp(x)
        sg = ex / (dt(1.0) + ex)
        err = K.rel_error_eps(sg, K.mp_sigmoid(x), dt)
        print(f"sg {dt.__name__}: {err.max():.4f} eps at x = {x[err.argmax()]!r}")
        assert sg.dtype == dt and _is_limit_of(err.max(), K.LIMIT_SG_EPS[dt])


def test_restated_chain_true_error():
    """g = log(1 + e^x) with the restated exp and log (fp64) / numpy's float32 ones, against the exact logarithm of the
    rounded 1 + e^x"""
    for dt in (F64, F32):
        x = K.SG_X.astype(dt)
        if dt is F64:
            ex = K.restated_exp_log(x)[0]
            g = K.restated_exp_log(1.0 + ex)[1]
        else:
            ex = np.exp(x)
            g = np.log(F32(1.0) + ex)
        err = K.true_ulp_error(g, K.mp_softplus_of_rounded(ex, dt), dt)
        print(f"chain {dt.__name__}: {err.max():.4f} ulp at x = {x[err.argmax()]!r}")
        assert g.dtype == dt and (g > 0).sum() > 1500 and (g == 0).sum() > 100
        assert _is_limit_of(err.max(), K.LIMIT_CHAIN_ULP[dt])


def test_trees_against_fsum():
    for dt in (F64, F32):
        w = K.wave_sum_table().astype(dt)
        for seg in (1, 2, 4, 8, 16, 32, 64):
            t = K.tree(w, np.add, seg)
            assert t.dtype == dt and t.shape == w.shape
            for row, trow in zip(w, t):
                for b in range(0, 64, seg):
                    exact, mass = math.fsum(map(float, row[b:b + seg])), math.fsum(map(abs, map(float, row[b:b + seg])))
                    assert (trow[b:b + seg] == trow[b]).all()
                    assert abs(float(trow[b]) - exact) <= 6 * K.EPS[dt] * mass, (dt, seg, b)
    m = K.wave_minmax_table()
    mn, mx = K.tree(m, np.fmin)[:, 0], K.tree(m, np.fmax)[:, 0]
    for row, a, b in zip(m, mn, mx):
        ok = row[~np.isnan(row)]
        if len(ok):
            assert a == ok.min() and b == ok.max()
        else:
            assert np.isnan(a) and np.isnan(b)


def test_dormancy_threshold_of_the_restated_chain():
    x = K.dormancy_table(F64)
    e, _ = K.restated_exp_log(x)
    _, g = K.restated_exp_log(1.0 + e)
    lo, hi = K.THRESHOLD_IN[F64]
    thr = K.threshold(x, g)
    print(f"fp64: log(1 + e^x) != 0 from x = {thr!r} (-53 ln 2 = {-53 * K.LN2!r})")
    assert lo < thr <= hi and (g[x < thr] == 0).all() and not np.signbit(g[x < thr]).any() and (g[x >= thr] > 0).all()
    assert abs(thr + 53 * K.LN2) < 1e-3
    x = K.dormancy_table(F32)
    g = K.softplus_np32(x)
    lo, hi = K.THRESHOLD_IN[F32]
    thr = K.threshold(x, g)
    print(f"fp32: log(1 + e^x) != 0 from x = {thr!r} (-24 ln 2 = {-24 * K.LN2!r})")
    assert g.dtype == F32 and lo < thr <= hi and (g[x < thr] == 0).all() and (g[x >= thr] > 0).all()
    assert abs(thr + 24 * K.LN2) < 1e-3
