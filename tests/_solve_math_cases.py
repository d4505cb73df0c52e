"""Case tables, numpy restatements and high-precision references for the solve's small primitives (csrc/fast_math.h and the
reductions / slacks / scan of csrc/mpc_device_impl.h).  Shared by tests/test_solve_math_cases.py (CPU: the tables and the
restatements themselves) and tests/test_solve_math_gpu.py (the device, through csrc/solve_probe.hip).

Everything here is deterministic: directed inputs first, fixed seeds where a sample is wanted.  The tables are functions
(cached), so importing this module costs nothing.

Limits (LIMIT_*): the worst error of the RESTATEMENT against mpmath on the tables below, rounded up to the next 0.05 --
measured, then written down here; tests/test_solve_math_cases.py re-measures them and fails when a table or a restatement has
moved away from its constant.  Errors of exp / log are in ulp of the true value; of exp's denormal results in denormal
quanta (2^-1074); of slacks and sg relative, in units of the format's eps (2^-52 / 2^-23)."""
import ctypes as C
import functools
import math

import mpmath
import numpy as np

from tests import _oracle

MP = mpmath.mp.clone()
MP.prec = 160                      # "120 bits or more"

F64, F32 = np.float64, np.float32
EPS = {F64: 2.0 ** -52, F32: 2.0 ** -23}
EMIN = {F64: -1022, F32: -126}     # exponent of the smallest normal
MANT = {F64: 52, F32: 23}
DBL_MIN, DBL_MAX = np.finfo(F64).tiny, np.finfo(F64).max
DENORM_MIN, DENORM_MAX = 5e-324, np.nextafter(DBL_MIN, 0.0)
LN2 = math.log(2.0)
INV_LN2 = 1.44269504088896338700e+00     # the constants of fast_exp / fast_log, as the header writes them
SQRT_HALF = 0.70710678118654752440
EXP_LO, EXP_HI = -745.2, 709.7

# collide_term's exact-zero pre-test: a term further than radius + FAR_MARGIN skips the chain, i.e. x <= -32 * FAR_MARGIN
FAR_MARGIN = {F64: 1.15625, F32: 0.6}
DORMANT_AT = {F64: -32.0 * FAR_MARGIN[F64], F32: float(F32(-32.0 * FAR_MARGIN[F32]))}      # -37, -19.2f
THRESHOLD_IN = {F64: (-37.0, -36.7), F32: (-19.2, -16.5)}             # (lo, hi]: where log(1 + e^x) stops being exactly 0

# measured on this module's tables (tests/test_solve_math_cases.py), rounded up to the next 0.05
LIMIT_EXP_ULP = 1.0
LIMIT_LOG_ULP = 0.8
LIMIT_EXP_DENORMAL_QUANTA = 0.75
LIMIT_SLACKS_EPS = {F64: 1.2, F32: 0.75}
LIMIT_SG_EPS = {F64: 1.3, F32: 1.6}
LIMIT_CHAIN_ULP = {F64: 0.75, F32: 2.35}     # g = log(1 + e^x) against the exact logarithm of the ROUNDED 1 + e^x, on SG_X (fp32: numpy's log)
LIMIT_RCP_ULP = 1.0                # the contract of rcp_f64 / the fp32 fast_rcp (fast_math.h), not a measurement
# On the device a reciprocal (allowed 1 ulp, multiplying a term no larger than the result) stands where the restatements
# divide: one eps more for slacks and sg, in both arithmetics.
DEVICE_LIMIT_SLACKS_EPS = {F64: LIMIT_SLACKS_EPS[F64] + 1.0, F32: LIMIT_SLACKS_EPS[F32] + 1.0}
DEVICE_LIMIT_SG_EPS = {F64: LIMIT_SG_EPS[F64] + 1.0, F32: LIMIT_SG_EPS[F32] + 1.0}


def round_up_005(v):
    return math.ceil(v / 0.05 - 1e-9) * 0.05


def neighbours(x, n, dtype=F64):
    """x and the n values of `dtype` next to it on either side, ascending in the bit pattern's order."""
    it = np.int64 if dtype is F64 else np.int32
    return (np.array(x, dtype).view(it) + np.arange(-n, n + 1, dtype=it)).view(dtype)


# ---------------------------------------------------------------------------------------------------------------- log
@functools.lru_cache(None)
def log_normal():
    """fast_log's directed arguments, all positive, finite and normal."""
    j = np.arange(1, 54)
    k = np.arange(-1022, 1024)
    rng = np.random.default_rng(5)
    below, above = np.nextafter(SQRT_HALF, 0.0), np.nextafter(SQRT_HALF, 1.0)
    km = np.arange(-1021, 1025)                         # 0.7071 * 2^k is normal from k = -1021; frexp's m * 2^k: up to 1024
    parts = [neighbours(c, 64) for c in (1.0, SQRT_HALF, math.sqrt(2.0), 0.5, 2.0)]
    parts += [1.0 + 2.0 ** -j[:52], 1.0 - 2.0 ** -j,    # (1 + 2^-53 is 1)
              2.0 ** k, np.ldexp(below, km), np.ldexp(SQRT_HALF, km), np.ldexp(above, km),
              np.array([DBL_MIN, DBL_MAX, np.nextafter(DBL_MIN, 1.0), np.nextafter(DBL_MAX, 0.0), 1.4056]),
              neighbours(1.4056, 64),                   # (where the restatement's error peaks on random arguments)
              1.0 + np.exp(np.linspace(-40.0, 3.0, 4097)),
              rng.uniform(0.5, 2.0, 20000), np.exp(rng.uniform(-60.0, 60.0, 4000))]   # and a sample: products of slacks
    x = np.concatenate(parts)
    assert np.all((x >= DBL_MIN) & (x <= DBL_MAX))
    return x


@functools.lru_cache(None)
def log_denormal():
    return np.concatenate([[DENORM_MAX, DENORM_MIN, 1e-310, 2.0 ** -1060, 3 * DENORM_MIN], np.ldexp(SQRT_HALF, np.arange(-1070, -1022, 6)),
                           neighbours(DENORM_MAX, 4)[:5]])


LOG_SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, -1.0, -DBL_MIN, np.nan, 1.0])
# what fast_log returns for them: -inf, -inf, +inf, NaN, NaN, NaN, NaN, +0


# ---------------------------------------------------------------------------------------------------------------- exp
@functools.lru_cache(None)
def exp_table():
    """fast_exp's directed arguments inside the clamp [-745.2, 709.7] (ends included)."""
    k = np.arange(-1080, 1030).astype(F64)
    rng = np.random.default_rng(6)
    half = (k + 0.5) * LN2
    parts = [k * LN2, np.nextafter(half, -np.inf), half, np.nextafter(half, np.inf),
             np.array([0.0, -0.0, 1e-17, -1e-17, 5e-324, EXP_LO, EXP_HI, 709.0]),
             np.linspace(EXP_LO, -708.3, 4096),
             rng.uniform(-40.0, 12.0, 20000), rng.uniform(EXP_LO, EXP_HI, 4000)]   # and a sample: -32 (rho - r) of live terms
    x = np.concatenate(parts)
    return x[(x >= EXP_LO) & (x <= EXP_HI)]


EXP_SPECIAL = np.array([np.inf, -np.inf, np.nan, 1e9, -1e9, np.nextafter(EXP_LO, -np.inf), np.nextafter(EXP_HI, np.inf)])
# fast_exp clamps: these equal fast_exp(709.7), (-745.2), (-745.2: fmax drops the NaN), (709.7), (-745.2), (-745.2), (709.7)
EXP_SPECIAL_AS = np.array([EXP_HI, EXP_LO, EXP_LO, EXP_HI, EXP_LO, EXP_LO, EXP_HI])


def restated_exp_log(x):
    """oracle/mpc_oracle.c's sexp(x) and slog(|x|): fast_math.h operation for operation (slog: for normal arguments)."""
    lib = _oracle.load_oracle()
    x = np.ascontiguousarray(x, F64)
    e, l = np.empty_like(x), np.empty_like(x)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.mpco_fast_math(vp(x), vp(e), vp(l), len(x))
    return e, l


# --------------------------------------------------------------------------------------------------------- reciprocal
def _mantissas(n, dtype=F64):
    """n evenly spaced mantissas in [1, 2), off the grid's own points so that the low bits are not all zero"""
    return (1.0 + (np.arange(n) + 0.6180339887498949) / n).astype(dtype)


@functools.lru_cache(None)
def rcp64_table():
    """rcp_f64's domain: x and 1 / x both normal."""
    m = _mantissas(1 << 16)
    blocks = [np.ldexp(m, e) for e in (-1021, -1, 0, 1, 1021)]
    pos = np.concatenate(blocks + [2.0 ** np.arange(-1022, 1023), neighbours(1.0, 64),
                                   np.exp(np.linspace(math.log(1e-12), math.log(1e12), 20001)),   # slacks, distances, kappa_sigma
                                   1.0 + np.exp(np.linspace(-40.0, 3.0, 4097))])                  # 1 + e^x of sg
    x = np.concatenate([pos, -np.concatenate(blocks)])
    with np.errstate(over="ignore"):
        assert np.all((np.abs(x) >= DBL_MIN) & (np.abs(1.0 / x) >= DBL_MIN) & np.isfinite(1.0 / x))
    return x


@functools.lru_cache(None)
def rcp32_table():
    """every float in [1, 2), then a mantissa sample at the two extreme exponents that keep 1 / x normal, in both signs"""
    every = (np.int32(0x3F800000) + np.arange(1 << 23, dtype=np.int32)).view(F32)
    m = _mantissas(1 << 12, F32)
    ext = np.concatenate([np.ldexp(m, -126), np.ldexp(m, 125)]).astype(F32)
    x = np.concatenate([every, ext, -ext, np.array([1.0, 2.0, 0.5, 3.0, 1e-3, 1e10], F32)])
    assert np.all((np.abs(x) >= np.finfo(F32).tiny) & (np.abs(1.0 / x.astype(F64)) >= np.finfo(F32).tiny))
    return x


def rcp_correctly_rounded(x):
    x = np.asarray(x)
    return 1.0 / x if x.dtype == F64 else (1.0 / x.astype(F64)).astype(F32)


def rcp_true_error(x, r, n_exact=4000):
    """-> (share correctly rounded, worst true error in ulp of the true value, its x).  Every result is measured in the next wider format (good
    to 2^-12 ulp for doubles, 2^-29 for floats); a correctly rounded one is off by <= 1/2 ulp whatever that says, and the
    others (all of them, or the n_exact worst by that estimate) are measured again with mpmath."""
    x, r = np.asarray(x), np.asarray(r)
    dt = x.dtype.type
    cr = rcp_correctly_rounded(x)
    good = r == cr
    wide = np.longdouble if dt is F64 else F64
    assert np.finfo(wide).nmant >= (63 if dt is F64 else 52)
    with np.errstate(all="ignore"):
        q = 1 / x.astype(wide)
        ulp = np.ldexp(wide(1), np.maximum(np.frexp(np.abs(q))[1] - 1, EMIN[dt]) - MANT[dt])   # of the TRUE value's binade
        est = np.abs(r.astype(wide) - q) / ulp
    est = np.where(np.isfinite(est), est, np.inf).astype(F64)       # (a NaN or inf result is an infinite error)
    bad = np.flatnonzero(~good)
    if len(bad) > n_exact:
        bad = bad[np.argsort(est[bad])[-n_exact:]]
    est[bad] = true_ulp_error(r[bad], [1 / MP.mpf(float(v)) for v in x[bad]], dt)
    return float(good.mean()), float(est.max()), float(x[np.argmax(est)])


# ---------------------------------------------------------------------------------------------------------- dormancy
@functools.lru_cache(None)
def dormancy_table(dtype):
    if dtype is F64:
        x = np.concatenate([np.linspace(-40.0, -37.0, 1 << 16), neighbours(-37.0, 64), np.linspace(-37.0, -36.5, 1 << 16)])
    else:
        x = np.concatenate([np.linspace(-24.0, -19.2, 1 << 16).astype(F32), neighbours(-19.2, 64, F32),
                            np.linspace(-19.2, -16.0, 1 << 16).astype(F32)])
    return np.unique(x)


SG_X = np.linspace(-40.0, 3.0, 4097)


def softplus_np32(x):
    """the chain in numpy float32: log(1 + exp(x))"""
    x = np.asarray(x, F32)
    return np.log(F32(1.0) + np.exp(x))


def threshold(x, g):
    """the smallest x whose g is not exactly +0; every x below it has g == 0 by construction"""
    nz = np.flatnonzero(g != 0.0)
    return float(np.sort(x[nz])[0])


# ------------------------------------------------------------------------------------------------------------ slacks
@functools.lru_cache(None)
def slacks_table(dtype):
    """-> (s, mu): mu = 1e-9 .. 0.1, s = +-mu * 10^e for e = -12 .. 12, and s = 0.  fp32: only the pairs whose mu^2, s^2 and
    mu^2 / (r + |s|) are normal floats."""
    mu = 10.0 ** np.arange(-9, 0).astype(F64)
    e = 10.0 ** np.arange(-12, 13).astype(F64)
    s = np.concatenate([np.outer(mu, e), -np.outer(mu, e), np.zeros((len(mu), 1))], axis=1) * 1.0371   # (no exact powers of ten)
    mu = np.repeat(mu[:, None], s.shape[1], axis=1) * 1.0093
    s, mu = s.reshape(-1).astype(dtype), mu.reshape(-1).astype(dtype)
    if dtype is F32:
        lo, hi = np.finfo(F32).tiny, np.finfo(F32).max
        s6, m6 = s.astype(F64), mu.astype(F64)
        r = np.sqrt(m6 * m6 + s6 * s6)
        q = [m6 * m6, np.where(s6 == 0, 1.0, s6 * s6), m6 * m6 / (r + np.abs(s6)), m6 + r + np.abs(s6)]
        ok = np.all([(v >= lo) & (v <= hi) for v in q], axis=0)
        s, mu = s[ok], mu[ok]
    return s, mu


def slacks_np(s, mu):
    """mpc_device_impl.h's slacks() in numpy, a correctly rounded division in place of the reciprocal"""
    s, mu = np.asarray(s), np.asarray(mu)
    a, r = np.abs(s), np.sqrt(mu * mu + s * s)
    ws, wb = mu + mu * mu / (r + a), mu + r + a
    return np.where(s > 0, ws, wb), np.where(s > 0, wb, ws)


def slacks_mp(s, mu):
    """-> lists of mpf: w1 = t - s, w2 = t + s at t = mu + sqrt(mu^2 + s^2), of the given (rounded) inputs"""
    w1, w2 = [], []
    for si, mi in zip(s, mu):
        si, mi = MP.mpf(float(si)), MP.mpf(float(mi))
        t = mi + MP.sqrt(mi * mi + si * si)
        w1.append(t - si); w2.append(t + si)
    return w1, w2


# ------------------------------------------------------------------------------------------ wave reductions and scan
def tree(v, op=np.add, seg=64):
    """The reduction ladders' order of operations on [..., 64]: pairs, quads, eights, sixteens inside a row, then the rows as
    (r0 + r1) + (r2 + r3); cut at `seg` for seg_sum.  Every lane gets its segment's result.  `op` commutes, so which lane of a
    pair is the left operand does not matter."""
    out = np.asarray(v)
    w = 1
    while w < seg:
        first = out.reshape(*out.shape[:-1], 64 // (2 * w), 2, w)[..., 0]
        with np.errstate(invalid="ignore"):             # (inf - inf of the min / max waves)
            out = np.repeat(op(first[..., 0], first[..., 1]), 2 * w, axis=-1)
        w *= 2
    return out


@functools.lru_cache(None)
def wave_sum_table():
    """finite waves [n][64] float64 (exact in float32 too but for the last block, which is rounded there): the 64 one-hot
    waves, the lane-index wave, and waves whose sum depends on the tree"""
    rng = np.random.default_rng(20240611)
    onehot = np.eye(64)
    lanes = np.arange(64.0)[None]
    mag = np.ldexp(rng.uniform(1.0, 2.0, (8, 32)), rng.integers(-30, 31, (8, 32)))
    pairs = np.concatenate([mag, -mag * (1.0 + rng.uniform(-1e-7, 1e-7, mag.shape))], axis=1)   # cancellation
    for w in pairs:
        rng.shuffle(w)
    return np.concatenate([onehot, 3.5 * onehot[::-1], lanes, pairs, rng.standard_normal((4, 64))])


@functools.lru_cache(None)
def wave_minmax_table():
    """waves for min / max beyond the finite ones: one NaN, all NaN, +inf, -inf, both.  (No +0 beside -0.)"""
    rng = np.random.default_rng(7)
    w = rng.uniform(1.0, 9.0, (6, 64)) * rng.choice([-1.0, 1.0], (6, 64))
    w[0, 37] = np.nan
    w[1, :] = np.nan
    w[2, 5] = np.inf
    w[3, 60] = -np.inf
    w[4, 17], w[4, 48] = np.inf, -np.inf
    w[5, 0], w[5, 63], w[5, 16] = np.nan, np.nan, np.inf
    return w


SCAN_N = (1, 2, 31, 32)
SCAN_ALPHA = (0.0, 1.0, 0.97, -0.5, 1.03)


@functools.lru_cache(None)
def scan_table():
    """-> x0, x1 [n][64], al0, al1 [n], N [n]: every (N, alpha) with another alpha on the second channel; lanes at or beyond N
    of either 32-lane half hold 0; the two halves hold different data."""
    rng = np.random.default_rng(99)
    x0, x1, a0, a1, Ns = [], [], [], [], []
    for N in SCAN_N:
        for i, al in enumerate(SCAN_ALPHA):
            on = (np.arange(64) & 31) < N
            x0.append(np.where(on, rng.standard_normal(64) * 10.0 ** rng.integers(-3, 4, 64), 0.0))
            x1.append(np.where(on, rng.standard_normal(64), 0.0))
            a0.append(al); a1.append(SCAN_ALPHA[(i + 2) % len(SCAN_ALPHA)]); Ns.append(N)
    return np.array(x0), np.array(x1), np.array(a0), np.array(a1), np.array(Ns)


def scan_mp(x, al):
    """the sequential recurrence x_e = b_e + alpha x_{e+1} inside each 32-lane half, and the bound's sum
    sum_j |alpha|^j |b_{e+j}| -> (values [n][64] of mpf, sums [n][64] float)"""
    vals, sums = [], []
    for row, a in zip(np.asarray(x, F64), np.asarray(al, F64)):
        a = MP.mpf(float(a))
        v, s = [None] * 64, [None] * 64
        for h in (0, 32):
            acc, accs = MP.mpf(0), MP.mpf(0)
            for e in range(31, -1, -1):
                b = MP.mpf(float(row[h + e]))
                acc, accs = b + a * acc, abs(b) + abs(a) * accs
                v[h + e], s[h + e] = acc, float(accs)
        vals.append(v); sums.append(s)
    return vals, np.array(sums)


# ------------------------------------------------------------------------------------------ high-precision measures
def true_ulp_error(got, true, dtype=F64):
    """|got - true| in ulp of the TRUE value (true: mpf per element); below the smallest normal an ulp is the denormal
    quantum, so there the figure is in quanta."""
    out = np.empty(len(got))
    for i, (g, t) in enumerate(zip(got, true)):
        g = float(g)
        if not math.isfinite(g):
            out[i] = np.inf
            continue
        if t == 0:
            out[i] = 0.0 if g == 0.0 else np.inf
            continue
        ex = max(int(MP.floor(MP.log(abs(t), 2))), EMIN[dtype])
        out[i] = float(abs(MP.mpf(g) - t) / MP.ldexp(MP.mpf(1), ex - MANT[dtype]))
    return out


def rel_error_eps(got, true, dtype=F64):
    """|got - true| / |true| in units of the format's eps"""
    return np.array([float(abs(MP.mpf(float(g)) - t) / abs(t)) for g, t in zip(got, true)]) / EPS[dtype]


def mp_exp(x):
    return [MP.exp(MP.mpf(float(v))) for v in x]


def mp_log(x):
    return [MP.log(MP.mpf(float(v))) for v in x]


def mp_softplus_of_rounded(ex, dtype):
    """log(1 + e^x) as the reference program forms it (not log1p): the exact logarithm of the ROUNDED sum 1 + ex, ex being the
    e^x the implementation under test produced in its format"""
    return mp_log((dtype(1.0) + np.asarray(ex, dtype)).astype(dtype))


def mp_sigmoid(x):
    return [1 / (1 + MP.exp(-MP.mpf(float(v)))) for v in x]
